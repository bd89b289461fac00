// Part-aware score passes for series that are concatenations of independent entities (MSL / SMAP channels, SMD machines): what the
// reference's adjust_anomaly_scores (utils.py:210-255) does at the seams, plus the Hundman threshold restarted per part (the moving
// average restarted per part is the segmented instantiation of the scan in mtadgat_evalcol.hip).  evaluation.score_parts describes the
// parts; tests/part_refs.py is the specification.
//
//   A part is a span [start, end) of score indices; the spans are disjoint and ascending (mtadgat_scan.h) and the kernels find the
//   part of an index by a binary search over the span ends (span_find).  A score that no span covers belongs to no part.
//   Reductions run over fixed row blocks of SPAN_RB with one slot per (part, block) and are combined in block order by one wave per
//   part: no atomics, the bits depend on the input alone.  No launch count depends on the number of parts.
//
//   k_part_minmax / k_part_minmax_final / k_part_adjust   blank the transitions around the seams, then min-max normalise per part
//   k_part_moments / k_part_moments_final                 sum, sum of squares and maximum per part
//   k_part_epsilon / k_part_epsilon_final                 find_epsilon's z table per part, the +-halo dilation clipped to the span:
//                                                         epsilon_tile (mtadgat_scan.h), which k_eval_epsilon runs over a whole column
//   k_part_flags                                          score_i > eps[part(i)]
//   k_part_scale                                          (a - median) / (1 + IQR) with the quantiles of the row's part, which
//                                                         mtadgat_eval_part_quantiles (mtadgat_evalcol.hip) selects
#include "../../include/mtadgat.h"      // the entry points' declarations
#include "mtadgat_scan.h"

namespace mtadgat {

// score i lies in [t - before, t + after] of some seam t: the first seam >= i - after is at most i + before (seams ascending)
__device__ __forceinline__ bool in_transition(const long* __restrict__ seam, long nseams, long i, long before, long after) {
    long lo = 0, hi = nseams;
    const long want = i - after;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (seam[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo < nseams && seam[lo] <= i + before;
}

// the values of `v` held by lanes 0 .. cnt - 1 added to acc in lane order (every lane computes the same sum)
__device__ __forceinline__ double wave_ordered_add(double acc, double v, int cnt) {
    for (int t = 0; t < cnt; ++t) acc += __shfl(v, t);
    return acc;
}

// ---- adjust ------------------------------------------------------------------------------------------------------------------------
// grid (part, slice): min / max of the non-NaN blanked values of every (row block, column) of the part; ct = columns per pass (a
// power of two <= 64), 256 / ct rows at a time
__global__ void __launch_bounds__(256) k_part_minmax(const float* __restrict__ x, long n, int d, long ld, const long* __restrict__ start,
                                                      const long* __restrict__ end, const long* __restrict__ seam, long nseams, long before,
                                                      long after, int ct, float* __restrict__ plo, float* __restrict__ phi) {
    __shared__ float slo[256];
    __shared__ float shi[256];
    const int tid = threadIdx.x;
    const long k = blockIdx.x;
    long s, e;
    span_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
    const int c = tid & (ct - 1), rsub = tid / ct, rp = 256 / ct;
    for (long b = blockIdx.y; b < nb; b += gridDim.y) {
        const long r0 = s + b * SPAN_RB;
        const int rows = e - r0 < SPAN_RB ? (int)(e - r0) : SPAN_RB;
        const long slot = slot0 + b;
        for (int c0 = 0; c0 < d; c0 += ct) {
            const int col = c0 + c;
            float lo = INFINITY, hi = -INFINITY;
            if (col < d) {
                for (int r = rsub; r < rows; r += rp) {
                    const long row = r0 + r;
                    const float v = in_transition(seam, nseams, row, before, after) ? 0.f : x[row * ld + col];
                    if (v == v) {
                        lo = fminf(lo, v);
                        hi = fmaxf(hi, v);
                    }
                }
            }
            slo[tid] = lo; shi[tid] = hi;
            __syncthreads();
            for (int st = rp >> 1; st > 0; st >>= 1) {
                if (rsub < st) {
                    slo[tid] = fminf(slo[tid], slo[tid + st * ct]);
                    shi[tid] = fmaxf(shi[tid], shi[tid + st * ct]);
                }
                __syncthreads();
            }
            if (rsub == 0 && col < d) {
                plo[slot * d + col] = slo[tid];
                phi[slot * d + col] = shi[tid];
            }
            __syncthreads();
        }
    }
}

// one wave per (part, column): lohi[(part * d + col) * 2] = { lo, hi } over the part's blocks (+inf, -inf: no non-NaN value); a zero is
// written as +0.0.  Minimum and maximum are exact, so the order of the blocks does not show.
__global__ void __launch_bounds__(64) k_part_minmax_final(long n, int d, const long* __restrict__ start, const long* __restrict__ end,
                                                           const float* __restrict__ plo, const float* __restrict__ phi,
                                                           double* __restrict__ lohi, double* __restrict__ lohi_out) {
    const long k = blockIdx.x;
    const int col = blockIdx.y, lane = threadIdx.x;
    long s, e;
    span_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
    float lo = INFINITY, hi = -INFINITY;
    for (long b = lane; b < nb; b += 64) {
        lo = fminf(lo, plo[(slot0 + b) * d + col]);
        hi = fmaxf(hi, phi[(slot0 + b) * d + col]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    if (lane == 0) {
        const long at = (k * d + col) * 2;
        const double l = (double)lo + 0.0, h = (double)hi + 0.0;
        lohi[at] = l; lohi[at + 1] = h;
        if (lohi_out) { lohi_out[at] = l; lohi_out[at + 1] = h; }
    }
}

// out = blanked x, normalised with its part's lo / hi when lohi is given: (x - lo) / (hi - lo) in float64, rounded once; +0.0 where
// hi <= lo; NaN stays NaN; a score outside every span is written through
__global__ void __launch_bounds__(256) k_part_adjust(const float* x, long n, int d, long ld, const long* __restrict__ start,
                                                      const long* __restrict__ end, long count, const long* __restrict__ seam, long nseams,
                                                      long before, long after, const double* __restrict__ lohi, float* out, long ld_out) {
    const long total = n * d;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long i = idx / d;
        const int col = (int)(idx - i * d);
        float v = x[i * ld + col];
        if (in_transition(seam, nseams, i, before, after)) v = 0.f;
        if (lohi && v == v) {
            long s;
            const long p = span_find(start, end, count, i, s);
            if (p >= 0) {
                const double lo = lohi[(p * d + col) * 2], hi = lohi[(p * d + col) * 2 + 1];
                v = hi > lo ? (float)(((double)v - lo) / (hi - lo) + 0.0) : 0.f;
            }
        }
        out[i * ld_out + col] = v;
    }
}

// ---- per-part moments and epsilon table --------------------------------------------------------------------------------------------
// the larger of m and v; a NaN wins and stays (numpy's max)
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

// grid (part, slice): per (part, row block) the float64 sum and sum of squares and the maximum
__global__ void __launch_bounds__(256) k_part_moments(const float* __restrict__ x, long n, const long* __restrict__ start,
                                                       const long* __restrict__ end, double* __restrict__ psum, double* __restrict__ psq,
                                                       float* __restrict__ pmax) {
    __shared__ double sm[256];
    __shared__ float smf[256];
    const int tid = threadIdx.x;
    const long k = blockIdx.x;
    long s, e;
    span_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
    for (long b = blockIdx.y; b < nb; b += gridDim.y) {
        const long r0 = s + b * SPAN_RB;
        const int rows = e - r0 < SPAN_RB ? (int)(e - r0) : SPAN_RB;
        double a = 0.0, q = 0.0;
        float m = -INFINITY;
        for (int r = tid; r < rows; r += 256) {
            const float f = x[r0 + r];
            const double v = (double)f;
            a += v;
            q += v * v;
            m = nan_max(m, f);
        }
        a = block_sum(a, sm);
        q = block_sum(q, sm);
        smf[tid] = m;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) smf[tid] = nan_max(smf[tid], smf[tid + st]);
            __syncthreads();
        }
        if (tid == 0) { psum[slot0 + b] = a; psq[slot0 + b] = q; pmax[slot0 + b] = smf[0]; }
        __syncthreads();
    }
}

// one wave per part: the block partials added in block order; mom[3 part] = { sum, sum of squares, maximum (-inf: empty part) }
__global__ void __launch_bounds__(64) k_part_moments_final(long n, const long* __restrict__ start, const long* __restrict__ end,
                                                            const double* __restrict__ psum, const double* __restrict__ psq,
                                                            const float* __restrict__ pmax, double* __restrict__ mom) {
    const long k = blockIdx.x;
    const int lane = threadIdx.x;
    long s, e;
    span_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
    double a = 0.0, q = 0.0;
    float m = -INFINITY;
    for (long base = 0; base < nb; base += 64) {
        const long b = base + lane;
        const int cnt = nb - base < 64 ? (int)(nb - base) : 64;
        a = wave_ordered_add(a, b < nb ? psum[slot0 + b] : 0.0, cnt);
        q = wave_ordered_add(q, b < nb ? psq[slot0 + b] : 0.0, cnt);
        const float mine = b < nb ? pmax[slot0 + b] : -INFINITY;
        for (int t = 0; t < cnt; ++t) m = nan_max(m, __shfl(mine, t));
    }
    if (lane == 0) { mom[3 * k] = a; mom[3 * k + 1] = q; mom[3 * k + 2] = (double)m; }
}

// grid (part, slice, z): for threshold eps[part * nz + z], per row block of the part, epsilon_tile's four sums with the part as the range
//   { sum of x < eps, its sum of squares, the count of x < eps, |{ i in the part : some |j| <= halo, i + j in the part, has x[i + j] >= eps }| }
__global__ void __launch_bounds__(256) k_part_epsilon(const float* __restrict__ x, long n, const long* __restrict__ start,
                                                       const long* __restrict__ end, const double* __restrict__ eps, int nz, int halo,
                                                       double* __restrict__ ptab) {
    __shared__ double sm[256];
    __shared__ unsigned long long hot[EPS_TILE_WORDS];
    const long k = blockIdx.x;
    const int z = blockIdx.z;
    const double ez = eps[k * nz + z];
    long s, e;
    span_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
    for (long b = blockIdx.y; b < nb; b += gridDim.y) {
        const long r0 = s + b * SPAN_RB;
        double a = 0.0, q = 0.0, cnt = 0.0, dil = 0.0;
        epsilon_tile(x, 1, s, e, r0, e - r0 < SPAN_RB ? (int)(e - r0) : SPAN_RB, ez, halo, hot, a, q, cnt, dil);
        a = block_sum(a, sm);                           // its barriers also close the reads of `hot`
        q = block_sum(q, sm);
        cnt = block_sum(cnt, sm);
        dil = block_sum(dil, sm);
        if (threadIdx.x == 0) {
            double* o = ptab + ((slot0 + b) * nz + z) * 4;
            o[0] = a; o[1] = q; o[2] = cnt; o[3] = dil;
        }
    }
}

// one wave per (part, z): the block rows of the table added in block order
__global__ void __launch_bounds__(64) k_part_epsilon_final(long n, const long* __restrict__ start, const long* __restrict__ end, int nz,
                                                            const double* __restrict__ ptab, double* __restrict__ tab) {
    const long k = blockIdx.x;
    const int z = blockIdx.y, lane = threadIdx.x;
    long s, e;
    span_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long base = 0; base < nb; base += 64) {
        const long b = base + lane;
        const int cnt = nb - base < 64 ? (int)(nb - base) : 64;
        const double* o = ptab + ((slot0 + (b < nb ? b : 0)) * nz + z) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = wave_ordered_add(acc[c], b < nb ? o[c] : 0.0, cnt);
    }
    if (lane == 0) {
        double* o = tab + (k * nz + z) * 4;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
    }
}

// ---- flags -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_part_flags(const float* __restrict__ x, long n, const long* __restrict__ start,
                                                     const long* __restrict__ end, long count, const double* __restrict__ thr,
                                                     unsigned char* __restrict__ flags) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        long s;
        const long p = span_find(start, end, count, i, s);
        flags[i] = (p >= 0 && (double)x[i] > thr[p]) ? 1 : 0;
    }
}

// ---- scale ---------------------------------------------------------------------------------------------------------------------------
// out = (a - median) / (1 + (q75 - q25)) with the quantiles q[(j * count + part) * d + col] (j = 0, 1, 2: q25, median, q75) of the
// row's part, in float32 with every operation rounded on its own; NaN for a row outside every span.  out may be a.
__global__ void __launch_bounds__(256) k_part_scale(const float* a, long n, int d, long ld, const long* __restrict__ start,
                                                     const long* __restrict__ end, long count, const float* __restrict__ q, float* out,
                                                     long ld_out) {
    __shared__ int owner[256];                          // the part of each of the block's rows: one search per row, not per element
    const int tid = threadIdx.x;
    const long per_q = count * d;
    for (long r0 = (long)blockIdx.x * 256; r0 < n; r0 += (long)gridDim.x * 256) {
        const int rows = n - r0 < 256 ? (int)(n - r0) : 256;
        if (tid < rows) {
            long s;
            owner[tid] = (int)span_find(start, end, count, r0 + tid, s);
        }
        __syncthreads();
        for (int j = tid; j < rows * d; j += 256) {
            const int r = j / d, col = j - r * d;
            const long p = owner[r];
            float v = __builtin_nanf("");
            if (p >= 0) {
                const float* qc = q + p * d + col;
                const float iqr = __fsub_rn(qc[2 * per_q], qc[0]);
                v = __fdiv_rn(__fsub_rn(a[(r0 + r) * ld + col], qc[per_q]), __fadd_rn(1.f, iqr));
            }
            out[(r0 + r) * ld_out + col] = v;
        }
        __syncthreads();
    }
}

}  // namespace mtadgat

using namespace mtadgat;

namespace {

constexpr int64_t N_MAX = 2147483647LL;

struct AdjustScratch {
    float *plo, *phi;
    double* lohi;
};
AdjustScratch adjust_scratch(ScratchCarver& c, int64_t n, int64_t count, int d) {
    const size_t cells = span_slots(n, count) * (size_t)d;
    AdjustScratch l;
    l.lohi = c.take<double>((size_t)count * (size_t)d * 2);
    l.plo = c.take<float>(cells);
    l.phi = c.take<float>(cells);
    return l;
}

struct EpsScratch {
    double *psum, *psq, *mom, *eps, *ptab, *tab;
    float* pmax;
};
EpsScratch eps_scratch(ScratchCarver& c, int64_t n, int64_t count, int nz) {
    const size_t slots = span_slots(n, count);
    EpsScratch l;
    l.psum = c.take<double>(slots);
    l.psq = c.take<double>(slots);
    l.mom = c.take<double>((size_t)count * 3);
    l.eps = c.take<double>((size_t)count * (size_t)nz);
    l.ptab = c.take<double>(slots * (size_t)nz * 4);
    l.tab = c.take<double>((size_t)count * (size_t)nz * 4);
    l.pmax = c.take<float>(slots);
    return l;
}

bool sizes_ok(int64_t n, int64_t count) { return n >= 1 && n <= N_MAX && count >= 1 && count <= N_MAX; }

unsigned capped_grid(long items) {
    const long blocks = (items + 255) / 256;
    return (unsigned)(blocks < 65536 ? blocks : 65536);
}

}  // namespace

extern "C" {

size_t mtadgat_eval_part_adjust_scratch(int64_t n, int d, int64_t count) {
    if (!sizes_ok(n, count) || d < 1 || d > 2048) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { adjust_scratch(c, n, count, d); });
}

int mtadgat_eval_part_adjust(const float* x_dev, int64_t n, int d, int64_t ld, const int64_t* start_dev, const int64_t* end_dev,
                             int64_t count, const int64_t* seam_dev, int64_t n_seams, int64_t before, int64_t after, int normalize,
                             void* scratch_dev, size_t scratch_bytes, float* out_dev, int64_t ld_out, double* lohi_dev, void* stream) {
    if (!x_dev || !start_dev || !end_dev || !out_dev || (n_seams > 0 && !seam_dev)) return record_error(-1, "part_adjust: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "part_adjust: n must lie in [1, 2^31 - 1]");
    if (count < 1 || count > N_MAX) return record_error(-1, "part_adjust: count must lie in [1, 2^31 - 1]");
    if (d < 1 || d > 2048) return record_error(-1, "part_adjust: d must lie in [1, 2048]");
    if (ld < d || ld_out < d) return record_error(-1, "part_adjust: ld < d");
    if (n_seams < 0 || n_seams > N_MAX || before < 0 || after < 0 || before > N_MAX || after > N_MAX)
        return record_error(-1, "part_adjust: needs 0 <= n_seams, before, after <= 2^31 - 1");
    if (!normalize && lohi_dev) return record_error(-1, "part_adjust: lo / hi are only computed with normalize");
    AdjustScratch l = {};
    if (normalize) {
        if (!scratch_dev) return record_error(-1, "part_adjust: null pointer");
        ScratchCarver carver(scratch_dev);
        l = adjust_scratch(carver, n, count, d);
        if (scratch_bytes < carver.bytes()) return record_error(-5, "part_adjust: scratch too small (see mtadgat_eval_part_adjust_scratch)");
        if ((uintptr_t)scratch_dev & 7) return record_error(-5, "part_adjust: scratch must be 8-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    const long* st = reinterpret_cast<const long*>(start_dev);
    const long* en = reinterpret_cast<const long*>(end_dev);
    const long* sm = reinterpret_cast<const long*>(seam_dev);
    if (normalize) {
        int ct = 1;
        while (ct < d && ct < 64) ct <<= 1;
        const long slices = span_slices(n, count, SPAN_RB);
        hipLaunchKernelGGL(k_part_minmax, dim3((unsigned)count, (unsigned)slices), dim3(256), 0, s, x_dev, (long)n, d, (long)ld, st, en, sm,
                           (long)n_seams, (long)before, (long)after, ct, l.plo, l.phi);
        hipLaunchKernelGGL(k_part_minmax_final, dim3((unsigned)count, (unsigned)d), dim3(64), 0, s, (long)n, d, st, en, (const float*)l.plo,
                           (const float*)l.phi, l.lohi, lohi_dev);
    }
    hipLaunchKernelGGL(k_part_adjust, dim3(capped_grid((long)n * d)), dim3(256), 0, s, x_dev, (long)n, d, (long)ld, st, en, (long)count, sm,
                       (long)n_seams, (long)before, (long)after, (const double*)(normalize ? l.lohi : nullptr), out_dev, (long)ld_out);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "part_adjust: kernel launch failed");
}

size_t mtadgat_eval_part_epsilon_scratch(int64_t n, int64_t count, int nz) {
    if (!sizes_ok(n, count) || nz < 1 || nz > 64) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { eps_scratch(c, n, count, nz); });
}

int mtadgat_eval_part_epsilon_moments(const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count, int nz,
                                      void* scratch_dev, size_t scratch_bytes, double* out_host, void* stream) {
    if (!x_dev || !start_dev || !end_dev || !scratch_dev || !out_host) return record_error(-1, "part_epsilon_moments: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "part_epsilon_moments: n must lie in [1, 2^31 - 1]");
    if (count < 1 || count > N_MAX) return record_error(-1, "part_epsilon_moments: count must lie in [1, 2^31 - 1]");
    if (nz < 1 || nz > 64) return record_error(-1, "part_epsilon_moments: nz must lie in [1, 64]");
    ScratchCarver carver(scratch_dev);
    const EpsScratch l = eps_scratch(carver, n, count, nz);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "part_epsilon_moments: scratch too small (see mtadgat_eval_part_epsilon_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "part_epsilon_moments: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long* st = reinterpret_cast<const long*>(start_dev);
    const long* en = reinterpret_cast<const long*>(end_dev);
    const long slices = span_slices(n, count, SPAN_RB);
    hipLaunchKernelGGL(k_part_moments, dim3((unsigned)count, (unsigned)slices), dim3(256), 0, s, x_dev, (long)n, st, en, l.psum, l.psq, l.pmax);
    hipLaunchKernelGGL(k_part_moments_final, dim3((unsigned)count), dim3(64), 0, s, (long)n, st, en, (const double*)l.psum, (const double*)l.psq,
                       (const float*)l.pmax, l.mom);
    if (hipGetLastError() != hipSuccess) return record_error(-3, "part_epsilon_moments: kernel launch failed");
    if (hipMemcpyAsync(out_host, l.mom, (size_t)count * 3 * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
        return record_error(-3, "part_epsilon_moments: copy failed");
    return hipStreamSynchronize(s) == hipSuccess ? 0 : record_error(-3, "part_epsilon_moments: stream failed");
}

int mtadgat_eval_part_epsilon_table(const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                                    const double* eps_host, int nz, int halo, void* scratch_dev, size_t scratch_bytes, double* out_host,
                                    void* stream) {
    if (!x_dev || !start_dev || !end_dev || !eps_host || !scratch_dev || !out_host) return record_error(-1, "part_epsilon_table: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "part_epsilon_table: n must lie in [1, 2^31 - 1]");
    if (count < 1 || count > N_MAX) return record_error(-1, "part_epsilon_table: count must lie in [1, 2^31 - 1]");
    if (nz < 1 || nz > 64) return record_error(-1, "part_epsilon_table: nz must lie in [1, 64]");
    if (halo < 0 || halo > EPS_HALO_MAX) return record_error(-1, "part_epsilon_table: halo must lie in [0, 128]");
    ScratchCarver carver(scratch_dev);
    const EpsScratch l = eps_scratch(carver, n, count, nz);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "part_epsilon_table: scratch too small (see mtadgat_eval_part_epsilon_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "part_epsilon_table: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long* st = reinterpret_cast<const long*>(start_dev);
    const long* en = reinterpret_cast<const long*>(end_dev);
    const size_t cells = (size_t)count * (size_t)nz;
    if (hipMemcpyAsync(l.eps, eps_host, cells * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
        return record_error(-3, "part_epsilon_table: copy failed");
    const long slices = span_slices(n, count, SPAN_RB);
    hipLaunchKernelGGL(k_part_epsilon, dim3((unsigned)count, (unsigned)slices, (unsigned)nz), dim3(256), 0, s, x_dev, (long)n, st, en,
                       (const double*)l.eps, nz, halo, l.ptab);
    hipLaunchKernelGGL(k_part_epsilon_final, dim3((unsigned)count, (unsigned)nz), dim3(64), 0, s, (long)n, st, en, nz, (const double*)l.ptab, l.tab);
    if (hipGetLastError() != hipSuccess) return record_error(-3, "part_epsilon_table: kernel launch failed");
    if (hipMemcpyAsync(out_host, l.tab, cells * 4 * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
        return record_error(-3, "part_epsilon_table: copy failed");
    return hipStreamSynchronize(s) == hipSuccess ? 0 : record_error(-3, "part_epsilon_table: stream failed");
}

int mtadgat_eval_part_flags(const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                            const double* thr_dev, unsigned char* flags_dev, void* stream) {
    if (!x_dev || !start_dev || !end_dev || !thr_dev || !flags_dev) return record_error(-1, "part_flags: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "part_flags: n must lie in [1, 2^31 - 1]");
    if (count < 1 || count > N_MAX) return record_error(-1, "part_flags: count must lie in [1, 2^31 - 1]");
    hipLaunchKernelGGL(k_part_flags, dim3(capped_grid((long)n)), dim3(256), 0, (hipStream_t)stream, x_dev, (long)n,
                       reinterpret_cast<const long*>(start_dev), reinterpret_cast<const long*>(end_dev), (long)count, thr_dev, flags_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "part_flags: kernel launch failed");
}

int mtadgat_eval_part_scale(const float* a_dev, int64_t n, int d, int64_t ld, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                            const float* q_dev, float* out_dev, int64_t ld_out, void* stream) {
    if (!a_dev || !start_dev || !end_dev || !q_dev || !out_dev) return record_error(-1, "part_scale: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "part_scale: n must lie in [1, 2^31 - 1]");
    if (count < 1 || count > N_MAX) return record_error(-1, "part_scale: count must lie in [1, 2^31 - 1]");
    if (d < 1 || d > 2048) return record_error(-1, "part_scale: d must lie in [1, 2048]");
    if (ld < d || ld_out < d) return record_error(-1, "part_scale: ld < d");
    hipLaunchKernelGGL(k_part_scale, dim3(capped_grid((long)n)), dim3(256), 0, (hipStream_t)stream, a_dev, (long)n, d, (long)ld,
                       reinterpret_cast<const long*>(start_dev), reinterpret_cast<const long*>(end_dev), (long)count, q_dev, out_dev,
                       (long)ld_out);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "part_scale: kernel launch failed");
}

}  // extern "C"
