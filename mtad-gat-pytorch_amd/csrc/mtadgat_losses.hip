// Squared errors of a call's windows against the series they were cut from (mtadgat_eval_window_sse), and sums over consecutive
// groups of windows (mtadgat_eval_group_sums): what Trainer.evaluate (training.py:188-228) reduces model(x) to, without the
// (n, W, out_dim) reconstructions leaving the chunk they were computed in.  tests/loss_refs.py is the specification.
//
//   window w, first row s_w = starts[w] or start0 + w * stride, columns dims[d] (or d):
//     window_sse[w, 0] = sum_d        (preds[w, d]     - series[s_w + W, dims[d]])^2        the forecast
//     window_sse[w, 1] = sum_{t < W} sum_d (recons[w, t, d] - series[s_w + t, dims[d]])^2   the reconstruction
//     dim_sse[0, d], dim_sse[1, d]: the same squares summed over the windows (and time steps) instead of over d
//   Every difference is one float32 subtraction; it is squared in float64 (exact: 24-bit operands) and summed in float64.
//
//   k_window_sse    grid: slabs of consecutive windows.  A 256-thread workgroup walks its slab a window at a time, thread
//                   (row group r, column c): rows t = r, r + rp, .. of the window's (W, out) reconstruction, column(s) c (+ 256 k
//                   beyond 256 columns) -- consecutive threads read consecutive floats, rp rows at a time.  Per window two
//                   block_sum (mtadgat_scan.h); per thread the running sums of its columns over the slab, combined over the
//                   row groups in group order at the end: one partial per (slab, kind, column).
//                   The masked instances (mtadgat_fit_masked_sse; tests/fit_mask_refs.py) replace an unobserved term by +0.0 and
//                   count the observed ones: four entries per window, four kinds per column, one more block_sum per window.
//   k_dim_sse_final one wave per (kind, column): the slabs' partials in a fixed order (lane l: slabs l, l + 64, .., then a fixed
//                   tree over the lanes), added to the running total a previous call left (accumulate) or written.
//   k_group_sums    one workgroup per group: thread t adds rows t, t + 256, .. of the group in order, then block_sum.
// No atomics: a window's pair depends on that window's data alone, the per-column sums on the inputs and on how the caller cut
// the windows into calls (the slab count is a function of (batch, out_dim)).
#include <algorithm>
#include <string>

#include "../../include/mtadgat.h"      // the entry points' declarations
#include "mtadgat_scan.h"

using namespace mtadgat;

namespace {

constexpr int64_t N_MAX = 2147483647LL;
constexpr int SSE_THREADS = 256;
constexpr int SSE_OUT_MAX = 2048;
constexpr int SSE_W_MAX = 512;
constexpr int GROUP_COLS_MAX = 64;

// Slabs of a call: enough workgroups for eight per CU of the 256 where the call has the windows (at least four per slab, so that
// a slab's partials are few beside what it read), fewer for wide outputs whose partials (2 out doubles per slab) would outgrow
// the windows they summarise.  Non-decreasing in batch: the scratch of a call serves every shorter call.
inline int sse_slabs(int64_t batch, int out) {
    const int64_t cap = std::min<int64_t>(2048, std::max<int64_t>(128, (int64_t(1) << 18) / out));
    return (int)std::max<int64_t>(1, std::min<int64_t>(cap, batch / 4));
}

struct SseScratch {
    double* running;     // (kinds, out): the per-column sums of the calls so far
    double* part;        // (kinds, out, nslab): this call's partials, slab fastest
    int nslab;
};
// kinds: 2 (forecast, reconstruction), or 4 with the masked call's two counts behind them
SseScratch sse_scratch(ScratchCarver& c, int64_t batch, int out, int kinds = 2) {
    SseScratch l;
    l.nslab = sse_slabs(batch, out);
    l.running = c.take<double>(kinds * (size_t)out, 16);
    l.part = c.take<double>(kinds * (size_t)out * l.nslab, 16);
    return l;
}

// What the masked instances take on top (mtadgat_fit_masked_sse): the samples' ages, as the preparation reports them; a term is
// counted iff its series sample is observed, age <= max_age.  The plain instances carry an empty record.
template <bool MASK>
struct SseMask {};
template <>
struct SseMask<true> {
    const int* age;      // (n_rows, F), row stride ld
    long ld;
    int max_age;
};
constexpr double COUNT_ROWS = 4096.0;                    // a window's two counts in one sum: N_f (<= 2048) + COUNT_ROWS N_r (<= 2^20), exact

// NC: columns per thread (1: out <= 256, one column c of row group r; 8: columns c + 256 k of every row).
// MASK: a window has four entries -- S_f, S_r with every unobserved term replaced by +0.0 (a select: a NaN under the mask does not
// reach the sum), N_f, N_r the observed terms -- and `part` four kinds.  The unmasked arithmetic is the masked one with every term kept.
template <int NC, bool MASK>
__global__ void __launch_bounds__(SSE_THREADS) k_window_sse(const float* __restrict__ preds, const float* __restrict__ recons, long batch, int W,
                                                            int out, const float* __restrict__ series, long ld,
                                                            const long* __restrict__ starts, long start0, long stride,
                                                            const int* __restrict__ dims, int nslab, double* __restrict__ wsse,
                                                            double* __restrict__ part, SseMask<MASK> mask) {
    __shared__ double sm[SSE_THREADS];
    const int tid = threadIdx.x;
    const int ct = NC == 1 ? out : SSE_THREADS;          // column lanes
    const int rp = SSE_THREADS / ct;                     // row groups (>= 1)
    const int r = tid / ct, c = tid - r * ct;
    const bool active = r < rp;
    int col[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int d = c + k * ct;
        col[k] = d < out ? (dims ? dims[d] : d) : 0;
    }
    double af[NC], ar[NC];                               // this thread's columns over the slab: forecast (row group 0), reconstruction
    double nf[MASK ? NC : 1], nr[MASK ? NC : 1];         // MASK: and their observed terms
#pragma unroll
    for (int k = 0; k < NC; ++k) af[k] = ar[k] = 0.0;
    if constexpr (MASK) {
#pragma unroll
        for (int k = 0; k < NC; ++k) nf[k] = nr[k] = 0.0;
    }
    const long sl = blockIdx.x;
    const long w0 = batch * sl / nslab, w1 = batch * (sl + 1) / nslab;
    for (long w = w0; w < w1; ++w) {
        const long s = starts ? starts[w] : start0 + w * stride;
        double fw = 0.0, rw = 0.0;
        int cf = 0, cr = 0;                              // MASK: this thread's observed terms of the window
        if (active) {
            const float* rr = recons + w * (long)W * out;
            const float* sr = series + s * ld;
            const int* ag = nullptr;
            if constexpr (MASK) ag = mask.age + s * mask.ld;
#pragma unroll 4
            for (int t = r; t < W; t += rp) {
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int d = c + k * ct;
                    if (NC == 1 || d < out) {
                        const float df = rr[(long)t * out + d] - sr[t * ld + col[k]];
                        if constexpr (MASK) {
                            const bool seen = ag[t * mask.ld + col[k]] <= mask.max_age;
                            const double q = seen ? (double)df * (double)df : 0.0;
                            rw += q;
                            ar[k] += q;
                            cr += seen ? 1 : 0;
                            nr[k] += seen ? 1.0 : 0.0;
                        } else {
                            const double q = (double)df * (double)df;
                            rw += q;
                            ar[k] += q;
                        }
                    }
                }
            }
            if (r == 0) {
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int d = c + k * ct;
                    if (NC == 1 || d < out) {
                        const float df = preds[w * out + d] - sr[W * ld + col[k]];
                        if constexpr (MASK) {
                            const bool seen = ag[W * mask.ld + col[k]] <= mask.max_age;
                            const double q = seen ? (double)df * (double)df : 0.0;
                            fw += q;
                            af[k] += q;
                            cf += seen ? 1 : 0;
                            nf[k] += seen ? 1.0 : 0.0;
                        } else {
                            const double q = (double)df * (double)df;
                            fw += q;
                            af[k] += q;
                        }
                    }
                }
            }
        }
        fw = block_sum(fw, sm);
        rw = block_sum(rw, sm);
        if constexpr (MASK) {
            const double both = block_sum((double)cf + COUNT_ROWS * (double)cr, sm);      // integers below 2^53: exact in any order
            if (tid == 0) {
                const double n_r = floor(both / COUNT_ROWS);
                wsse[4 * w] = fw;
                wsse[4 * w + 1] = rw;
                wsse[4 * w + 2] = both - COUNT_ROWS * n_r;
                wsse[4 * w + 3] = n_r;
            }
        } else if (tid == 0) {
            wsse[2 * w] = fw;
            wsse[2 * w + 1] = rw;
        }
    }
    if (!part) return;                                   // (uniform)
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int d = c + k * ct;
        sm[tid] = ar[k];
        __syncthreads();
        if (r == 0 && d < out) {
            double v = 0.0;
            for (int j = 0; j < rp; ++j) v += sm[j * ct + c];
            part[((long)out + d) * nslab + sl] = v;
            part[(long)d * nslab + sl] = af[k];
        }
        __syncthreads();
        if constexpr (MASK) {
            sm[tid] = nr[k];
            __syncthreads();
            if (r == 0 && d < out) {
                double v = 0.0;
                for (int j = 0; j < rp; ++j) v += sm[j * ct + c];
                part[(3 * (long)out + d) * nslab + sl] = v;
                part[(2 * (long)out + d) * nslab + sl] = nf[k];
            }
            __syncthreads();
        }
    }
}

// grid: 2 out waves, four to a workgroup
__global__ void __launch_bounds__(256) k_dim_sse_final(const double* __restrict__ part, int cells, int nslab, int accumulate,
                                                       double* __restrict__ running, double* __restrict__ dim_sse) {
    const int lane = threadIdx.x & 63;
    const int cell = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= cells) return;                           // (wave-uniform)
    const double* p = part + (long)cell * nslab;
    double v = 0.0;
    for (int sl = lane; sl < nslab; sl += 64) v += p[sl];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) {
        if (accumulate) v = running[cell] + v;
        running[cell] = v;
        dim_sse[cell] = v;
    }
}

// grid: groups
__global__ void __launch_bounds__(256) k_group_sums(const double* __restrict__ x, long n, int cols, long group, double* __restrict__ out) {
    __shared__ double sm[256];
    const long g = blockIdx.x;
    const long i0 = g * group, i1 = i0 + group < n ? i0 + group : n;
    for (int c = 0; c < cols; ++c) {
        double v = 0.0;
#pragma unroll 4
        for (long i = i0 + threadIdx.x; i < i1; i += 256) v += x[i * cols + c];
        v = block_sum(v, sm);
        if (threadIdx.x == 0) out[g * cols + c] = v;
    }
}

bool progression_ok(int64_t start0, int64_t stride, int64_t batch, int W, int64_t n_rows) {
    if (start0 < 0 || stride < 0) return false;
    const int64_t room = n_rows - 1 - W - start0;        // the last window's first row may lie this far behind start0
    if (room < 0) return false;
    return batch == 1 || stride == 0 || (batch - 1) <= room / stride;
}

// mtadgat_eval_window_sse (MASK false: two entries per window, two kinds per dimension) and mtadgat_fit_masked_sse (MASK true: four)
template <bool MASK>
int window_sse_call(const char* what, const float* preds_dev, const float* recons_dev, int64_t batch, int W, int out_dim,
                    const float* series_dev, int64_t n_rows, int F, int64_t ld_series, const int64_t* starts_dev, int64_t start0,
                    int64_t stride, const int32_t* dims_dev, SseMask<MASK> mask, int accumulate, double* window_dev, double* dim_dev,
                    void* scratch_dev, size_t scratch_bytes, void* stream) {
    const std::string w(what);
    auto refuse = [&](int code, const char* msg) { return record_error(code, (w + msg).c_str()); };
    if (!preds_dev || !recons_dev || !series_dev || !window_dev || !scratch_dev) return refuse(-1, ": null pointer");
    if (batch < 1 || batch > N_MAX) return refuse(-1, ": batch must lie in [1, 2^31 - 1]");
    if (out_dim < 1 || out_dim > SSE_OUT_MAX) return refuse(-1, ": out_dim must lie in [1, 2048]");
    if (W < 1 || W > SSE_W_MAX) return refuse(-1, ": W must lie in [1, 512]");
    if (F < 1 || ld_series < F) return refuse(-1, ": ld_series < F or F < 1");
    if (!dims_dev && out_dim > F) return refuse(-1, ": out_dim > F needs dims_dev");
    if (n_rows < (int64_t)W + 1) return refuse(-1, ": the series is shorter than a window and its target row");
    if (accumulate != 0 && accumulate != 1) return refuse(-1, ": accumulate must be 0 or 1");
    if (!starts_dev && !progression_ok(start0, stride, batch, W, n_rows))
        return refuse(-1, ": windows start0 + w*stride .. +W and their target rows do not lie inside the series");
    constexpr int kinds = MASK ? 4 : 2;
    ScratchCarver carver(scratch_dev);
    const SseScratch l = sse_scratch(carver, batch, out_dim, kinds);
    if (scratch_bytes < carver.bytes()) return refuse(-5, ": scratch too small (see the call's _scratch function)");
    if ((uintptr_t)scratch_dev & 15) return refuse(-5, ": scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long* st = reinterpret_cast<const long*>(starts_dev);
    double* part = dim_dev ? l.part : nullptr;
    if (out_dim <= SSE_THREADS)
        hipLaunchKernelGGL((k_window_sse<1, MASK>), dim3((unsigned)l.nslab), dim3(SSE_THREADS), 0, s, preds_dev, recons_dev, (long)batch, W,
                           out_dim, series_dev, (long)ld_series, st, (long)start0, (long)stride, dims_dev, l.nslab, window_dev, part, mask);
    else
        hipLaunchKernelGGL((k_window_sse<8, MASK>), dim3((unsigned)l.nslab), dim3(SSE_THREADS), 0, s, preds_dev, recons_dev, (long)batch, W,
                           out_dim, series_dev, (long)ld_series, st, (long)start0, (long)stride, dims_dev, l.nslab, window_dev, part, mask);
    if (dim_dev)
        hipLaunchKernelGGL(k_dim_sse_final, dim3((unsigned)((kinds * out_dim + 3) / 4)), dim3(256), 0, s, (const double*)l.part,
                           kinds * out_dim, l.nslab, accumulate, l.running, dim_dev);
    return hipGetLastError() == hipSuccess ? 0 : refuse(-3, ": kernel launch failed");
}

}  // namespace

extern "C" {

size_t mtadgat_eval_window_sse_scratch(int64_t batch, int out_dim) {
    if (batch < 1 || batch > N_MAX || out_dim < 1 || out_dim > SSE_OUT_MAX) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { sse_scratch(c, batch, out_dim); });
}

int mtadgat_eval_window_sse(const float* preds_dev, const float* recons_dev, int64_t batch, int W, int out_dim, const float* series_dev,
                            int64_t n_rows, int F, int64_t ld_series, const int64_t* starts_dev, int64_t start0, int64_t stride,
                            const int32_t* dims_dev, int accumulate, double* window_sse_dev, double* dim_sse_dev, void* scratch_dev,
                            size_t scratch_bytes, void* stream) {
    return window_sse_call<false>("window_sse", preds_dev, recons_dev, batch, W, out_dim, series_dev, n_rows, F, ld_series, starts_dev, start0,
                                  stride, dims_dev, SseMask<false>{}, accumulate, window_sse_dev, dim_sse_dev, scratch_dev, scratch_bytes,
                                  stream);
}

size_t mtadgat_fit_masked_sse_scratch(int64_t batch, int out_dim) {
    if (batch < 1 || batch > N_MAX || out_dim < 1 || out_dim > SSE_OUT_MAX) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { sse_scratch(c, batch, out_dim, 4); });
}

int mtadgat_fit_masked_sse(const float* preds_dev, const float* recons_dev, int64_t batch, int W, int out_dim, const float* series_dev,
                           int64_t n_rows, int F, int64_t ld_series, const int64_t* starts_dev, int64_t start0, int64_t stride,
                           const int32_t* dims_dev, const int32_t* age_dev, int64_t ld_age, int32_t max_age, int accumulate,
                           double* window_dev, double* dim_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    if (!age_dev) return record_error(-1, "fit_masked_sse: null pointer");
    if (ld_age < F) return record_error(-1, "fit_masked_sse: ld_age < F");
    SseMask<true> mask;
    mask.age = age_dev;
    mask.ld = (long)ld_age;
    mask.max_age = (int)max_age;
    return window_sse_call<true>("fit_masked_sse", preds_dev, recons_dev, batch, W, out_dim, series_dev, n_rows, F, ld_series, starts_dev,
                                 start0, stride, dims_dev, mask, accumulate, window_dev, dim_dev, scratch_dev, scratch_bytes, stream);
}

int mtadgat_eval_group_sums(const double* x_dev, int64_t n, int cols, int64_t group, double* out_dev, void* stream) {
    if (!x_dev || !out_dev) return record_error(-1, "group_sums: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "group_sums: n must lie in [1, 2^31 - 1]");
    if (cols < 1 || cols > GROUP_COLS_MAX) return record_error(-1, "group_sums: cols must lie in [1, 64]");
    if (group < 1) return record_error(-1, "group_sums: group must be >= 1");
    if (group > n) group = n;                            // (one short group)
    const int64_t G = (n + group - 1) / group;
    hipLaunchKernelGGL(k_group_sums, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, x_dev, (long)n, cols, (long)group, out_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "group_sums: kernel launch failed");
}

}  // extern "C"
