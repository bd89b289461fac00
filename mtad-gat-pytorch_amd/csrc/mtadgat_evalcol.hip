// Per-column order statistics and the exponentially weighted mean of the anomaly scores (reference prediction.py:65-165:
// --scale_scores, --use_mov_av), so that the Predictor's post-processing stays on the device with the scores.
//
//   Shared primitives (the wave sum, the order bits of a float, the spans, the scratch carver) come from mtadgat_scan.h.
//   k_eval_colq_*: np.percentile ("linear") of every column of an (n, d) array for nq probabilities at once.  The two order
//       statistics each probability needs are EXACT: a most-significant-digit radix select (four 8-bit digits) on the
//       order-preserving 32-bit key of the float, all columns and all 2 nq ranks per pass.  Histograms are built with integer
//       atomics in LDS and merged with integer atomics in memory -- integer sums do not depend on their order, so two runs give
//       the same bits -- and the digit of every (column, rank) is chosen on the device between the passes.  Nothing is sorted.
//   k_colqv_* and the VALID instantiation of k_eval_colq_hist: the same select over the non-NaN entries of every column
//       (mtadgat_eval_column_quantiles_valid, np.nanpercentile): a count pass gives every column's number of valid entries, the ranks
//       are set per column from it, and every NaN takes one key above +inf that no such rank reaches.
//   k_partq_* and the segmented instantiations of k_eval_colq_hist / _pick: the same select for every (part, column) of a
//       concatenated series (mtadgat_eval_part_quantiles), by two routes chosen per part on the device.  A part of at most PARTQ_LONG
//       rows is selected inside one workgroup, bins, prefixes and ranks in LDS (k_partq_short).  A longer part runs the four passes
//       with bins in memory, its rows cut into chunks of PARTQ_LONG, one workgroup per (chunk, column tile); its bins are slot
//       floor(start / PARTQ_LONG) -- long parts are disjoint and longer than PARTQ_LONG, so no two share a slot, and the slots
//       number n / PARTQ_LONG + 1 whatever the number of parts.
//   k_ewm_chunk / _carry / _apply: pandas' ewm(span).mean() (adjust=True) as a blocked scan in float64: chunk-local scans, one wave
//       that composes the chunk carries in chunk order, and a pass that applies carry and closed-form denominator.  No atomics.
//       One template, instantiated for the whole array (mtadgat_eval_ewm), restarted at every span of a concatenated series
//       (mtadgat_eval_ewm_parts) and over the observed rows of a gappy series, on (N, D) pairs (mtadgat_eval_ewm_valid).
#include <string>

#include "../../include/mtadgat.h"      // the entry points' declarations
#include "mtadgat_scan.h"

namespace mtadgat {

// ---- column quantiles ------------------------------------------------------------------------------------------------------------
constexpr int CQ_CT = 8;        // columns per workgroup: 8 neighbouring lanes read 8 neighbouring columns of a row
constexpr int CQ_RT = 6;        // ranks per workgroup: CQ_RT * CQ_CT histograms of 256 bins = 48 KiB of LDS
constexpr int CQ_ROWS = 256 / CQ_CT;

// the select's key: the order bits as they stand, so -0.0 sorts just below +0.0 (both are 0 in the interpolation)
__device__ __forceinline__ unsigned colq_key(float v) { return float_order_bits(v); }
__device__ __forceinline__ float colq_value(unsigned k) { return float_from_order_bits(k); }
// the key of the select that skips NaN: +inf is 0xff800000, so 0xffffffff (the bits 0x7fffffff, itself a NaN) lies above every number
__device__ __forceinline__ unsigned colq_valid_key(float v) { return v != v ? 0xffffffffu : float_order_bits(v); }
// position of probability q among n sorted values: lo = floor(q (n - 1)) in float64, the weight of s[lo + 1] returned in *frac
__device__ __forceinline__ unsigned colq_rank(double q, long n, double* frac) {
    const double pos = __dmul_rn(q, (double)(n - 1));     // rounded product: a fused pos - lo would use the unrounded one
    const double lo = floor(pos);
    if (frac) *frac = __dsub_rn(pos, lo);
    return (unsigned)lo;
}

constexpr int CQ_INLINE = 8;    // up to this many probabilities travel in the kernel arguments: no host-to-device copy
struct ColqProbs {
    double v[CQ_INLINE];
};

// state[(col * R + r) * 2] = { key bits chosen so far, rank still to find among the keys that share them }
// inl: the probabilities are in `pv` and are written to q for the interpolation; otherwise q already holds them
__global__ void k_eval_colq_init(double* __restrict__ q, ColqProbs pv, int inl, int nq, long n, int d, unsigned* __restrict__ state,
                                 unsigned* __restrict__ nanflag, unsigned* __restrict__ hist) {
    const int R = 2 * nq;
    if (inl && blockIdx.x == 0 && threadIdx.x < nq) q[threadIdx.x] = pv.v[threadIdx.x];
    const long nstate = (long)d * R;
    const long nhist = nstate * 256;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nhist; i += (long)gridDim.x * blockDim.x) {
        hist[i] = 0u;
        if (i < nstate) {
            const int r = (int)(i % R);
            const unsigned lo = colq_rank(inl ? pv.v[r >> 1] : q[r >> 1], n, nullptr);
            const unsigned hi = (long)lo + 1 < n ? lo + 1 : (unsigned)(n - 1);
            state[2 * i] = 0u;
            state[2 * i + 1] = (r & 1) ? hi : lo;
        }
        if (i < d) nanflag[i] = 0u;
    }
}

// the same select for ONE given rank per column (R = 1): sorted[rank] of every column, for launch_column_rank
__global__ void k_eval_colq_init_rank(unsigned rank, int d, unsigned* __restrict__ state, unsigned* __restrict__ nanflag,
                                      unsigned* __restrict__ hist) {
    const long nhist = (long)d * 256;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nhist; i += (long)gridDim.x * blockDim.x) {
        hist[i] = 0u;
        if (i < d) {
            state[2 * i] = 0u;
            state[2 * i + 1] = rank;
            nanflag[i] = 0u;
        }
    }
}

constexpr int PARTQ_LONG = 16 * SPAN_RB;     // a part longer than this many rows takes the route with bins in memory

// One radix pass over the rows first, first + step, .. below `last` of the workgroup's CQ_CT columns: for every (column, rank) the
// histogram of digit (key >> shift) & 255 over the keys whose higher digits equal the rank's prefix, built in `h` and merged into
// `hist`.  state / hist start at the cell of (column 0, rank 0), nanflag at column 0.  Every thread of the workgroup calls it
// (barriers inside; one more before `h` is used again).  VALID: the select over the non-NaN entries -- every NaN, whatever its sign
// or payload, takes the one key above +inf (colq_valid_key), which no rank below the column's valid count can reach; nanflag is
// not touched.
template <bool VALID>
__device__ __forceinline__ void colq_hist_rows(const float* __restrict__ a, int d, long ld, int R, int shift, long first, long last, long step,
                                               const unsigned* __restrict__ state, unsigned* __restrict__ hist,
                                               unsigned* __restrict__ nanflag, unsigned* h) {
    const int tid = threadIdx.x;
    const int c = tid & (CQ_CT - 1);
    const int col = blockIdx.x * CQ_CT + c;
    const int r0 = blockIdx.z * CQ_RT;
    const int nr = R - r0 < CQ_RT ? R - r0 : CQ_RT;
    for (int i = tid; i < CQ_RT * CQ_CT * 256; i += 256) h[i] = 0u;
    const unsigned high = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    unsigned pfx[CQ_RT];
#pragma unroll
    for (int r = 0; r < CQ_RT; ++r) pfx[r] = (col < d && r < nr) ? state[2 * ((long)col * R + r0 + r)] : 0u;
    __syncthreads();
    if (col < d) {
        bool seen_nan = false;
        for (long row = first; row < last; row += step) {
            const float v = a[row * ld + col];
            if constexpr (!VALID) seen_nan = seen_nan || (v != v);
            const unsigned key = VALID ? colq_valid_key(v) : colq_key(v);
            const unsigned bin = (key >> shift) & 255u;
#pragma unroll
            for (int r = 0; r < CQ_RT; ++r)
                if (r < nr && ((key ^ pfx[r]) & high) == 0u) atomicAdd(&h[(r * CQ_CT + c) * 256 + bin], 1u);
        }
        if constexpr (!VALID)
            if (seen_nan && shift == 24 && blockIdx.z == 0) atomicOr(&nanflag[col], 1u);
    }
    __syncthreads();
    for (int i = tid; i < nr * CQ_CT * 256; i += 256) {
        const unsigned v = h[i];
        const int cc = blockIdx.x * CQ_CT + ((i >> 8) & (CQ_CT - 1));
        if (v && cc < d) atomicAdd(&hist[((long)cc * R + r0 + (i >> 8) / CQ_CT) * 256 + (i & 255)], v);
    }
}

// One pass, instantiated three times (VALID, with !SEG only: the column's non-NaN entries, see colq_hist_rows).  !SEG: the whole
// column, grid = (column tiles, row slices, rank groups), the rows walked grid-stride; no span array is read.  SEG: grid = (column tiles, chunks of PARTQ_LONG rows, rank groups); a chunk meets at most two long parts --
// the one that covers its first row and the one that starts inside it, which is the owner of slot `chunk` -- and adds its rows of
// each to that part's bins.  Chunks that meet no long part leave at once.
template <bool SEG, bool VALID = false>
__global__ void __launch_bounds__(256) k_eval_colq_hist(const float* __restrict__ a, long n, int d, long ld, int R, int shift,
                                                         const unsigned* __restrict__ state, unsigned* __restrict__ hist,
                                                         unsigned* __restrict__ nanflag, const long* __restrict__ start,
                                                         const long* __restrict__ end, long count, const int* __restrict__ slotmap) {
    __shared__ unsigned h[CQ_RT * CQ_CT * 256];
    const long sub = threadIdx.x >> 3;                    // CQ_ROWS rows at a time
    if constexpr (!SEG) {
        colq_hist_rows<VALID>(a, d, ld, R, shift, (long)blockIdx.y * CQ_ROWS + sub, n, (long)gridDim.y * CQ_ROWS, state, hist, nanflag, h);
    } else {
        const long cells = (long)d * R;
        for (long b = blockIdx.y; b <= n / PARTQ_LONG; b += gridDim.y) {
            const long c0 = b * PARTQ_LONG, c1 = c0 + PARTQ_LONG;
            for (int which = 0; which < 2; ++which) {
                long p = -1, s = 0, e = 0;
                if (which == 0) {
                    if (c0 < n) p = span_find(start, end, count, c0, s);
                } else {
                    p = slotmap[b];
                }
                if (p < 0) continue;
                span_bounds(start, end, p, n, s, e);
                if (e - s <= PARTQ_LONG || (which == 1 && s == c0)) continue;      // short; or met as the part that covers c0
                const long slot = s / PARTQ_LONG;
                const long lo = s > c0 ? s : c0, hi = e < c1 ? e : c1;
                colq_hist_rows<false>(a, d, ld, R, shift, lo + sub, hi, (long)CQ_ROWS, state + 2 * slot * cells, hist + slot * cells * 256,
                               nanflag + p * d, h);
                __syncthreads();
            }
        }
    }
}

// One wave on the 256 bins at `bins` that hold more than state[1] keys in all: the digit whose bin holds that rank is appended to the
// prefix state[0], the rank made relative to the bin.  Lane l brings the bins 4 l .. 4 l + 3.  True in the one lane that chose, with
// the new prefix in *key.
__device__ __forceinline__ bool colq_pick_digit(const uint4 b, unsigned prefix, unsigned k, int shift, unsigned* key, unsigned* rest) {
    const int lane = threadIdx.x & 63;
    const unsigned mine = b.x + b.y + b.z + b.w;
    const unsigned incl = wave_inclusive_sum(mine);
    unsigned below = incl - mine;
    if (!(below <= k && k < incl)) return false;
    unsigned digit = 4u * lane;
    if (k >= below + b.x) { below += b.x; ++digit;
        if (k >= below + b.y) { below += b.y; ++digit;
            if (k >= below + b.z) { below += b.z; ++digit; } } }
    *key = prefix | (digit << shift);
    *rest = k - below;
    return true;
}

// One wave per (column, rank): the digit whose bin holds the rank, appended to the prefix; the bins are cleared for the next pass.
// After the last digit the prefix is the key of the order statistic.  SEG: grid = (column x rank, slots); the cells of a slot that
// a long part owns, the order statistic written to that part's place; a free slot is skipped.
template <bool SEG>
__global__ void __launch_bounds__(64) k_eval_colq_pick(unsigned* __restrict__ state, unsigned* __restrict__ hist, int shift,
                                                        float* __restrict__ ord, long cells, long nslots, const int* __restrict__ slotmap) {
    const int lane = threadIdx.x;
    for (long b = SEG ? blockIdx.y : 0; b < (SEG ? nslots : 1); b += SEG ? gridDim.y : 1) {
        long idx = blockIdx.x, at = blockIdx.x;
        if constexpr (SEG) {
            const long p = slotmap[b];
            if (p < 0) continue;
            idx = b * cells + blockIdx.x;
            at = p * cells + blockIdx.x;
        }
        uint4* bins = reinterpret_cast<uint4*>(hist + idx * 256) + lane;
        const uint4 bv = *bins;
        *bins = make_uint4(0u, 0u, 0u, 0u);
        unsigned key, rest;
        if (colq_pick_digit(bv, state[2 * idx], state[2 * idx + 1], shift, &key, &rest)) {      // exactly one lane
            state[2 * idx] = key;
            state[2 * idx + 1] = rest;
            if (shift == 0) ord[at] = colq_value(key);
        }
    }
}

// ---- quantiles of the non-NaN entries (mtadgat_eval_column_quantiles_valid) ---------------------------------------------------------
// The select above with VALID keys and the ranks of every column taken from the column's own count m of non-NaN entries:
//   k_colqv_init    clears the bins and the counts (and writes inline probabilities to q);
//   k_colqv_count   m[col]: integer sums in LDS and memory, independent of their order;
//   k_colqv_ranks   lo = floor(q (m - 1)), hi = min(lo + 1, m - 1) per (column, probability); rank 0 for m = 0 (never interpolated);
//   k_colqv_interp  as k_eval_colq_interp with m in the place of n; NaN for m = 0; the counts as int64.
__global__ void k_colqv_init(double* __restrict__ q, ColqProbs pv, int inl, int nq, int d, unsigned* __restrict__ m,
                             unsigned* __restrict__ hist) {
    if (inl && blockIdx.x == 0 && threadIdx.x < nq) q[threadIdx.x] = pv.v[threadIdx.x];
    const long nhist = (long)d * 2 * nq * 256;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nhist; i += (long)gridDim.x * blockDim.x) {
        hist[i] = 0u;
        if (i < d) m[i] = 0u;
    }
}

// grid = (column tiles, row slices): thread (row group, column) walks its rows grid-stride
__global__ void __launch_bounds__(256) k_colqv_count(const float* __restrict__ a, long n, int d, long ld, unsigned* __restrict__ m) {
    __shared__ unsigned cnt[CQ_CT];
    const int tid = threadIdx.x, c = tid & (CQ_CT - 1);
    const int col = blockIdx.x * CQ_CT + c;
    if (tid < CQ_CT) cnt[tid] = 0u;
    __syncthreads();
    unsigned mine = 0u;
    if (col < d)
        for (long row = (long)blockIdx.y * CQ_ROWS + (tid >> 3); row < n; row += (long)gridDim.y * CQ_ROWS) {
            const float v = a[row * ld + col];
            mine += v == v ? 1u : 0u;
        }
    if (mine) atomicAdd(&cnt[c], mine);
    __syncthreads();
    if (tid < CQ_CT && col < d && cnt[tid]) atomicAdd(&m[col], cnt[tid]);
}

__global__ void k_colqv_ranks(const double* __restrict__ q, ColqProbs pv, int inl, int nq, int d, const unsigned* __restrict__ m,
                              unsigned* __restrict__ state) {
    const int R = 2 * nq;
    const long nstate = (long)d * R;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nstate; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i % R);
        const long mm = (long)m[i / R];
        unsigned rank = 0u;
        if (mm > 0) {
            const unsigned lo = colq_rank(inl ? pv.v[r >> 1] : q[r >> 1], mm, nullptr);
            const unsigned hi = (long)lo + 1 < mm ? lo + 1 : (unsigned)(mm - 1);
            rank = (r & 1) ? hi : lo;
        }
        state[2 * i] = 0u;
        state[2 * i + 1] = rank;
    }
}

__global__ void k_colqv_interp(const float* __restrict__ ord, const double* __restrict__ q, const unsigned* __restrict__ m, int d, int nq,
                               float* __restrict__ out, long* __restrict__ count) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)nq * d) return;
    const int qi = (int)(i / d), col = (int)(i % d);
    const long mm = (long)m[col];
    if (count && qi == 0) count[col] = mm;
    float r = __builtin_bit_cast(float, 0x7fc00000u);
    if (mm > 0) {
        double frac;
        colq_rank(q[qi], mm, &frac);
        const double lo = ord[((long)col * nq + qi) * 2], hi = ord[((long)col * nq + qi) * 2 + 1];
        r = (float)(lo + (hi - lo) * frac);
    }
    out[i] = r;
}

// ---- quantiles per part ----------------------------------------------------------------------------------------------------------
// ord[((part * d + col) * nq + qi) * 2] = { s[lo], s[hi] } of the part's slice of the column, nanflag[part * d + col] as for a column.
__global__ void k_partq_free(int* __restrict__ slotmap, long nslots) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (long)gridDim.x * blockDim.x) slotmap[i] = -1;
}

// The workgroup that meets a long part writes it into its slot, clears the slot's bins and the part's NaN flags and sets the ranks to
// find; the parts are walked grid-stride.
__global__ void __launch_bounds__(256) k_partq_slots(long n, int d, const long* __restrict__ start, const long* __restrict__ end, long count,
                                                      ColqProbs pv, int nq, int* __restrict__ slotmap, unsigned* __restrict__ state,
                                                      unsigned* __restrict__ hist, unsigned* __restrict__ nanflag) {
    const int tid = threadIdx.x, R = 2 * nq;
    const long cells = (long)d * R;
    for (long k = blockIdx.x; k < count; k += gridDim.x) {
        long s, e;
        span_bounds(start, end, k, n, s, e);
        const long len = e - s;
        if (len <= PARTQ_LONG) continue;
        const long slot = s / PARTQ_LONG;
        if (tid == 0) slotmap[slot] = (int)k;
        uint4* bins = reinterpret_cast<uint4*>(hist + slot * cells * 256);
        for (long i = tid; i < cells * 64; i += 256) bins[i] = make_uint4(0u, 0u, 0u, 0u);
        for (long i = tid; i < cells; i += 256) {
            const int r = (int)(i % R);
            const unsigned lo = colq_rank(pv.v[r >> 1], len, nullptr);
            const unsigned hi = (long)lo + 1 < len ? lo + 1 : (unsigned)(len - 1);
            state[2 * (slot * cells + i)] = 0u;
            state[2 * (slot * cells + i) + 1] = (r & 1) ? hi : lo;
        }
        for (int c = tid; c < d; c += 256) nanflag[k * d + c] = 0u;
    }
}

// grid = (part, column tile): the whole select of a part of 1 .. PARTQ_LONG rows for ct columns (a power of two <= CQ_CT, chosen from
// d: at d = 1 all 256 threads walk rows) and CQ_RT ranks at a time.  Four digit passes over the part's rows -- the first from memory,
// the rest from L2 -- with the bins in LDS; between them one wave per (column, rank) picks the digit.  A bin of column c sits at
// bin ^ 4 c of its histogram: the ct columns of a row that share a digit, as the leading digits of scores do, fall into ct
// different banks, and the four bins a lane picks from stay one 16-byte word.  Nothing of the histogram reaches memory.
__global__ void __launch_bounds__(256) k_partq_short(const float* __restrict__ a, long n, int d, long ld, const long* __restrict__ start,
                                                      const long* __restrict__ end, ColqProbs pv, int nq, int ct, float* __restrict__ ord,
                                                      unsigned* __restrict__ nanflag) {
    __shared__ __attribute__((aligned(16))) unsigned h[CQ_RT * CQ_CT * 256];
    __shared__ unsigned spfx[CQ_RT * CQ_CT], srank[CQ_RT * CQ_CT], snan[CQ_CT];
    const long k = blockIdx.x;
    long s, e;
    span_bounds(start, end, k, n, s, e);
    const long len = e - s;
    if (len < 1 || len > PARTQ_LONG) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = tid & (ct - 1), rsub = tid / ct, rp = 256 / ct;
    const int col0 = blockIdx.y * ct, col = col0 + c;
    const int R = 2 * nq;
    if (tid < CQ_CT) snan[tid] = 0u;
    for (int r0 = 0; r0 < R; r0 += CQ_RT) {
        const int nr = R - r0 < CQ_RT ? R - r0 : CQ_RT;
        for (int i = tid; i < nr * ct; i += 256) {
            const int r = r0 + i / ct;
            const unsigned lo = colq_rank(pv.v[r >> 1], len, nullptr);
            const unsigned hi = (long)lo + 1 < len ? lo + 1 : (unsigned)(len - 1);
            spfx[i] = 0u;
            srank[i] = (r & 1) ? hi : lo;
        }
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = tid; i < nr * ct * 256; i += 256) h[i] = 0u;
            __syncthreads();
            const unsigned high = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
            unsigned pfx[CQ_RT];
#pragma unroll
            for (int r = 0; r < CQ_RT; ++r) pfx[r] = r < nr ? spfx[r * ct + c] : 0u;
            if (col < d) {
                bool seen_nan = false;
                for (long row = rsub; row < len; row += rp) {
                    const float v = a[(s + row) * ld + col];
                    seen_nan = seen_nan || (v != v);
                    const unsigned key = colq_key(v);
                    const unsigned bin = ((key >> shift) & 255u) ^ (unsigned)(c << 2);
#pragma unroll
                    for (int r = 0; r < CQ_RT; ++r)
                        if (r < nr && ((key ^ pfx[r]) & high) == 0u) atomicAdd(&h[(r * ct + c) * 256 + bin], 1u);
                }
                if (seen_nan && shift == 24 && r0 == 0) atomicOr(&snan[c], 1u);
            }
            __syncthreads();
            for (int pair = wave; pair < nr * ct; pair += 4) {
                const uint4 bv = reinterpret_cast<const uint4*>(h + pair * 256)[lane ^ (pair & (ct - 1))];
                unsigned key, rest;
                if (colq_pick_digit(bv, spfx[pair], srank[pair], shift, &key, &rest)) {
                    spfx[pair] = key;
                    srank[pair] = rest;
                }
            }
            __syncthreads();
        }
        for (int i = tid; i < nr * ct; i += 256) {
            const int cc = col0 + (i & (ct - 1));
            if (cc < d) ord[(k * d + cc) * R + r0 + i / ct] = colq_value(spfx[i]);
        }
        __syncthreads();
    }
    if (tid < ct && col < d) nanflag[k * d + col] = snan[tid];
}

// out[qi][part][col], interpolated as for a column with the part's length; NaN for an empty part (whose ord was never written)
__global__ void k_partq_interp(const float* __restrict__ ord, ColqProbs pv, const unsigned* __restrict__ nanflag, long n, int d, int nq,
                               const long* __restrict__ start, const long* __restrict__ end, long count, float* __restrict__ out) {
    const long per_q = count * d, total = per_q * nq;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int qi = (int)(i / per_q);
        const long cell = i - qi * per_q;               // part * d + col
        long s, e;
        span_bounds(start, end, cell / d, n, s, e);
        float r = __builtin_nanf("");
        if (e > s && !nanflag[cell]) {
            double frac;
            colq_rank(pv.v[qi], e - s, &frac);
            const double lo = ord[(cell * nq + qi) * 2], hi = ord[(cell * nq + qi) * 2 + 1];
            r = (float)(lo + (hi - lo) * frac);
        }
        out[i] = r;
    }
}

// out[qi][col] = s[lo] + (s[hi] - s[lo]) (pos - lo) in float64, rounded once; NaN for a column that holds a NaN
__global__ void k_eval_colq_interp(const float* __restrict__ ord, const double* __restrict__ q, const unsigned* __restrict__ nanflag,
                                   long n, int d, int nq, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)nq * d) return;
    const int qi = (int)(i / d), col = (int)(i % d);
    double frac;
    colq_rank(q[qi], n, &frac);
    const double lo = ord[((long)col * nq + qi) * 2], hi = ord[((long)col * nq + qi) * 2 + 1];
    const double v = lo + (hi - lo) * frac;
    out[i] = nanflag[col] ? __builtin_nanf("") : (float)v;
}

// ---- exponentially weighted mean -------------------------------------------------------------------------------------------------
// One scan, instantiated three times.
// SEG: the mean restarts at the start of every span [start, end) (disjoint and ascending, mtadgat_scan.h; a score outside every span
// is a span of its own and gives NaN): the scan carries (sum, "a span started inside") pairs, so a part never sees its predecessor's
// sum -- nothing is subtracted.  !SEG: one span [0, n) -- no span arrays are read, every flag is a compile-time false and F is never
// touched; the arithmetic, and so the bits, are those of SEG with that one span.
// VALID: the mean over observed rows, a NaN input being an unobserved row.  The scan carries (N, D), N_t = (obs ? x_t : 0) + b N_{t-1},
// D_t = (obs ? 1 : 0) + b D_{t-1}; the result is N_t / D_t at an observed row (D_t >= 1 there) and the canonical NaN elsewhere.
// !VALID: the scan carries N alone and D_t is the closed form (1 - b^(t - s + 1)) / alpha; nothing of D is read, shuffled or stored.
// Either way N goes through the same float64 operations in the same order, and D, where it is carried, through N's.
// <false, false> is mtadgat_eval_ewm, <true, false> mtadgat_eval_ewm_parts, <false, true> mtadgat_eval_ewm_valid.  <true, true> has no
// caller and is not instantiated: a span start resets N and D alike and a row outside every span stores NaN, so it takes one more
// instantiation of launch_ewm and an entry point, nothing here.
constexpr int EWM_L = 1024;      // elements per chunk: 256 threads x 4

struct EwmSum {
    double n, d;                 // d: VALID only
};

// the terms of one sample: x, and with VALID (x, 1) at an observed row and (0, 0) at a NaN
template <bool VALID>
__device__ __forceinline__ void ewm_terms(float f, double& v, double& o) {
    if constexpr (VALID) {
        const bool obs = f == f;
        v = obs ? (double)f : 0.0;
        o = obs ? 1.0 : 0.0;
    } else {
        v = (double)f;
    }
}

// this thread's four elements: the terms of N and D, whether a span starts there and the start of its span (-1: outside every span);
// an index beyond n is an unobserved row
template <bool SEG, bool VALID>
__device__ __forceinline__ void ewm_load(const float* __restrict__ x, long n, long base, const long* __restrict__ start,
                                         const long* __restrict__ end, long count, double (&v)[4], double (&o)[4], bool (&rs)[4],
                                         long (&st)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = base + j;
        v[j] = 0.0; o[j] = 0.0; rs[j] = false; st[j] = 0;
        if constexpr (!SEG) {
            ewm_terms<VALID>(i < n ? x[i] : (VALID ? __builtin_nanf("") : 0.f), v[j], o[j]);
        } else if (i < n) {
            ewm_terms<VALID>(x[i], v[j], o[j]);
            long s = 0;
            const long p = span_find(start, end, count, i, s);
            rs[j] = p < 0 || i == s;
            st[j] = p < 0 ? -1 : s;
        }
    }
}

// (N, D) just before this thread's four elements for N_t = x_t + b N_{t-1}, N = 0 before a span start, started from `carry` before
// the chunk.  Wave scan by shuffles (factor b^(4 off) at distance off) on (sums, flag) -- a piece in which a span starts ignores
// what precedes it -- then the four wave totals composed in order.  *any: a span starts somewhere in the chunk.
// sm: 4 doubles, 8 with VALID (N and D of a wave side by side); smf: 4 ints (SEG only).
template <bool SEG, bool VALID>
__device__ __forceinline__ EwmSum ewm_prefix(const double (&x)[4], const double (&o)[4], const bool (&rs)[4], double b, EwmSum carry,
                                             double* sm, int* smf, bool* any) {
    constexpr int NC = VALID ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = x[0], d = o[0];
    int fl = SEG && rs[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        s = (SEG && rs[j] ? 0.0 : s) * b + x[j];
        if constexpr (VALID) d = (SEG && rs[j] ? 0.0 : d) * b + o[j];
        fl |= SEG && rs[j];
    }
    double f = (b * b) * (b * b);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(s, off);
        const double td = VALID ? __shfl_up(d, off) : 0.0;
        const int tf = SEG ? __shfl_up(fl, off) : 0;
        if (lane >= off) {
            if (!fl) s = t * f + s;
            if constexpr (VALID)
                if (!fl) d = td * f + d;
            fl |= tf;
        }
        f *= f;
    }                                                   // f = b^256
    if (lane == 63) {
        sm[NC * wave] = s;
        if constexpr (VALID) sm[NC * wave + 1] = d;
        if constexpr (SEG) smf[wave] = fl;
    }
    double ex = __shfl_up(s, 1);
    double exd = VALID ? __shfl_up(d, 1) : 0.0;
    int exf = SEG ? __shfl_up(fl, 1) : 0;
    if (lane == 0) { ex = 0.0; exd = 0.0; exf = 0; }
    __syncthreads();
    EwmSum in = carry;
    for (int w = 0; w < wave; ++w) {
        in.n = (SEG && smf[w] ? 0.0 : in.n) * f + sm[NC * w];
        if constexpr (VALID) in.d = (SEG && smf[w] ? 0.0 : in.d) * f + sm[NC * w + 1];
    }
    *any = SEG && (smf[0] | smf[1] | smf[2] | smf[3]) != 0;
    EwmSum r;
    r.n = ex + (exf ? 0.0 : in.n) * pow(b, (double)(4 * lane));
    r.d = VALID ? exd + (exf ? 0.0 : in.d) * pow(b, (double)(4 * lane)) : 0.0;
    return r;
}

// S[c] = N at the end of chunk c when nothing precedes it -- with VALID S[2 c], S[2 c + 1] = (N, D) --, F[c] = a span starts inside
// chunk c (SEG only)
template <bool SEG, bool VALID>
__global__ void __launch_bounds__(256) k_ewm_chunk(const float* __restrict__ x, long n, const long* __restrict__ start,
                                                    const long* __restrict__ end, long count, double b, double* __restrict__ S,
                                                    int* __restrict__ F) {
    constexpr int NC = VALID ? 2 : 1;
    __shared__ double sm[4 * NC];
    __shared__ int smf[4];
    double v[4], o[4];
    bool rs[4], any;
    long st[4];
    ewm_load<SEG, VALID>(x, n, (long)blockIdx.x * EWM_L + 4 * threadIdx.x, start, end, count, v, o, rs, st);
    EwmSum s = ewm_prefix<SEG, VALID>(v, o, rs, b, EwmSum{0.0, 0.0}, sm, smf, &any);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.n = (rs[j] ? 0.0 : s.n) * b + v[j];
        if constexpr (VALID) s.d = (rs[j] ? 0.0 : s.d) * b + o[j];
    }
    if (threadIdx.x == 255) {
        S[NC * blockIdx.x] = s.n;
        if constexpr (VALID) S[NC * blockIdx.x + 1] = s.d;
        if constexpr (SEG) F[blockIdx.x] = any ? 1 : 0;
    }
}

// carry[c] = N (with VALID (N, D), laid out as S) just before chunk c: carry[c] = (F[c-1] ? 0 : carry[c-1] b^L) + S[c-1], 64 chunks
// per step of one wave, in chunk order
template <bool SEG, bool VALID>
__global__ void __launch_bounds__(64) k_ewm_carry(const double* __restrict__ S, const int* __restrict__ F, long nchunks, double fL,
                                                   double* __restrict__ carry) {
    constexpr int NC = VALID ? 2 : 1;
    const int lane = threadIdx.x;
    const double fl = pow(fL, (double)lane);
    double run = 0.0, rund = 0.0;
    for (long base = 0; base < nchunks; base += 64) {
        const long i = base + lane;
        double s = i < nchunks ? S[NC * i] : 0.0;
        double d = VALID && i < nchunks ? S[NC * i + 1] : 0.0;
        int g = SEG && i < nchunks ? F[i] : 0;
        double f = fL;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double t = __shfl_up(s, off);
            const double td = VALID ? __shfl_up(d, off) : 0.0;
            const int tg = SEG ? __shfl_up(g, off) : 0;
            if (lane >= off) {
                if (!g) s = t * f + s;
                if constexpr (VALID)
                    if (!g) d = td * f + d;
                g |= tg;
            }
            f *= f;
        }                                               // f = fL^64
        double ex = __shfl_up(s, 1);
        double exd = VALID ? __shfl_up(d, 1) : 0.0;
        int exg = SEG ? __shfl_up(g, 1) : 0;
        if (lane == 0) { ex = 0.0; exd = 0.0; exg = 0; }
        if (i < nchunks) {
            carry[NC * i] = (exg ? 0.0 : run) * fl + ex;
            if constexpr (VALID) carry[NC * i + 1] = (exg ? 0.0 : rund) * fl + exd;
        }
        const bool reset = SEG && __shfl(g, 63);
        run = (reset ? 0.0 : run) * f + __shfl(s, 63);
        if constexpr (VALID) rund = (reset ? 0.0 : rund) * f + __shfl(d, 63);
    }
}

// y[t] = N_t / D_t, NaN outside every span.  !VALID: D_t = (1 - b^(t - s + 1)) / alpha with s the start of t's span.  VALID: the
// scanned D_t, and the canonical NaN at an unobserved row.  y may be x: a thread reads its four elements before it writes them, and
// no other thread touches them.
template <bool SEG, bool VALID>
__global__ void __launch_bounds__(256) k_ewm_apply(const float* x, long n, const long* __restrict__ start, const long* __restrict__ end,
                                                    long count, double b, double alpha, const double* __restrict__ carry, float* y) {
    constexpr int NC = VALID ? 2 : 1;
    __shared__ double sm[4 * NC];
    __shared__ int smf[4];
    double v[4], o[4];
    bool rs[4], any;
    long st[4];
    const long base = (long)blockIdx.x * EWM_L + 4 * threadIdx.x;
    ewm_load<SEG, VALID>(x, n, base, start, end, count, v, o, rs, st);
    EwmSum c;
    c.n = carry[NC * blockIdx.x];
    c.d = VALID ? carry[NC * blockIdx.x + 1] : 0.0;
    EwmSum s = ewm_prefix<SEG, VALID>(v, o, rs, b, c, sm, smf, &any);
    const float none = __builtin_bit_cast(float, 0x7fc00000u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.n = (rs[j] ? 0.0 : s.n) * b + v[j];
        if constexpr (VALID) s.d = (rs[j] ? 0.0 : s.d) * b + o[j];
        if (base + j < n) {
            if constexpr (VALID)
                y[base + j] = st[j] >= 0 && o[j] != 0.0 ? (float)(s.n / s.d) : none;
            else
                y[base + j] = st[j] < 0 ? none : (float)(s.n / ((1.0 - pow(b, (double)(base + j - st[j] + 1))) / alpha));
        }
    }
}

}  // namespace mtadgat

using namespace mtadgat;

namespace {

struct ColqScratch {
    double* q;
    unsigned *hist, *state, *nanflag;
    float* ord;
};
ColqScratch colq_scratch(ScratchCarver& c, int64_t d, int64_t nq) {
    const size_t cells = (size_t)d * 2 * (size_t)nq;
    ColqScratch l;
    l.q = c.take<double>(nq);
    l.hist = c.take<unsigned>(cells * 256, 16);         // the pick kernel reads the bins as 16-byte words
    l.state = c.take<unsigned>(cells * 2, 4);           // 4-byte regions back to back
    l.nanflag = c.take<unsigned>(d, 4);
    l.ord = c.take<float>(cells, 4);
    return l;
}

// the four digit passes of the select for R ranks per column, on an initialised state
template <bool VALID>
void colq_passes(const float* a_dev, long n, int d, long ld, int R, unsigned* state, unsigned* hist, unsigned* nanflag, float* ord,
                 hipStream_t s) {
    // bounded grid: about 1024 workgroups in all, each walking at least four row groups
    const long cells = (long)d * R;
    const int tiles = (d + CQ_CT - 1) / CQ_CT, groups = (R + CQ_RT - 1) / CQ_RT;
    long slices = (n + 4 * CQ_ROWS - 1) / (4 * CQ_ROWS);
    const long cap = 1024 / ((long)tiles * groups) > 0 ? 1024 / ((long)tiles * groups) : 1;
    if (slices > cap) slices = cap;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL((k_eval_colq_hist<false, VALID>), dim3(tiles, (unsigned)slices, groups), dim3(256), 0, s, a_dev, (long)n, d, (long)ld, R, shift,
                           (const unsigned*)state, hist, nanflag, (const long*)nullptr, (const long*)nullptr, 0L, (const int*)nullptr);
        hipLaunchKernelGGL(k_eval_colq_pick<false>, dim3((unsigned)cells), dim3(64), 0, s, state, hist, shift, ord, cells, 1L, (const int*)nullptr);
    }
}

// per part: the order statistics and the NaN flags; per slot of the long route: the owner, the select's state and the bins
struct PartqScratch {
    unsigned *hist, *state, *nanflag;
    float* ord;
    int* slotmap;
    long nslots;
};
PartqScratch partq_scratch(ScratchCarver& c, int64_t n, int64_t d, int64_t count, int64_t nq) {
    const size_t cells = (size_t)d * 2 * (size_t)nq;
    PartqScratch l;
    l.nslots = n > PARTQ_LONG ? (long)(n / PARTQ_LONG + 1) : 0;     // no part of n <= PARTQ_LONG rows is long
    l.hist = c.take<unsigned>((size_t)l.nslots * cells * 256, 16);
    l.state = c.take<unsigned>((size_t)l.nslots * cells * 2, 4);
    l.slotmap = c.take<int>((size_t)l.nslots, 4);
    l.nanflag = c.take<unsigned>((size_t)count * (size_t)d, 4);
    l.ord = c.take<float>((size_t)count * cells, 4);
    return l;
}

constexpr int64_t N_MAX = 2147483647LL;

// S and carry: per chunk one element each, its components side by side (mtadgat_eval_ewm: 16 bytes per chunk, mtadgat_eval_ewm_valid:
// 32); the segmented scan adds one int per chunk
struct EwmScratch {
    double *S, *carry;
    int* F;
    long nchunks;
};
EwmScratch ewm_scratch(ScratchCarver& c, int64_t n, bool seg, bool valid) {
    EwmScratch l;
    l.nchunks = (long)((n + EWM_L - 1) / EWM_L);
    const size_t doubles = (size_t)l.nchunks * (valid ? 2 : 1);
    l.S = c.take<double>(doubles);
    l.carry = c.take<double>(doubles);
    l.F = seg ? c.take<int>(l.nchunks) : nullptr;
    return l;
}

// chunk-local scans, one wave that composes the chunk carries, the pass that applies carry and denominator; false: a launch failed
template <bool SEG, bool VALID>
bool launch_ewm(const float* x, int64_t n, const long* st, const long* en, long count, double alpha, const EwmScratch& l, float* out,
                hipStream_t s) {
    const double b = 1.0 - alpha;
    hipLaunchKernelGGL((k_ewm_chunk<SEG, VALID>), dim3((unsigned)l.nchunks), dim3(256), 0, s, x, (long)n, st, en, count, b, l.S, l.F);
    hipLaunchKernelGGL((k_ewm_carry<SEG, VALID>), dim3(1), dim3(64), 0, s, (const double*)l.S, (const int*)l.F, l.nchunks,
                       pow(b, (double)EWM_L), l.carry);
    hipLaunchKernelGGL((k_ewm_apply<SEG, VALID>), dim3((unsigned)l.nchunks), dim3(256), 0, s, x, (long)n, st, en, count, b, alpha,
                       (const double*)l.carry, out);
    return hipGetLastError() == hipSuccess;
}

// The checks, the carving and the launches of the three entry points, which differ in `who` (the prefix of the error texts and the
// name of the scratch query) and in the spans: SEG takes start, end and count, the others pass none.
int ewm_fail(int code, const char* who, const std::string& what) { return record_error(code, (std::string(who) + ": " + what).c_str()); }

template <bool SEG, bool VALID>
int run_ewm(const char* who, const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count, double alpha,
            void* scratch_dev, size_t scratch_bytes, float* out_dev, void* stream) {
    if (!x_dev || (SEG && (!start_dev || !end_dev)) || !scratch_dev || !out_dev) return ewm_fail(-1, who, "null pointer");
    if (n < 1 || n > N_MAX) return ewm_fail(-1, who, "n must lie in [1, 2^31 - 1]");
    if (SEG && (count < 1 || count > N_MAX)) return ewm_fail(-1, who, "count must lie in [1, 2^31 - 1]");
    if (!(alpha > 0.0 && alpha <= 1.0)) return ewm_fail(-1, who, "alpha outside (0, 1]");
    ScratchCarver carver(scratch_dev);
    const EwmScratch l = ewm_scratch(carver, n, SEG, VALID);
    if (scratch_bytes < carver.bytes()) return ewm_fail(-5, who, std::string("scratch too small (see mtadgat_eval_") + who + "_scratch)");
    if ((uintptr_t)scratch_dev & 7) return ewm_fail(-5, who, "scratch must be 8-byte aligned");
    const long *st = reinterpret_cast<const long*>(start_dev), *en = reinterpret_cast<const long*>(end_dev);
    if (!launch_ewm<SEG, VALID>(x_dev, n, st, en, (long)count, alpha, l, out_dev, (hipStream_t)stream))
        return ewm_fail(-3, who, "kernel launch failed");
    return 0;
}

}  // namespace

namespace mtadgat {

size_t column_rank_scratch(int d) { return scratch_bytes_of([&](ScratchCarver& c) { colq_scratch(c, d, 1); }); }

int launch_column_rank(const float* a_dev, long n, int d, long ld, long rank, void* scratch_dev, const float** ord_dev, hipStream_t s) {
    ScratchCarver carver(scratch_dev);
    const ColqScratch l = colq_scratch(carver, d, 1);
    const long init_blocks = ((long)d * 256 + 255) / 256;
    hipLaunchKernelGGL(k_eval_colq_init_rank, dim3((unsigned)(init_blocks < 2048 ? init_blocks : 2048)), dim3(256), 0, s, (unsigned)rank, d, l.state,
                       l.nanflag, l.hist);
    colq_passes<false>(a_dev, n, d, ld, 1, l.state, l.hist, l.nanflag, l.ord, s);
    *ord_dev = l.ord;
    return (int)hipGetLastError();
}

}  // namespace mtadgat

extern "C" {

size_t mtadgat_eval_column_quantiles_scratch(int64_t n, int d, int nq) {
    if (n < 1 || d < 1 || nq < 1) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { colq_scratch(c, d, nq); });
}

int mtadgat_eval_column_quantiles(const float* a_dev, int64_t n, int d, int64_t ld, const double* q_host, int nq, void* scratch_dev,
                                  size_t scratch_bytes, float* out_dev, void* stream) {
    if (!a_dev || !q_host || !scratch_dev || !out_dev) return record_error(-1, "column_quantiles: null pointer");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "column_quantiles: n must lie in [1, 2^31 - 1]");
    if (d < 1 || d > 2048) return record_error(-1, "column_quantiles: d must lie in [1, 2048]");
    if (ld < d) return record_error(-1, "column_quantiles: ld < d");
    if (nq < 1 || nq > 4096) return record_error(-1, "column_quantiles: nq must lie in [1, 4096]");
    for (int i = 0; i < nq; ++i)
        if (!(q_host[i] >= 0.0 && q_host[i] <= 1.0)) return record_error(-1, "column_quantiles: q outside [0, 1]");
    ScratchCarver carver(scratch_dev);
    const ColqScratch l = colq_scratch(carver, d, nq);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "column_quantiles: scratch too small (see mtadgat_eval_column_quantiles_scratch)");
    if ((uintptr_t)scratch_dev & 15) return record_error(-5, "column_quantiles: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = 2 * nq;
    const long cells = (long)d * R;
    // q_host is not touched after this call returns: few probabilities ride in the kernel arguments, more are copied and waited for
    ColqProbs pv = {};
    const int inl = nq <= CQ_INLINE;
    if (inl) {
        for (int i = 0; i < nq; ++i) pv.v[i] = q_host[i];
    } else if (hipMemcpyAsync(l.q, q_host, nq * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        return record_error(-3, "column_quantiles: copy of q failed");
    }
    const long init_blocks = (cells * 256 + 255) / 256;
    hipLaunchKernelGGL(k_eval_colq_init, dim3((unsigned)(init_blocks < 2048 ? init_blocks : 2048)), dim3(256), 0, s, l.q, pv, inl, nq, (long)n, d,
                       l.state, l.nanflag, l.hist);
    colq_passes<false>(a_dev, (long)n, d, (long)ld, R, l.state, l.hist, l.nanflag, l.ord, s);
    const long outs = (long)nq * d;
    hipLaunchKernelGGL(k_eval_colq_interp, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, (const float*)l.ord, (const double*)l.q,
                       (const unsigned*)l.nanflag, (long)n, d, nq, out_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "column_quantiles: kernel launch failed");
}

size_t mtadgat_eval_column_quantiles_valid_scratch(int64_t n, int d, int nq) { return mtadgat_eval_column_quantiles_scratch(n, d, nq); }

// the layout of mtadgat_eval_column_quantiles; its NaN flags hold the columns' valid counts
int mtadgat_eval_column_quantiles_valid(const float* a_dev, int64_t n, int d, int64_t ld, const double* q_host, int nq, void* scratch_dev,
                                        size_t scratch_bytes, float* out_dev, int64_t* count_dev, void* stream) {
    if (!a_dev || !q_host || !scratch_dev || !out_dev) return record_error(-1, "column_quantiles_valid: null pointer");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "column_quantiles_valid: n must lie in [1, 2^31 - 1]");
    if (d < 1 || d > 2048) return record_error(-1, "column_quantiles_valid: d must lie in [1, 2048]");
    if (ld < d) return record_error(-1, "column_quantiles_valid: ld < d");
    if (nq < 1 || nq > 4096) return record_error(-1, "column_quantiles_valid: nq must lie in [1, 4096]");
    for (int i = 0; i < nq; ++i)
        if (!(q_host[i] >= 0.0 && q_host[i] <= 1.0)) return record_error(-1, "column_quantiles_valid: q outside [0, 1]");
    ScratchCarver carver(scratch_dev);
    const ColqScratch l = colq_scratch(carver, d, nq);
    if (scratch_bytes < carver.bytes())
        return record_error(-5, "column_quantiles_valid: scratch too small (see mtadgat_eval_column_quantiles_valid_scratch)");
    if ((uintptr_t)scratch_dev & 15) return record_error(-5, "column_quantiles_valid: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int R = 2 * nq;
    const long cells = (long)d * R;
    ColqProbs pv = {};
    const int inl = nq <= CQ_INLINE;
    if (inl) {
        for (int i = 0; i < nq; ++i) pv.v[i] = q_host[i];
    } else if (hipMemcpyAsync(l.q, q_host, nq * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        return record_error(-3, "column_quantiles_valid: copy of q failed");
    }
    unsigned* m = l.nanflag;
    const long init_blocks = (cells * 256 + 255) / 256;
    hipLaunchKernelGGL(k_colqv_init, dim3((unsigned)(init_blocks < 2048 ? init_blocks : 2048)), dim3(256), 0, s, l.q, pv, inl, nq, d, m, l.hist);
    const int tiles = (d + CQ_CT - 1) / CQ_CT;
    long slices = (n + 4 * CQ_ROWS - 1) / (4 * CQ_ROWS);
    const long cap = 1024 / tiles > 0 ? 1024 / tiles : 1;
    if (slices > cap) slices = cap;
    hipLaunchKernelGGL(k_colqv_count, dim3(tiles, (unsigned)slices), dim3(256), 0, s, a_dev, (long)n, d, (long)ld, m);
    const long rank_blocks = (cells + 255) / 256;
    hipLaunchKernelGGL(k_colqv_ranks, dim3((unsigned)(rank_blocks < 2048 ? rank_blocks : 2048)), dim3(256), 0, s, (const double*)l.q, pv, inl, nq,
                       d, (const unsigned*)m, l.state);
    colq_passes<true>(a_dev, (long)n, d, (long)ld, R, l.state, l.hist, (unsigned*)nullptr, l.ord, s);
    const long outs = (long)nq * d;
    hipLaunchKernelGGL(k_colqv_interp, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, (const float*)l.ord, (const double*)l.q,
                       (const unsigned*)m, d, nq, out_dev, reinterpret_cast<long*>(count_dev));
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "column_quantiles_valid: kernel launch failed");
}

int mtadgat_eval_partq_long(void) { return PARTQ_LONG; }

size_t mtadgat_eval_part_quantiles_scratch(int64_t n, int d, int64_t count, int nq) {
    if (n < 1 || n > N_MAX || count < 1 || count > N_MAX || d < 1 || d > 2048 || nq < 1 || nq > CQ_INLINE) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { partq_scratch(c, n, d, count, nq); });
}

int mtadgat_eval_part_quantiles(const float* a_dev, int64_t n, int d, int64_t ld, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                                const double* q_host, int nq, void* scratch_dev, size_t scratch_bytes, float* out_dev, void* stream) {
    if (!a_dev || !start_dev || !end_dev || !q_host || !scratch_dev || !out_dev) return record_error(-1, "part_quantiles: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "part_quantiles: n must lie in [1, 2^31 - 1]");
    if (count < 1 || count > N_MAX) return record_error(-1, "part_quantiles: count must lie in [1, 2^31 - 1]");
    if (d < 1 || d > 2048) return record_error(-1, "part_quantiles: d must lie in [1, 2048]");
    if (ld < d) return record_error(-1, "part_quantiles: ld < d");
    if (nq < 1 || nq > CQ_INLINE) return record_error(-1, "part_quantiles: nq must lie in [1, 8]");
    ColqProbs pv = {};
    for (int i = 0; i < nq; ++i) {
        if (!(q_host[i] >= 0.0 && q_host[i] <= 1.0)) return record_error(-1, "part_quantiles: q outside [0, 1]");
        pv.v[i] = q_host[i];
    }
    ScratchCarver carver(scratch_dev);
    const PartqScratch l = partq_scratch(carver, n, d, count, nq);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "part_quantiles: scratch too small (see mtadgat_eval_part_quantiles_scratch)");
    if ((uintptr_t)scratch_dev & 15) return record_error(-5, "part_quantiles: scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long *st = reinterpret_cast<const long*>(start_dev), *en = reinterpret_cast<const long*>(end_dev);
    const int R = 2 * nq;
    const long cells = (long)d * R;
    int ct = 1;
    while (ct < d && ct < CQ_CT) ct <<= 1;
    hipLaunchKernelGGL(k_partq_short, dim3((unsigned)count, (unsigned)((d + ct - 1) / ct)), dim3(256), 0, s, a_dev, (long)n, d, (long)ld, st, en, pv,
                       nq, ct, l.ord, l.nanflag);
    if (l.nslots > 0) {
        const unsigned ys = (unsigned)(l.nslots < 65535 ? l.nslots : 65535);
        const int tiles = (d + CQ_CT - 1) / CQ_CT, groups = (R + CQ_RT - 1) / CQ_RT;
        hipLaunchKernelGGL(k_partq_free, dim3((unsigned)((l.nslots + 255) / 256)), dim3(256), 0, s, l.slotmap, l.nslots);
        hipLaunchKernelGGL(k_partq_slots, dim3((unsigned)(count < 4096 ? count : 4096)), dim3(256), 0, s, (long)n, d, st, en, (long)count, pv, nq,
                           l.slotmap, l.state, l.hist, l.nanflag);
        for (int shift = 24; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(k_eval_colq_hist<true>, dim3(tiles, ys, groups), dim3(256), 0, s, a_dev, (long)n, d, (long)ld, R, shift,
                               (const unsigned*)l.state, l.hist, l.nanflag, st, en, (long)count, (const int*)l.slotmap);
            hipLaunchKernelGGL(k_eval_colq_pick<true>, dim3((unsigned)cells, ys), dim3(64), 0, s, l.state, l.hist, shift, l.ord, cells, l.nslots,
                               (const int*)l.slotmap);
        }
    }
    const long outs = (long)nq * count * d;
    const long blocks = (outs + 255) / 256;
    hipLaunchKernelGGL(k_partq_interp, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, (const float*)l.ord, pv,
                       (const unsigned*)l.nanflag, (long)n, d, nq, st, en, (long)count, out_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "part_quantiles: kernel launch failed");
}

size_t mtadgat_eval_ewm_scratch(int64_t n) {
    if (n < 1) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { ewm_scratch(c, n, false, false); });
}

int mtadgat_eval_ewm(const float* x_dev, int64_t n, double alpha, void* scratch_dev, size_t scratch_bytes, float* out_dev, void* stream) {
    return run_ewm<false, false>("ewm", x_dev, n, nullptr, nullptr, 0, alpha, scratch_dev, scratch_bytes, out_dev, stream);
}

size_t mtadgat_eval_ewm_parts_scratch(int64_t n) {
    if (n < 1 || n > N_MAX) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { ewm_scratch(c, n, true, false); });
}

int mtadgat_eval_ewm_parts(const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count, double alpha,
                           void* scratch_dev, size_t scratch_bytes, float* out_dev, void* stream) {
    return run_ewm<true, false>("ewm_parts", x_dev, n, start_dev, end_dev, count, alpha, scratch_dev, scratch_bytes, out_dev, stream);
}

size_t mtadgat_eval_ewm_valid_scratch(int64_t n) {
    if (n < 1 || n > N_MAX) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { ewm_scratch(c, n, false, true); });
}

int mtadgat_eval_ewm_valid(const float* x_dev, int64_t n, double alpha, void* scratch_dev, size_t scratch_bytes, float* out_dev, void* stream) {
    return run_ewm<false, true>("ewm_valid", x_dev, n, nullptr, nullptr, 0, alpha, scratch_dev, scratch_bytes, out_dev, stream);
}

}  // extern "C"
