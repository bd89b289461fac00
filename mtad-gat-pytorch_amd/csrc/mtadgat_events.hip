// From thresholded anomaly scores to ranked events, on the device with the scores (evaluation.anomaly_events):
//
//   k_eval_runs_*: the maximal runs of flagged samples as ordered [start, end) pairs, near-by runs merged, short events dropped.
//       Three stream compactions of the same shape -- samples -> raw runs, raw runs -> merged runs (a run opens an event when the
//       gap before it is wider than merge_gap and closes one when the gap after it is), merged runs -> events of at least
//       min_length -- each the blocked scan of counts of mtadgat_scan.h over the "opens" predicate.  The k-th "closes" item pairs
//       with the k-th "opens" item, so that one scan ranks both.  No atomics, nothing sorted: the output order is the input order.
//   k_eval_run_part / _final: per-run peak, mean, per-column means, hit counts and the top columns.  Rows are cut into blocks of
//       SPAN_RB rows per run; a workgroup reduces a block with lanes on columns (coalesced rows) in a fixed tree and stores the
//       partial in the block's own slot; one wave per run then adds the slots in block order, so the bits depend on the data and
//       on SPAN_RB only, not on the grid.  The top columns are top_k rounds of a wave-wide arg-max over an ordered integer key.
//   k_eval_first_hit: the first flagged sample of every run, one wave per run, 64 samples per step, ballot + count-trailing-zeros.
#include "../../include/mtadgat.h"      // the entry points' declarations
#include "mtadgat_scan.h"

namespace mtadgat {

constexpr long NO_INDEX = 0x7fffffffffffffffL;

// flag_i = score_i > threshold (float64, or float32 with cmp_f32: k_eval_adjust's convention; NaN and equality are not flagged),
// or label_i != 0 when `label` is given
struct FlagSrc {
    const float* score;
    const unsigned char* label;
    double t64;
    float t32;
    int cmp_f32;
};
__device__ __forceinline__ bool flag_at(const FlagSrc& f, long i) {
    if (f.label) return f.label[i] != 0;
    const float s = f.score[i];
    return f.cmp_f32 ? (s > f.t32) : ((double)s > f.t64);
}

// ---- the three compactions: which items open / close an output run, and where rank r of either goes -----------------------------
struct RawRuns {                 // items: the n samples
    FlagSrc f;
    int* s;
    int* e;
    __device__ bool opens(long i, long) const { return flag_at(f, i) && (i == 0 || !flag_at(f, i - 1)); }
    __device__ bool closes(long i, long n) const { return flag_at(f, i) && (i + 1 == n || !flag_at(f, i + 1)); }
    __device__ void put_open(long r, long i) const { s[r] = (int)i; }
    __device__ void put_close(long r, long i) const { e[r] = (int)(i + 1); }
};
struct MergeRuns {               // items: the raw runs
    const int* s;
    const int* e;
    long gap;
    int* ms;
    int* me;
    __device__ bool opens(long k, long) const { return k == 0 || (long)s[k] - (long)e[k - 1] > gap; }
    __device__ bool closes(long k, long n) const { return k + 1 == n || (long)s[k + 1] - (long)e[k] > gap; }
    __device__ void put_open(long r, long k) const { ms[r] = s[k]; }
    __device__ void put_close(long r, long k) const { me[r] = e[k]; }
};
struct KeepRuns {                // items: the merged runs; ranks past the caller's capacity are counted, not written
    const int* s;
    const int* e;
    long min_length;
    long cap;
    long* out_s;
    long* out_e;
    __device__ bool opens(long k, long) const { return (long)e[k] - (long)s[k] >= min_length; }
    __device__ bool closes(long k, long n) const { return opens(k, n); }
    __device__ void put_open(long r, long k) const { if (r < cap) out_s[r] = s[k]; }
    __device__ void put_close(long r, long k) const { if (r < cap) out_e[r] = e[k]; }
};

// the item count of a stage: known on the host for the samples, left on the device by the previous stage's carry kernel for the runs
__device__ __forceinline__ long item_count(const long* n_dev, long n_host) { return n_dev ? *n_dev : n_host; }

// T[c] = number of opening items in chunk c
template <class Op>
__global__ void __launch_bounds__(256) k_eval_runs_count(Op op, const long* __restrict__ n_dev, long n_host, unsigned* __restrict__ T) {
    __shared__ unsigned sm[4];
    const long n = item_count(n_dev, n_host);
    const long base = (long)blockIdx.x * CHUNK_L;
    if (base >= n) return;
    const ChunkRank open = chunk_rank(base, [&](long i) { return i < n && op.opens(i, n); }, sm);
    if (threadIdx.x == 0) T[blockIdx.x] = open.total;
}

// every opening item to rank (openings before it), every closing item to rank (openings up to and including it) - 1
template <class Op>
__global__ void __launch_bounds__(256) k_eval_runs_emit(Op op, const long* __restrict__ n_dev, long n_host, const unsigned* __restrict__ C) {
    __shared__ unsigned sm[4];
    const long n = item_count(n_dev, n_host);
    const long base = (long)blockIdx.x * CHUNK_L;
    if (base >= n) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long i = base + wave * 256 + r * 64 + lane;
        q[r] = i < n && op.closes(i, n);
    }
    const ChunkRank open = chunk_rank(base, [&](long i) { return i < n && op.opens(i, n); }, sm);
    const long rank0 = C[blockIdx.x];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long i = base + wave * 256 + r * 64 + lane;
        const bool p = open.set[r];
        const long ex = rank0 + rank_before(open, r);
        if (p) op.put_open(ex, i);
        if (q[r]) op.put_close(ex + (p ? 1 : 0) - 1, i);           // a closing item lies in a run that opened at or before it
    }
}

// ---- per-run statistics ----------------------------------------------------------------------------------------------------------
// (value, index) of the larger value, the smaller index among equals
__device__ __forceinline__ void peak_merge(float& best, long& arg, float v, long i) {
    if (v > best || (v == best && i < arg)) { best = v; arg = i; }
}

// grid (run, slice): the slices of a run share out its row blocks; ct = columns per pass (a power of two <= 64), 256 / ct rows at a time
__global__ void __launch_bounds__(256) k_eval_run_part(const float* __restrict__ score, long n, const long* __restrict__ start,
                                                        const long* __restrict__ end, const float* __restrict__ per_dim, int d, long ld,
                                                        const double* __restrict__ thr, int ct, double* __restrict__ ssum,
                                                        float* __restrict__ smax, long* __restrict__ sarg, double* __restrict__ psum,
                                                        int* __restrict__ phit) {
    __shared__ double smd[256];
    __shared__ long sml[256];
    __shared__ float smf[256];
    __shared__ int smi[256];
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
        double sum = 0.0;
        float best = -INFINITY;
        long arg = NO_INDEX;
        for (int r = tid; r < rows; r += 256) {
            const float v = score[r0 + r];
            sum += (double)v;
            peak_merge(best, arg, v != v ? -INFINITY : v, r0 + r);
        }
        smd[tid] = sum; smf[tid] = best; sml[tid] = arg;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) {
                smd[tid] += smd[tid + st];
                peak_merge(smf[tid], sml[tid], smf[tid + st], sml[tid + st]);
            }
            __syncthreads();
        }
        if (tid == 0) { ssum[slot] = smd[0]; smax[slot] = smf[0]; sarg[slot] = sml[0]; }
        __syncthreads();
        if (!per_dim) continue;
        for (int c0 = 0; c0 < d; c0 += ct) {
            const int col = c0 + c;
            double a = 0.0;
            int h = 0;
            if (col < d) {
                const double t = thr ? thr[col] : 0.0;
                for (int r = rsub; r < rows; r += rp) {
                    const float v = per_dim[(r0 + r) * ld + col];
                    a += (double)v;
                    if (thr) h += ((double)v >= t) ? 1 : 0;
                }
            }
            smd[tid] = a; smi[tid] = h;
            __syncthreads();
            for (int st = rp >> 1; st > 0; st >>= 1) {
                if (rsub < st) { smd[tid] += smd[tid + st * ct]; smi[tid] += smi[tid + st * ct]; }
                __syncthreads();
            }
            if (rsub == 0 && col < d) {
                psum[slot * d + col] = smd[tid];
                if (thr) phit[slot * d + col] = smi[tid];
            }
            __syncthreads();
        }
    }
}

// ranking key of a column mean: larger value first, the lower column among equals (-0 = +0), NaN after every number; 0 = taken
__device__ __forceinline__ unsigned long long rank_key(float m, int col) {
    unsigned ord = 1u;
    if (m == m) {
        ord = float_order_bits(m == 0.f ? 0.f : m);                 // -inf maps to 0x007fffff
    }
    return ((unsigned long long)ord << 32) | (unsigned long long)(0xffffffffu - (unsigned)col);
}

// one wave per run: the block partials added in block order, the means, then top_k rounds of arg-max over the column keys
__global__ void __launch_bounds__(64) k_eval_run_final(long n, const long* __restrict__ start, const long* __restrict__ end, int d,
                                                        int has_thr, int top_k, const double* __restrict__ ssum,
                                                        const float* __restrict__ smax, const long* __restrict__ sarg,
                                                        const double* __restrict__ psum, const int* __restrict__ phit,
                                                        long* __restrict__ peak, float* __restrict__ peak_score,
                                                        float* __restrict__ mean_score, float* __restrict__ fmeans,
                                                        int* __restrict__ top_idx, float* __restrict__ top_val, int* __restrict__ fhits) {
    __shared__ unsigned long long key[2048];
    __shared__ float val[2048];
    const long k = blockIdx.x;
    const int lane = threadIdx.x;
    long s, e;
    span_bounds(start, end, k, n, s, e);
    const long len = e - s;
    const long nb = (len + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
    if (lane == 0) {
        double sum = 0.0;
        float best = -INFINITY;
        long arg = NO_INDEX;
        for (long b = 0; b < nb; ++b) {
            sum += ssum[slot0 + b];
            peak_merge(best, arg, smax[slot0 + b], sarg[slot0 + b]);
        }
        peak[k] = arg == NO_INDEX ? -1L : arg;                      // an empty run: no peak, NaN statistics
        peak_score[k] = nb ? best : __builtin_nanf("");
        mean_score[k] = (float)(sum / (double)len);
    }
    if (d < 1) return;
    for (int col = lane; col < d; col += 64) {
        double a = 0.0;
        int h = 0;
        for (long b = 0; b < nb; ++b) {
            a += psum[(slot0 + b) * d + col];
            if (has_thr) h += phit[(slot0 + b) * d + col];
        }
        const float m = (float)(a / (double)len);
        fmeans[k * d + col] = m;
        if (has_thr) fhits[k * d + col] = h;
        key[col] = rank_key(m, col);
        val[col] = m;
    }
    __syncthreads();
    for (int t = 0; t < top_k; ++t) {
        unsigned long long bk = 0ull;
        for (int col = lane; col < d; col += 64) bk = key[col] > bk ? key[col] : bk;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)bk, off), hi = __shfl_xor((unsigned)(bk >> 32), off);
            const unsigned long long o = ((unsigned long long)hi << 32) | lo;
            bk = o > bk ? o : bk;
        }
        const int col = (int)(0xffffffffu - (unsigned)bk);          // top_k <= d: a column is always left
        if (lane == 0) {
            top_idx[k * top_k + t] = col;
            top_val[k * top_k + t] = val[col];
            key[col] = 0ull;
        }
        __syncthreads();
    }
}

// first[k] = the smallest flagged index of run k, or -1: one wave per run, 64 samples per step
__global__ void __launch_bounds__(256) k_eval_first_hit(FlagSrc f, long n, const long* __restrict__ start, const long* __restrict__ end,
                                                         long count, long* __restrict__ first) {
    const long k = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= count) return;
    long s, e;
    span_bounds(start, end, k, n, s, e);
    long hit = -1;
    for (long base = s; base < e; base += 64) {
        const long i = base + lane;
        const unsigned long long m = __ballot(i < e && flag_at(f, i));
        if (m) { hit = base + __builtin_ctzll(m); break; }
    }
    if (lane == 0) first[k] = hit;
}

}  // namespace mtadgat

using namespace mtadgat;

namespace {

struct RunsScratch {
    long* counts;                // raw, merged and kept counts
    unsigned *T, *C;
    int *rs, *re, *ms, *me;
    long nchunks, max_raw;
};
RunsScratch runs_scratch(ScratchCarver& c, int64_t n) {
    RunsScratch l;
    l.nchunks = (long)((n + CHUNK_L - 1) / CHUNK_L);
    l.max_raw = (long)((n + 1) / 2);                // flagged and unflagged samples alternate
    l.counts = c.take<long>(4);
    l.T = c.take<unsigned>(l.nchunks);
    l.C = c.take<unsigned>(l.nchunks);
    l.rs = c.take<int>(l.max_raw);
    l.re = c.take<int>(l.max_raw);
    l.ms = c.take<int>(l.max_raw);
    l.me = c.take<int>(l.max_raw);
    return l;
}

struct StatsScratch {
    double* ssum;
    long* sarg;
    float* smax;
    double* psum;
    int* phit;
};
StatsScratch stats_scratch(ScratchCarver& c, int64_t n, int64_t count, int d) {
    const size_t slots = span_slots(n, count);
    StatsScratch l;
    l.ssum = c.take<double>(slots);
    l.sarg = c.take<long>(slots);
    l.smax = c.take<float>(slots);
    l.psum = c.take<double>(slots * (size_t)d);
    l.phit = c.take<int>(slots * (size_t)d);
    return l;
}

template <class Op>
void compact(const Op& op, long grid, const long* n_dev, long n_host, unsigned* T, unsigned* C, long* total, hipStream_t s) {
    hipLaunchKernelGGL(k_eval_runs_count<Op>, dim3((unsigned)grid), dim3(256), 0, s, op, n_dev, n_host, T);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, (const unsigned*)T, n_dev, grid, C, total);
    hipLaunchKernelGGL(k_eval_runs_emit<Op>, dim3((unsigned)grid), dim3(256), 0, s, op, n_dev, n_host, C);
}

FlagSrc flag_source(const float* score, const unsigned char* label, double threshold, int compare_f32) {
    FlagSrc f;
    f.score = score;
    f.label = label;
    f.t64 = threshold;
    f.t32 = (float)threshold;
    f.cmp_f32 = compare_f32;
    return f;
}

}  // namespace

extern "C" {

int mtadgat_eval_runs_chunk(void) { return CHUNK_L; }

size_t mtadgat_eval_runs_scratch(int64_t n) {
    if (n < 1 || n > 2147483647LL) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { runs_scratch(c, n); });
}

int mtadgat_eval_runs(const float* score_dev, const unsigned char* label_dev, int64_t n, double threshold, int compare_f32,
                      int64_t merge_gap, int64_t min_length, int64_t max_runs, void* scratch_dev, size_t scratch_bytes,
                      int64_t* start_dev, int64_t* end_dev, int64_t* count_host, void* stream) {
    if ((!score_dev && !label_dev) || !scratch_dev || !start_dev || !end_dev || !count_host) return record_error(-1, "runs: null pointer");
    if (score_dev && label_dev) return record_error(-1, "runs: give scores or labels, not both");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "runs: n must lie in [1, 2^31 - 1]");
    if (merge_gap < 0) return record_error(-1, "runs: merge_gap must be >= 0");
    if (min_length < 1) return record_error(-1, "runs: min_length must be >= 1");
    if (max_runs < 1) return record_error(-1, "runs: max_runs must be >= 1");
    ScratchCarver carver(scratch_dev);
    const RunsScratch l = runs_scratch(carver, n);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "runs: scratch too small (see mtadgat_eval_runs_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "runs: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // the run counts stay on the device between the stages, so the later grids cover the most runs n samples can hold
    const long run_grid = (l.max_raw + CHUNK_L - 1) / CHUNK_L;
    compact(RawRuns{flag_source(score_dev, label_dev, threshold, compare_f32), l.rs, l.re}, l.nchunks, nullptr, (long)n, l.T, l.C, l.counts, s);
    compact(MergeRuns{l.rs, l.re, (long)merge_gap, l.ms, l.me}, run_grid, l.counts, 0L, l.T, l.C, l.counts + 1, s);
    compact(KeepRuns{l.ms, l.me, (long)min_length, (long)max_runs, reinterpret_cast<long*>(start_dev), reinterpret_cast<long*>(end_dev)}, run_grid,
            l.counts + 1, 0L, l.T, l.C, l.counts + 2, s);
    if (hipGetLastError() != hipSuccess) return record_error(-3, "runs: kernel launch failed");
    if (hipMemcpyAsync(count_host, l.counts + 2, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) return record_error(-3, "runs: copy failed");
    if (hipStreamSynchronize(s) != hipSuccess) return record_error(-3, "runs: stream failed");
    if (*count_host > max_runs) return record_error(-5, "runs: more runs than max_runs (the count is set: call again with that capacity)");
    return 0;
}

size_t mtadgat_eval_run_stats_scratch(int64_t n, int64_t count, int d) {
    if (n < 1 || n > 2147483647LL || count < 0 || count > 2147483647LL || d < 0 || d > 2048) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { stats_scratch(c, n, count, d); });
}

int mtadgat_eval_run_stats(const float* score_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                           const float* per_dim_dev, int d, int64_t ld, const double* thr_dev, int top_k, void* scratch_dev,
                           size_t scratch_bytes, int64_t* peak_dev, float* peak_score_dev, float* mean_score_dev,
                           float* feature_means_dev, int* top_idx_dev, float* top_val_dev, int* feature_hits_dev, void* stream) {
    if (!score_dev || !start_dev || !end_dev || !scratch_dev || !peak_dev || !peak_score_dev || !mean_score_dev)
        return record_error(-1, "run_stats: null pointer");
    if (per_dim_dev && (!feature_means_dev || !top_idx_dev || !top_val_dev)) return record_error(-1, "run_stats: null pointer (per_dim outputs)");
    if (thr_dev && (!per_dim_dev || !feature_hits_dev)) return record_error(-1, "run_stats: null pointer (thresholds need per_dim and feature_hits)");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "run_stats: n must lie in [1, 2^31 - 1]");
    if (count < 0 || count > 2147483647LL) return record_error(-1, "run_stats: count must lie in [0, 2^31 - 1]");
    if (per_dim_dev) {
        if (d < 1 || d > 2048) return record_error(-1, "run_stats: d must lie in [1, 2048]");
        if (ld < d) return record_error(-1, "run_stats: ld < d");
        if (top_k < 1 || top_k > d || top_k > 64) return record_error(-1, "run_stats: top_k must lie in [1, min(d, 64)]");
    } else {
        d = 0;
    }
    ScratchCarver carver(scratch_dev);
    const StatsScratch l = stats_scratch(carver, n, count, d);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "run_stats: scratch too small (see mtadgat_eval_run_stats_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "run_stats: scratch must be 8-byte aligned");
    if (count == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int ct = 1;
    while (ct < d && ct < 64) ct <<= 1;
    const long slices = span_slices(n, count, SPAN_RB);
    const long* st = reinterpret_cast<const long*>(start_dev);
    const long* en = reinterpret_cast<const long*>(end_dev);
    hipLaunchKernelGGL(k_eval_run_part, dim3((unsigned)count, (unsigned)slices), dim3(256), 0, s, score_dev, (long)n, st, en, per_dim_dev, d,
                       (long)ld, thr_dev, ct, l.ssum, l.smax, l.sarg, l.psum, l.phit);
    hipLaunchKernelGGL(k_eval_run_final, dim3((unsigned)count), dim3(64), 0, s, (long)n, st, en, d, thr_dev ? 1 : 0, top_k, l.ssum, l.smax, l.sarg, l.psum,
                       l.phit, reinterpret_cast<long*>(peak_dev), peak_score_dev, mean_score_dev, feature_means_dev, top_idx_dev, top_val_dev,
                       feature_hits_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "run_stats: kernel launch failed");
}

int mtadgat_eval_first_hit(const float* score_dev, const unsigned char* label_dev, int64_t n, double threshold, int compare_f32,
                           const int64_t* start_dev, const int64_t* end_dev, int64_t count, int64_t* first_dev, void* stream) {
    if ((!score_dev && !label_dev) || !start_dev || !end_dev || !first_dev) return record_error(-1, "first_hit: null pointer");
    if (score_dev && label_dev) return record_error(-1, "first_hit: give scores or labels, not both");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "first_hit: n must lie in [1, 2^31 - 1]");
    if (count < 0 || count > 2147483647LL) return record_error(-1, "first_hit: count must lie in [0, 2^31 - 1]");
    if (count == 0) return 0;
    hipLaunchKernelGGL(k_eval_first_hit, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       flag_source(score_dev, label_dev, threshold, compare_f32), (long)n, reinterpret_cast<const long*>(start_dev),
                       reinterpret_cast<const long*>(end_dev), (long)count, reinterpret_cast<long*>(first_dev));
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "first_hit: kernel launch failed");
}

}  // extern "C"
