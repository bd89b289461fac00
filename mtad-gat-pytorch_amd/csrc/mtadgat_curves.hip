// Ranking a score array on the device (evaluation.score_order, ranking_curve, ranking_metrics):
//
//   k_sort_*: a least-significant-digit radix sort of 64-bit keys with a 32-bit payload, 8 bits per pass, for as many passes as the
//       caller's key bits need (four for a float32 order key).  A pass is three steps: every tile of SORT_TILE items counts its
//       digits (k_sort_hist), one exclusive scan runs over the (digit, tile) table in digit-major order (k_scan_*: one block up to
//       SORT_LEVEL2 tiles, above that block sums, one wave over the sums, and the blocks again), and every tile writes its items
//       behind the table's entry (k_sort_scatter).  An item's rank among the items of its tile with the same digit is: the items
//       of earlier waves (a 4 x 256 LDS table), plus the items of earlier 64-item rounds of its wave (the same table, advanced
//       after each round), plus the lower lanes of its round with the same digit -- eight __ballot masks, one per digit bit,
//       intersected to the 64-bit mask of the lanes that share the digit, and __popcll of the part below the lane.  A wave owns
//       consecutive items, so equal digits keep their input order: the sort is stable, and since nothing is an atomic the output is
//       a function of the input alone.
//   order key of a float32 (order_key below, exported as mtadgat_eval_order_key): -0 becomes +0, the sign bit is flipped for
//       non-negative values and all bits for negative ones, the result is inverted for descending order, every NaN is 0xffffffff.
//   k_seg_*: the adjusted scores.  Labelled segments are the runs of mtadgat_eval_runs on the labels.  Per segment the largest
//       non-NaN score and the number of non-NaN scores come from fixed row blocks (the scheme of k_eval_run_part / _final).
//       "point": every sample of the segment takes that maximum (sample 0 keeps its own score: the reference's back-fill never
//       reaches index 0).  PA%K: the labelled samples are sorted by (segment << 32 | descending key); a segment's span starts at
//       the exclusive scan of the segment lengths, NaNs end the span, entry m - 1 of the span is the m-th largest score, and a
//       sample takes max(own, that) when the segment has m non-NaN scores.
//   k_curve_*: after the global sort of (descending key of the adjusted score, label bit): a tie group ends where the key
//       differs from the next one; one blocked scan (the count / carry / emit pattern of mtadgat_events.hip) ranks the group ends
//       and counts the positives up to each, and the emit pass writes thresholds / tp / fp of the numeric groups.  One reduction in a
//       fixed order -- 16 consecutive groups per lane, a 256-lane tree, then the block partials 256 apart and the same tree --
//       gives the doubled AUROC numerator (int64), the average-precision sum (float64) and the arg-max of F1 (value, then lowest
//       index).
#include "mtadgat_device.h"

// the run extraction of mtadgat_events.hip (include/mtadgat.h): the labelled segments
extern "C" size_t mtadgat_eval_runs_scratch(int64_t n);
extern "C" int mtadgat_eval_runs(const float* score_dev, const unsigned char* label_dev, int64_t n, double threshold, int compare_f32,
                                 int64_t merge_gap, int64_t min_length, int64_t max_runs, void* scratch_dev, size_t scratch_bytes,
                                 int64_t* start_dev, int64_t* end_dev, int64_t* count_host, void* stream);

namespace mtadgat {

constexpr int SORT_ITEMS = 8;                    // 64-item rounds per wave and tile
constexpr int SORT_TILE = 256 * SORT_ITEMS;      // 4 waves, each with SORT_ITEMS * 64 consecutive items
constexpr int SCAN_BLOCK = 4096;                 // table entries per block of the scan: 256 lanes x 16
constexpr int SORT_LEVEL2 = SCAN_BLOCK / 256;    // tiles up to which one block scans the whole (digit, tile) table
constexpr int CURVE_L = 1024;                    // items per chunk of the curve scan
constexpr int RED_L = 4096;                      // tie groups per block of the reduction: 256 lanes x 16
constexpr int SEG_RB = 1024;                     // rows per block of the segment reductions
constexpr unsigned NAN_KEY = 0xffffffffu;
constexpr long NO_GROUP = 0x7fffffffffffffffL;

__host__ __device__ inline unsigned order_key(float v, int descending) {
    if (v != v) return NAN_KEY;
    if (v == 0.f) v = 0.f;
    unsigned u = __builtin_bit_cast(unsigned, v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return descending ? ~u : u;
}
// the float32 behind a descending key (not for NAN_KEY)
__device__ __forceinline__ float key_value(unsigned k) {
    const unsigned u = ~k;
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// ---- sort ------------------------------------------------------------------------------------------------------------------------
// the digits of this thread's SORT_ITEMS items and their ranks inside the wave among equal digits; wcnt[w][d] ends as the number of
// items of wave w with digit d.  Every thread of the block calls it (barriers inside).
__device__ __forceinline__ void tile_ranks(const unsigned long long* __restrict__ keys, long n, long tile, int shift, unsigned (*wcnt)[256],
                                           unsigned long long (&key)[SORT_ITEMS], unsigned (&rank)[SORT_ITEMS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = threadIdx.x; t < 4 * 256; t += 256) (&wcnt[0][0])[t] = 0u;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const long base = tile * SORT_TILE + (long)wave * (SORT_ITEMS * 64);
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const long i = base + r * 64 + lane;
        const bool valid = i < n;
        key[r] = valid ? keys[i] : 0ull;
        const unsigned d = (unsigned)(key[r] >> shift) & 255u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const unsigned before = wcnt[wave][d];
        __syncthreads();
        const unsigned lower = (unsigned)__popcll(same & below);
        rank[r] = before + lower;
        if (valid && lower == 0u) wcnt[wave][d] = before + (unsigned)__popcll(same);
        __syncthreads();
    }
}

// cnt[d * ntiles + tile] = items of the tile with digit d
__global__ void __launch_bounds__(256) k_sort_hist(const unsigned long long* __restrict__ keys, long n, long ntiles, int shift,
                                                    unsigned* __restrict__ cnt) {
    __shared__ unsigned wcnt[4][256];
    unsigned long long key[SORT_ITEMS];
    unsigned rank[SORT_ITEMS];
    tile_ranks(keys, n, blockIdx.x, shift, wcnt, key, rank);
    const int d = threadIdx.x;
    cnt[(long)d * ntiles + blockIdx.x] = (wcnt[0][d] + wcnt[1][d]) + (wcnt[2][d] + wcnt[3][d]);
}

// every item to cnt[d * ntiles + tile] (now the exclusive scan) + its rank inside the tile among the items with digit d
__global__ void __launch_bounds__(256) k_sort_scatter(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ pay, long n,
                                                       long ntiles, int shift, const unsigned* __restrict__ cnt,
                                                       unsigned long long* __restrict__ keys_out, unsigned* __restrict__ pay_out) {
    __shared__ unsigned wcnt[4][256];
    unsigned long long key[SORT_ITEMS];
    unsigned rank[SORT_ITEMS];
    tile_ranks(keys, n, blockIdx.x, shift, wcnt, key, rank);
    {
        const int d = threadIdx.x;
        const unsigned c0 = wcnt[0][d], c1 = wcnt[1][d], c2 = wcnt[2][d];
        const unsigned g = cnt[(long)d * ntiles + blockIdx.x];
        wcnt[0][d] = g; wcnt[1][d] = g + c0; wcnt[2][d] = g + c0 + c1; wcnt[3][d] = g + c0 + c1 + c2;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * SORT_TILE + (long)wave * (SORT_ITEMS * 64);
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const long i = base + r * 64 + lane;
        if (i < n) {
            const unsigned d = (unsigned)(key[r] >> shift) & 255u;
            const long to = (long)wcnt[wave][d] + rank[r];
            if (to < n) {                        // always: the table sums to n
                keys_out[to] = key[r];
                pay_out[to] = pay[i];
            }
        }
    }
}

// ---- exclusive scan of an unsigned array of m entries in place (sums below 2^32) ----
__device__ __forceinline__ unsigned block_exclusive(unsigned mine, unsigned* sm, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned s = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(s, off);
        if (lane >= off) s += t;
    }
    if (lane == 63) sm[wave] = s;
    __syncthreads();
    unsigned before = 0u;
    for (int w = 0; w < wave; ++w) before += sm[w];
    total = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return before + s - mine;
}

__global__ void __launch_bounds__(256) k_scan_sum(const unsigned* __restrict__ a, long m, unsigned* __restrict__ S) {
    __shared__ unsigned sm[4];
    const long i0 = (long)blockIdx.x * SCAN_BLOCK + threadIdx.x * 16;
    unsigned c = 0u;
#pragma unroll
    for (int e = 0; e < 16; ++e) c += (i0 + e < m) ? a[i0 + e] : 0u;
    unsigned total;
    block_exclusive(c, sm, total);
    if (threadIdx.x == 0) S[blockIdx.x] = total;
}

// S (nb entries) to its exclusive scan, 64 entries per step of one wave; *total (may be null) = the sum
__global__ void __launch_bounds__(64) k_scan_carry(unsigned* __restrict__ S, long nb, long* __restrict__ total) {
    const int lane = threadIdx.x;
    unsigned run = 0u;
    for (long base = 0; base < nb; base += 64) {
        const long i = base + lane;
        const unsigned mine = i < nb ? S[i] : 0u;
        unsigned s = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned t = __shfl_up(s, off);
            if (lane >= off) s += t;
        }
        if (i < nb) S[i] = run + s - mine;
        run += __shfl(s, 63);
    }
    if (total && lane == 0) *total = (long)run;
}

// S null: one block, base 0
__global__ void __launch_bounds__(256) k_scan_apply(unsigned* __restrict__ a, long m, const unsigned* __restrict__ S) {
    __shared__ unsigned sm[4];
    const long i0 = (long)blockIdx.x * SCAN_BLOCK + threadIdx.x * 16;
    unsigned v[16];
    unsigned c = 0u;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        v[e] = (i0 + e < m) ? a[i0 + e] : 0u;
        c += v[e];
    }
    unsigned total;
    unsigned at = block_exclusive(c, sm, total) + (S ? S[blockIdx.x] : 0u);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (i0 + e < m) a[i0 + e] = at;
        at += v[e];
    }
}

// ---- keys ------------------------------------------------------------------------------------------------------------------------
// payload: the index (label null) or the label bit
__global__ void __launch_bounds__(256) k_order_keys(const float* __restrict__ score, const unsigned char* __restrict__ label, long n,
                                                     int descending, unsigned long long* __restrict__ keys, unsigned* __restrict__ pay) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = (unsigned long long)order_key(score[i], descending);
    pay[i] = label ? (label[i] ? 1u : 0u) : (unsigned)i;
}

__global__ void __launch_bounds__(256) k_order_out(const unsigned* __restrict__ pay, long n, long* __restrict__ order) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) order[i] = (long)pay[i];
}

// ---- labelled segments -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void seg_bounds(const long* __restrict__ start, const long* __restrict__ end, long k, long n, long& s, long& e) {
    s = start[k];
    e = end[k];
    if (s < 0) s = 0;
    if (e > n) e = n;
    if (e < s) e = s;
}
// segments are disjoint and ascending: s / SEG_RB + k + b is different for every (k, b) and below n / SEG_RB + count + 1
__device__ __forceinline__ long seg_slot0(long s, long k) { return s / SEG_RB + k; }
// the larger of two maxima, NaN standing for "no number yet"
__device__ __forceinline__ float max_number(float a, float b) { return a != a ? b : (b != b ? a : (b > a ? b : a)); }

// grid (segment, slice): per row block the largest non-NaN score (NaN: none) and the number of non-NaN scores
__global__ void __launch_bounds__(256) k_seg_part(const float* __restrict__ score, long n, const long* __restrict__ start,
                                                   const long* __restrict__ end, float* __restrict__ pmax, unsigned* __restrict__ pcnt) {
    __shared__ float smf[256];
    __shared__ unsigned smc[256];
    const int tid = threadIdx.x;
    const long k = blockIdx.x;
    long s, e;
    seg_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SEG_RB - 1) / SEG_RB;
    const long slot0 = seg_slot0(s, k);
    for (long b = blockIdx.y; b < nb; b += gridDim.y) {
        const long r0 = s + b * SEG_RB;
        const int rows = e - r0 < SEG_RB ? (int)(e - r0) : SEG_RB;
        float best = __builtin_nanf("");
        unsigned c = 0u;
        for (int r = tid; r < rows; r += 256) {
            const float v = score[r0 + r];
            best = max_number(best, v);
            c += v == v ? 1u : 0u;
        }
        smf[tid] = best; smc[tid] = c;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) { smf[tid] = max_number(smf[tid], smf[tid + st]); smc[tid] += smc[tid + st]; }
            __syncthreads();
        }
        if (tid == 0) { pmax[slot0 + b] = smf[0]; pcnt[slot0 + b] = smc[0]; }
        __syncthreads();
    }
}

// one wave per segment: the block partials joined, and the segment's length for the span scan
__global__ void __launch_bounds__(256) k_seg_final(long n, const long* __restrict__ start, const long* __restrict__ end, long count,
                                                    const float* __restrict__ pmax, const unsigned* __restrict__ pcnt,
                                                    float* __restrict__ seg_max, unsigned* __restrict__ seg_numbers, unsigned* __restrict__ seg_off) {
    const long k = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= count) return;
    long s, e;
    seg_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SEG_RB - 1) / SEG_RB;
    const long slot0 = seg_slot0(s, k);
    float best = __builtin_nanf("");
    unsigned c = 0u;
    for (long b = lane; b < nb; b += 64) {
        best = max_number(best, pmax[slot0 + b]);
        c += pcnt[slot0 + b];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        best = max_number(best, __shfl_xor(best, off));
        c += __shfl_xor(c, off);
    }
    if (lane == 0) { seg_max[k] = best; seg_numbers[k] = c; seg_off[k] = (unsigned)(e - s); }
}

// grid (segment, slice): the labelled samples to their span, keyed (segment << 32 | descending key)
__global__ void __launch_bounds__(256) k_seg_keys(const float* __restrict__ score, long n, const long* __restrict__ start,
                                                   const long* __restrict__ end, const unsigned* __restrict__ seg_off,
                                                   unsigned long long* __restrict__ keys, unsigned* __restrict__ pay) {
    const long k = blockIdx.x;
    long s, e;
    seg_bounds(start, end, k, n, s, e);
    const long off = seg_off[k];
    for (long i = s + (long)blockIdx.y * 256 + threadIdx.x; i < e; i += (long)gridDim.y * 256) {
        const long to = off + (i - s);
        if (to < n) {
            keys[to] = ((unsigned long long)k << 32) | (unsigned long long)order_key(score[i], 1);
            pay[to] = (unsigned)i;
        }
    }
}

// seg_value[k] = the m-th largest non-NaN score of segment k, m = K * length / 100 + 1, or NaN when it has fewer
__global__ void __launch_bounds__(256) k_seg_kth(long n, const long* __restrict__ start, const long* __restrict__ end, long count, int K,
                                                  const unsigned* __restrict__ seg_off, const unsigned* __restrict__ seg_numbers,
                                                  const unsigned long long* __restrict__ keys, float* __restrict__ seg_value) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    long s, e;
    seg_bounds(start, end, k, n, s, e);
    const long m = (long)K * (e - s) / 100 + 1;
    const long at = (long)seg_off[k] + m - 1;
    seg_value[k] = ((long)seg_numbers[k] >= m && at < n) ? key_value((unsigned)keys[at]) : __builtin_nanf("");
}

// grid (segment, slice).  point: every sample but sample 0 takes the segment's value; otherwise max(own, value), NaN read as "none"
__global__ void __launch_bounds__(256) k_seg_broadcast(const float* __restrict__ score, long n, const long* __restrict__ start,
                                                        const long* __restrict__ end, const float* __restrict__ seg_value, int point,
                                                        float* __restrict__ adjusted) {
    const long k = blockIdx.x;
    long s, e;
    seg_bounds(start, end, k, n, s, e);
    const float v = seg_value[k];
    for (long i = s + (long)blockIdx.y * 256 + threadIdx.x; i < e; i += (long)gridDim.y * 256) {
        const float own = score[i];
        adjusted[i] = point ? (i == 0 ? own : v) : max_number(own, v);
    }
}

// ---- curve -----------------------------------------------------------------------------------------------------------------------
// item j of the sorted order: a positive? the last of a numeric tie group?
struct CurveItems {
    const unsigned long long* keys;
    const unsigned* pay;
    __device__ bool positive(long j) const { return pay[j] != 0u; }
    __device__ bool group_end(long j, long n) const {
        const unsigned k = (unsigned)keys[j];
        return k != NAN_KEY && (j + 1 == n || (unsigned)keys[j + 1] != k);
    }
};

__global__ void __launch_bounds__(256) k_curve_count(CurveItems it, long n, unsigned* __restrict__ Tp, unsigned* __restrict__ Te) {
    __shared__ unsigned smp[4], sme[4];
    const long base = (long)blockIdx.x * CURVE_L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned p = 0u, e = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long j = base + wave * 256 + r * 64 + lane;
        p += (unsigned)__popcll(__ballot(j < n && it.positive(j)));
        e += (unsigned)__popcll(__ballot(j < n && it.group_end(j, n)));
    }
    if (lane == 0) { smp[wave] = p; sme[wave] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        Tp[blockIdx.x] = (smp[0] + smp[1]) + (smp[2] + smp[3]);
        Te[blockIdx.x] = (sme[0] + sme[1]) + (sme[2] + sme[3]);
    }
}

// thresholds / tp / fp of every numeric tie group, at the group's rank
__global__ void __launch_bounds__(256) k_curve_emit(CurveItems it, long n, const unsigned* __restrict__ Cp, const unsigned* __restrict__ Ce,
                                                     float* __restrict__ thresholds, long* __restrict__ tp, long* __restrict__ fp) {
    __shared__ unsigned smp[4], sme[4];
    const long base = (long)blockIdx.x * CURVE_L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool p[4], e[4];
    unsigned long long mp[4], me[4];
    unsigned cp = 0u, ce = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long j = base + wave * 256 + r * 64 + lane;
        p[r] = j < n && it.positive(j);
        e[r] = j < n && it.group_end(j, n);
        mp[r] = __ballot(p[r]);
        me[r] = __ballot(e[r]);
        cp += (unsigned)__popcll(mp[r]);
        ce += (unsigned)__popcll(me[r]);
    }
    if (lane == 0) { smp[wave] = cp; sme[wave] = ce; }
    __syncthreads();
    long pos = Cp[blockIdx.x], rank = Ce[blockIdx.x];
    for (int w = 0; w < wave; ++w) { pos += smp[w]; rank += sme[w]; }
    const unsigned long long upto = ((1ull << lane) - 1ull) | (1ull << lane), below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long j = base + wave * 256 + r * 64 + lane;
        if (e[r]) {
            const long g = rank + __popcll(me[r] & below);
            const long t = pos + __popcll(mp[r] & upto);
            if (g < n) {                         // always: at most n groups
                thresholds[g] = key_value((unsigned)it.keys[j]);
                tp[g] = t;
                fp[g] = j + 1 - t;
            }
        }
        pos += __popcll(mp[r]);
        rank += __popcll(me[r]);
    }
}

struct CurvePart {
    long auc2;            // sum of tp_g (2 (n_neg - FP_g) + fp_g)
    double ap;            // sum of tp_g TP_g / (TP_g + FP_g)
    double f1;            // the largest F1 (-1: none) and the lowest group that attains it
    long arg;
};

// evaluation._scores_from_counts' F1 in float64, every operation rounded on its own as numpy rounds it
__device__ __forceinline__ double guarded_f1(double tp, double fp, double fn) {
#pragma clang fp contract(off)
    const double prec = tp / (tp + fp + 0.00001);
    const double rec = tp / (tp + fn + 0.00001);
    return 2 * prec * rec / (prec + rec + 0.00001);
}
__device__ __forceinline__ double precision_term(double tpg, double tp, double fp) {
#pragma clang fp contract(off)
    const double prec = tp / (tp + fp);
    return tpg * prec;
}
__device__ __forceinline__ void part_join(CurvePart& a, const CurvePart& b) {
#pragma clang fp contract(off)
    a.auc2 += b.auc2;
    a.ap = a.ap + b.ap;
    if (b.f1 > a.f1 || (b.f1 == a.f1 && b.arg < a.arg)) { a.f1 = b.f1; a.arg = b.arg; }
}
__device__ __forceinline__ void part_tree(CurvePart& mine, CurvePart* sm) {
    const int tid = threadIdx.x;
    sm[tid] = mine;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) part_join(sm[tid], sm[tid + st]);
        __syncthreads();
    }
    mine = sm[0];
}

// totals[0] = positives, totals[1] = G (left by the carries of the curve scan)
__global__ void __launch_bounds__(256) k_curve_reduce(const long* __restrict__ tp, const long* __restrict__ fp, long n,
                                                       const long* __restrict__ totals, CurvePart* __restrict__ parts) {
    __shared__ CurvePart sm[256];
    const long G = totals[1], n_pos = totals[0], n_neg = n - n_pos;
    const long g0 = (long)blockIdx.x * RED_L;
    if (g0 >= G) return;
    CurvePart mine = {0L, 0.0, -1.0, NO_GROUP};
    long g = g0 + threadIdx.x * 16;
    long tp_prev = (g > 0 && g < G) ? tp[g - 1] : 0L, fp_prev = (g > 0 && g < G) ? fp[g - 1] : 0L;
    for (int e = 0; e < 16 && g < G; ++e, ++g) {
        const long TP = tp[g], FP = fp[g];
        const long tpg = TP - tp_prev, fpg = FP - fp_prev;
        CurvePart one;
        one.auc2 = tpg * (2 * (n_neg - FP) + fpg);
        one.ap = precision_term((double)tpg, (double)TP, (double)FP);
        one.f1 = guarded_f1((double)TP, (double)FP, (double)(n_pos - TP));
        one.arg = g;
        part_join(mine, one);
        tp_prev = TP; fp_prev = FP;
    }
    part_tree(mine, sm);
    if (threadIdx.x == 0) parts[blockIdx.x] = mine;
}

// summary: G, n_pos, n_neg, nan_pos, nan_neg, doubled AUROC numerator, average-precision sum (bits), best group, its TP, FP, threshold (bits)
__global__ void __launch_bounds__(256) k_curve_final(const float* __restrict__ thresholds, const long* __restrict__ tp, const long* __restrict__ fp,
                                                      long n, const long* __restrict__ totals, const CurvePart* __restrict__ parts,
                                                      long* __restrict__ summary) {
    __shared__ CurvePart sm[256];
    const long G = totals[1], n_pos = totals[0], n_neg = n - n_pos;
    const long nparts = (G + RED_L - 1) / RED_L;
    CurvePart mine = {0L, 0.0, -1.0, NO_GROUP};
    for (long p = threadIdx.x; p < nparts; p += 256) part_join(mine, parts[p]);
    part_tree(mine, sm);
    if (threadIdx.x != 0) return;
    const long numeric_pos = G ? tp[G - 1] : 0L, numeric_neg = G ? fp[G - 1] : 0L;
    const long nan_pos = n_pos - numeric_pos, nan_neg = n_neg - numeric_neg;
    summary[0] = G; summary[1] = n_pos; summary[2] = n_neg; summary[3] = nan_pos; summary[4] = nan_neg;
    summary[5] = mine.auc2 + nan_pos * nan_neg;              // the NaN samples: one last tie group below every number
    summary[6] = __builtin_bit_cast(long, mine.ap);
    const long best = G ? mine.arg : -1L;
    summary[7] = best;
    summary[8] = best >= 0 ? tp[best] : 0L;
    summary[9] = best >= 0 ? fp[best] : 0L;
    summary[10] = best >= 0 ? (long)__builtin_bit_cast(unsigned, thresholds[best]) : 0L;
    summary[11] = 0L;
}

}  // namespace mtadgat

using namespace mtadgat;

namespace {

size_t up8(size_t v) { return (v + 7) / 8 * 8; }

long tiles_of(int64_t n) { return (long)((n + SORT_TILE - 1) / SORT_TILE); }
long scan_blocks(long m) { return (m + SCAN_BLOCK - 1) / SCAN_BLOCK; }

struct SortLayout {
    size_t keys_a, keys_b, pay_a, pay_b, cnt, sums, bytes;      // byte offsets
};
SortLayout sort_layout(int64_t n, size_t at) {
    SortLayout l;
    const size_t table = 256 * (size_t)tiles_of(n);
    l.keys_a = at;
    l.keys_b = l.keys_a + 8 * (size_t)n;
    l.pay_a = l.keys_b + 8 * (size_t)n;
    l.pay_b = l.pay_a + up8(4 * (size_t)n);
    l.cnt = l.pay_b + up8(4 * (size_t)n);
    l.sums = l.cnt + up8(4 * table);
    l.bytes = l.sums + up8(4 * (size_t)scan_blocks((long)table));
    return l;
}

struct SortBuffers {
    unsigned long long* keys[2];
    unsigned* pay[2];
    unsigned* cnt;
    unsigned* sums;
};
SortBuffers sort_buffers(char* base, const SortLayout& l) {
    SortBuffers b;
    b.keys[0] = reinterpret_cast<unsigned long long*>(base + l.keys_a);
    b.keys[1] = reinterpret_cast<unsigned long long*>(base + l.keys_b);
    b.pay[0] = reinterpret_cast<unsigned*>(base + l.pay_a);
    b.pay[1] = reinterpret_cast<unsigned*>(base + l.pay_b);
    b.cnt = reinterpret_cast<unsigned*>(base + l.cnt);
    b.sums = reinterpret_cast<unsigned*>(base + l.sums);
    return b;
}

// exclusive scan of a[0 .. m) in place; sums holds scan_blocks(m) entries
void scan_in_place(unsigned* a, long m, unsigned* sums, hipStream_t s) {
    const long nb = scan_blocks(m);
    if (nb <= 1) {
        hipLaunchKernelGGL(k_scan_apply, dim3(1), dim3(256), 0, s, a, m, (const unsigned*)nullptr);
        return;
    }
    hipLaunchKernelGGL(k_scan_sum, dim3((unsigned)nb), dim3(256), 0, s, (const unsigned*)a, m, sums);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, sums, nb, (long*)nullptr);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(256), 0, s, a, m, (const unsigned*)sums);
}

// sorts the m items of keys[0] / pay[0] by their low key_bits bits; returns the index (0 or 1) of the buffers that hold the result
int radix_sort(const SortBuffers& b, long m, int key_bits, hipStream_t s) {
    const long ntiles = tiles_of(m);
    int cur = 0;
    for (int shift = 0; shift < key_bits; shift += 8) {
        hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)ntiles), dim3(256), 0, s, (const unsigned long long*)b.keys[cur], m, ntiles, shift, b.cnt);
        scan_in_place(b.cnt, 256 * ntiles, b.sums, s);
        hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)ntiles), dim3(256), 0, s, (const unsigned long long*)b.keys[cur],
                           (const unsigned*)b.pay[cur], m, ntiles, shift, (const unsigned*)b.cnt, b.keys[1 - cur], b.pay[1 - cur]);
        cur = 1 - cur;
    }
    return cur;
}

struct CurveLayout {
    SortLayout sort;
    size_t totals, summary, Tp, Te, parts, adjusted, runs, seg_start, seg_end, pmax, pcnt, seg_max, seg_numbers, seg_off, seg_sums, bytes;
    size_t runs_bytes;
    long nchunks, nparts, max_seg;
};
CurveLayout curve_layout(int64_t n, int adjust) {
    CurveLayout l;
    l.nchunks = (long)((n + CURVE_L - 1) / CURVE_L);
    l.nparts = (long)((n + RED_L - 1) / RED_L);
    l.max_seg = (long)((n + 1) / 2);
    l.totals = 0;                                  // positives, G, labelled samples (int64), padded to 32 bytes
    l.summary = 32;                                // 12 int64
    l.Tp = l.summary + 96;
    l.Te = l.Tp + up8(4 * (size_t)l.nchunks);
    l.parts = l.Te + up8(4 * (size_t)l.nchunks);
    l.sort = sort_layout(n, l.parts + sizeof(CurvePart) * (size_t)l.nparts);
    l.adjusted = l.sort.bytes;
    l.bytes = l.adjusted;
    l.runs_bytes = 0;
    if (adjust) {
        const size_t slots = (size_t)(n / SEG_RB) + (size_t)l.max_seg + 2;
        l.runs_bytes = mtadgat_eval_runs_scratch(n);
        l.runs = l.adjusted + up8(4 * (size_t)n);
        l.seg_start = l.runs + up8(l.runs_bytes);
        l.seg_end = l.seg_start + 8 * (size_t)l.max_seg;
        l.pmax = l.seg_end + 8 * (size_t)l.max_seg;
        l.pcnt = l.pmax + up8(4 * slots);
        l.seg_max = l.pcnt + up8(4 * slots);
        l.seg_numbers = l.seg_max + up8(4 * (size_t)l.max_seg);
        l.seg_off = l.seg_numbers + up8(4 * (size_t)l.max_seg);
        l.seg_sums = l.seg_off + up8(4 * (size_t)l.max_seg);
        l.bytes = l.seg_sums + up8(4 * (size_t)scan_blocks(l.max_seg));
    }
    return l;
}

// slices per segment of the (segment, slice) grids: the results do not depend on it
long seg_slices(int64_t n, int64_t count, long per_slice) {
    const long most = (long)((n + per_slice - 1) / per_slice);
    long slices = 8192 / count;
    slices = slices < 4 ? 4 : (slices > 1024 ? 1024 : slices);
    return slices > most ? most : slices;
}

}  // namespace

extern "C" {

uint32_t mtadgat_eval_order_key(float value, int descending) { return order_key(value, descending); }
int mtadgat_eval_sort_tile(void) { return SORT_TILE; }
int mtadgat_eval_sort_scan_tiles(void) { return SORT_LEVEL2; }

size_t mtadgat_eval_score_order_scratch(int64_t n) {
    if (n < 1 || n > 2147483647LL) return 0;
    return sort_layout(n, 0).bytes;
}

int mtadgat_eval_score_order(const float* score_dev, int64_t n, int descending, void* scratch_dev, size_t scratch_bytes, int64_t* order_dev,
                             void* stream) {
    if (!score_dev || !scratch_dev || !order_dev) return record_error(-1, "score_order: null pointer");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "score_order: n must lie in [1, 2^31 - 1]");
    const SortLayout l = sort_layout(n, 0);
    if (scratch_bytes < l.bytes) return record_error(-5, "score_order: scratch too small (see mtadgat_eval_score_order_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "score_order: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const SortBuffers b = sort_buffers(static_cast<char*>(scratch_dev), l);
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_order_keys, dim3(grid), dim3(256), 0, s, score_dev, (const unsigned char*)nullptr, (long)n, descending ? 1 : 0, b.keys[0],
                       b.pay[0]);
    const int at = radix_sort(b, (long)n, 32, s);
    hipLaunchKernelGGL(k_order_out, dim3(grid), dim3(256), 0, s, (const unsigned*)b.pay[at], (long)n, reinterpret_cast<long*>(order_dev));
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "score_order: kernel launch failed");
}

size_t mtadgat_eval_curve_scratch(int64_t n, int adjust) {
    if (n < 1 || n > 2147483647LL || adjust < 0 || adjust > 2) return 0;
    return curve_layout(n, adjust).bytes;
}

int mtadgat_eval_curve(const float* score_dev, const unsigned char* label_dev, int64_t n, int adjust, int k_percent, void* scratch_dev,
                       size_t scratch_bytes, float* thresholds_dev, int64_t* tp_dev, int64_t* fp_dev, int64_t* summary_host, void* stream) {
    if (!score_dev || !label_dev || !scratch_dev || !thresholds_dev || !tp_dev || !fp_dev || !summary_host)
        return record_error(-1, "curve: null pointer");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "curve: n must lie in [1, 2^31 - 1]");
    if (adjust < 0 || adjust > 2) return record_error(-1, "curve: adjust must be 0 (none), 1 (point) or 2 (PA%K)");
    if (adjust == 2 && (k_percent < 0 || k_percent > 100)) return record_error(-1, "curve: K must lie in [0, 100]");
    const CurveLayout l = curve_layout(n, adjust);
    if (scratch_bytes < l.bytes) return record_error(-5, "curve: scratch too small (see mtadgat_eval_curve_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "curve: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(scratch_dev);
    long* totals = reinterpret_cast<long*>(base + l.totals);
    long* summary = reinterpret_cast<long*>(base + l.summary);
    unsigned* Tp = reinterpret_cast<unsigned*>(base + l.Tp);
    unsigned* Te = reinterpret_cast<unsigned*>(base + l.Te);
    CurvePart* parts = reinterpret_cast<CurvePart*>(base + l.parts);
    const SortBuffers b = sort_buffers(base, l.sort);
    const float* ranked = score_dev;

    if (adjust) {
        float* adjusted = reinterpret_cast<float*>(base + l.adjusted);
        long* seg_start = reinterpret_cast<long*>(base + l.seg_start);
        long* seg_end = reinterpret_cast<long*>(base + l.seg_end);
        float* pmax = reinterpret_cast<float*>(base + l.pmax);
        unsigned* pcnt = reinterpret_cast<unsigned*>(base + l.pcnt);
        float* seg_max = reinterpret_cast<float*>(base + l.seg_max);
        unsigned* seg_numbers = reinterpret_cast<unsigned*>(base + l.seg_numbers);
        unsigned* seg_off = reinterpret_cast<unsigned*>(base + l.seg_off);
        unsigned* seg_sums = reinterpret_cast<unsigned*>(base + l.seg_sums);
        int64_t count = 0;
        const int rc = mtadgat_eval_runs(nullptr, label_dev, n, 0.0, 0, 0, 1, l.max_seg, base + l.runs, l.runs_bytes,
                                         reinterpret_cast<int64_t*>(seg_start), reinterpret_cast<int64_t*>(seg_end), &count, stream);
        if (rc != 0) return rc;
        if (hipMemcpyAsync(adjusted, score_dev, 4 * (size_t)n, hipMemcpyDeviceToDevice, s) != hipSuccess) return record_error(-3, "curve: copy failed");
        if (count > 0) {
            const dim3 by_rows((unsigned)count, (unsigned)seg_slices(n, count, SEG_RB)), by_items((unsigned)count, (unsigned)seg_slices(n, count, 256));
            const unsigned waves = (unsigned)((count + 3) / 4);
            hipLaunchKernelGGL(k_seg_part, by_rows, dim3(256), 0, s, score_dev, (long)n, (const long*)seg_start, (const long*)seg_end, pmax, pcnt);
            hipLaunchKernelGGL(k_seg_final, dim3(waves), dim3(256), 0, s, (long)n, (const long*)seg_start, (const long*)seg_end, (long)count,
                               (const float*)pmax, (const unsigned*)pcnt, seg_max, seg_numbers, seg_off);
            const float* seg_value = seg_max;
            if (adjust == 2) {
                // spans: the exclusive scan of the segment lengths; every labelled sample lies in one segment, so they fill [0, labelled)
                int64_t labelled = 0;
                hipLaunchKernelGGL(k_scan_sum, dim3((unsigned)scan_blocks((long)count)), dim3(256), 0, s, (const unsigned*)seg_off, (long)count, seg_sums);
                hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, seg_sums, scan_blocks((long)count), totals + 2);
                hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)scan_blocks((long)count)), dim3(256), 0, s, seg_off, (long)count, (const unsigned*)seg_sums);
                if (hipMemcpyAsync(&labelled, totals + 2, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipStreamSynchronize(s) != hipSuccess)
                    return record_error(-3, "curve: stream failed");
                if (labelled < 1 || labelled > n) return record_error(-3, "curve: the segments do not match the labels");
                hipLaunchKernelGGL(k_seg_keys, by_items, dim3(256), 0, s, score_dev, (long)n, (const long*)seg_start, (const long*)seg_end,
                                   (const unsigned*)seg_off, b.keys[0], b.pay[0]);
                int seg_bits = 0;
                while (seg_bits < 31 && ((int64_t)1 << seg_bits) < count) ++seg_bits;
                const int at = radix_sort(b, (long)labelled, 32 + seg_bits, s);
                hipLaunchKernelGGL(k_seg_kth, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, (long)n, (const long*)seg_start,
                                   (const long*)seg_end, (long)count, k_percent, (const unsigned*)seg_off, (const unsigned*)seg_numbers,
                                   (const unsigned long long*)b.keys[at], seg_max);
            }
            hipLaunchKernelGGL(k_seg_broadcast, by_items, dim3(256), 0, s, score_dev, (long)n, (const long*)seg_start, (const long*)seg_end, seg_value,
                               adjust == 1 ? 1 : 0, adjusted);
        }
        ranked = adjusted;
    }

    hipLaunchKernelGGL(k_order_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ranked, label_dev, (long)n, 1, b.keys[0], b.pay[0]);
    const int at = radix_sort(b, (long)n, 32, s);
    const CurveItems items{b.keys[at], b.pay[at]};
    hipLaunchKernelGGL(k_curve_count, dim3((unsigned)l.nchunks), dim3(256), 0, s, items, (long)n, Tp, Te);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, Tp, l.nchunks, totals);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, Te, l.nchunks, totals + 1);
    hipLaunchKernelGGL(k_curve_emit, dim3((unsigned)l.nchunks), dim3(256), 0, s, items, (long)n, (const unsigned*)Tp, (const unsigned*)Te,
                       thresholds_dev, reinterpret_cast<long*>(tp_dev), reinterpret_cast<long*>(fp_dev));
    hipLaunchKernelGGL(k_curve_reduce, dim3((unsigned)l.nparts), dim3(256), 0, s, reinterpret_cast<const long*>(tp_dev),
                       reinterpret_cast<const long*>(fp_dev), (long)n, (const long*)totals, parts);
    hipLaunchKernelGGL(k_curve_final, dim3(1), dim3(256), 0, s, (const float*)thresholds_dev, reinterpret_cast<const long*>(tp_dev),
                       reinterpret_cast<const long*>(fp_dev), (long)n, (const long*)totals, (const CurvePart*)parts, summary);
    if (hipGetLastError() != hipSuccess) return record_error(-3, "curve: kernel launch failed");
    if (hipMemcpyAsync(summary_host, summary, 12 * sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) return record_error(-3, "curve: copy failed");
    if (hipStreamSynchronize(s) != hipSuccess) return record_error(-3, "curve: stream failed");
    return 0;
}

}  // extern "C"
