// Ranking a score array on the device (evaluation.score_order, ranking_curve, ranking_metrics):
//
//   k_sort_*: a least-significant-digit radix sort of 64-bit keys with a 32-bit payload, 8 bits per pass, for as many passes as the
//       caller's key bits need (four for a float32 order key).  A pass is three steps: every tile of SORT_TILE items counts its
//       digits (k_sort_hist), one exclusive scan runs over the (digit, tile) table in digit-major order (k_scan_*: one block up to
//       SORT_LEVEL2 tiles, above that block sums, mtadgat_scan.h's carry wave over the sums, and the blocks again), and every tile writes its items
//       behind the table's entry (k_sort_scatter).  An item's rank among the items of its tile with the same digit is: the items
//       of earlier waves (a 4 x 256 LDS table), plus the items of earlier 64-item rounds of its wave (the same table, advanced
//       after each round), plus the lower lanes of its round with the same digit -- eight __ballot masks, one per digit bit,
//       intersected to the 64-bit mask of the lanes that share the digit, and __popcll of the part below the lane.  A wave owns
//       consecutive items, so equal digits keep their input order: the sort is stable, and since nothing is an atomic the output is
//       a function of the input alone.
//   order key of a float32 (order_key below, exported as mtadgat_eval_order_key): -0 becomes +0, the sign bit is flipped for
//       non-negative values and all bits for negative ones, the result is inverted for descending order, every NaN is 0xffffffff.
//   k_seg_*: the adjusted scores.  Labelled segments are the runs of mtadgat_eval_runs on the labels.  Per segment the largest
//       non-NaN score and the number of non-NaN scores come from fixed row blocks (the spans of mtadgat_scan.h).
//       "point": every sample of the segment takes that maximum (sample 0 keeps its own score: the reference's back-fill never
//       reaches index 0).  PA%K: the labelled samples are sorted by (segment << 32 | descending key); a segment's span starts at
//       the exclusive scan of the segment lengths, NaNs end the span, entry m - 1 of the span is the m-th largest score, and a
//       sample takes max(own, that) when the segment has m non-NaN scores.
//   k_curve_*: after the global sort of (descending key of the adjusted score, label bit): a tie group ends where the key
//       differs from the next one; one blocked scan of counts (mtadgat_scan.h) over two predicates ranks the group ends
//       and counts the positives up to each, and the emit pass writes thresholds / tp / fp of the numeric groups.  One reduction in a
//       fixed order -- 16 consecutive groups per lane, a 256-lane tree, then the block partials 256 apart and the same tree --
//       gives the doubled AUROC numerator (int64), the average-precision sum (float64) and the arg-max of F1 (value, then lowest
//       index).
#include "../../include/mtadgat.h"      // mtadgat_eval_runs: the labelled segments
#include "mtadgat_scan.h"

namespace mtadgat {

constexpr int SORT_ITEMS = 8;                    // 64-item rounds per wave and tile
constexpr int SORT_TILE = 256 * SORT_ITEMS;      // 4 waves, each with SORT_ITEMS * 64 consecutive items
constexpr int SCAN_BLOCK = 4096;                 // table entries per block of the scan: 256 lanes x 16
constexpr int SORT_LEVEL2 = SCAN_BLOCK / 256;    // tiles up to which one block scans the whole (digit, tile) table
constexpr int RED_L = 4096;                      // tie groups per block of the reduction: 256 lanes x 16
constexpr unsigned NAN_KEY = 0xffffffffu;
constexpr long NO_GROUP = 0x7fffffffffffffffL;

__host__ __device__ inline unsigned order_key(float v, int descending) {
    if (v != v) return NAN_KEY;
    const unsigned u = float_order_bits(v == 0.f ? 0.f : v);
    return descending ? ~u : u;
}
// the float32 behind a descending key (not for NAN_KEY)
__device__ __forceinline__ float key_value(unsigned k) { return float_from_order_bits(~k); }

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
    span_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
    for (long b = blockIdx.y; b < nb; b += gridDim.y) {
        const long r0 = s + b * SPAN_RB;
        const int rows = e - r0 < SPAN_RB ? (int)(e - r0) : SPAN_RB;
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
    span_bounds(start, end, k, n, s, e);
    const long nb = (e - s + SPAN_RB - 1) / SPAN_RB;
    const long slot0 = span_slot0(s, k);
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
    span_bounds(start, end, k, n, s, e);
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
    span_bounds(start, end, k, n, s, e);
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
    span_bounds(start, end, k, n, s, e);
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
    ChunkRank pos, end;
    chunk_rank2((long)blockIdx.x * CHUNK_L, [&](long j) { return j < n && it.positive(j); }, [&](long j) { return j < n && it.group_end(j, n); },
                smp, sme, pos, end);
    if (threadIdx.x == 0) {
        Tp[blockIdx.x] = pos.total;
        Te[blockIdx.x] = end.total;
    }
}

// thresholds / tp / fp of every numeric tie group, at the group's rank
__global__ void __launch_bounds__(256) k_curve_emit(CurveItems it, long n, const unsigned* __restrict__ Cp, const unsigned* __restrict__ Ce,
                                                     float* __restrict__ thresholds, long* __restrict__ tp, long* __restrict__ fp) {
    __shared__ unsigned smp[4], sme[4];
    const long base = (long)blockIdx.x * CHUNK_L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ChunkRank pos, end;
    chunk_rank2(base, [&](long j) { return j < n && it.positive(j); }, [&](long j) { return j < n && it.group_end(j, n); }, smp, sme, pos, end);
    const long pos0 = Cp[blockIdx.x], rank0 = Ce[blockIdx.x];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long j = base + wave * 256 + r * 64 + lane;
        if (end.set[r]) {
            const long g = rank0 + rank_before(end, r);
            const long t = pos0 + rank_upto(pos, r);            // the positives up to and including this item
            if (g < n) {                         // always: at most n groups
                thresholds[g] = key_value((unsigned)it.keys[j]);
                tp[g] = t;
                fp[g] = j + 1 - t;
            }
        }
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

long tiles_of(int64_t n) { return (long)((n + SORT_TILE - 1) / SORT_TILE); }
long scan_blocks(long m) { return (m + SCAN_BLOCK - 1) / SCAN_BLOCK; }

struct SortBuffers {
    unsigned long long* keys[2];
    unsigned* pay[2];
    unsigned* cnt;
    unsigned* sums;
};
SortBuffers sort_scratch(ScratchCarver& c, int64_t n) {
    const size_t table = 256 * (size_t)tiles_of(n);
    SortBuffers b;
    b.keys[0] = c.take<unsigned long long>(n);
    b.keys[1] = c.take<unsigned long long>(n);
    b.pay[0] = c.take<unsigned>(n);
    b.pay[1] = c.take<unsigned>(n);
    b.cnt = c.take<unsigned>(table);
    b.sums = c.take<unsigned>(scan_blocks((long)table));
    return b;
}

// exclusive scan of a[0 .. m) in place; sums holds scan_blocks(m) entries; *total (device, may be null) = the sum.  One block
// scans alone unless the total is wanted: the carry kernel is the one that leaves it.
void scan_in_place(unsigned* a, long m, unsigned* sums, hipStream_t s, long* total = nullptr) {
    const long nb = scan_blocks(m);
    if (nb <= 1 && !total) {
        hipLaunchKernelGGL(k_scan_apply, dim3(1), dim3(256), 0, s, a, m, (const unsigned*)nullptr);
        return;
    }
    hipLaunchKernelGGL(k_scan_sum, dim3((unsigned)nb), dim3(256), 0, s, (const unsigned*)a, m, sums);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, (const unsigned*)sums, (const long*)nullptr, nb, sums, total);
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

struct CurveScratch {
    long* totals;                // positives, G, labelled samples
    long* summary;
    unsigned *Tp, *Te;
    CurvePart* parts;
    SortBuffers sort;
    float* adjusted;             // from here on: with an adjustment only
    char* runs;
    size_t runs_bytes;
    long *seg_start, *seg_end;
    float* pmax;
    unsigned* pcnt;
    float* seg_max;
    unsigned *seg_numbers, *seg_off, *seg_sums;
    long nchunks, nparts, max_seg;
};
CurveScratch curve_scratch(ScratchCarver& c, int64_t n, int adjust) {
    CurveScratch l = {};
    l.nchunks = (long)((n + CHUNK_L - 1) / CHUNK_L);
    l.nparts = (long)((n + RED_L - 1) / RED_L);
    l.max_seg = (long)((n + 1) / 2);
    l.totals = c.take<long>(4);
    l.summary = c.take<long>(12);
    l.Tp = c.take<unsigned>(l.nchunks);
    l.Te = c.take<unsigned>(l.nchunks);
    l.parts = c.take<CurvePart>(l.nparts);
    l.sort = sort_scratch(c, n);
    if (adjust) {
        const size_t slots = span_slots(n, l.max_seg);
        l.runs_bytes = mtadgat_eval_runs_scratch(n);
        l.adjusted = c.take<float>(n);
        l.runs = c.take<char>(l.runs_bytes);
        l.seg_start = c.take<long>(l.max_seg);
        l.seg_end = c.take<long>(l.max_seg);
        l.pmax = c.take<float>(slots);
        l.pcnt = c.take<unsigned>(slots);
        l.seg_max = c.take<float>(l.max_seg);
        l.seg_numbers = c.take<unsigned>(l.max_seg);
        l.seg_off = c.take<unsigned>(l.max_seg);
        l.seg_sums = c.take<unsigned>(scan_blocks(l.max_seg));
    }
    return l;
}

}  // namespace

extern "C" {

uint32_t mtadgat_eval_order_key(float value, int descending) { return order_key(value, descending); }
int mtadgat_eval_sort_tile(void) { return SORT_TILE; }
int mtadgat_eval_sort_scan_tiles(void) { return SORT_LEVEL2; }

size_t mtadgat_eval_score_order_scratch(int64_t n) {
    if (n < 1 || n > 2147483647LL) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { sort_scratch(c, n); });
}

int mtadgat_eval_score_order(const float* score_dev, int64_t n, int descending, void* scratch_dev, size_t scratch_bytes, int64_t* order_dev,
                             void* stream) {
    if (!score_dev || !scratch_dev || !order_dev) return record_error(-1, "score_order: null pointer");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "score_order: n must lie in [1, 2^31 - 1]");
    ScratchCarver carver(scratch_dev);
    const SortBuffers b = sort_scratch(carver, n);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "score_order: scratch too small (see mtadgat_eval_score_order_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "score_order: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_order_keys, dim3(grid), dim3(256), 0, s, score_dev, (const unsigned char*)nullptr, (long)n, descending ? 1 : 0, b.keys[0],
                       b.pay[0]);
    const int at = radix_sort(b, (long)n, 32, s);
    hipLaunchKernelGGL(k_order_out, dim3(grid), dim3(256), 0, s, (const unsigned*)b.pay[at], (long)n, reinterpret_cast<long*>(order_dev));
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "score_order: kernel launch failed");
}

size_t mtadgat_eval_curve_scratch(int64_t n, int adjust) {
    if (n < 1 || n > 2147483647LL || adjust < 0 || adjust > 2) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { curve_scratch(c, n, adjust); });
}

int mtadgat_eval_curve(const float* score_dev, const unsigned char* label_dev, int64_t n, int adjust, int k_percent, void* scratch_dev,
                       size_t scratch_bytes, float* thresholds_dev, int64_t* tp_dev, int64_t* fp_dev, int64_t* summary_host, void* stream) {
    if (!score_dev || !label_dev || !scratch_dev || !thresholds_dev || !tp_dev || !fp_dev || !summary_host)
        return record_error(-1, "curve: null pointer");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "curve: n must lie in [1, 2^31 - 1]");
    if (adjust < 0 || adjust > 2) return record_error(-1, "curve: adjust must be 0 (none), 1 (point) or 2 (PA%K)");
    if (adjust == 2 && (k_percent < 0 || k_percent > 100)) return record_error(-1, "curve: K must lie in [0, 100]");
    ScratchCarver carver(scratch_dev);
    const CurveScratch l = curve_scratch(carver, n, adjust);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "curve: scratch too small (see mtadgat_eval_curve_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "curve: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const SortBuffers& b = l.sort;
    const float* ranked = score_dev;

    if (adjust) {
        int64_t count = 0;
        const int rc = mtadgat_eval_runs(nullptr, label_dev, n, 0.0, 0, 0, 1, l.max_seg, l.runs, l.runs_bytes,
                                         reinterpret_cast<int64_t*>(l.seg_start), reinterpret_cast<int64_t*>(l.seg_end), &count, stream);
        if (rc != 0) return rc;
        if (hipMemcpyAsync(l.adjusted, score_dev, 4 * (size_t)n, hipMemcpyDeviceToDevice, s) != hipSuccess) return record_error(-3, "curve: copy failed");
        if (count > 0) {
            const dim3 by_rows((unsigned)count, (unsigned)span_slices(n, count, SPAN_RB)), by_items((unsigned)count, (unsigned)span_slices(n, count, 256));
            const unsigned waves = (unsigned)((count + 3) / 4);
            hipLaunchKernelGGL(k_seg_part, by_rows, dim3(256), 0, s, score_dev, (long)n, (const long*)l.seg_start, (const long*)l.seg_end, l.pmax, l.pcnt);
            hipLaunchKernelGGL(k_seg_final, dim3(waves), dim3(256), 0, s, (long)n, (const long*)l.seg_start, (const long*)l.seg_end, (long)count,
                               (const float*)l.pmax, (const unsigned*)l.pcnt, l.seg_max, l.seg_numbers, l.seg_off);
            const float* seg_value = l.seg_max;
            if (adjust == 2) {
                // spans: the exclusive scan of the segment lengths; every labelled sample lies in one segment, so they fill [0, labelled)
                int64_t labelled = 0;
                scan_in_place(l.seg_off, (long)count, l.seg_sums, s, l.totals + 2);
                if (hipMemcpyAsync(&labelled, l.totals + 2, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipStreamSynchronize(s) != hipSuccess)
                    return record_error(-3, "curve: stream failed");
                if (labelled < 1 || labelled > n) return record_error(-3, "curve: the segments do not match the labels");
                hipLaunchKernelGGL(k_seg_keys, by_items, dim3(256), 0, s, score_dev, (long)n, (const long*)l.seg_start, (const long*)l.seg_end,
                                   (const unsigned*)l.seg_off, b.keys[0], b.pay[0]);
                int seg_bits = 0;
                while (seg_bits < 31 && ((int64_t)1 << seg_bits) < count) ++seg_bits;
                const int at = radix_sort(b, (long)labelled, 32 + seg_bits, s);
                hipLaunchKernelGGL(k_seg_kth, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, (long)n, (const long*)l.seg_start,
                                   (const long*)l.seg_end, (long)count, k_percent, (const unsigned*)l.seg_off, (const unsigned*)l.seg_numbers,
                                   (const unsigned long long*)b.keys[at], l.seg_max);
            }
            hipLaunchKernelGGL(k_seg_broadcast, by_items, dim3(256), 0, s, score_dev, (long)n, (const long*)l.seg_start, (const long*)l.seg_end, seg_value,
                               adjust == 1 ? 1 : 0, l.adjusted);
        }
        ranked = l.adjusted;
    }

    hipLaunchKernelGGL(k_order_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ranked, label_dev, (long)n, 1, b.keys[0], b.pay[0]);
    const int at = radix_sort(b, (long)n, 32, s);
    const CurveItems items{b.keys[at], b.pay[at]};
    hipLaunchKernelGGL(k_curve_count, dim3((unsigned)l.nchunks), dim3(256), 0, s, items, (long)n, l.Tp, l.Te);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, (const unsigned*)l.Tp, (const long*)nullptr, l.nchunks, l.Tp, l.totals);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, (const unsigned*)l.Te, (const long*)nullptr, l.nchunks, l.Te, l.totals + 1);
    hipLaunchKernelGGL(k_curve_emit, dim3((unsigned)l.nchunks), dim3(256), 0, s, items, (long)n, (const unsigned*)l.Tp, (const unsigned*)l.Te,
                       thresholds_dev, reinterpret_cast<long*>(tp_dev), reinterpret_cast<long*>(fp_dev));
    hipLaunchKernelGGL(k_curve_reduce, dim3((unsigned)l.nparts), dim3(256), 0, s, reinterpret_cast<const long*>(tp_dev),
                       reinterpret_cast<const long*>(fp_dev), (long)n, (const long*)l.totals, l.parts);
    hipLaunchKernelGGL(k_curve_final, dim3(1), dim3(256), 0, s, (const float*)thresholds_dev, reinterpret_cast<const long*>(tp_dev),
                       reinterpret_cast<const long*>(fp_dev), (long)n, (const long*)l.totals, (const CurvePart*)l.parts, l.summary);
    if (hipGetLastError() != hipSuccess) return record_error(-3, "curve: kernel launch failed");
    if (hipMemcpyAsync(summary_host, l.summary, 12 * sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) return record_error(-3, "curve: copy failed");
    if (hipStreamSynchronize(s) != hipSuccess) return record_error(-3, "curve: stream failed");
    return 0;
}

}  // extern "C"
