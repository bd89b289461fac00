// Scan, rank, reduction and layout primitives of the evaluation kernels (mtadgat_eval.hip, mtadgat_evalcol.hip, mtadgat_evalmask.hip,
// mtadgat_events.hip, mtadgat_curves.hip, mtadgat_parts.hip): what at least two of their kernels or entry points share.  The
// primitives here run in a fixed order -- no atomics -- so what they return is a function of the input alone.  Two callers do not
// keep that up to their result: k_eval_moments and k_eval_epsilon (mtadgat_eval.hip) add their per-workgroup sums with float64
// atomicAdd, in whatever order the workgroups finish (evaluation._choose_epsilon carries a 1e-9 margin for it).
//
//   blocked scan of counts: per-chunk totals (chunk_rank), one wave that turns the totals into the chunks' starting ranks in
//       chunk order (k_scan_carry), and a pass that recomputes the predicate and places every item at start + rank inside the
//       chunk (chunk_rank again).  Within a wave the rank is the population count of the __ballot mask below the lane.
//   block_sum: the float64 sum over a 256-thread workgroup by a fixed tree.
//   spans: runs or segments [start, end) that are disjoint and ascending, reduced in fixed row blocks with one slot per block.
//   epsilon_tile: find_epsilon's four sums for a tile of SPAN_RB rows under one threshold, the dilation from ballot words in LDS --
//       the body of both k_eval_epsilon (mtadgat_eval.hip: a column, the tiles walked grid-stride) and k_part_epsilon
//       (mtadgat_parts.hip: a span, one slot per tile).
//   ScratchCarver: one description of a scratch layout for the size query and for the call.
#ifndef MTADGAT_SCAN_H
#define MTADGAT_SCAN_H
#include "mtadgat_device.h"

namespace mtadgat {

constexpr int CHUNK_L = 1024;    // items per chunk of the rank scans: 4 waves x 4 rounds x 64 lanes
constexpr int SPAN_RB = 1024;    // rows per block of the span reductions

// ---- float32 <-> unsigned of the same order ----------------------------------------------------------------------------------------
// Negative: all bits flipped; non-negative: sign bit set.  As the bits stand, -0.0 sorts just below +0.0 and a NaN beyond the
// infinity of its sign.  The callers differ ON PURPOSE in what they put on top and are not to be merged: the column quantiles
// (colq_key) take the bits as they are -- a NaN only has to be counted, the column's result is NaN anyway; the top-column ranking
// (rank_key) reads -0 as +0 and puts NaN below every number; the score order (order_key) reads -0 as +0 and gives every NaN the
// one key 0xffffffff, last in both directions.
__host__ __device__ inline unsigned float_order_bits(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float float_from_order_bits(unsigned k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- sums over a wave and a workgroup ----------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned wave_inclusive_sum(unsigned v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// the sum of `mine` over the lower threads of a 256-thread workgroup, and over all of them; sm: 4 entries (barriers inside)
__device__ __forceinline__ unsigned block_exclusive(unsigned mine, unsigned* sm, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned s = wave_inclusive_sum(mine);
    if (lane == 63) sm[wave] = s;
    __syncthreads();
    unsigned before = 0u;
    for (int w = 0; w < wave; ++w) before += sm[w];
    total = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return before + s - mine;
}

// the sum of v over a 256-thread workgroup by a fixed tree; sm: 256 doubles (barriers inside)
__device__ __forceinline__ double block_sum(double v, double* sm) {
    const int tid = threadIdx.x;
    sm[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sm[tid] += sm[tid + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// C[i] = T[0] + .. + T[i - 1] (C may be T), 64 entries per step of one wave in entry order; *total (may be null) = the sum.
// The number of entries: the chunks of *items when the item count was left on the device by an earlier stage, else `entries`.
static __global__ void __launch_bounds__(64) k_scan_carry(const unsigned* T, const long* __restrict__ items, long entries, unsigned* C,
                                                          long* __restrict__ total) {
    if (items) entries = (*items + CHUNK_L - 1) / CHUNK_L;
    const int lane = threadIdx.x;
    unsigned run = 0u;
    for (long base = 0; base < entries; base += 64) {
        const long i = base + lane;
        const unsigned mine = i < entries ? T[i] : 0u;
        const unsigned s = wave_inclusive_sum(mine);
        if (i < entries) C[i] = run + s - mine;
        run += __shfl(s, 63);
    }
    if (total && lane == 0) *total = (long)run;
}

// ---- ranks inside a chunk ------------------------------------------------------------------------------------------------------------
// A 256-thread workgroup over the CHUNK_L items from `base`: wave w, round r, lane l looks at item base + 256 w + 64 r + l.
struct ChunkRank {
    bool set[4];                 // the predicate of this lane's item in each of the wave's rounds
    unsigned long long mask[4];  // and its ballot over the wave
    unsigned before[4];          // items of the chunk with the predicate set ahead of that round
    unsigned total;              // all of them
};
// the ballots, and the wave's count into sm[wave]; a barrier, then chunk_prefix
template <class Pred>
__device__ __forceinline__ void chunk_ballot(long base, Pred pred, ChunkRank& k, unsigned* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned c = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        k.set[r] = pred(base + wave * 256 + r * 64 + lane);
        k.mask[r] = __ballot(k.set[r]);
        c += (unsigned)__popcll(k.mask[r]);
    }
    if (lane == 0) sm[wave] = c;
}
__device__ __forceinline__ void chunk_prefix(ChunkRank& k, const unsigned* sm) {
    const int wave = threadIdx.x >> 6;
    unsigned at = 0u;
    for (int w = 0; w < wave; ++w) at += sm[w];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        k.before[r] = at;
        at += (unsigned)__popcll(k.mask[r]);
    }
    k.total = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
// one predicate, or two side by side behind the same barrier; sm: 4 entries each.  Every thread of the workgroup calls it.
template <class Pred>
__device__ __forceinline__ ChunkRank chunk_rank(long base, Pred pred, unsigned* sm) {
    ChunkRank k;
    chunk_ballot(base, pred, k, sm);
    __syncthreads();
    chunk_prefix(k, sm);
    return k;
}
template <class PredA, class PredB>
__device__ __forceinline__ void chunk_rank2(long base, PredA pa, PredB pb, unsigned* sma, unsigned* smb, ChunkRank& a, ChunkRank& b) {
    chunk_ballot(base, pa, a, sma);
    chunk_ballot(base, pb, b, smb);
    __syncthreads();
    chunk_prefix(a, sma);
    chunk_prefix(b, smb);
}
// rank of this lane's item of round r among the set items of the chunk: those ahead of it, or those up to and including it
__device__ __forceinline__ unsigned rank_before(const ChunkRank& k, int r) {
    return k.before[r] + (unsigned)__popcll(k.mask[r] & ((1ull << (threadIdx.x & 63)) - 1ull));
}
__device__ __forceinline__ unsigned rank_upto(const ChunkRank& k, int r) {
    return k.before[r] + (unsigned)__popcll(k.mask[r] & ((2ull << (threadIdx.x & 63)) - 1ull));
}

// ---- spans -------------------------------------------------------------------------------------------------------------------------
// span k cut to [0, n]; an empty or inverted span has length 0
__device__ __forceinline__ void span_bounds(const long* __restrict__ start, const long* __restrict__ end, long k, long n, long& s, long& e) {
    s = start[k];
    e = end[k];
    if (s < 0) s = 0;
    if (e > n) e = n;
    if (e < s) e = s;
}
// the span of index i (0 <= i < n): the first span whose end lies beyond i, if it starts at or before i; -1: no span covers i.
// s: that span's start cut to 0.
__device__ __forceinline__ long span_find(const long* __restrict__ start, const long* __restrict__ end, long count, long i, long& s) {
    long lo = 0, hi = count;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (end[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= count) return -1;
    s = start[lo] < 0 ? 0 : start[lo];
    return s <= i ? lo : -1;
}
// slot of row block b of span k: spans are disjoint and ascending, so floor(s / SPAN_RB) + k + b is different for every (k, b)
// and stays below n / SPAN_RB + count + 1
__device__ __forceinline__ long span_slot0(long s, long k) { return s / SPAN_RB + k; }
inline size_t span_slots(int64_t n, int64_t count) { return (size_t)(n / SPAN_RB) + (size_t)count + 2; }

// slices per span of a (span, slice) grid, a slice taking per_slice samples at a time: enough workgroups for a few long spans, few
// idle ones for many short spans; the results do not depend on it
inline long span_slices(int64_t n, int64_t count, long per_slice) {
    const long most = (long)((n + per_slice - 1) / per_slice);
    long slices = 8192 / count;
    slices = slices < 4 ? 4 : (slices > 1024 ? 1024 : slices);
    return slices > most ? most : slices;
}

// ---- find_epsilon's z table, one tile ------------------------------------------------------------------------------------------------
constexpr int EPS_HALO_MAX = 128;                                    // widest dilation halo staged in LDS
constexpr int EPS_TILE_WORDS = (SPAN_RB + 2 * EPS_HALO_MAX) / 64;    // `hot` of epsilon_tile: 64-bit words

// Rows [r0, r0 + rows) (rows <= SPAN_RB) of the range [lo, hi) of an array with row stride ld, under the threshold ez.  Added to this
// thread's partial sums, rows r = tid, tid + 256, ... in that order:
//   a += x, q += x^2, cnt += 1 where x < ez;  dil += 1 where some |j| <= halo with lo <= row + j < hi has x[row + j] >= ez
// The tile's rows and their halo, cut to [lo, hi), are staged once in `hot` as the flags x >= ez, one bit each (a wave's __ballot is a
// 64-bit word of them: bit t is sample r0 - halo + t), so a row's window of 2 halo + 1 flags is at most five masked words.  A halo
// beyond EPS_HALO_MAX reads the window from memory.  Every thread of a 256-thread workgroup calls it (one barrier inside); the caller
// puts a barrier between a tile's reads of `hot` and the next call.
__device__ __forceinline__ void epsilon_tile(const float* __restrict__ x, long ld, long lo, long hi, long r0, int rows, double ez, int halo,
                                             unsigned long long* hot, double& a, double& q, double& cnt, double& dil) {
    const int tid = threadIdx.x, lane = threadIdx.x & 63;
    const bool staged = halo <= EPS_HALO_MAX;
    if (staged) {
        for (int t0 = tid - lane; t0 < rows + 2 * halo; t0 += 256) {         // wave-uniform
            const long at = r0 - halo + t0 + lane;
            const unsigned long long m = __ballot(at >= lo && at < hi && (double)x[at * ld] >= ez);
            if (lane == 0) hot[t0 >> 6] = m;
        }
    }
    __syncthreads();
    for (int r = tid; r < rows; r += 256) {
        const double v = (double)x[(r0 + r) * ld];
        if (v < ez) { a += v; q += v * v; cnt += 1.0; }
        bool any = false;
        if (staged) {
            const int b0 = r, b1 = r + 2 * halo;                              // the window of row r, in tile bits
            for (int w = b0 >> 6; w <= b1 >> 6; ++w) {
                unsigned long long mask = ~0ull;
                if (w == b0 >> 6) mask &= ~0ull << (b0 & 63);
                if (w == b1 >> 6) mask &= ~0ull >> (63 - (b1 & 63));
                any = any || (hot[w] & mask) != 0ull;
            }
        } else {
            const long k0 = r0 + r - halo < lo ? lo : r0 + r - halo, k1 = r0 + r + halo >= hi ? hi - 1 : r0 + r + halo;
            for (long k = k0; k <= k1; ++k) any = any || ((double)x[k * ld] >= ez);
        }
        dil += any ? 1.0 : 0.0;
    }
}

// ---- scratch layouts ---------------------------------------------------------------------------------------------------------------
// A layout is a function that takes its regions from a carver in order.  Run over a null base it gives the bytes to ask for,
// run over the caller's pointer the typed pointers: the size of a scratch query and the pointers carved from it cannot drift.
// A region starts at a multiple of `align` bytes and its size is rounded up to one.
class ScratchCarver {
public:
    explicit ScratchCarver(void* base) : base_(static_cast<char*>(base)) {}
    template <class T>
    T* take(size_t count, size_t align = 8) {
        at_ = round_up(at_, align);
        T* p = base_ ? reinterpret_cast<T*>(base_ + at_) : nullptr;
        at_ += round_up(sizeof(T) * count, align);
        return p;
    }
    size_t bytes() const { return at_; }

private:
    static size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
    char* base_;
    size_t at_ = 0;
};
// the bytes a layout takes
template <class Layout>
size_t scratch_bytes_of(Layout layout) {
    ScratchCarver c(nullptr);
    layout(c);
    return c.bytes();
}

}  // namespace mtadgat
#endif  // MTADGAT_SCAN_H
