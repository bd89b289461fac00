// Scan, rank and layout primitives of the evaluation kernels (mtadgat_events.hip, mtadgat_curves.hip, mtadgat_evalcol.hip): what
// at least two of their kernels or entry points share.  Everything is an integer operation in a fixed order -- no atomics --
// so a result is a function of the input alone.
//
//   blocked scan of counts: per-chunk totals (chunk_rank), one wave that turns the totals into the chunks' starting ranks in
//       chunk order (k_scan_carry), and a pass that recomputes the predicate and places every item at start + rank inside the
//       chunk (chunk_rank again).  Within a wave the rank is the population count of the __ballot mask below the lane.
//   spans: runs or segments [start, end) that are disjoint and ascending, reduced in fixed row blocks with one slot per block.
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
