// The window sampler of the series trainer (mtadgat_fit_windows; fitting.training_windows): the starts s in [0, n_rows - W) whose
// rows s .. s + W lie in one part of a concatenated series, whose target row s + W has an observed sample among the compared columns
// and whose rows s .. s + W - 1 hold at least min_count observed samples.  A sample is observed iff age <= max_age, `age` as the
// preparation reports it.  tests/fit_mask_refs.py is the specification.
//
//   k_fitwin_rows    one wave per row (grid-stride): lanes over the row's columns, __ballot / popcount.  Per row one word: the count
//                    of observed samples over all F columns (<= 2048) and, in bit 31, whether one of the columns `dims` is observed.
//   k_fitwin_sums    per chunk of CHUNK_L rows the sum of the counts (<= 2^21: unsigned).
//   k_fitwin_carry   one wave: the chunks' starting sums in chunk order, int64 (the whole series may hold 2^42 samples).
//   k_fitwin_scan    E[r] = the observed samples of rows 0 .. r - 1, int64: window s holds E[s + W] - E[s].
//   k_fitwin_count, k_scan_carry, k_fitwin_emit
//                    the stream compaction of mtadgat_scan.h over the predicate; the part of a start is a binary search in the
//                    offsets (span_find), so no launch depends on the number of parts.
// All integer arithmetic, no atomics: identical calls give identical bits.
#include <algorithm>

#include "../../include/mtadgat.h"      // the entry points' declarations
#include "mtadgat_scan.h"

using namespace mtadgat;

namespace {

constexpr int64_t N_MAX = 2147483647LL;
constexpr int WIN_W_MAX = 512;             // the limits of mtadgat_fit_gather
constexpr int WIN_F_MAX = 2048;
constexpr unsigned WIN_GRID_MAX = 1u << 16;  // workgroups of the grid-stride row kernel
constexpr unsigned TARGET_BIT = 0x80000000u;

// grid-stride: four waves, a row each
__global__ void __launch_bounds__(256) k_fitwin_rows(const int* __restrict__ age, long ld, int max_age, long n_rows, int F,
                                                     const int* __restrict__ dims, int out, unsigned* __restrict__ rowcnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long r = (long)blockIdx.x * 4 + wave; r < n_rows; r += (long)gridDim.x * 4) {      // (wave-uniform)
        unsigned cnt = (unsigned)F;
        bool target = true;
        if (age) {
            const int* a = age + r * ld;
            cnt = 0u;
            for (int c0 = 0; c0 < F; c0 += 64) {
                const int c = c0 + lane;
                cnt += (unsigned)__popcll(__ballot(c < F && a[c] <= max_age));
            }
            target = false;
            for (int d0 = 0; d0 < out; d0 += 64) {
                const int d = d0 + lane;
                target = target || __ballot(d < out && a[dims ? dims[d] : d] <= max_age) != 0ull;
            }
        }
        if (lane == 0) rowcnt[r] = cnt | (target ? TARGET_BIT : 0u);
    }
}

// this thread's four consecutive rows of the chunk from `base`: their counts, and the sum
__device__ __forceinline__ unsigned four_counts(const unsigned* __restrict__ rowcnt, long base, long n_rows, unsigned v[4]) {
    unsigned sum = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long r = base + 4 * threadIdx.x + j;
        v[j] = r < n_rows ? (rowcnt[r] & ~TARGET_BIT) : 0u;
        sum += v[j];
    }
    return sum;
}

// grid: chunks of CHUNK_L rows
__global__ void __launch_bounds__(256) k_fitwin_sums(const unsigned* __restrict__ rowcnt, long n_rows, unsigned* __restrict__ T) {
    __shared__ unsigned sm[4];
    unsigned v[4], total;
    block_exclusive(four_counts(rowcnt, (long)blockIdx.x * CHUNK_L, n_rows, v), sm, total);
    if (threadIdx.x == 0) T[blockIdx.x] = total;
}

// one wave: C[i] = T[0] + .. + T[i - 1] in int64
__global__ void __launch_bounds__(64) k_fitwin_carry(const unsigned* __restrict__ T, long entries, long* __restrict__ C) {
    const int lane = threadIdx.x;
    long run = 0;
    for (long base = 0; base < entries; base += 64) {
        const long i = base + lane;
        const unsigned mine = i < entries ? T[i] : 0u;
        const unsigned s = wave_inclusive_sum(mine);                     // (64 chunks of at most 2^21: no overflow)
        if (i < entries) C[i] = run + (long)(s - mine);
        run += (long)__shfl(s, 63);
    }
}

// grid: chunks of CHUNK_L rows
__global__ void __launch_bounds__(256) k_fitwin_scan(const unsigned* __restrict__ rowcnt, long n_rows, const long* __restrict__ C,
                                                     long* __restrict__ E) {
    __shared__ unsigned sm[4];
    const long base = (long)blockIdx.x * CHUNK_L;
    unsigned v[4], total;
    const unsigned mine = four_counts(rowcnt, base, n_rows, v);
    long at = C[blockIdx.x] + (long)block_exclusive(mine, sm, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long r = base + 4 * threadIdx.x + j;
        if (r < n_rows) E[r] = at;
        at += (long)v[j];
    }
}

// the three rules of a start; n = n_rows - W starts, so row s + W exists for every one of them
struct WinPred {
    const unsigned* rowcnt;
    const long* E;
    const long* off;         // parts + 1 offsets, or null: one part
    long parts, n, min_count;
    int W;
    __device__ bool operator()(long s) const {
        if (s >= n) return false;
        if (!(rowcnt[s + W] & TARGET_BIT)) return false;
        if (E[s + W] - E[s] < min_count) return false;
        if (off) {
            long first;
            const long p = span_find(off, off + 1, parts, s, first);
            if (p < 0 || s + W >= off[p + 1]) return false;
        }
        return true;
    }
};

// grid: chunks of CHUNK_L starts
__global__ void __launch_bounds__(256) k_fitwin_count(WinPred pred, unsigned* __restrict__ T) {
    __shared__ unsigned sm[4];
    const ChunkRank k = chunk_rank((long)blockIdx.x * CHUNK_L, pred, sm);
    if (threadIdx.x == 0) T[blockIdx.x] = k.total;
}

__global__ void __launch_bounds__(256) k_fitwin_emit(WinPred pred, const unsigned* __restrict__ C, long* __restrict__ starts) {
    __shared__ unsigned sm[4];
    const long base = (long)blockIdx.x * CHUNK_L;
    const ChunkRank k = chunk_rank(base, pred, sm);
    const long rank0 = C[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (k.set[r]) starts[rank0 + rank_before(k, r)] = base + wave * 256 + r * 64 + lane;
}

struct WinScratch {
    unsigned* rowcnt;    // (n_rows)
    long* E;             // (n_rows)
    long* rowC;          // (chunks): the row chunks' starting sums
    unsigned* T;         // (chunks): the row chunks' sums, then the start chunks' counts
    unsigned* C;         // (chunks): the start chunks' starting ranks
    long chunks;
};
WinScratch win_scratch(ScratchCarver& c, int64_t n_rows) {
    WinScratch l;
    l.chunks = (long)((n_rows + CHUNK_L - 1) / CHUNK_L);
    l.E = c.take<long>((size_t)n_rows);
    l.rowC = c.take<long>((size_t)l.chunks);
    l.rowcnt = c.take<unsigned>((size_t)n_rows);
    l.T = c.take<unsigned>((size_t)l.chunks);
    l.C = c.take<unsigned>((size_t)l.chunks);
    return l;
}

}  // namespace

extern "C" {

size_t mtadgat_fit_windows_scratch(int64_t n_rows) {
    if (n_rows < 1 || n_rows > N_MAX) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { win_scratch(c, n_rows); });
}

int mtadgat_fit_windows(const int32_t* age_dev, int64_t ld_age, int32_t max_age, int64_t n_rows, int F, int W, const int32_t* dims_dev,
                        int out_dim, const int64_t* part_offsets_dev, int64_t parts, int64_t min_count, int64_t* starts_dev,
                        int64_t* count_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    if (!starts_dev || !count_dev || !scratch_dev) return record_error(-1, "fit_windows: null pointer");
    if (W < 1 || W > WIN_W_MAX) return record_error(-1, "fit_windows: W must lie in [1, 512]");
    if (F < 1 || F > WIN_F_MAX) return record_error(-1, "fit_windows: F must lie in [1, 2048]");
    if (age_dev && ld_age < F) return record_error(-1, "fit_windows: ld_age < F");
    if (n_rows < (int64_t)W || n_rows > N_MAX) return record_error(-1, "fit_windows: n_rows must lie in [W, 2^31 - 1]");
    if (out_dim < 1 || out_dim > WIN_F_MAX) return record_error(-1, "fit_windows: out_dim must lie in [1, 2048]");
    if (!dims_dev && out_dim > F) return record_error(-1, "fit_windows: out_dim > F needs dims_dev");
    if (part_offsets_dev && (parts < 1 || parts > N_MAX)) return record_error(-1, "fit_windows: parts must lie in [1, 2^31 - 1]");
    if (min_count < 0) return record_error(-1, "fit_windows: min_count must be >= 0");
    if (scratch_bytes < mtadgat_fit_windows_scratch(n_rows)) return record_error(-5, "fit_windows: scratch too small (see mtadgat_fit_windows_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "fit_windows: scratch must be 8-byte aligned");
    ScratchCarver carver(scratch_dev);
    const WinScratch l = win_scratch(carver, n_rows);
    hipStream_t s = (hipStream_t)stream;
    const long rows = (long)n_rows, n = rows - W;
    const long start_chunks = (n + CHUNK_L - 1) / CHUNK_L;               // (0 when the series is one window long: no start)
    const unsigned row_grid = (unsigned)std::min<long>((rows + 3) / 4, WIN_GRID_MAX);
    hipLaunchKernelGGL(k_fitwin_rows, dim3(row_grid), dim3(256), 0, s, age_dev, (long)ld_age, (int)max_age, rows, F, dims_dev, out_dim, l.rowcnt);
    hipLaunchKernelGGL(k_fitwin_sums, dim3((unsigned)l.chunks), dim3(256), 0, s, (const unsigned*)l.rowcnt, rows, l.T);
    hipLaunchKernelGGL(k_fitwin_carry, dim3(1), dim3(64), 0, s, (const unsigned*)l.T, l.chunks, l.rowC);
    hipLaunchKernelGGL(k_fitwin_scan, dim3((unsigned)l.chunks), dim3(256), 0, s, (const unsigned*)l.rowcnt, rows, (const long*)l.rowC, l.E);
    WinPred pred;
    pred.rowcnt = l.rowcnt;
    pred.E = l.E;
    pred.off = reinterpret_cast<const long*>(part_offsets_dev);
    pred.parts = (long)parts;
    pred.n = n;
    pred.min_count = (long)min_count;
    pred.W = W;
    if (start_chunks > 0) hipLaunchKernelGGL(k_fitwin_count, dim3((unsigned)start_chunks), dim3(256), 0, s, pred, l.T);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(64), 0, s, (const unsigned*)l.T, (const long*)nullptr, start_chunks, l.C,
                       reinterpret_cast<long*>(count_dev));
    if (start_chunks > 0)
        hipLaunchKernelGGL(k_fitwin_emit, dim3((unsigned)start_chunks), dim3(256), 0, s, pred, (const unsigned*)l.C, reinterpret_cast<long*>(starts_dev));
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "fit_windows: kernel launch failed");
}

}  // extern "C"
