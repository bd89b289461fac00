// Preparing raw telemetry on the device: the per-column min-max scaler of the reference's utils.normalize_data (NaN replaced, a
// MinMaxScaler fitted on the training series and applied to both), the fill of missing samples, the inverse transform and the same
// arithmetic as per-stream state for live rows (preparation.py; entry points mtadgat_prep_*).  tests/prep_refs.py is the specification.
//
//   A gap is a sample that is not finite (NaN, +inf, -inf).  A column's record (PrepColumn = mtadgat_prep_column) holds lo, hi, the
//   float32 scale = 1 / (hi - lo) (1 where hi - lo < 10 eps32), offset = 0 - lo scale, the mean and the number of valid samples.
//   Rows are cut into fixed blocks of PREP_RB; per-(column, block) partials live in scratch as [column][block] and are combined in
//   block order: no atomics, the bits depend on the input alone.
//
//   k_prep_fit_partial / k_prep_fit_final   min, max, count and float64 sum per (column, block); one wave per column adds the blocks
//                                           in order and derives the record
//   k_prep_apply                            y = fl(fl(v scale) + offset), v = x or the zero / NaN fill of a gap: one pass
//   k_prep_tail / k_prep_carry / k_prep_resolve
//                                           the hold fill and the age as a blocked max-scan of "last valid row" down each column:
//                                           (1) per (column, block) the last valid raw VALUE, whether there is one, and the number of
//                                           trailing gap rows, counted from the last seam inside the block; (2) one wave per column
//                                           scans the blocks in order with an associative "later valid wins, a seam cuts" operator and
//                                           leaves every block its carry-in; (3) a workgroup resolves its block 64 rows at a time: the
//                                           tile goes through LDS with coalesced loads, lanes sit on rows, __ballot(valid) is the
//                                           64-row mask and the last valid row at or before a lane is 63 - clz(mask & ((2 << lane) - 1))
//                                           (the ballot idiom of chunk_rank, mtadgat_scan.h).  Values, not row indices, are carried,
//                                           so the in-place form never reads a row another block has overwritten.
//   k_prep_inverse                          x = fl(fl(y - offset) / scale), optionally through a column map
//   k_prep_stream_push / k_prep_stream_reset   one wave per stream: last valid raw value, "heard one" and age per (stream, column)
//
//   Seams: the parts are disjoint ascending spans [start, end) (mtadgat_scan.h); every span start and every span end is a seam, and a
//   fill never looks across one.  Rows that no span covers thus form stretches of their own.  Without spans the series is one part.
#include <string>

#include "../../include/mtadgat.h"      // mtadgat_prep_column
#include "mtadgat_scan.h"

// Every float32 operation of this file is rounded on its own: hipcc contracts a * b + c to an FMA by default -- through __fmul_rn /
// __fadd_rn too, which are plain operators compiled under the header's own setting -- and MinMaxScaler's bits are those of the
// separate multiply and add.  So the arithmetic below is written with operators, under this pragma.
#pragma clang fp contract(off)

namespace mtadgat {

constexpr int PREP_RB = 512;      // rows per block: 8 groups of 64 rows
constexpr int PREP_CT = 64;        // columns per tile
constexpr int PREP_PITCH = 65;     // widest LDS row pitch of a tile

struct PrepColumn {
    float lo, hi, scale, offset, mean;
    int n_valid;
};
static_assert(sizeof(PrepColumn) == sizeof(mtadgat_prep_column) && sizeof(PrepColumn) == 24, "the record of include/mtadgat.h");

enum PrepFill { PREP_FILL_NONE = 0, PREP_FILL_ZERO = 1, PREP_FILL_HOLD = 2 };
enum PrepGaps { PREP_GAPS_IGNORE = 0, PREP_GAPS_ZERO = 1 };

__device__ __forceinline__ bool prep_valid(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u; }

// y = fl(fl(v scale) + offset), optionally clipped to [0, 1] (a NaN stays)
__device__ __forceinline__ float prep_scale(float v, const PrepColumn& k, int clip) {
    const float m = v * k.scale;
    float y = m + k.offset;
    if (clip) y = y < 0.f ? 0.f : (y > 1.f ? 1.f : y);
    return y;
}

// the last seam at or before row i: the largest span start or span end <= i, 0 when there is none
__device__ __forceinline__ long prep_seam_before(const long* __restrict__ start, const long* __restrict__ end, long count, long i) {
    long best = 0;
    for (int which = 0; which < 2; ++which) {
        const long* a = which ? end : start;
        long lo = 0, hi = count;                            // the number of entries <= i
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (a[mid] <= i) lo = mid + 1;
            else hi = mid;
        }
        if (lo > 0 && a[lo - 1] > best) best = a[lo - 1];
    }
    return best;
}

// threads of a 256-thread workgroup on a tile of cw <= 64 columns: column tid % cw, rows tid / cw, tid / cw + rp, ...
struct PrepWalk {
    int c, rsub, rp;
    bool on;
};
__device__ __forceinline__ PrepWalk prep_walk(int cw) {
    PrepWalk w;
    w.rp = 256 / cw;
    w.c = threadIdx.x % cw;
    w.rsub = threadIdx.x / cw;
    w.on = w.rsub < w.rp;
    return w;
}

// ---- fit -----------------------------------------------------------------------------------------------------------------------------
// grid (row block, column tile): per (column, block) min, max and count of the samples and their float64 sum -- each thread its rows
// in ascending order, then a fixed tree over the threads of a column.  gaps = zero: a gap is the sample 0.0.
__global__ void __launch_bounds__(256) k_prep_fit_partial(const float* __restrict__ x, long n, int d, long ld, int gaps, long nb,
                                                           float* __restrict__ plo, float* __restrict__ phi, int* __restrict__ pcnt,
                                                           double* __restrict__ psum) {
    __shared__ float slo[256];
    __shared__ float shi[256];
    __shared__ int scn[256];
    __shared__ double ssm[256];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int c0 = blockIdx.y * PREP_CT;
    const int cw = d - c0 < PREP_CT ? d - c0 : PREP_CT;
    const long r0 = b * PREP_RB;
    const int rows = n - r0 < PREP_RB ? (int)(n - r0) : PREP_RB;
    const PrepWalk w = prep_walk(cw);
    float lo = INFINITY, hi = -INFINITY;
    int cnt = 0;
    double sum = 0.0;
    if (w.on) {
        for (int r = w.rsub; r < rows; r += w.rp) {
            float v = x[(r0 + r) * ld + c0 + w.c];
            bool ok = prep_valid(v);
            if (!ok && gaps == PREP_GAPS_ZERO) { v = 0.f; ok = true; }
            if (ok) {
                lo = fminf(lo, v);
                hi = fmaxf(hi, v);
                cnt += 1;
                sum += (double)v;
            }
        }
    }
    slo[tid] = lo; shi[tid] = hi; scn[tid] = cnt; ssm[tid] = sum;
    __syncthreads();
    int top = 1;
    while (top < w.rp) top <<= 1;
    for (int st = top >> 1; st > 0; st >>= 1) {
        if (w.on && w.rsub < st && w.rsub + st < w.rp) {
            const int o = tid + st * cw;
            slo[tid] = fminf(slo[tid], slo[o]);
            shi[tid] = fmaxf(shi[tid], shi[o]);
            scn[tid] += scn[o];
            ssm[tid] += ssm[o];
        }
        __syncthreads();
    }
    if (w.on && w.rsub == 0) {
        const long at = (long)(c0 + w.c) * nb + b;
        plo[at] = slo[tid]; phi[at] = shi[tid]; pcnt[at] = scn[tid]; psum[at] = ssm[tid];
    }
}

// one wave per column: min / max / count over the blocks (exact in any order), the sums added in block order, then the record
__global__ void __launch_bounds__(64) k_prep_fit_final(int d, long nb, const float* __restrict__ plo, const float* __restrict__ phi,
                                                        const int* __restrict__ pcnt, const double* __restrict__ psum,
                                                        PrepColumn* __restrict__ rec) {
    const int col = blockIdx.x, lane = threadIdx.x;
    const long at0 = (long)col * nb;
    float lo = INFINITY, hi = -INFINITY;
    long cnt = 0;
    double sum = 0.0;
    for (long base = 0; base < nb; base += 64) {
        const long b = base + lane;
        const int m = nb - base < 64 ? (int)(nb - base) : 64;
        if (b < nb) {
            lo = fminf(lo, plo[at0 + b]);
            hi = fmaxf(hi, phi[at0 + b]);
            cnt += pcnt[at0 + b];
        }
        const double mine = b < nb ? psum[at0 + b] : 0.0;
        for (int t = 0; t < m; ++t) sum += __shfl(mine, t);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
        cnt += __shfl_xor(cnt, off);
    }
    if (lane == 0) {
        PrepColumn k;
        if (cnt == 0) { lo = 0.f; hi = 0.f; sum = 0.0; }
        k.lo = lo + 0.f;                                        // a zero is stored as +0.0
        k.hi = hi + 0.f;
        const float range = k.hi - k.lo;
        k.scale = 1.f / (range < 10.f * 1.1920929e-07f ? 1.f : range);
        const float m = k.lo * k.scale;
        k.offset = 0.f - m;
        k.mean = cnt ? (float)(sum / (double)cnt) : 0.f;
        k.n_valid = (int)cnt;
        rec[col] = k;
    }
}

// ---- transform without a scan ----------------------------------------------------------------------------------------------------
// fill none / zero and no age: out = scaled x, a gap NaN or the scaled 0.0.  out may be x.
__global__ void __launch_bounds__(256) k_prep_apply(const float* x, long n, int d, long ld, const PrepColumn* __restrict__ rec, int fill,
                                                     int clip, float* out, long ld_out) {
    const int tid = threadIdx.x;
    for (long r0 = (long)blockIdx.x * 64; r0 < n; r0 += (long)gridDim.x * 64) {
        const int rows = n - r0 < 64 ? (int)(n - r0) : 64;
        for (int j = tid; j < rows * d; j += 256) {
            const int r = j / d, col = j - r * d;
            float v = x[(r0 + r) * ld + col];
            if (!prep_valid(v)) v = fill == PREP_FILL_ZERO ? 0.f : __builtin_nanf("");
            out[(r0 + r) * ld_out + col] = prep_scale(v, rec[col], clip);
        }
    }
}

// ---- transform with a scan: hold fill and / or age ---------------------------------------------------------------------------------
// carry flags: bit 0 a valid sample is known, bit 1 a seam lies inside the block or at its first row (what came before is cut off)
constexpr int PREP_HAS = 1, PREP_CUT = 2;

// (1) grid (row block, column tile): per (column, block), over the block's rows from its last seam on, the last valid raw value, whether
// there is one, and the gap rows behind it (all of those rows when there is none)
__global__ void __launch_bounds__(256) k_prep_tail(const float* __restrict__ x, long n, int d, long ld, const long* __restrict__ start,
                                                    const long* __restrict__ end, long count, long nb, int* __restrict__ cflags,
                                                    float* __restrict__ cval, int* __restrict__ cage) {
    __shared__ int slr[256];
    __shared__ float slv[256];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int c0 = blockIdx.y * PREP_CT;
    const int cw = d - c0 < PREP_CT ? d - c0 : PREP_CT;
    const long r0 = b * PREP_RB;
    const int rows = n - r0 < PREP_RB ? (int)(n - r0) : PREP_RB;
    const long seam = count > 0 ? prep_seam_before(start, end, count, r0 + rows - 1) : 0;
    const int first = seam > r0 ? (int)(seam - r0) : 0;         // the rows [first, rows) count
    const PrepWalk w = prep_walk(cw);
    int lastr = -1;
    float lastv = 0.f;
    if (w.on) {
        for (int r = w.rsub; r < rows; r += w.rp) {
            const float v = x[(r0 + r) * ld + c0 + w.c];
            if (r >= first && prep_valid(v)) { lastr = r; lastv = v; }
        }
    }
    slr[tid] = lastr; slv[tid] = lastv;
    __syncthreads();
    int top = 1;
    while (top < w.rp) top <<= 1;
    for (int st = top >> 1; st > 0; st >>= 1) {
        if (w.on && w.rsub < st && w.rsub + st < w.rp) {
            const int o = tid + st * cw;
            if (slr[o] > slr[tid]) { slr[tid] = slr[o]; slv[tid] = slv[o]; }
        }
        __syncthreads();
    }
    if (w.on && w.rsub == 0) {
        const long at = (long)(c0 + w.c) * nb + b;
        const bool has = slr[tid] >= 0;
        cflags[at] = (has ? PREP_HAS : 0) | (seam >= r0 ? PREP_CUT : 0);
        cval[at] = slv[tid];
        cage[at] = has ? rows - 1 - slr[tid] : rows - first;
    }
}

struct PrepCarry {
    int flags;
    float val;
    int age;
};
// the state after a then b
__device__ __forceinline__ PrepCarry prep_then(const PrepCarry& a, const PrepCarry& b) {
    if (b.flags & PREP_CUT) return b;
    PrepCarry r;
    const bool has = b.flags & PREP_HAS;
    r.flags = a.flags | (b.flags & PREP_HAS);
    r.val = has ? b.val : a.val;
    r.age = has ? b.age : a.age + b.age;
    return r;
}
__device__ __forceinline__ PrepCarry prep_shfl_up(const PrepCarry& v, int off) {
    PrepCarry r;
    r.flags = __shfl_up(v.flags, off);
    r.val = __shfl_up(v.val, off);
    r.age = __shfl_up(v.age, off);
    return r;
}

// (2) one wave per column: the blocks' summaries become their carry-ins (the state at the row before the block), 64 blocks per step in
// block order
__global__ void __launch_bounds__(64) k_prep_carry(long nb, int* __restrict__ cflags, float* __restrict__ cval, int* __restrict__ cage) {
    const int lane = threadIdx.x;
    const long at0 = (long)blockIdx.x * nb;
    PrepCarry run = {0, 0.f, 0};
    for (long base = 0; base < nb; base += 64) {
        const long b = base + lane;
        PrepCarry v = {0, 0.f, 0};
        if (b < nb) { v.flags = cflags[at0 + b]; v.val = cval[at0 + b]; v.age = cage[at0 + b]; }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const PrepCarry t = prep_shfl_up(v, off);
            if (lane >= off) v = prep_then(t, v);
        }
        const PrepCarry before = prep_shfl_up(v, 1);
        const PrepCarry in = lane == 0 ? run : prep_then(run, before);
        if (b < nb) { cflags[at0 + b] = in.flags; cval[at0 + b] = in.val; cage[at0 + b] = in.age; }
        PrepCarry last;
        last.flags = __shfl(v.flags, 63);
        last.val = __shfl(v.val, 63);
        last.age = __shfl(v.age, 63);
        run = prep_then(run, last);
    }
}

// (3) grid (row block, column tile): the block's rows 64 at a time.  The tile is read into LDS (float4 where `vec_in`: the tile is the
// whole width of a contiguous, 16-byte aligned array), wave w resolves columns w, w + 4, ... with its lanes on the rows, writes the
// prepared value (and the age) back into LDS, and the tile is stored the way it was loaded.  An odd row pitch keeps the column walk
// off shared banks.  out may be x.
__global__ void __launch_bounds__(256) k_prep_resolve(const float* x, long n, int d, long ld, const PrepColumn* __restrict__ rec, int fill,
                                                       int clip, const long* __restrict__ start, const long* __restrict__ end, long count,
                                                       long nb, const int* __restrict__ cflags, const float* __restrict__ cval,
                                                       const int* __restrict__ cage, float* out, long ld_out, int* __restrict__ age_out,
                                                       int vec_in, int vec_out) {
    __shared__ float tile[64 * PREP_PITCH];
    __shared__ int atile[64 * PREP_PITCH];
    __shared__ int seg[PREP_RB];                                // a row's seam relative to the block's first row; -1: before it
    __shared__ int st_has[PREP_CT];
    __shared__ float st_val[PREP_CT];
    __shared__ int st_age[PREP_CT];
    const int tid = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = blockIdx.x;
    const int c0 = blockIdx.y * PREP_CT;
    const int cw = d - c0 < PREP_CT ? d - c0 : PREP_CT;
    const int pitch = cw | 1;
    const long r0 = b * PREP_RB;
    const int rows = n - r0 < PREP_RB ? (int)(n - r0) : PREP_RB;
    for (int r = tid; r < rows; r += 256) {
        const long s = count > 0 ? prep_seam_before(start, end, count, r0 + r) : 0;
        seg[r] = s < r0 ? -1 : (int)(s - r0);
    }
    if (tid < cw) {
        const long at = (long)(c0 + tid) * nb + b;
        st_has[tid] = cflags[at] & PREP_HAS;
        st_val[tid] = cval[at];
        st_age[tid] = cage[at];
    }
    __syncthreads();
    for (int gb = 0; gb < rows; gb += 64) {
        const int grows = rows - gb < 64 ? rows - gb : 64;
        const int total = grows * cw;
        const float* src = x + (r0 + gb) * ld + c0;
        if (vec_in) {
            const float4* src4 = reinterpret_cast<const float4*>(src);
            for (int q = tid; 4 * q < total; q += 256) {
                float v[4];
                if (4 * q + 3 < total) {
                    const float4 f = src4[q];
                    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                } else {
                    for (int t = 0; t < 4; ++t) v[t] = 4 * q + t < total ? src[4 * q + t] : 0.f;
                }
                for (int t = 0; t < 4; ++t) {
                    const int j = 4 * q + t;
                    if (j < total) tile[(j / cw) * pitch + j % cw] = v[t];
                }
            }
        } else {
            for (int j = tid; j < total; j += 256) {
                const int r = j / cw, c = j - r * cw;
                tile[r * pitch + c] = src[r * ld + c];
            }
        }
        __syncthreads();
        const bool row_on = lane < grows;
        const int rel = row_on ? seg[gb + lane] : 0;
        const int from = rel > gb ? rel - gb : 0;               // the group's lanes below `from` are beyond the row's seam
        for (int c = wave; c < cw; c += 4) {
            const float v = row_on ? tile[lane * pitch + c] : 0.f;
            const bool ok = row_on && prep_valid(v);
            const int in_has = st_has[c];
            const float in_val = st_val[c];
            const int in_age = st_age[c];
            const unsigned long long mask = __ballot(ok) & ((2ull << lane) - 1ull) & (~0ull << from);
            const int j = mask ? 63 - __clzll((long long)mask) : 0;
            const float held = __shfl(v, j);
            int has, age;
            float val;
            if (mask) { has = 1; val = held; age = lane - j; }
            else if (rel >= gb) { has = 0; val = 0.f; age = gb + lane - rel + 1; }      // the part starts in this group
            else { has = in_has; val = in_val; age = in_age + lane + 1; }
            const PrepColumn k = rec[c0 + c];
            float raw = v;
            if (!ok) raw = fill == PREP_FILL_HOLD ? (has ? val : k.mean) : (fill == PREP_FILL_ZERO ? 0.f : __builtin_nanf(""));
            if (row_on) {
                tile[lane * pitch + c] = prep_scale(raw, k, clip);
                atile[lane * pitch + c] = age;
            }
            if (lane == grows - 1) { st_has[c] = has; st_val[c] = val; st_age[c] = age; }
        }
        __syncthreads();
        float* dst = out + (r0 + gb) * ld_out + c0;
        if (vec_out) {
            float4* dst4 = reinterpret_cast<float4*>(dst);
            int4* age4 = age_out ? reinterpret_cast<int4*>(age_out + (r0 + gb) * (long)d) : nullptr;
            for (int q = tid; 4 * q < total; q += 256) {
                if (4 * q + 3 < total) {
                    float f[4];
                    int a[4];
                    for (int t = 0; t < 4; ++t) {
                        const int jj = 4 * q + t, at = (jj / cw) * pitch + jj % cw;
                        f[t] = tile[at];
                        a[t] = atile[at];
                    }
                    dst4[q] = make_float4(f[0], f[1], f[2], f[3]);
                    if (age4) age4[q] = make_int4(a[0], a[1], a[2], a[3]);
                } else {
                    for (int jj = 4 * q; jj < total; ++jj) {
                        const int at = (jj / cw) * pitch + jj % cw;
                        dst[jj] = tile[at];
                        if (age_out) age_out[(r0 + gb) * (long)d + jj] = atile[at];
                    }
                }
            }
        } else {
            for (int j = tid; j < total; j += 256) {
                const int r = j / cw, c = j - r * cw;
                dst[r * ld_out + c] = tile[r * pitch + c];
                if (age_out) age_out[(r0 + gb + r) * (long)d + c0 + c] = atile[r * pitch + c];
            }
        }
        __syncthreads();
    }
}

// ---- inverse -----------------------------------------------------------------------------------------------------------------------
// out[i, j] = fl(fl(y[i, j] - offset) / scale) of scaler column dims[j] (j without dims); NaN for a column outside the scaler
__global__ void __launch_bounds__(256) k_prep_inverse(const float* y, long n, int d, long ld, const PrepColumn* __restrict__ rec, int d_scaler,
                                                       const int* __restrict__ dims, float* out, long ld_out) {
    const int tid = threadIdx.x;
    for (long r0 = (long)blockIdx.x * 64; r0 < n; r0 += (long)gridDim.x * 64) {
        const int rows = n - r0 < 64 ? (int)(n - r0) : 64;
        for (int j = tid; j < rows * d; j += 256) {
            const int r = j / d, col = j - r * d;
            const int sc = dims ? dims[col] : col;
            float v = __builtin_nanf("");
            if (sc >= 0 && sc < d_scaler) v = (y[(r0 + r) * ld + col] - rec[sc].offset) / rec[sc].scale;
            out[(r0 + r) * ld_out + col] = v;
        }
    }
}

// ---- streams -----------------------------------------------------------------------------------------------------------------------
struct PrepStreamHeader {
    long S, d;
};
struct PrepStreamPtrs {
    PrepStreamHeader* hd;
    int* has;
    float* val;
    int* age;
};

namespace {

size_t prep_up16(size_t v) { return (v + 15) / 16 * 16; }
size_t prep_stream_bytes(long S, long d) { return prep_up16(sizeof(PrepStreamHeader)) + 3 * prep_up16(4 * (size_t)S * (size_t)d); }
PrepStreamPtrs prep_stream_ptrs(void* state, long S, long d) {
    char* b = static_cast<char*>(state);
    const size_t cells = prep_up16(4 * (size_t)S * (size_t)d);
    PrepStreamPtrs p;
    p.hd = reinterpret_cast<PrepStreamHeader*>(b);
    b += prep_up16(sizeof(PrepStreamHeader));
    p.has = reinterpret_cast<int*>(b);
    p.val = reinterpret_cast<float*>(b + cells);
    p.age = reinterpret_cast<int*>(b + 2 * cells);
    return p;
}

}  // namespace

// grid (ceil(n / 4)) x 256 threads: one wave per selected stream, lanes on the columns, the T rows in order
__global__ void __launch_bounds__(256) k_prep_stream_push(PrepStreamPtrs p, long S, int d, const float* __restrict__ rows,
                                                           const long* __restrict__ streams, long n, long T,
                                                           const PrepColumn* __restrict__ rec, int fill, int clip, float* __restrict__ out,
                                                           int* __restrict__ age_out) {
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= n) return;
    const long s = streams ? streams[j] : j;
    const bool ok_stream = p.hd->S == S && p.hd->d == d && s >= 0 && s < S;
    for (int c = lane; c < d; c += 64) {
        if (!ok_stream) {
            for (long t = 0; t < T; ++t) {
                out[(j * T + t) * d + c] = __builtin_nanf("");
                if (age_out) age_out[(j * T + t) * d + c] = -1;
            }
            continue;
        }
        const PrepColumn k = rec[c];
        int has = p.has[s * d + c], age = p.age[s * d + c];
        float val = p.val[s * d + c];
        for (long t = 0; t < T; ++t) {
            const long at = (j * T + t) * d + c;
            float v = rows[at];
            if (prep_valid(v)) {
                has = 1; val = v; age = 0;
            } else {
                age += 1;
                v = fill == PREP_FILL_HOLD ? (has ? val : k.mean) : (fill == PREP_FILL_ZERO ? 0.f : __builtin_nanf(""));
            }
            out[at] = prep_scale(v, k, clip);
            if (age_out) age_out[at] = age;
        }
        p.has[s * d + c] = has;
        p.val[s * d + c] = val;
        p.age[s * d + c] = age;
    }
}

// the selected streams (streams == nullptr: 0 .. n - 1) back to "nothing heard yet"; init: the header is written too
__global__ void __launch_bounds__(256) k_prep_stream_reset(PrepStreamPtrs p, long S, int d, const long* __restrict__ streams, long n, int init) {
    if (init && blockIdx.x == 0 && threadIdx.x == 0) { p.hd->S = S; p.hd->d = d; }
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= n) return;
    const long s = streams ? streams[j] : j;
    if (s < 0 || s >= S || (!init && (p.hd->S != S || p.hd->d != d))) return;
    for (int c = lane; c < d; c += 64) {
        p.has[s * d + c] = 0;
        p.val[s * d + c] = 0.f;
        p.age[s * d + c] = 0;
    }
}

}  // namespace mtadgat

using namespace mtadgat;

namespace {

constexpr int64_t PREP_N_MAX = 2147483647LL;

long prep_blocks(int64_t n) { return (long)((n + PREP_RB - 1) / PREP_RB); }
unsigned prep_tiles(int d) { return (unsigned)((d + PREP_CT - 1) / PREP_CT); }

struct FitScratch {
    double* psum;
    float *plo, *phi;
    int* pcnt;
};
FitScratch fit_scratch(ScratchCarver& c, int64_t n, int d) {
    const size_t cells = (size_t)prep_blocks(n) * (size_t)d;
    FitScratch l;
    l.psum = c.take<double>(cells);
    l.plo = c.take<float>(cells);
    l.phi = c.take<float>(cells);
    l.pcnt = c.take<int>(cells);
    return l;
}

struct ScanScratch {
    int* cflags;
    float* cval;
    int* cage;
};
ScanScratch scan_scratch(ScratchCarver& c, int64_t n, int d) {
    const size_t cells = (size_t)prep_blocks(n) * (size_t)d;
    ScanScratch l;
    l.cflags = c.take<int>(cells);
    l.cval = c.take<float>(cells);
    l.cage = c.take<int>(cells);
    return l;
}

bool prep_sizes_ok(int64_t n, int d) { return n >= 1 && n <= PREP_N_MAX && d >= 1 && d <= 2048; }
bool prep_needs_scan(int fill, int want_age) { return fill == PREP_FILL_HOLD || want_age; }

unsigned prep_row_grid(int64_t n) {
    const int64_t chunks = (n + 63) / 64;
    return (unsigned)(chunks < 65536 ? chunks : 65536);
}

// the checks every (n, d, ld) array argument gets
const char* prep_array_error(int64_t n, int d, int64_t ld, int64_t ld_out) {
    if (n < 1 || n > PREP_N_MAX) return "n must lie in [1, 2^31 - 1]";
    if (d < 1 || d > 2048) return "d must lie in [1, 2048]";
    if (ld < d || ld_out < d) return "ld < d";
    if (ld > PREP_N_MAX || ld_out > PREP_N_MAX) return "ld must lie below 2^31";
    return nullptr;
}

}  // namespace

extern "C" {

int mtadgat_prep_rows_per_block(void) { return PREP_RB; }

size_t mtadgat_prep_fit_scratch(int64_t n, int d) {
    if (!prep_sizes_ok(n, d)) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { fit_scratch(c, n, d); });
}

int mtadgat_prep_fit(const float* x_dev, int64_t n, int d, int64_t ld, int gaps, void* scratch_dev, size_t scratch_bytes,
                     mtadgat_prep_column* scaler_dev, void* stream) {
    if (!x_dev || !scratch_dev || !scaler_dev) return record_error(-1, "prep_fit: null pointer");
    if (const char* e = prep_array_error(n, d, ld, ld)) return record_error(-1, (std::string("prep_fit: ") + e).c_str());
    if (gaps != PREP_GAPS_IGNORE && gaps != PREP_GAPS_ZERO) return record_error(-1, "prep_fit: gaps must be 0 (ignore) or 1 (zero)");
    ScratchCarver carver(scratch_dev);
    const FitScratch l = fit_scratch(carver, n, d);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "prep_fit: scratch too small (see mtadgat_prep_fit_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "prep_fit: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long nb = prep_blocks(n);
    hipLaunchKernelGGL(k_prep_fit_partial, dim3((unsigned)nb, prep_tiles(d)), dim3(256), 0, s, x_dev, (long)n, d, (long)ld, gaps, nb, l.plo,
                       l.phi, l.pcnt, l.psum);
    hipLaunchKernelGGL(k_prep_fit_final, dim3((unsigned)d), dim3(64), 0, s, d, nb, (const float*)l.plo, (const float*)l.phi,
                       (const int*)l.pcnt, (const double*)l.psum, reinterpret_cast<PrepColumn*>(scaler_dev));
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "prep_fit: kernel launch failed");
}

size_t mtadgat_prep_transform_scratch(int64_t n, int d, int fill, int want_age) {
    if (!prep_sizes_ok(n, d) || fill < PREP_FILL_NONE || fill > PREP_FILL_HOLD) return 0;
    if (!prep_needs_scan(fill, want_age)) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { scan_scratch(c, n, d); });
}

int mtadgat_prep_transform(const float* x_dev, int64_t n, int d, int64_t ld, const mtadgat_prep_column* scaler_dev, int fill, int clip,
                           const int64_t* start_dev, const int64_t* end_dev, int64_t count, void* scratch_dev, size_t scratch_bytes,
                           float* out_dev, int64_t ld_out, int32_t* age_dev, void* stream) {
    if (!x_dev || !scaler_dev || !out_dev) return record_error(-1, "prep_transform: null pointer");
    if (const char* e = prep_array_error(n, d, ld, ld_out)) return record_error(-1, (std::string("prep_transform: ") + e).c_str());
    if (fill < PREP_FILL_NONE || fill > PREP_FILL_HOLD) return record_error(-1, "prep_transform: fill must be 0 (none), 1 (zero) or 2 (hold)");
    if (count < 0 || count > PREP_N_MAX) return record_error(-1, "prep_transform: count must lie in [0, 2^31 - 1]");
    if (count > 0 && (!start_dev || !end_dev)) return record_error(-1, "prep_transform: null pointer");
    if (out_dev == x_dev && ld_out != ld) return record_error(-1, "prep_transform: in place needs ld_out == ld");
    hipStream_t s = (hipStream_t)stream;
    const PrepColumn* rec = reinterpret_cast<const PrepColumn*>(scaler_dev);
    if (!prep_needs_scan(fill, age_dev != nullptr)) {
        hipLaunchKernelGGL(k_prep_apply, dim3(prep_row_grid(n)), dim3(256), 0, s, x_dev, (long)n, d, (long)ld, rec, fill, clip ? 1 : 0, out_dev,
                           (long)ld_out);
        return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "prep_transform: kernel launch failed");
    }
    if (!scratch_dev) return record_error(-1, "prep_transform: null pointer");
    ScratchCarver carver(scratch_dev);
    const ScanScratch l = scan_scratch(carver, n, d);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "prep_transform: scratch too small (see mtadgat_prep_transform_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "prep_transform: scratch must be 8-byte aligned");
    const long nb = prep_blocks(n);
    const long* st = reinterpret_cast<const long*>(start_dev);
    const long* en = reinterpret_cast<const long*>(end_dev);
    const dim3 grid((unsigned)nb, prep_tiles(d));
    // float4 traffic: one tile spans the whole width of a contiguous array whose base (and the age's) is 16-byte aligned
    const int vec_in = d <= PREP_CT && ld == d && ((uintptr_t)x_dev & 15) == 0;
    const int vec_out = d <= PREP_CT && ld_out == d && ((uintptr_t)out_dev & 15) == 0 && ((uintptr_t)age_dev & 15) == 0;
    hipLaunchKernelGGL(k_prep_tail, grid, dim3(256), 0, s, x_dev, (long)n, d, (long)ld, st, en, (long)count, nb, l.cflags, l.cval, l.cage);
    hipLaunchKernelGGL(k_prep_carry, dim3((unsigned)d), dim3(64), 0, s, nb, l.cflags, l.cval, l.cage);
    hipLaunchKernelGGL(k_prep_resolve, grid, dim3(256), 0, s, x_dev, (long)n, d, (long)ld, rec, fill, clip ? 1 : 0, st, en, (long)count, nb,
                       (const int*)l.cflags, (const float*)l.cval, (const int*)l.cage, out_dev, (long)ld_out, age_dev, vec_in, vec_out);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "prep_transform: kernel launch failed");
}

int mtadgat_prep_inverse(const float* y_dev, int64_t n, int d, int64_t ld, const mtadgat_prep_column* scaler_dev, int d_scaler,
                         const int32_t* dims_dev, float* out_dev, int64_t ld_out, void* stream) {
    if (!y_dev || !scaler_dev || !out_dev) return record_error(-1, "prep_inverse: null pointer");
    if (const char* e = prep_array_error(n, d, ld, ld_out)) return record_error(-1, (std::string("prep_inverse: ") + e).c_str());
    if (d_scaler < 1 || d_scaler > 2048) return record_error(-1, "prep_inverse: d_scaler must lie in [1, 2048]");
    if (!dims_dev && d > d_scaler) return record_error(-1, "prep_inverse: more columns than the scaler has, and no dims");
    if (out_dev == y_dev && ld_out != ld) return record_error(-1, "prep_inverse: in place needs ld_out == ld");
    hipLaunchKernelGGL(k_prep_inverse, dim3(prep_row_grid(n)), dim3(256), 0, (hipStream_t)stream, y_dev, (long)n, d, (long)ld,
                       reinterpret_cast<const PrepColumn*>(scaler_dev), d_scaler, dims_dev, out_dev, (long)ld_out);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "prep_inverse: kernel launch failed");
}

size_t mtadgat_prep_stream_state_bytes(int64_t n_streams, int d) {
    if (n_streams < 1 || n_streams > PREP_N_MAX || d < 1 || d > 2048) return 0;
    return prep_stream_bytes((long)n_streams, d);
}

int mtadgat_prep_stream_init(void* state_dev, int64_t n_streams, int d, void* stream) {
    if (!state_dev) return record_error(-1, "prep_stream_init: null pointer");
    if (n_streams < 1 || n_streams > PREP_N_MAX || d < 1 || d > 2048)
        return record_error(-1, "prep_stream_init: needs 1 <= n_streams <= 2^31 - 1 and 1 <= d <= 2048");
    if ((uintptr_t)state_dev & 15) return record_error(-1, "prep_stream_init: the state must be 16-byte aligned");
    hipLaunchKernelGGL(k_prep_stream_reset, dim3((unsigned)((n_streams + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       prep_stream_ptrs(state_dev, (long)n_streams, d), (long)n_streams, d, (const long*)nullptr, (long)n_streams, 1);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "prep_stream_init: kernel launch failed");
}

int mtadgat_prep_stream_push(void* state_dev, int64_t n_streams, int d, const float* rows_dev, const int64_t* streams_dev, int64_t n,
                             int64_t T, const mtadgat_prep_column* scaler_dev, int fill, int clip, float* out_dev, int32_t* age_dev,
                             void* stream) {
    if (!state_dev || !rows_dev || !scaler_dev || !out_dev) return record_error(-1, "prep_stream_push: null pointer");
    if (n_streams < 1 || n_streams > PREP_N_MAX || d < 1 || d > 2048)
        return record_error(-1, "prep_stream_push: needs 1 <= n_streams <= 2^31 - 1 and 1 <= d <= 2048");
    if (n < 1 || n > n_streams) return record_error(-1, "prep_stream_push: n must lie in [1, n_streams]");
    if (T < 1 || T > PREP_N_MAX || n * T > PREP_N_MAX) return record_error(-1, "prep_stream_push: needs T >= 1 and n T <= 2^31 - 1");
    if (fill < PREP_FILL_NONE || fill > PREP_FILL_HOLD) return record_error(-1, "prep_stream_push: fill must be 0 (none), 1 (zero) or 2 (hold)");
    if ((uintptr_t)state_dev & 15) return record_error(-1, "prep_stream_push: the state must be 16-byte aligned");
    hipLaunchKernelGGL(k_prep_stream_push, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       prep_stream_ptrs(state_dev, (long)n_streams, d), (long)n_streams, d, rows_dev, reinterpret_cast<const long*>(streams_dev),
                       (long)n, (long)T, reinterpret_cast<const PrepColumn*>(scaler_dev), fill, clip ? 1 : 0, out_dev, age_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "prep_stream_push: kernel launch failed");
}

int mtadgat_prep_stream_reset(void* state_dev, int64_t n_streams, int d, const int64_t* streams_dev, int64_t n, void* stream) {
    if (!state_dev) return record_error(-1, "prep_stream_reset: null pointer");
    if (n_streams < 1 || n_streams > PREP_N_MAX || d < 1 || d > 2048)
        return record_error(-1, "prep_stream_reset: needs 1 <= n_streams <= 2^31 - 1 and 1 <= d <= 2048");
    if (n < 1 || n > n_streams) return record_error(-1, "prep_stream_reset: n must lie in [1, n_streams]");
    if ((uintptr_t)state_dev & 15) return record_error(-1, "prep_stream_reset: the state must be 16-byte aligned");
    hipLaunchKernelGGL(k_prep_stream_reset, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       prep_stream_ptrs(state_dev, (long)n_streams, d), (long)n_streams, d, reinterpret_cast<const long*>(streams_dev), (long)n, 0);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "prep_stream_reset: kernel launch failed");
}

}  // extern "C"
