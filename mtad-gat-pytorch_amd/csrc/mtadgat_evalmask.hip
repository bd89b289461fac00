// Scores of a gappy series (evaluation.scored_rows, anomaly_scores(age=), moving_average / find_epsilon(skip_nan=True)): a score exists
// exactly where mtadgat_fit_windows would have drawn a training window, and NaN means "no score".  tests/score_mask_refs.py is the
// specification.  (The exact select that skips NaN, mtadgat_eval_column_quantiles_valid, is an instantiation of the column select in
// mtadgat_evalcol.hip.)
//
//   k_mark_clear / k_mark_set   keep[i] = 1 for the starts mtadgat_fit_windows left on the device, 0 elsewhere; the count is read
//                               on the device.
//   k_eval_scores_masked        k_eval_scores' expression where the target sample is observed and the row is kept, the canonical NaN
//                               elsewhere; the mean over the observed terms in column order, by a select.
//   k_eval_row_means_valid      that mean over the non-NaN entries of the rows of an array that was scaled after masking.
//   k_ewmv_chunk / _carry / _apply
//                               the exponentially weighted mean over observed rows: the blocked float64 scan of k_ewm_* on (N, D)
//                               pairs, N_t = (obs ? x_t : 0) + b N_{t-1}, D_t = (obs ? 1 : 0) + b D_{t-1}.
//   k_momv_blocks / _columns    per column the float64 sum, sum of squares and count of the non-NaN entries: per-block partials by
//                               the fixed tree of block_sum, then one wave per column that adds them in block order.
// No atomics at all: identical calls give identical bits.
#include "../../include/mtadgat.h"      // the entry points' declarations
#include "mtadgat_scan.h"

namespace mtadgat {

// ---- which scores exist ------------------------------------------------------------------------------------------------------------
__global__ void k_mark_clear(unsigned char* __restrict__ keep, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) keep[i] = 0;
}
// a start outside [0, n) is ignored, a count beyond n read as n: nothing is written outside keep
__global__ void k_mark_set(const long* __restrict__ starts, const long* __restrict__ count, long n, unsigned char* __restrict__ keep) {
    long c = *count;
    c = c < 0 ? 0 : (c > n ? n : c);
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < c; j += (long)gridDim.x * blockDim.x) {
        const long s = starts[j];
        if (s >= 0 && s < n) keep[s] = 1;
    }
}

// ---- masked scores -----------------------------------------------------------------------------------------------------------------
// one thread per row, the columns in order as in k_eval_scores: with everything observed and kept the same operations on the same
// operands, so the same bits
__global__ void k_eval_scores_masked(const float* __restrict__ preds, const float* __restrict__ recons, const float* __restrict__ actual,
                                     long n, int d, long ld_actual, const int* __restrict__ dims, float gamma, const int* __restrict__ age,
                                     long ld_age, int max_age, const unsigned char* __restrict__ keep, float* __restrict__ per_dim,
                                     float* __restrict__ global, int* __restrict__ count) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool kept = keep ? keep[i] != 0 : true;
    const float none = __builtin_bit_cast(float, 0x7fc00000u);
    float acc = 0.f;
    int cnt = 0;
    for (int k = 0; k < d; ++k) {
        const int col = dims ? dims[k] : k;
        const bool obs = kept && age[i * ld_age + col] <= max_age;
        const float t = actual[i * ld_actual + col];
        const float a = fabsf(preds[i * d + k] - t) + gamma * fabsf(recons[i * d + k] - t);
        if (per_dim) per_dim[i * d + k] = obs ? a : none;
        if (obs) {
            acc += a;
            ++cnt;
        }
    }
    if (global) global[i] = cnt > 0 ? acc / (float)cnt : none;
    if (count) count[i] = cnt;
}

// global[i] = the float32 sum of row i's non-NaN entries in column order / their number: k_eval_scores_masked's mean for per-dimension
// scores that were scaled after the mask was applied
__global__ void k_eval_row_means_valid(const float* __restrict__ a, long n, int d, long ld, float* __restrict__ global, int* __restrict__ count) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f;
    int cnt = 0;
    for (int k = 0; k < d; ++k) {
        const float v = a[i * ld + k];
        if (v == v) {
            acc += v;
            ++cnt;
        }
    }
    global[i] = cnt > 0 ? acc / (float)cnt : __builtin_bit_cast(float, 0x7fc00000u);
    if (count) count[i] = cnt;
}

// ---- exponentially weighted mean over observed rows ------------------------------------------------------------------------------------
constexpr int EWMV_L = 1024;     // elements per chunk: 256 threads x 4

struct Pair {
    double n, d;
};

__device__ __forceinline__ void ewmv_load(const float* x, long n, long base, double (&v)[4], double (&o)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = base + j;
        const float f = i < n ? x[i] : __builtin_nanf("");
        const bool obs = f == f;
        v[j] = obs ? (double)f : 0.0;
        o[j] = obs ? 1.0 : 0.0;
    }
}

// (N, D) just before this thread's four elements, started from `carry` before the chunk: k_ewm's wave scan by shuffles (factor
// b^(4 off) at distance off) on both components, then the four wave totals composed in order.  sm: 8 doubles.
__device__ __forceinline__ Pair ewmv_prefix(const double (&v)[4], const double (&o)[4], double b, Pair carry, double* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sn = v[0], sd = o[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        sn = sn * b + v[j];
        sd = sd * b + o[j];
    }
    double f = (b * b) * (b * b);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double tn = __shfl_up(sn, off), td = __shfl_up(sd, off);
        if (lane >= off) {
            sn = tn * f + sn;
            sd = td * f + sd;
        }
        f *= f;
    }                                                   // f = b^256
    if (lane == 63) {
        sm[2 * wave] = sn;
        sm[2 * wave + 1] = sd;
    }
    double exn = __shfl_up(sn, 1), exd = __shfl_up(sd, 1);
    if (lane == 0) exn = exd = 0.0;
    __syncthreads();
    Pair in = carry;
    for (int w = 0; w < wave; ++w) {
        in.n = in.n * f + sm[2 * w];
        in.d = in.d * f + sm[2 * w + 1];
    }
    const double fl = pow(b, (double)(4 * lane));
    Pair r;
    r.n = exn + in.n * fl;
    r.d = exd + in.d * fl;
    return r;
}

// S[2 c], S[2 c + 1] = (N, D) at the end of chunk c when nothing precedes it
__global__ void __launch_bounds__(256) k_ewmv_chunk(const float* x, long n, double b, double* __restrict__ S) {
    __shared__ double sm[8];
    double v[4], o[4];
    ewmv_load(x, n, (long)blockIdx.x * EWMV_L + 4 * threadIdx.x, v, o);
    Pair zero;
    zero.n = zero.d = 0.0;
    Pair s = ewmv_prefix(v, o, b, zero, sm);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.n = s.n * b + v[j];
        s.d = s.d * b + o[j];
    }
    if (threadIdx.x == 255) {
        S[2 * blockIdx.x] = s.n;
        S[2 * blockIdx.x + 1] = s.d;
    }
}

// carry[c] = (N, D) just before chunk c: carry[c] = carry[c - 1] b^L + S[c - 1], 64 chunks per step of one wave, in chunk order
__global__ void __launch_bounds__(64) k_ewmv_carry(const double* __restrict__ S, long nchunks, double fL, double* __restrict__ carry) {
    const int lane = threadIdx.x;
    const double fl = pow(fL, (double)lane);
    double runn = 0.0, rund = 0.0;
    for (long base = 0; base < nchunks; base += 64) {
        const long i = base + lane;
        double sn = i < nchunks ? S[2 * i] : 0.0, sd = i < nchunks ? S[2 * i + 1] : 0.0;
        double f = fL;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double tn = __shfl_up(sn, off), td = __shfl_up(sd, off);
            if (lane >= off) {
                sn = tn * f + sn;
                sd = td * f + sd;
            }
            f *= f;
        }                                               // f = fL^64
        double exn = __shfl_up(sn, 1), exd = __shfl_up(sd, 1);
        if (lane == 0) exn = exd = 0.0;
        if (i < nchunks) {
            carry[2 * i] = runn * fl + exn;
            carry[2 * i + 1] = rund * fl + exd;
        }
        runn = runn * f + __shfl(sn, 63);
        rund = rund * f + __shfl(sd, 63);
    }
}

// y[t] = N_t / D_t at an observed row (D_t >= 1 there), the canonical NaN at an unobserved one.  y may be x: a thread reads its four
// elements before it writes them, and no other thread touches them.
__global__ void __launch_bounds__(256) k_ewmv_apply(const float* x, long n, double b, const double* __restrict__ carry, float* y) {
    __shared__ double sm[8];
    double v[4], o[4];
    const long base = (long)blockIdx.x * EWMV_L + 4 * threadIdx.x;
    ewmv_load(x, n, base, v, o);
    Pair c;
    c.n = carry[2 * blockIdx.x];
    c.d = carry[2 * blockIdx.x + 1];
    Pair s = ewmv_prefix(v, o, b, c, sm);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.n = s.n * b + v[j];
        s.d = s.d * b + o[j];
        if (base + j < n) y[base + j] = o[j] != 0.0 ? (float)(s.n / s.d) : __builtin_bit_cast(float, 0x7fc00000u);
    }
}

// ---- moments of the non-NaN entries ----------------------------------------------------------------------------------------------------
constexpr int MOMV_BLOCKS = 256;  // most workgroups per column of the first stage

// part[(col * gridDim.x + block) * 3] = { sum, sum of squares, count } over the rows block * 256 + tid, + gridDim.x * 256, ..
__global__ void __launch_bounds__(256) k_momv_blocks(const float* __restrict__ e, long n, long ld, double* __restrict__ part) {
    __shared__ double sm[256];
    e += blockIdx.y;
    double s = 0.0, s2 = 0.0, c = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float f = e[i * ld];
        if (f == f) {
            const double v = (double)f;
            s += v;
            s2 += v * v;
            c += 1.0;
        }
    }
    s = block_sum(s, sm);
    s2 = block_sum(s2, sm);
    c = block_sum(c, sm);
    if (threadIdx.x == 0) {
        double* p = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        p[0] = s; p[1] = s2; p[2] = c;
    }
}

// one wave per column: lane l adds the blocks l, l + 64, .. in that order, then the lanes are added by a fixed tree
__global__ void __launch_bounds__(64) k_momv_columns(const double* __restrict__ part, int blocks, double* __restrict__ out) {
    const int lane = threadIdx.x;
    const double* p = part + (long)blockIdx.x * blocks * 3;
    double v[3] = {0.0, 0.0, 0.0};
    for (int b = lane; b < blocks; b += 64)
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] += p[b * 3 + q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] += __shfl_down(v[q], off);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 3; ++q) out[(long)blockIdx.x * 3 + q] = v[q];
}

}  // namespace mtadgat

using namespace mtadgat;

namespace {

constexpr int64_t N_MAX = 2147483647LL;

// S and carry: two doubles per chunk each
struct EwmvScratch {
    double *S, *carry;
    long nchunks;
};
EwmvScratch ewmv_scratch(ScratchCarver& c, int64_t n) {
    EwmvScratch l;
    l.nchunks = (long)((n + EWMV_L - 1) / EWMV_L);
    l.S = c.take<double>(2 * (size_t)l.nchunks);
    l.carry = c.take<double>(2 * (size_t)l.nchunks);
    return l;
}

// the blocks' partials, then the (d, 3) result
struct MomvScratch {
    double *part, *out;
    int blocks;
};
MomvScratch momv_scratch(ScratchCarver& c, int64_t n, int64_t d) {
    MomvScratch l;
    const int64_t bx = (n + 255) / 256;
    l.blocks = (int)(bx < MOMV_BLOCKS ? bx : MOMV_BLOCKS);
    l.part = c.take<double>((size_t)d * (size_t)l.blocks * 3);
    l.out = c.take<double>((size_t)d * 3);
    return l;
}

}  // namespace

extern "C" {

int mtadgat_eval_mark_rows(const int64_t* starts_dev, const int64_t* count_dev, int64_t n, uint8_t* keep_dev, void* stream) {
    if (!starts_dev || !count_dev || !keep_dev) return record_error(-1, "mark_rows: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "mark_rows: n must lie in [1, 2^31 - 1]");
    hipStream_t s = (hipStream_t)stream;
    const long blocks = (n + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(k_mark_clear, dim3(grid), dim3(256), 0, s, keep_dev, (long)n);
    hipLaunchKernelGGL(k_mark_set, dim3(grid), dim3(256), 0, s, reinterpret_cast<const long*>(starts_dev),
                       reinterpret_cast<const long*>(count_dev), (long)n, keep_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "mark_rows: kernel launch failed");
}

int mtadgat_eval_scores_masked(const float* preds_dev, const float* recons_dev, const float* actual_dev, int64_t n, int d, int64_t ld_actual,
                               const int32_t* dims_dev, float gamma, const int32_t* age_dev, int64_t ld_age, int32_t max_age,
                               const uint8_t* keep_dev, float* per_dim_dev, float* global_dev, int32_t* count_dev, void* stream) {
    if (!preds_dev || !recons_dev || !actual_dev || !age_dev) return record_error(-1, "scores_masked: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "scores_masked: n must lie in [1, 2^31 - 1]");
    if (d < 1 || d > 2048) return record_error(-1, "scores_masked: d must lie in [1, 2048]");
    if (!dims_dev && (ld_actual < d || ld_age < d)) return record_error(-1, "scores_masked: ld_actual or ld_age < d needs dims_dev");
    if (ld_actual < 1 || ld_age < 1) return record_error(-1, "scores_masked: ld_actual and ld_age must be >= 1");
    hipLaunchKernelGGL(k_eval_scores_masked, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, preds_dev, recons_dev,
                       actual_dev, (long)n, d, (long)ld_actual, dims_dev, gamma, age_dev, (long)ld_age, (int)max_age, keep_dev, per_dim_dev,
                       global_dev, count_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "scores_masked: kernel launch failed");
}

int mtadgat_eval_row_means_valid(const float* a_dev, int64_t n, int d, int64_t ld, float* global_dev, int32_t* count_dev, void* stream) {
    if (!a_dev || !global_dev) return record_error(-1, "row_means_valid: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "row_means_valid: n must lie in [1, 2^31 - 1]");
    if (d < 1 || d > 2048) return record_error(-1, "row_means_valid: d must lie in [1, 2048]");
    if (ld < d) return record_error(-1, "row_means_valid: ld < d");
    hipLaunchKernelGGL(k_eval_row_means_valid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a_dev, (long)n, d, (long)ld,
                       global_dev, count_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "row_means_valid: kernel launch failed");
}

size_t mtadgat_eval_ewm_valid_scratch(int64_t n) {
    if (n < 1 || n > N_MAX) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { ewmv_scratch(c, n); });
}

int mtadgat_eval_ewm_valid(const float* x_dev, int64_t n, double alpha, void* scratch_dev, size_t scratch_bytes, float* out_dev, void* stream) {
    if (!x_dev || !scratch_dev || !out_dev) return record_error(-1, "ewm_valid: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "ewm_valid: n must lie in [1, 2^31 - 1]");
    if (!(alpha > 0.0 && alpha <= 1.0)) return record_error(-1, "ewm_valid: alpha outside (0, 1]");
    ScratchCarver carver(scratch_dev);
    const EwmvScratch l = ewmv_scratch(carver, n);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "ewm_valid: scratch too small (see mtadgat_eval_ewm_valid_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "ewm_valid: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const double b = 1.0 - alpha;
    hipLaunchKernelGGL(k_ewmv_chunk, dim3((unsigned)l.nchunks), dim3(256), 0, s, x_dev, (long)n, b, l.S);
    hipLaunchKernelGGL(k_ewmv_carry, dim3(1), dim3(64), 0, s, (const double*)l.S, l.nchunks, pow(b, (double)EWMV_L), l.carry);
    hipLaunchKernelGGL(k_ewmv_apply, dim3((unsigned)l.nchunks), dim3(256), 0, s, x_dev, (long)n, b, (const double*)l.carry, out_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "ewm_valid: kernel launch failed");
}

size_t mtadgat_eval_moments_valid_scratch(int64_t n, int d) {
    if (n < 1 || n > N_MAX || d < 1 || d > 2048) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { momv_scratch(c, n, d); });
}

int mtadgat_eval_moments_valid(const float* e_dev, int64_t n, int d, int64_t ld, void* scratch_dev, size_t scratch_bytes, double* out_host,
                               void* stream) {
    if (!e_dev || !scratch_dev || !out_host) return record_error(-1, "moments_valid: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "moments_valid: n must lie in [1, 2^31 - 1]");
    if (d < 1 || d > 2048) return record_error(-1, "moments_valid: d must lie in [1, 2048]");
    if (ld < d) return record_error(-1, "moments_valid: ld < d");
    ScratchCarver carver(scratch_dev);
    const MomvScratch l = momv_scratch(carver, n, d);
    if (scratch_bytes < carver.bytes()) return record_error(-5, "moments_valid: scratch too small (see mtadgat_eval_moments_valid_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "moments_valid: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_momv_blocks, dim3((unsigned)l.blocks, (unsigned)d), dim3(256), 0, s, e_dev, (long)n, (long)ld, l.part);
    hipLaunchKernelGGL(k_momv_columns, dim3((unsigned)d), dim3(64), 0, s, (const double*)l.part, l.blocks, l.out);
    if (hipGetLastError() != hipSuccess) return record_error(-3, "moments_valid: kernel launch failed");
    if (hipMemcpyAsync(out_host, l.out, 3 * (size_t)d * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
        return record_error(-3, "moments_valid: copy failed");
    return hipStreamSynchronize(s) == hipSuccess ? 0 : record_error(-3, "moments_valid: stream failed");
}

}  // extern "C"
