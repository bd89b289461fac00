// Scores of a gappy series (evaluation.scored_rows, anomaly_scores(age=), moving_average / find_epsilon(skip_nan=True)): a score exists
// exactly where mtadgat_fit_windows would have drawn a training window, and NaN means "no score".  tests/score_mask_refs.py is the
// specification.  (The exact select that skips NaN, mtadgat_eval_column_quantiles_valid, and the moving average over observed rows,
// mtadgat_eval_ewm_valid, are instantiations of the column select and of the exponentially weighted scan in mtadgat_evalcol.hip.)
//
//   k_mark_clear / k_mark_set   keep[i] = 1 for the starts mtadgat_fit_windows left on the device, 0 elsewhere; the count is read
//                               on the device.
//   k_eval_scores_masked        k_eval_scores' expression where the target sample is observed and the row is kept, the canonical NaN
//                               elsewhere; the mean over the observed terms in column order, by a select.
//   k_eval_row_means_valid      that mean over the non-NaN entries of the rows of an array that was scaled after masking.
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
