// What surrounds mtadgat_forward_train / mtadgat_backward in an optimisation step on the windows of a device-resident series
// (fitting.SeriesTrainer): the window gather, the cotangents of the reference's loss sqrt(mse) + sqrt(mse) (training.py:100-130),
// the gradient norm with the step's set-up, and Adam.  tests/fit_refs.py is the specification.
//
//   k_fit_gather     x[w, t, :] = series[starts[w] + t, 0:F].  A thread takes four consecutive floats of the contiguous output,
//                    walking (w, t, f) across row and window ends; it reads them one float at a time -- series rows start at any
//                    multiple of 4 bytes (F = 5, 55) -- and stores them as one float4 where the output is 16-byte aligned.
//   k_fit_loss_grad  d_preds = float(double(preds - y) c_f), d_recons = float(double(recons - x) c_r) with c = 1 / (N rmse),
//                    rmse = sqrt(S / N) in float64 from the two batch sums S that mtadgat_eval_window_sse + mtadgat_eval_group_sums
//                    left on the device; y and x are read from the series.  The leading workgroups take the reconstruction, the
//                    rest the forecast; four consecutive outputs per thread as in the gather.  The masked instance
//                    (mtadgat_fit_masked_loss_grad; tests/fit_mask_refs.py) takes N from the batch's counts of observed terms and
//                    writes +0.0f where the series sample is not observed.
//   k_fit_sqnorm     per block of FIT_NORM_CHUNK gradient entries the float64 sum of double(g)^2: thread t adds entries t, t + 256, ..
//                    of the block in that order, then block_sum (mtadgat_scan.h).
//   k_fit_finish     one workgroup: the blocks' partials in the same order (thread t: partials t, t + 256, .., block_sum), then
//                    thread 0 writes the step record and the row of the log ring.
//   k_fit_adam       element-wise over (p, g, m, v) in float64 from the record, every result rounded to float32 once.
// No atomics, every sum in a fixed order: identical calls give identical bits.
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/mtadgat.h"      // the entry points' declarations, MTADGAT_FIT_STATE_FIELDS
#include "mtadgat_scan.h"

using namespace mtadgat;

namespace {

constexpr int64_t N_MAX = 2147483647LL;
constexpr int FIT_THREADS = 256;
constexpr int FIT_W_MAX = 512;             // the limits of mtadgat_eval_window_sse, whose sums the cotangents are formed from
constexpr int FIT_OUT_MAX = 2048;
constexpr int FIT_NORM_CHUNK = 4096;       // gradient entries per partial of the norm: 16 per thread
constexpr unsigned FIT_GRID_MAX = 1u << 16;  // workgroups of the grid-stride kernels

// the fields of the step record (float64 each): include/mtadgat.h, _native.FIT_STATE_FIELDS
enum { ST_T = 0, ST_CALLS, ST_CLIP, ST_STEP_SIZE, ST_BC2S, ST_APPLIED, ST_NORM_SQ, ST_NORM, ST_FIELDS };
static_assert(ST_FIELDS == MTADGAT_FIT_STATE_FIELDS, "the record of include/mtadgat.h");

inline unsigned grid_for(long quads) {
    const long blocks = (quads + FIT_THREADS - 1) / FIT_THREADS;
    return (unsigned)std::min<long>(std::max<long>(blocks, 1), FIT_GRID_MAX);
}

// position of a flat index into (windows, T, C) and its walk
struct Walk {
    long w;
    int t, c;
    __device__ Walk(long e, int T, int C) {
        const long row = e / C;
        c = (int)(e - row * C);
        w = row / T;
        t = (int)(row - w * T);
    }
    __device__ void next(int T, int C) {
        if (++c == C) {
            c = 0;
            if (++t == T) { t = 0; ++w; }
        }
    }
};

__global__ void __launch_bounds__(FIT_THREADS) k_fit_gather(const float* __restrict__ series, long ld, const long* __restrict__ starts,
                                                            long total, int W, int F, int vec, float* __restrict__ x) {
    const long quads = (total + 3) / 4;
    for (long q = (long)blockIdx.x * FIT_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * FIT_THREADS) {
        const long e0 = q * 4;
        const int n = total - e0 < 4 ? (int)(total - e0) : 4;
        Walk k(e0, W, F);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                v[j] = series[(starts[k.w] + k.t) * ld + k.c];
                k.next(W, F);
            }
        if (vec && n == 4) {
            *reinterpret_cast<float4*>(x + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) x[e0 + j] = v[j];
        }
    }
}

__device__ __forceinline__ bool finite64(double x) { return fabs(x) <= 1.79769313486231570815e308; }

// 1 / (N rmse) of one head and its rmse: 0 where the rmse is 0 (every residual is: the gradient of sqrt at 0 is taken as 0, torch
// gives 0 / 0), NaN where the sum is not finite (an infinite sum would otherwise give c = 0 and hide itself)
__device__ __forceinline__ double cotangent_scale(double S, double N, double& rmse) {
    rmse = sqrt(S / N);
    if (!finite64(S)) return NAN;
    return rmse == 0.0 ? 0.0 : 1.0 / (N * rmse);
}

// the masked step's scale (mtadgat_fit_masked_loss_grad): N counts the observed terms; a head without any has rmse 0 and c = 0
__device__ __forceinline__ double masked_cotangent_scale(double S, double N, double& rmse) {
    rmse = N > 0.0 ? sqrt(S / N) : 0.0;
    if (!finite64(S)) return NAN;
    return (N == 0.0 || rmse == 0.0) ? 0.0 : 1.0 / (N * rmse);
}

// What the masked instance takes on top: the samples' ages; an entry whose series sample is not observed (age > max_age) gets +0.0f
template <bool MASK>
struct GradMask {};
template <>
struct GradMask<true> {
    const int* age;      // (n_rows, F), row stride ld
    long ld;
    int max_age;
};

// grid: blocks_r workgroups over the reconstruction's quads, then the forecast's.  sums: (S_f, S_r), MASK: (S_f, S_r, N_f, N_r)
template <bool MASK>
__global__ void __launch_bounds__(FIT_THREADS) k_fit_loss_grad(const float* __restrict__ preds, const float* __restrict__ recons, long batch,
                                                               int W, int out, const float* __restrict__ series, long ld,
                                                               const long* __restrict__ starts, const int* __restrict__ dims,
                                                               const double* __restrict__ sums, unsigned blocks_r, int vec,
                                                               float* __restrict__ d_preds, float* __restrict__ d_recons,
                                                               double* __restrict__ rmse_out, GradMask<MASK> mask) {
    const bool fore = blockIdx.x >= blocks_r;                          // (workgroup-uniform)
    const int T = fore ? 1 : W, t0 = fore ? W : 0;                      // the forecast is compared with row s + W
    const float* __restrict__ src = fore ? preds : recons;
    float* __restrict__ dst = fore ? d_preds : d_recons;
    const long total = batch * T * out;
    double rmse, c;
    if constexpr (MASK) c = masked_cotangent_scale(sums[fore ? 0 : 1], sums[fore ? 2 : 3], rmse);
    else c = cotangent_scale(sums[fore ? 0 : 1], (double)total, rmse);
    const unsigned b0 = fore ? blockIdx.x - blocks_r : blockIdx.x, nb = fore ? gridDim.x - blocks_r : blocks_r;
    if (b0 == 0 && threadIdx.x == 0) rmse_out[fore ? 0 : 1] = rmse;
    const long quads = (total + 3) / 4;
    for (long q = (long)b0 * FIT_THREADS + threadIdx.x; q < quads; q += (long)nb * FIT_THREADS) {
        const long e0 = q * 4;
        const int n = total - e0 < 4 ? (int)(total - e0) : 4;
        const bool v4 = vec && n == 4;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (v4) {
            const float4 f = *reinterpret_cast<const float4*>(src + e0);
            a[0] = f.x; a[1] = f.y; a[2] = f.z; a[3] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) a[j] = src[e0 + j];
        }
        Walk k(e0, T, out);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                const long row = starts[k.w] + t0 + k.t;
                const int col = dims ? dims[k.c] : k.c;
                const float y = series[row * ld + col];
                const float df = a[j] - y;                              // ONE float32 subtraction: window_sse's difference
                a[j] = (float)((double)df * c);
                if constexpr (MASK) {
                    if (mask.age[row * mask.ld + col] > mask.max_age) a[j] = 0.f;      // (a select: a NaN product does not pass)
                }
                k.next(T, out);
            }
        if (v4) {
            *reinterpret_cast<float4*>(dst + e0) = make_float4(a[0], a[1], a[2], a[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) dst[e0 + j] = a[j];
        }
    }
}

// grid: ceil(n / FIT_NORM_CHUNK)
__global__ void __launch_bounds__(FIT_THREADS) k_fit_sqnorm(const float* __restrict__ g, long n, double* __restrict__ part) {
    __shared__ double sm[FIT_THREADS];
    const long i0 = (long)blockIdx.x * FIT_NORM_CHUNK, i1 = i0 + FIT_NORM_CHUNK < n ? i0 + FIT_NORM_CHUNK : n;
    double v = 0.0;
#pragma unroll 4
    for (long i = i0 + threadIdx.x; i < i1; i += FIT_THREADS) {
        const double x = (double)g[i];
        v += x * x;                                                    // (the square of a float32 is exact in float64)
    }
    v = block_sum(v, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// b^t by squaring, the multiplications in THE order of fit_refs.int_power: both sides of a comparison get the same bits
__device__ __forceinline__ double int_power(double b, long t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

// one workgroup
__global__ void __launch_bounds__(FIT_THREADS) k_fit_finish(const double* __restrict__ part, long nparts, const double* __restrict__ rmse,
                                                            double lr, double beta1, double beta2, double max_norm, int skip_nonfinite,
                                                            double* __restrict__ state, double* __restrict__ log, long capacity) {
    __shared__ double sm[FIT_THREADS];
    double v = 0.0;
    for (long i = threadIdx.x; i < nparts; i += FIT_THREADS) v += part[i];
    v = block_sum(v, sm);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(v), rf = rmse[0], rr = rmse[1];
    const bool finite = finite64(norm) && finite64(rf) && finite64(rr);
    const double applied = (skip_nonfinite && !finite) ? 0.0 : 1.0;
    // (a record the caller did not zero must not send the log's row out of the ring)
    const double c0 = state[ST_CALLS], t0 = state[ST_T];
    const long calls = c0 >= 0.0 && c0 < 9.0e15 ? (long)c0 : 0;
    const long t = (t0 >= 0.0 && t0 < 9.0e15 ? (long)t0 : 0) + (applied != 0.0 ? 1 : 0);
    double clip = 1.0;
    if (max_norm >= 0.0) {
        clip = max_norm / (norm + 1e-6);
        if (clip > 1.0) clip = 1.0;                                     // (a NaN norm stays NaN: torch's clamp)
    }
    state[ST_CALLS] = (double)(calls + 1);
    state[ST_APPLIED] = applied;
    state[ST_NORM_SQ] = v;
    state[ST_NORM] = norm;
    if (applied != 0.0) {
        state[ST_T] = (double)t;
        state[ST_CLIP] = clip;
        state[ST_STEP_SIZE] = lr / (1.0 - int_power(beta1, t));
        state[ST_BC2S] = sqrt(1.0 - int_power(beta2, t));
    }
    double* row = log + (calls % capacity) * 4;
    row[0] = rf;
    row[1] = rr;
    row[2] = norm;
    row[3] = applied;
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, double clip, double step_size, double bc2s, double lr,
                                         double beta1, double beta2, double eps, double wd, int decoupled) {
#pragma clang fp contract(off)                                          // every product rounded: the arithmetic of fit_refs.adam_step
    double pd = (double)p, gd = (double)g * clip;
    if (wd != 0.0) {
        if (decoupled) pd = pd * (1.0 - lr * wd);
        else gd = gd + wd * pd;
    }
    const double md = beta1 * (double)m + (1.0 - beta1) * gd;
    const double vd = beta2 * (double)v + (1.0 - beta2) * (gd * gd);
    pd = pd - step_size * (md / (sqrt(vd) / bc2s + eps));
    p = (float)pd;
    m = (float)md;
    v = (float)vd;
}

__global__ void __launch_bounds__(FIT_THREADS) k_fit_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long n, const double* __restrict__ state, double lr,
                                                          double beta1, double beta2, double eps, double wd, int decoupled, int vec) {
    if (state[ST_APPLIED] == 0.0) return;                               // (uniform) a skipped step writes nothing
    const double clip = state[ST_CLIP], step_size = state[ST_STEP_SIZE], bc2s = state[ST_BC2S];
    const long quads = (n + 3) / 4;
    for (long q = (long)blockIdx.x * FIT_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * FIT_THREADS) {
        const long e0 = q * 4;
        const int k = n - e0 < 4 ? (int)(n - e0) : 4;
        if (vec && k == 4) {
            float4 P = *reinterpret_cast<float4*>(p + e0), M = *reinterpret_cast<float4*>(m + e0), V = *reinterpret_cast<float4*>(v + e0);
            const float4 G = *reinterpret_cast<const float4*>(g + e0);
            adam_one(P.x, G.x, M.x, V.x, clip, step_size, bc2s, lr, beta1, beta2, eps, wd, decoupled);
            adam_one(P.y, G.y, M.y, V.y, clip, step_size, bc2s, lr, beta1, beta2, eps, wd, decoupled);
            adam_one(P.z, G.z, M.z, V.z, clip, step_size, bc2s, lr, beta1, beta2, eps, wd, decoupled);
            adam_one(P.w, G.w, M.w, V.w, clip, step_size, bc2s, lr, beta1, beta2, eps, wd, decoupled);
            *reinterpret_cast<float4*>(p + e0) = P;
            *reinterpret_cast<float4*>(m + e0) = M;
            *reinterpret_cast<float4*>(v + e0) = V;
        } else {
            for (int j = 0; j < k; ++j) adam_one(p[e0 + j], g[e0 + j], m[e0 + j], v[e0 + j], clip, step_size, bc2s, lr, beta1, beta2, eps, wd, decoupled);
        }
    }
}

inline bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }
inline bool unit_open(double b) { return b >= 0.0 && b < 1.0; }          // (false for a NaN)

// mtadgat_fit_loss_grad (MASK false) and mtadgat_fit_masked_loss_grad (MASK true)
template <bool MASK>
int loss_grad_call(const char* what, const float* preds_dev, const float* recons_dev, int64_t batch, int W, int out_dim,
                   const float* series_dev, int64_t n_rows, int F, int64_t ld_series, const int64_t* starts_dev, const int32_t* dims_dev,
                   GradMask<MASK> mask, const double* sums_dev, float* d_preds_dev, float* d_recons_dev, double* rmse_dev, void* stream) {
    const std::string w(what);
    auto refuse = [&](int code, const char* msg) { return record_error(code, (w + msg).c_str()); };
    if (!preds_dev || !recons_dev || !series_dev || !starts_dev || !sums_dev || !d_preds_dev || !d_recons_dev || !rmse_dev)
        return refuse(-1, ": null pointer");
    if (batch < 1 || batch > N_MAX) return refuse(-1, ": batch must lie in [1, 2^31 - 1]");
    if (out_dim < 1 || out_dim > FIT_OUT_MAX) return refuse(-1, ": out_dim must lie in [1, 2048]");
    if (W < 1 || W > FIT_W_MAX) return refuse(-1, ": W must lie in [1, 512]");
    if (F < 1 || ld_series < F) return refuse(-1, ": ld_series < F or F < 1");
    if (!dims_dev && out_dim > F) return refuse(-1, ": out_dim > F needs dims_dev");
    if (n_rows < (int64_t)W + 1) return refuse(-1, ": the series is shorter than a window and its target row");
    const unsigned blocks_r = grid_for(((long)batch * W * out_dim + 3) / 4), blocks_f = grid_for(((long)batch * out_dim + 3) / 4);
    const int vec = aligned16(preds_dev) && aligned16(recons_dev) && aligned16(d_preds_dev) && aligned16(d_recons_dev) ? 1 : 0;
    hipLaunchKernelGGL(k_fit_loss_grad<MASK>, dim3(blocks_r + blocks_f), dim3(FIT_THREADS), 0, (hipStream_t)stream, preds_dev, recons_dev,
                       (long)batch, W, out_dim, series_dev, (long)ld_series, reinterpret_cast<const long*>(starts_dev), dims_dev, sums_dev,
                       blocks_r, vec, d_preds_dev, d_recons_dev, rmse_dev, mask);
    return hipGetLastError() == hipSuccess ? 0 : refuse(-3, ": kernel launch failed");
}

}  // namespace

extern "C" {

int mtadgat_fit_gather(const float* series_dev, int64_t n_rows, int F, int64_t ld_series, const int64_t* starts_dev, int64_t batch, int W,
                       float* x_dev, void* stream) {
    if (!series_dev || !starts_dev || !x_dev) return record_error(-1, "fit_gather: null pointer");
    if (batch < 1 || batch > N_MAX) return record_error(-1, "fit_gather: batch must lie in [1, 2^31 - 1]");
    if (W < 1 || W > FIT_W_MAX) return record_error(-1, "fit_gather: W must lie in [1, 512]");
    if (F < 1 || F > FIT_OUT_MAX || ld_series < F) return record_error(-1, "fit_gather: ld_series < F or F outside [1, 2048]");
    if (n_rows < (int64_t)W) return record_error(-1, "fit_gather: the series is shorter than a window");
    const long total = (long)batch * W * F;
    hipLaunchKernelGGL(k_fit_gather, dim3(grid_for((total + 3) / 4)), dim3(FIT_THREADS), 0, (hipStream_t)stream, series_dev, (long)ld_series,
                       reinterpret_cast<const long*>(starts_dev), total, W, F, aligned16(x_dev) ? 1 : 0, x_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "fit_gather: kernel launch failed");
}

int mtadgat_fit_loss_grad(const float* preds_dev, const float* recons_dev, int64_t batch, int W, int out_dim, const float* series_dev,
                          int64_t n_rows, int F, int64_t ld_series, const int64_t* starts_dev, const int32_t* dims_dev,
                          const double* sums_dev, float* d_preds_dev, float* d_recons_dev, double* rmse_dev, void* stream) {
    return loss_grad_call<false>("fit_loss_grad", preds_dev, recons_dev, batch, W, out_dim, series_dev, n_rows, F, ld_series, starts_dev,
                                 dims_dev, GradMask<false>{}, sums_dev, d_preds_dev, d_recons_dev, rmse_dev, stream);
}

int mtadgat_fit_masked_loss_grad(const float* preds_dev, const float* recons_dev, int64_t batch, int W, int out_dim, const float* series_dev,
                                 int64_t n_rows, int F, int64_t ld_series, const int64_t* starts_dev, const int32_t* dims_dev,
                                 const int32_t* age_dev, int64_t ld_age, int32_t max_age, const double* sums_dev, float* d_preds_dev,
                                 float* d_recons_dev, double* rmse_dev, void* stream) {
    if (!age_dev) return record_error(-1, "fit_masked_loss_grad: null pointer");
    if (ld_age < F) return record_error(-1, "fit_masked_loss_grad: ld_age < F");
    GradMask<true> mask;
    mask.age = age_dev;
    mask.ld = (long)ld_age;
    mask.max_age = (int)max_age;
    return loss_grad_call<true>("fit_masked_loss_grad", preds_dev, recons_dev, batch, W, out_dim, series_dev, n_rows, F, ld_series, starts_dev,
                                dims_dev, mask, sums_dev, d_preds_dev, d_recons_dev, rmse_dev, stream);
}

size_t mtadgat_fit_prepare_scratch(int64_t n) {
    if (n < 1 || n > N_MAX) return 0;
    return scratch_bytes_of([&](ScratchCarver& c) { c.take<double>((size_t)((n + FIT_NORM_CHUNK - 1) / FIT_NORM_CHUNK)); });
}

int mtadgat_fit_prepare(const float* grads_dev, int64_t n, const double* rmse_dev, double lr, double beta1, double beta2, double max_norm,
                        int skip_nonfinite, double* state_dev, double* log_dev, int64_t capacity, void* scratch_dev, size_t scratch_bytes,
                        void* stream) {
    if (!grads_dev || !rmse_dev || !state_dev || !log_dev || !scratch_dev) return record_error(-1, "fit_prepare: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "fit_prepare: n must lie in [1, 2^31 - 1]");
    if (!(lr >= 0.0) || std::isinf(lr)) return record_error(-1, "fit_prepare: lr must be finite and >= 0");
    if (!unit_open(beta1) || !unit_open(beta2)) return record_error(-1, "fit_prepare: betas must lie in [0, 1)");
    if (std::isnan(max_norm)) return record_error(-1, "fit_prepare: max_norm is NaN (negative: no clipping)");
    if (skip_nonfinite != 0 && skip_nonfinite != 1) return record_error(-1, "fit_prepare: skip_nonfinite must be 0 or 1");
    if (capacity < 1 || capacity > N_MAX) return record_error(-1, "fit_prepare: the log's capacity must lie in [1, 2^31 - 1]");
    if (scratch_bytes < mtadgat_fit_prepare_scratch(n)) return record_error(-5, "fit_prepare: scratch too small (see mtadgat_fit_prepare_scratch)");
    if ((uintptr_t)scratch_dev & 7) return record_error(-5, "fit_prepare: scratch must be 8-byte aligned");
    ScratchCarver carver(scratch_dev);
    const long nparts = (long)((n + FIT_NORM_CHUNK - 1) / FIT_NORM_CHUNK);
    double* part = carver.take<double>((size_t)nparts);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_fit_sqnorm, dim3((unsigned)nparts), dim3(FIT_THREADS), 0, s, grads_dev, (long)n, part);
    hipLaunchKernelGGL(k_fit_finish, dim3(1), dim3(FIT_THREADS), 0, s, (const double*)part, nparts, rmse_dev, lr, beta1, beta2, max_norm,
                       skip_nonfinite, state_dev, log_dev, (long)capacity);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "fit_prepare: kernel launch failed");
}

int mtadgat_fit_adam(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n, const double* state_dev,
                     double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, void* stream) {
    if (!params_dev || !grads_dev || !exp_avg_dev || !exp_avg_sq_dev || !state_dev) return record_error(-1, "fit_adam: null pointer");
    if (n < 1 || n > N_MAX) return record_error(-1, "fit_adam: n must lie in [1, 2^31 - 1]");
    if (!(lr >= 0.0) || std::isinf(lr)) return record_error(-1, "fit_adam: lr must be finite and >= 0");
    if (!unit_open(beta1) || !unit_open(beta2)) return record_error(-1, "fit_adam: betas must lie in [0, 1)");
    if (!(eps >= 0.0) || std::isinf(eps)) return record_error(-1, "fit_adam: eps must be finite and >= 0");
    if (!(weight_decay >= 0.0) || std::isinf(weight_decay)) return record_error(-1, "fit_adam: weight_decay must be finite and >= 0");
    if (decoupled != 0 && decoupled != 1) return record_error(-1, "fit_adam: decoupled must be 0 or 1");
    const int vec = aligned16(params_dev) && aligned16(grads_dev) && aligned16(exp_avg_dev) && aligned16(exp_avg_sq_dev) ? 1 : 0;
    hipLaunchKernelGGL(k_fit_adam, dim3(grid_for((n + 3) / 4)), dim3(FIT_THREADS), 0, (hipStream_t)stream, params_dev, grads_dev, exp_avg_dev,
                       exp_avg_sq_dev, (long)n, state_dev, lr, beta1, beta2, eps, weight_decay, decoupled, vec);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "fit_adam: kernel launch failed");
}

}  // extern "C"
