// Score attribution (mtadgat_score_attribution): gradient and Integrated Gradients of the anomaly score of Predictor.get_score
// (reference prediction.py:65-91) with respect to the W + 1 series rows it reads.  For a score index i the slice
// S = series[i : i + W + 1] feeds two windows, A = S[0 : W] (its forecast is compared with the target row) and B = S[1 : W + 1]
// (its last reconstructed step is), and the target y = S[W, dims].  The library evaluates A and B with the training forward
// (no dropout) and the data-only backward; these kernels do the rest:
//   k_attr_gather   the A / B windows of a chunk of (index, step) units, interpolated b + alpha_k (S - b), read straight from
//                   the device-resident series, and the units' targets
//   k_attr_seed     d a / d preds, d a / d recons (only row W - 1 of B's reconstruction is non-zero) and d a / d y
//   k_attr_combine  A's d x into rows 0 .. W - 1, B's into rows 1 .. W, d a / d y into row W, summed over the steps in step
//                   order; after the last step (S - b) * sum / m (IG) or the sum itself (gradient)
// Every output element is written by one thread that adds its terms in a fixed order: no atomics, results are bit-identical
// from run to run, and the step sum does not depend on where the chunks cut it.
#include "mtadgat_device.h"
#include "mtadgat_kernels.h"

namespace mtadgat {

namespace {

__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }     // sign(0) = 0, as torch's abs backward

__device__ __forceinline__ float slice_value(const AttrArgs& a, long p, int k, int r, int f) {
    const float s = a.series[(a.idx[p] + r) * (long)a.F + f];
    if (a.steps == 0) return s;
    const float b = a.base_kind == 0 ? 0.f : (a.base_kind == 1 ? a.base[f] : a.base[(long)r * a.F + f]);
    const float alpha = ((float)k + 0.5f) / (float)a.steps;
    return b + alpha * (s - b);
}

__device__ __forceinline__ float base_value(const AttrArgs& a, int r, int f) {
    return a.base_kind == 0 ? 0.f : (a.base_kind == 1 ? a.base[f] : a.base[(long)r * a.F + f]);
}

unsigned grid_for(long n) {
    const long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace

__global__ __launch_bounds__(256) void k_attr_gather(const AttrArgs a) {
    const int W = a.W, F = a.F, od = a.od;
    const int ms = a.steps > 0 ? a.steps : 1;
    const long nu = a.nu;
    const long nslice = nu * (W + 1) * (long)F;
    const long total = nslice + nu * od;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        if (e < nslice) {
            const long v = e / ((long)(W + 1) * F);
            const int rf = (int)(e - v * (W + 1) * (long)F);
            const int r = rf / F, f = rf - r * F;
            const long u = a.u0 + v;
            const float val = slice_value(a, u / ms, (int)(u % ms), r, f);
            if (r < W) a.X[(v * W + r) * (long)F + f] = val;                    // window A, row r
            if (r >= 1) a.X[((nu + v) * W + r - 1) * (long)F + f] = val;        // window B, row r - 1
        } else {
            const long q = e - nslice;
            const long v = q / od;
            const int d = (int)(q - v * od);
            const long u = a.u0 + v;
            a.Y[q] = slice_value(a, u / ms, (int)(u % ms), W, a.dims[d]);
        }
    }
}

__global__ __launch_bounds__(256) void k_attr_seed(const AttrArgs a) {
    const int W = a.W, od = a.od;
    const long nu = a.nu;
    const long np = 2 * nu * od, nr = 2 * nu * (long)W * od;
    const long total = np + nr + nu * od;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        if (e < np) {                                   // d a / d preds: A windows only
            const long v = e / od;
            const int d = (int)(e - v * od);
            a.dpreds[e] = v < nu ? a.dim_w[d] * sgn(a.preds[e] - a.Y[v * od + d]) : 0.f;
        } else if (e < np + nr) {                       // d a / d recons: row W - 1 of the B windows only
            const long q = e - np;
            const long v = q / ((long)W * od);
            const int td = (int)(q - v * W * (long)od);
            const int t = td / od, d = td - t * od;
            a.drecons[q] = (v >= nu && t == W - 1) ? a.gamma * a.dim_w[d] * sgn(a.recons[q] - a.Y[(v - nu) * od + d]) : 0.f;
        } else {                                        // d a / d y (the target row's direct term)
            const long q = e - np - nr;
            const long v = q / od;
            const int d = (int)(q - v * od);
            const float y = a.Y[q];
            const float gp = a.dim_w[d] * sgn(a.preds[q] - y);
            const float gr = a.gamma * a.dim_w[d] * sgn(a.recons[((nu + v) * W + W - 1) * (long)od + d] - y);
            a.gy[q] = -gp - gr;
        }
    }
}

__global__ __launch_bounds__(256) void k_attr_combine(const AttrArgs a) {
    const int W = a.W, F = a.F, od = a.od;
    const int ms = a.steps > 0 ? a.steps : 1;
    const long nu = a.nu, u0 = a.u0, u1 = a.u0 + a.nu;
    const long p0 = u0 / ms, p1 = (u1 - 1) / ms;      // indices this chunk touches
    const long per = (long)(W + 1) * F;
    const long total = (p1 - p0 + 1) * per;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long p = p0 + e / per;
        const int rf = (int)(e % per);
        const int r = rf / F, f = rf - r * F;
        const long ua = max(u0, p * ms), ub = min(u1, (p + 1) * ms);
        float* o = a.out + p * per + rf;
        float acc = ua == p * ms ? 0.f : *o;            // the steps of earlier chunks
        for (long u = ua; u < ub; ++u) {
            const long v = u - u0;
            float c = 0.f;
            if (r < W) c += a.dx[(v * W + r) * (long)F + f];
            if (r >= 1) c += a.dx[((nu + v) * W + r - 1) * (long)F + f];
            if (r == W)
                for (int d = 0; d < od; ++d)
                    if (a.dims[d] == f) c += a.gy[v * od + d];
            acc += c;
        }
        if (ub == (p + 1) * ms && a.steps > 0) {
            const float s = a.series[(a.idx[p] + r) * (long)F + f];
            const float b = base_value(a, r, f);
            acc = (s - b) * (acc / (float)a.steps);
        }
        *o = acc;
    }
}

int launch_attr_gather(const AttrArgs& a, hipStream_t s) {
    if (a.nu <= 0) return 0;
    hipLaunchKernelGGL(k_attr_gather, dim3(grid_for(a.nu * ((long)(a.W + 1) * a.F + a.od))), dim3(256), 0, s, a);
    LAUNCH_CHECK();
    return 0;
}

int launch_attr_seed(const AttrArgs& a, hipStream_t s) {
    if (a.nu <= 0) return 0;
    hipLaunchKernelGGL(k_attr_seed, dim3(grid_for(a.nu * (long)a.od * (2 * (long)a.W + 3))), dim3(256), 0, s, a);
    LAUNCH_CHECK();
    return 0;
}

int launch_attr_combine(const AttrArgs& a, hipStream_t s) {
    if (a.nu <= 0) return 0;
    const int ms = a.steps > 0 ? a.steps : 1;
    const long np = (a.u0 + a.nu - 1) / ms - a.u0 / ms + 1;
    hipLaunchKernelGGL(k_attr_combine, dim3(grid_for(np * (long)(a.W + 1) * a.F)), dim3(256), 0, s, a);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace mtadgat
