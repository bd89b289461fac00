// Mean of the attention maps over the windows of a call (mtadgat_attention_mean / _series_mean): the (n, K, K) softmax
// matrices of a chunk -- the post-softmax `attention` of FeatureAttentionLayer / TemporalAttentionLayer.forward
// (modules.py:85-89, :184-188), eval mode -- reduced to one (K, K) matrix without atomics, in two stages:
//   k_att_mean_part   per slab of consecutive windows of the chunk: compensated sum over its windows, added (or, for the
//                     call's first chunk, written) into that slab's running (sum, compensation) pair
//   k_att_mean_final  per element: compensated sum of the slabs' pairs over the windows of the call
// Every slab adds its windows in index order and the chunks arrive in order on one stream, so the result is the same bit
// for bit from run to run for a given chunk size.  Sums are Neumaier-compensated fp32: the error of a 65 536-window mean
// stays near one fp32 rounding of the result.
#include <algorithm>

#include "mtadgat_device.h"

namespace mtadgat {

namespace {

// (s, c) += x, Neumaier: s + c carries the sum, c the rounding errors of the additions into s
__device__ __forceinline__ void nadd(float& s, float& c, float x) {
    const float t = s + x;
    c += fabsf(s) >= fabsf(x) ? (s - t) + x : (x - t) + s;
    s = t;
}

template <int V>
struct Vec;
template <>
struct Vec<4> {
    __device__ static void get(const float* p, float (&v)[4]) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    __device__ static void put(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <>
struct Vec<1> {
    __device__ static void get(const float* p, float (&v)[1]) { v[0] = *p; }
    __device__ static void put(float* p, const float (&v)[1]) { *p = v[0]; }
};

constexpr int AM_THREADS = 256;
constexpr int AM_UNROLL = 4;     // windows whose loads are in flight together

// grid (column blocks, slabs).  Thread: VEC consecutive elements of the flattened (K, K) map.  A: (n, KK) maps of the chunk,
// PS / PC: (nslab, KK) running sums / compensations.  VEC = 4 needs KK % 4 == 0 (every window's map 16-byte aligned).
template <int VEC>
__global__ __launch_bounds__(AM_THREADS) void k_att_mean_part(const float* __restrict__ A, long n, long KK, int nslab, int first,
                                                              float* __restrict__ PS, float* __restrict__ PC) {
    const long e = ((long)blockIdx.x * AM_THREADS + threadIdx.x) * VEC;
    if (e >= KK) return;
    const int sl = blockIdx.y;
    const long w0 = n * sl / nslab, w1 = n * (sl + 1) / nslab;
    float s[VEC], c[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = c[k] = 0.f;
    const float* p = A + w0 * KK + e;
    long w = w0;
    for (; w + AM_UNROLL <= w1; w += AM_UNROLL, p += AM_UNROLL * KK) {
        float v[AM_UNROLL][VEC];
#pragma unroll
        for (int u = 0; u < AM_UNROLL; ++u) Vec<VEC>::get(p + u * KK, v[u]);
#pragma unroll
        for (int u = 0; u < AM_UNROLL; ++u)
#pragma unroll
            for (int k = 0; k < VEC; ++k) nadd(s[k], c[k], v[u][k]);
    }
    for (; w < w1; ++w, p += KK) {
        float v[VEC];
        Vec<VEC>::get(p, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) nadd(s[k], c[k], v[k]);
    }
    float* ps = PS + (long)sl * KK + e;
    float* pc = PC + (long)sl * KK + e;
    if (!first) {     // fold this chunk's pair into the slab's running pair
        float rs[VEC], rc[VEC];
        Vec<VEC>::get(ps, rs);
        Vec<VEC>::get(pc, rc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            nadd(rs[k], rc[k], s[k]);
            s[k] = rs[k];
            c[k] = rc[k] + c[k];
        }
    }
    Vec<VEC>::put(ps, s);
    Vec<VEC>::put(pc, c);
}

template <int VEC>
__global__ __launch_bounds__(AM_THREADS) void k_att_mean_final(const float* __restrict__ PS, const float* __restrict__ PC, long KK,
                                                               int nslab, float n_total, float* __restrict__ out) {
    const long e = ((long)blockIdx.x * AM_THREADS + threadIdx.x) * VEC;
    if (e >= KK) return;
    float s[VEC], c[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = c[k] = 0.f;
    for (int sl = 0; sl < nslab; ++sl) {
        float vs[VEC], vc[VEC];
        Vec<VEC>::get(PS + (long)sl * KK + e, vs);
        Vec<VEC>::get(PC + (long)sl * KK + e, vc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            nadd(s[k], c[k], vs[k]);
            c[k] += vc[k];
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) out[e + k] = (s[k] + c[k]) / n_total;     // (the caller's output: no alignment assumed)
}

inline int am_vec(long KK) { return KK % 4 == 0 ? 4 : 1; }
inline unsigned am_blocks(long KK) { return (unsigned)((KK / am_vec(KK) + AM_THREADS - 1) / AM_THREADS); }

}  // namespace

// Enough slabs that the first stage launches ~8 workgroups per CU of the 256 (W = 100: 10 column blocks x 205 slabs; F = 25:
// 3 x 683), at least 16 windows per slab so that a slab's loads stay in flight, one slab where the column blocks alone fill
// the machine (K = 2048: 4 096 column blocks).  A function of (n, K) only: the workspace query and the call agree on any device.
int att_mean_slabs(long n, int K) {
    const long KK = (long)K * K;
    const long want = (2048L + am_blocks(KK) - 1) / am_blocks(KK);
    long s = std::min<long>(want, std::max<long>(1, n / 16));
    s = std::min<long>(s, 1024);
    return (int)std::max<long>(1, s);
}

int launch_att_mean_part(const float* A, long n, int K, int nslab, int first, float* PS, float* PC, hipStream_t s) {
    if (n <= 0) return 0;
    const long KK = (long)K * K;
    const dim3 grid(am_blocks(KK), (unsigned)nslab);
    if (am_vec(KK) == 4)
        hipLaunchKernelGGL(k_att_mean_part<4>, grid, dim3(AM_THREADS), 0, s, A, n, KK, nslab, first, PS, PC);
    else
        hipLaunchKernelGGL(k_att_mean_part<1>, grid, dim3(AM_THREADS), 0, s, A, n, KK, nslab, first, PS, PC);
    LAUNCH_CHECK();
    return 0;
}

int launch_att_mean_final(const float* PS, const float* PC, int K, int nslab, long n_total, float* out, hipStream_t s) {
    const long KK = (long)K * K;
    if (am_vec(KK) == 4)
        hipLaunchKernelGGL(k_att_mean_final<4>, dim3(am_blocks(KK)), dim3(AM_THREADS), 0, s, PS, PC, KK, nslab, (float)n_total, out);
    else
        hipLaunchKernelGGL(k_att_mean_final<1>, dim3(am_blocks(KK)), dim3(AM_THREADS), 0, s, PS, PC, KK, nslab, (float)n_total, out);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace mtadgat
