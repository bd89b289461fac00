// k_attend: graph attention of the layers beyond k_gat_wide (more than 512 nodes or node dimensions) + launcher
#include "mtadgat_device.h"

namespace mtadgat {

namespace {

#ifndef MTADGAT_ATTEND_DEPTH
#define MTADGAT_ATTEND_DEPTH 2
#endif

// ---------------------------------------------------------------------------
// attend: complete-graph attention of one layer through an (B, K, K) score matrix in memory,
// reference FeatureAttentionLayer.forward (modules.py:65-95) / TemporalAttentionLayer.forward
// (modules.py:166-193), in three launches:
//   k_attend          scores e_ij (+ bias) of a block of IB query rows x 64 JPL keys of one window -> S
//   k_attend_softmax  S <- softmax over j, in place, a wave per row (K <= 2048)
//   k_bgemm           h = sigmoid(S V) on the fp32 matrix pipe (mtadgat_bwdw.hip, sigmoid epilogue)
// Serves the feature layer of F > 512 (K = F up to 2048 keys, D = W) and the temporal layer of
// F > 512 (K = W, D = F, E = 2F up to 4096 embedding columns); k_gat_wide keeps every layer up to 512.
//
// GATv2 score, re-associated:
//   e_ij = c_i + d_j + sum_{k in P} |L'_ik + R'_jk| - sum_{k in N} |L'_ik + R'_jk| + bias_ij
// with L', R', c, d produced by k_rowgemm from the packed projection (columns
// [0,PT) = L', [PT,2PT) = R', 2PT = c, 2PT+1 = d of each node's row in LR).
// GAT (v1): e_ij = LeakyReLU(c_i + d_j) + bias_ij (PT = 0).
//
// lane <-> key node j (JPL nodes per lane), the inner loop is 2 VALU ops/element.
// ---------------------------------------------------------------------------
// one 8-wide k tile of the pairwise term for all IB query rows.
//   r[jj][e]  : R'[k0+e][j]  for this lane's key nodes j (one VGPR each)
//   lt[x]     : L' tile, lane n of every 16-lane row holds L'[row 2x + (n>>3)][k0 + (n&7)]
// so L'_ik reaches all lanes through a DPP row broadcast fused into the add: 2 VALU ops/element
// (v_add_f32_dpp + v_add_f32 |t|), no scalar loads, no LDS.  Measured on MI355X (scratch
// microbenchmark): DPP add 4.3 cycles, |abs| accumulate 2.7 cycles per wave64
// instruction with >= 2 waves/SIMD.  A software-pipelined variant (no back-to-back dependent pair,
// no s_nop) measured slower because its extra live temporaries cost a wave of occupancy.
template <int JPL, int IB, bool NEG>
__device__ __forceinline__ void attend_tile(float (&acc)[IB][JPL], const float (&r)[JPL][8], const float (&lt)[IB / 2]) {
#pragma unroll
    for (int x = 0; x < IB / 2; ++x) {
        const float lv = lt[x];
        static_for<0, 16>([&](auto nn) {
            constexpr int N = decltype(nn)::value;
            constexpr int e = N & 7;
            const int ib = 2 * x + (N >> 3);
#pragma unroll
            for (int jj = 0; jj < JPL; ++jj) {
                const float t = row_bcast<N>(lv) + r[jj][e];
                if (NEG)
                    acc[ib][jj] -= fabsf(t);
                else
                    acc[ib][jj] += fabsf(t);
            }
        });
    }
}

template <int JPL, int IB>
__global__ __launch_bounds__(64, 3) void k_attend(const AttendArgs a) {
    static_assert(IB % 2 == 0 && IB <= 32, "IB");
    constexpr int NL = IB / 2;
    const int lane = threadIdx.x;
    // block -> (window, key block, row block), row blocks fastest: the row blocks of one key block share its R'^T columns in L2
    const long blk = blockIdx.x;
    const int nrb = (a.K + IB - 1) / IB, nkb = (a.K + 64 * JPL - 1) / (64 * JPL);
    const long win = blk / ((long)nrb * nkb);
    const int rem = (int)(blk - win * nrb * nkb);
    const int kb = rem / nrb, rb = rem - kb * nrb;
    const int i0 = rb * IB, j0 = kb * 64 * JPL;
    const int nrows = min(IB, a.K - i0);
    const int K = a.K, ldl = a.ldl, PT = a.ord ? a.ord[1] : a.PT, Kp = a.Kp;
    const float* __restrict__ Lrow0 = a.LC + (win * K + i0) * (long)ldl;
    const float* __restrict__ RTw = a.RT + win * (long)a.rt_rows * Kp;

    float acc[IB][JPL];
#pragma unroll
    for (int ib = 0; ib < IB; ++ib)
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) acc[ib][jj] = 0.f;

    int jc[JPL];                  // this lane's key nodes, clamped (results past K are dropped below)
    const float* Rp[JPL];
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        const int j = j0 + jj * 64 + lane;
        jc[jj] = j < K ? j : K - 1;
        Rp[jj] = RTw + jc[jj];
    }
    // rows past the end of the block are clamped duplicates; their results are dropped below
    int loff[NL];
    {
        const int n16 = lane & 15;
#pragma unroll
        for (int x = 0; x < NL; ++x) {
            const int i = 2 * x + (n16 >> 3);
            loff[x] = (i < nrows ? i : nrows - 1) * ldl + (n16 & 7);
        }
    }
    if (PT > 0) {
        // register ring over the k tiles: tile t+DEPTH-1 is requested before tile t is consumed
        constexpr int DEPTH = MTADGAT_ATTEND_DEPTH;
        float rr[DEPTH][JPL][8], lr[DEPTH][NL];
        const int ntile = PT >> 3;
        auto fetch = [&](int st, int tile) {
            const int k1 = (tile < ntile ? tile : ntile - 1) << 3;
#pragma unroll
            for (int jj = 0; jj < JPL; ++jj)
#pragma unroll
                for (int e = 0; e < 8; ++e) rr[st][jj][e] = Rp[jj][(long)(k1 + e) * Kp];
#pragma unroll
            for (int x = 0; x < NL; ++x) lr[st][x] = Lrow0[loff[x] + k1];
        };
#pragma unroll
        for (int st = 0; st < DEPTH - 1; ++st) fetch(st, st);
        const int ptile = (a.ord ? a.ord[0] : a.P8) >> 3;
        for (int t0 = 0; t0 < ntile; t0 += DEPTH) {
#pragma unroll
            for (int st = 0; st < DEPTH; ++st) {
                const int t = t0 + st;
                if (t < ntile) {
                    fetch((st + DEPTH - 1) % DEPTH, t + DEPTH - 1);
                    if (t < ptile)
                        attend_tile<JPL, IB, false>(acc, rr[st], lr[st]);
                    else
                        attend_tile<JPL, IB, true>(acc, rr[st], lr[st]);
                }
            }
        }
    }

    // e_ij = c_i + d_j + pair term (GATv2) / LeakyReLU(c_i + d_j) (GAT v1), + bias_ij
    float dj[JPL];
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) dj[jj] = Rp[jj][(long)PT * Kp];
    const float cvec = Lrow0[(long)(lane < nrows ? lane : nrows - 1) * ldl + PT];   // lane ib holds c_ib
    float* __restrict__ Sw = a.S + (win * K + i0) * (long)K;
#pragma unroll
    for (int ib = 0; ib < IB; ++ib) {
        const float ci = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cvec), ib));
        const int irow = i0 + (ib < nrows ? ib : nrows - 1);
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) {
            float v = acc[ib][jj] + ci + dj[jj];
            if (a.v1) v = fmaxf(v, 0.f) + a.alpha * fminf(v, 0.f);
            if (a.bias) v += a.bias[(long)irow * K + jc[jj]];
            const int j = j0 + jj * 64 + lane;
            if (ib < nrows && j < K) Sw[(long)ib * K + j] = v;
        }
    }
}

// softmax over the keys of each score row (reference modules.py:85-89 / :184-188), in place; one wave per row,
// the row in registers (32 per lane: K <= 2048)
__global__ __launch_bounds__(256) void k_attend_softmax(float* __restrict__ S, long rows, int K) {
    constexpr int NJ = 32;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* __restrict__ p = S + row * K;
    float e[NJ];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        const int j = q * 64 + lane;
        e[q] = j < K ? p[j] : -INFINITY;
        m = fmaxf(m, e[q]);
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        e[q] = (q * 64 + lane < K) ? soft_exp(e[q] - m) : 0.f;
        sum += e[q];
    }
    sum = wave_sum(sum);
    const float inv = soft_rcp(sum);
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        const int j = q * 64 + lane;
        if (j < K) p[j] = e[q] * inv;
    }
}

}  // namespace

int launch_attend(const AttendArgs& a, const DropArgs* drop, unsigned drop_stream, hipStream_t s) {
    if (a.nwin <= 0) return 0;
    if (a.K < 1 || a.K > MTADGAT_ATTEND_MAX_K) return -2;
    constexpr int JPL = 2, IB = 16;
    const long nrb = (a.K + IB - 1) / IB, nkb = (a.K + 64 * JPL - 1) / (64 * JPL);
    const long grid = a.nwin * nrb * nkb;
    if (grid > 0x7fffffffL) return -2;
    hipLaunchKernelGGL((k_attend<JPL, IB>), dim3((unsigned)grid), dim3(64), 0, s, a);
    LAUNCH_CHECK();
    const long rows = a.nwin * a.K;
    if ((rows + 3) / 4 > 0x7fffffffL) return -2;
    hipLaunchKernelGGL(k_attend_softmax, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a.S, rows, a.K);
    LAUNCH_CHECK();
    // h_i = sigmoid(sum_j att'_ij V_j), att' = dropout(att) (same counter stream as k_gat_wide): C_b(i, d) = out[b so_w + i so_i + d so_d]
    return launch_bgemm_sigmoid(a.S, (long)a.K * a.K, a.K, 1, a.V, (long)a.K * a.ldv, a.ldv, 1, a.out, a.so_w, a.so_i, a.so_d,
                                a.K, a.D, a.K, a.nwin, drop, drop_stream, a.K, s);
}

}  // namespace mtadgat
