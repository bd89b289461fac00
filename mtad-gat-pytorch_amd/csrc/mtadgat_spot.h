// Peaks-over-threshold thresholds (SPOT, Siffer et al., KDD 2017): the generalized Pareto fit and the per-score step, written once.
//
// The scalar logic below is __host__ __device__ and is parameterised only by "sum this function over the peaks": a Peaks type
// supplies moments() and sums() over the m stored excesses Y_i > 0, oldest first, in ONE summation order -- lane l adds its elements
// i = l (mod 64) in ascending order, then an xor butterfly (32, 16, .. 1) combines the lanes.  RingPeaks does that with a wave over
// a column's ring in memory; HostPeaks emulates the same order on the host (mtadgat_spot_fit_host).  Kernels (mtadgat_spot.hip:
// k_spot_calibrate, k_spot_run; mtadgat_stream.hip: k_stream_score<true>) and the host hook therefore run the same statements.
// All arithmetic is float64 and nothing is contracted into fused multiply-adds, so the two sides differ in libm's last bits only.
//
// The definition is this package's own reading of the paper (Grimshaw's reduction to the roots of one scalar function), not a
// port of the reference's spot.py, whose optimiser-based root search cannot be reproduced bit for bit; tests/spot_refs.py is the
// specification.
//   Ymean = sum(Y) / m,   u(x) = 1 + sum(log(1 + x Y_i)) / m,   v(x) = sum(1 / (1 + x Y_i)) / m,   w(x) = u(x) v(x) - 1
//   candidates, in this order: the exponential tail (gamma, sigma) = (0, Ymean); the roots of w in (-1/Ymax + e, -1e-3 / Ymean),
//   ascending (e = 1e-8, or 1 / (32 Ymax) when 1/Ymax < 2e; skipped when empty); the roots of w in (2 (Ymean - Ymin) / (Ymean Ymin),
//   2 (Ymean - Ymin) / Ymin^2), ascending, when Ymean > Ymin.  The left interval stops at -1e-3 / Ymean, not at -e: w has a double
//   root at 0 and its sign that close to it is rounding noise; a root lost there has |gamma| < ~1e-3 and the exponential candidate
//   stands in for it.
//   roots: w at 32 points lo + (hi - lo) k / 31; adjacent finite values whose (w < 0) differ bracket a root; 64 bisections, the end
//   whose (w < 0) equals the midpoint's is replaced; the root is the last interval's midpoint.  A root x gives gamma = u(x) - 1,
//   sigma = gamma / x, kept when sigma is finite and positive and gamma != 0.
//   choice: the largest finite L = -m log sigma - (1 + 1/gamma) sum(log(1 + (gamma / sigma) Y_i))  (L = -m (1 + log Ymean) for
//   gamma = 0); ties go to the earlier candidate.
//   threshold, r = q n / Nt:  z = t + (sigma / gamma) (r^-gamma - 1), or t - sigma log r for gamma = 0.
#ifndef MTADGAT_SPOT_H
#define MTADGAT_SPOT_H
#include <hip/hip_runtime.h>
#include <math.h>

namespace mtadgat {

constexpr long SPOT_MAGIC = 0x53504f5431LL;     // "SPOT1"
constexpr long SPOT_MIN_PEAKS = 8, SPOT_MAX_PEAKS = 4096, SPOT_MIN_INIT = 16;

struct SpotHeader {          // 64 bytes; written by k_spot_calibrate, checked by every kernel against its arguments
    long magic, S, P, dynamic, n_init;
    double q, level;
    long pad;
};
struct SpotCol {             // 64 bytes per column
    double t, z, gamma, sigma;       // initial threshold, alarm threshold, the fitted tail
    long n, Nt;                      // observations, excesses ever seen (the ring holds the last min(Nt, P) of them)
    long err;                        // 0, or why calibration refused the column (SPOT_ERR_*)
    long pad;
};
constexpr long SPOT_ERR_FEW = 1, SPOT_ERR_NAN = 2, SPOT_ERR_MEAN = 3;

// byte offsets into a state of S columns with rings of P excesses: header | S columns | S rings of P float64
__host__ __device__ inline size_t spot_cols_offset() { return sizeof(SpotHeader); }
__host__ __device__ inline size_t spot_ring_offset(long S) { return sizeof(SpotHeader) + sizeof(SpotCol) * (size_t)S; }
__host__ __device__ inline size_t spot_state_bytes(long S, long P) { return spot_ring_offset(S) + 8 * (size_t)S * (size_t)P; }

struct SpotFit {
    double gamma, sigma, z;
};

__host__ __device__ inline bool spot_finite(double v) { return __builtin_isfinite(v); }

// u(x) and w(x)
template <class Peaks>
__host__ __device__ inline void spot_uw(const Peaks& pk, double x, double* u, double* w) {
#pragma clang fp contract(off)
    double sl, si;
    pk.sums(x, &sl, &si);
    const double m = (double)pk.m;
    const double uu = 1.0 + sl / m;
    const double vv = si / m;
    *u = uu;
    *w = uu * vv - 1.0;
}

// the candidate of root x, taken when it is valid and its likelihood is finite and larger than the best so far
template <class Peaks>
__host__ __device__ inline void spot_consider(const Peaks& pk, double x, SpotFit* best, double* bestL) {
#pragma clang fp contract(off)
    double u, w;
    spot_uw(pk, x, &u, &w);
    const double g = u - 1.0;
    const double s = g / x;
    if (!(spot_finite(s) && s > 0.0) || g == 0.0 || g != g) return;
    double sl, si;
    pk.sums(g / s, &sl, &si);
    const double L = -(double)pk.m * log(s) - (1.0 + 1.0 / g) * sl;
    if (spot_finite(L) && L > *bestL) {
        *bestL = L;
        best->gamma = g;
        best->sigma = s;
    }
}

// the roots of w in (lo, hi), ascending, each offered to spot_consider
template <class Peaks>
__host__ __device__ inline void spot_roots(const Peaks& pk, double lo, double hi, SpotFit* best, double* bestL) {
#pragma clang fp contract(off)
    double xp = lo, up, wp;
    spot_uw(pk, xp, &up, &wp);
    for (int k = 1; k < 32; ++k) {
        const double xk = lo + (hi - lo) * (double)k / 31.0;
        double uk, wk;
        spot_uw(pk, xk, &uk, &wk);
        if (spot_finite(wp) && spot_finite(wk) && ((wp < 0.0) != (wk < 0.0))) {
            double l = xp, h = xk;
            const bool lneg = wp < 0.0;
            for (int it = 0; it < 64; ++it) {
                const double mid = (l + h) / 2.0;
                double um, wm;
                spot_uw(pk, mid, &um, &wm);
                if ((wm < 0.0) == lneg) l = mid; else h = mid;
            }
            spot_consider(pk, (l + h) / 2.0, best, bestL);
        }
        xp = xk;
        wp = wk;
    }
}

// the fit over the stored peaks and the threshold for n observations, Nt excesses, initial threshold t and risk q
template <class Peaks>
__host__ __device__ inline SpotFit spot_fit(const Peaks& pk, long n, long Nt, double t, double q) {
#pragma clang fp contract(off)
    double ymin, ymax, ysum;
    pk.moments(&ymin, &ymax, &ysum);
    const double m = (double)pk.m;
    const double ymean = ysum / m;
    SpotFit best{0.0, ymean, 0.0};
    double bestL = -m * (1.0 + log(ymean));
    if (!spot_finite(bestL)) bestL = -INFINITY;
    double eps = 1e-8;
    if (1.0 / ymax < 2.0 * eps) eps = 1.0 / (32.0 * ymax);
    const double llo = -1.0 / ymax + eps, lhi = -1e-3 / ymean;
    if (llo < lhi) spot_roots(pk, llo, lhi, &best, &bestL);
    if (ymean > ymin) {
        const double a = 2.0 * (ymean - ymin);
        spot_roots(pk, a / (ymean * ymin), a / (ymin * ymin), &best, &bestL);
    }
    const double r = q * (double)n / (double)Nt;
    if (best.gamma != 0.0)
        best.z = t + (best.sigma / best.gamma) * (pow(r, -best.gamma) - 1.0);
    else
        best.z = t - best.sigma * log(r);
    return best;
}

// the summation order of a wave, on the host: 64 accumulators filled in ascending order, then the butterfly
struct HostPeaks {
    const double* y;
    long m;
    static double butterfly(double* acc) {
        double tmp[64];
        for (int off = 32; off > 0; off >>= 1) {
            for (int l = 0; l < 64; ++l) tmp[l] = acc[l] + acc[l ^ off];
            for (int l = 0; l < 64; ++l) acc[l] = tmp[l];
        }
        return acc[0];
    }
    void moments(double* ymin, double* ymax, double* ysum) const {
        double acc[64] = {0.0};
        double lo = y[0], hi = y[0];
        for (long i = 0; i < m; ++i) {
            acc[i & 63] += y[i];
            lo = y[i] < lo ? y[i] : lo;
            hi = y[i] > hi ? y[i] : hi;
        }
        *ymin = lo; *ymax = hi; *ysum = butterfly(acc);
    }
    void sums(double x, double* slog, double* sinv) const {
#pragma clang fp contract(off)
        double al[64] = {0.0}, ai[64] = {0.0};
        for (long i = 0; i < m; ++i) {
            const double a = 1.0 + x * y[i];
            al[i & 63] += log(a);
            ai[i & 63] += 1.0 / a;
        }
        *slog = butterfly(al); *sinv = butterfly(ai);
    }
};

#if defined(__HIPCC__)
__device__ __forceinline__ double spot_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the last m = min(Nt, P) excesses of one column's ring, oldest first, read by one wave
struct RingPeaks {
    const double* ring;
    long P, start, m;
    int lane;
    __device__ __forceinline__ double at(long i) const {
        long k = start + i;
        if (k >= P) k -= P;
        return ring[k];
    }
    __device__ inline void moments(double* ymin, double* ymax, double* ysum) const {
        double acc = 0.0, lo = INFINITY, hi = -INFINITY;
        for (long i = lane; i < m; i += 64) {
            const double v = at(i);
            acc += v;
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double a = __shfl_xor(lo, off), b = __shfl_xor(hi, off);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        *ymin = lo; *ymax = hi; *ysum = spot_wave_sum(acc);
    }
    __device__ inline void sums(double x, double* slog, double* sinv) const {
#pragma clang fp contract(off)
        double al = 0.0, ai = 0.0;
        for (long i = lane; i < m; i += 64) {
            const double a = 1.0 + x * at(i);
            al += log(a);
            ai += 1.0 / a;
        }
        *slog = spot_wave_sum(al); *sinv = spot_wave_sum(ai);
    }
};

__device__ __forceinline__ RingPeaks spot_ring_peaks(const double* ring, long P, long Nt, int lane) {
    return RingPeaks{ring, P, Nt > P ? Nt % P : 0, Nt > P ? P : Nt, lane};
}

// One score x against one column's state, by one wave (every lane holds the same `c`; lane 0 writes the ring).  Returns the flag;
// the threshold the row was compared with is c.z BEFORE the call.  A NaN changes nothing and is not flagged; x > z is flagged and,
// alarms not being absorbed, leaves the state alone; otherwise, when adaptive, an x > t joins the ring (the oldest excess leaves a
// full one), Nt and n advance and the tail is refitted, and any other x advances n.  A static state never changes.
__device__ inline bool spot_step(SpotCol& c, double* ring, long P, double q, bool adaptive, double x, int lane) {
    if (x != x) return false;
    if (x > c.z) return true;
    if (!adaptive) return false;
    if (x > c.t) {
        if (lane == 0) ring[c.Nt % P] = x - c.t;
        __threadfence_block();               // the store has reached the L1 this wave's other lanes read through
        c.Nt += 1;
        c.n += 1;
        const SpotFit f = spot_fit(spot_ring_peaks(ring, P, c.Nt, lane), c.n, c.Nt, c.t, q);
        c.gamma = f.gamma;
        c.sigma = f.sigma;
        c.z = f.z;
    } else {
        c.n += 1;
    }
    return false;
}

__device__ __forceinline__ bool spot_header_matches(const SpotHeader* hd, long S, long P) {
    return hd->magic == SPOT_MAGIC && hd->S == S && hd->P == P;
}
#endif  // __HIPCC__

}  // namespace mtadgat
#endif
