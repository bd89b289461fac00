// Scoring live streams row by row with the state kept on the device (streaming.StreamScorer; entry points mtadgat_stream_* in
// mtadgat_capi.cpp).  One allocation per scorer holds a header, the target dimensions and scale vectors, a StreamSlot and a pending
// forecast per stream, and the histories: S mirrored rings of R = W + max_block - 1 rows (stream_window_start, mtadgat_kernels.h)
// that together form one flat (S * 2R, F) array mtadgat_forward_series reads as a series.
//
//   k_stream_stage: the T new rows of each of the n selected streams into both copies of their ring slots, and the n * T window
//       starts -- the window ENDING at each new row -- in (stream, t) order.  It reads the row counters and moves nothing: staging
//       the same rows twice is harmless, so a caller may repeat the forward behind it (re-packed weights) before it commits.
//   k_stream_score: one wave per stream.  Per new row, lanes on the output columns form a[d] = |pending[d] - x[d]| + gamma
//       |recon_last[d] - x[d]| in float64 (optionally (a - center[d]) / (1 + spread[d])), add them in a fixed order -- each lane its
//       columns in ascending order, then a butterfly over the lanes -- and round the mean once to float32.  The moving average, the
//       threshold compare and the event state machine then advance by one sample, wave-uniform; lane 0 stores.  Rows are walked in
//       order, so the bits depend on the data and on the order of pushes per stream only, not on how rows are cut into pushes.
//       The kernel is the only writer of the slots: it advances the row counter last.  Its second instance, k_stream_score<true>,
//       takes each row's threshold from the stream's column of a SPOT state (mtadgat_spot.h: spot_step, after the smoothing) and
//       advances that column too; the fixed-threshold instance compiles to the code it had before the variant existed.
//   k_stream_flush: the still-open event of each selected stream, and / or the stream's reset to its initial state (ring zeroed).
// No atomics.  A stream index outside [0, S) writes "nothing here" (NaN / -1 / 0) and touches no state.
#include "../../include/mtadgat.h"      // the entry points' declarations
#include "mtadgat_device.h"
#include "mtadgat_spot.h"

namespace mtadgat {

namespace {

size_t up16(size_t v) { return (v + 15) / 16 * 16; }

struct StreamPtrs {
    const StreamHeader* hd;
    const int* dims;
    const float* center;
    const float* spread;
    StreamSlot* slots;
    float* pending;
    float* ring;
};

}  // namespace

StreamLayout stream_layout(long S, long max_block, long W, long F, long d) {
    StreamLayout l;
    l.R = W + max_block - 1;
    l.dims = up16(sizeof(StreamHeader));
    l.center = l.dims + up16(4 * (size_t)d);
    l.spread = l.center + up16(4 * (size_t)d);
    l.slots = l.spread + up16(4 * (size_t)d);
    l.pending = l.slots + up16(sizeof(StreamSlot) * (size_t)S);
    l.ring = l.pending + up16(4 * (size_t)S * (size_t)d);
    l.bytes = l.ring + up16(4 * (size_t)S * 2 * (size_t)l.R * (size_t)F);
    return l;
}

namespace {

StreamPtrs stream_ptrs(void* state, const StreamGeom& g) {
    const StreamLayout l = stream_layout(g.S, g.R - g.W + 1, g.W, g.F, g.d);
    char* b = static_cast<char*>(state);
    StreamPtrs p;
    p.hd = reinterpret_cast<const StreamHeader*>(b);
    p.dims = reinterpret_cast<const int*>(b + l.dims);
    p.center = reinterpret_cast<const float*>(b + l.center);
    p.spread = reinterpret_cast<const float*>(b + l.spread);
    p.slots = reinterpret_cast<StreamSlot*>(b + l.slots);
    p.pending = reinterpret_cast<float*>(b + l.pending);
    p.ring = reinterpret_cast<float*>(b + l.ring);
    return p;
}

// the state was initialised for the geometry the caller launches with
__device__ __forceinline__ bool geom_matches(const StreamHeader* hd, const StreamGeom& g) {
    return hd->S == g.S && hd->R == g.R && hd->W == g.W && hd->F == g.F && hd->d == g.d;
}

__device__ __forceinline__ long stream_of(const long* __restrict__ streams, long j) { return streams ? streams[j] : j; }

}  // namespace

// grid (n): one workgroup per selected stream
__global__ void __launch_bounds__(256) k_stream_stage(StreamPtrs p, StreamGeom g, const float* __restrict__ rows,
                                                       const long* __restrict__ streams, long T, long* __restrict__ starts) {
    const long j = blockIdx.x;
    const long s = stream_of(streams, j);
    const bool ok = geom_matches(p.hd, g) && s >= 0 && s < g.S && T <= p.hd->max_block;
    const long count = ok ? p.slots[s].count : 0;
    const long base = (ok ? s : 0) * 2 * g.R;                  // an unknown stream: in-bounds starts, nothing written
    if (starts)
        for (long t = threadIdx.x; t < T; t += blockDim.x) starts[j * T + t] = base + (ok ? stream_window_start(count, t, g.W, g.R) : 0);
    if (!ok) return;
    const long TF = T * g.F;
    for (long i = threadIdx.x; i < TF; i += blockDim.x) {
        const long t = i / g.F, c = i - t * g.F;
        const long slot = stream_row_slot(count + t, g.R);
        const float v = rows[j * TF + i];
        p.ring[(base + slot) * g.F + c] = v;
        p.ring[(base + slot + g.R) * g.F + c] = v;
    }
}

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

struct Closed {
    long start, end, peak;
    float peak_score, mean;
};
__device__ __forceinline__ Closed no_event() { return Closed{-1, -1, -1, __builtin_nanf(""), __builtin_nanf("")}; }
// the open event of `sl` as it stands: [ev_start, ev_last + 1), or nothing when it is shorter than min_length
__device__ __forceinline__ Closed event_of(const StreamSlot& sl, long min_length) {
    const long len = sl.ev_last + 1 - sl.ev_start;
    if (!sl.ev_open || len < min_length) return no_event();
    return Closed{sl.ev_start, sl.ev_last + 1, sl.ev_peak, sl.ev_peak_score, (float)(sl.ev_sum / (double)len)};
}
__device__ __forceinline__ void put_closed(const StreamOut& o, long at, const Closed& c) {
    if (o.closed_start) o.closed_start[at] = c.start;
    if (o.closed_end) o.closed_end[at] = c.end;
    if (o.closed_peak) o.closed_peak[at] = c.peak;
    if (o.closed_peak_score) o.closed_peak_score[at] = c.peak_score;
    if (o.closed_mean) o.closed_mean[at] = c.mean;
}

}  // namespace

// grid (ceil(n / 4)) x 256 threads: one wave per selected stream
template <bool SPOT>
__global__ void __launch_bounds__(256) k_stream_score(StreamPtrs p, StreamGeom g, const float* __restrict__ rows,
                                                       const long* __restrict__ streams, long n, long T, const float* __restrict__ preds,
                                                       const float* __restrict__ recons_last, double threshold,
                                                       const double* __restrict__ thresholds, StreamOut o, StreamSpot sp) {
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= n) return;
    const long s = stream_of(streams, j);
    const int d = (int)g.d;
    const float nanf32 = __builtin_nanf("");
    if (!geom_matches(p.hd, g) || s < 0 || s >= g.S || T > p.hd->max_block ||
        (SPOT && !spot_header_matches(static_cast<const SpotHeader*>(sp.state), g.S, sp.max_peaks))) {
        for (long t = 0; t < T; ++t) {
            const long at = j * T + t;
            if constexpr (SPOT)
                if (lane == 0 && sp.thresholds_out) sp.thresholds_out[at] = __builtin_nan("");
            if (o.per_dim)
                for (int col = lane; col < d; col += 64) o.per_dim[at * d + col] = nanf32;
            if (lane == 0) {
                if (o.scores) o.scores[at] = nanf32;
                if (o.flags) o.flags[at] = 0;
                put_closed(o, at, no_event());
            }
        }
        return;
    }
    const StreamHeader hd = *p.hd;
    StreamSlot sl = p.slots[s];                                 // wave-uniform copy; lane 0 stores it back
    const double thr = thresholds ? thresholds[s] : threshold;
    // the stream's SPOT column: a wave-uniform copy like the slot; lane 0 stores it back
    SpotCol sc{};
    SpotCol* spot_cols = nullptr;
    double* spot_ring = nullptr;
    double spot_q = 0.0;
    bool spot_adaptive = false;
    if constexpr (SPOT) {
        char* sb = static_cast<char*>(sp.state);
        const SpotHeader* sh = reinterpret_cast<const SpotHeader*>(sb);
        spot_cols = reinterpret_cast<SpotCol*>(sb + spot_cols_offset());
        spot_ring = reinterpret_cast<double*>(sb + spot_ring_offset(g.S)) + s * sp.max_peaks;
        spot_q = sh->q;
        spot_adaptive = sh->dynamic != 0;
        sc = spot_cols[s];
    }
    for (long t = 0; t < T; ++t) {
        const long at = j * T + t;
        const long k = sl.count + t;                            // this row's number in its stream
        const bool scored = k >= g.W;                           // its window and the forecast from the row before both exist
        double acc = 0.0;
        for (int col = lane; col < d; col += 64) {
            const double x = (double)rows[at * g.F + p.dims[col]];
            const double f = (double)(t == 0 ? p.pending[s * d + col] : preds[(at - 1) * d + col]);
            double a = fabs(f - x) + hd.gamma * fabs((double)recons_last[at * d + col] - x);
            if (hd.scaled) a = (a - (double)p.center[col]) / (1.0 + (double)p.spread[col]);
            if (o.per_dim) o.per_dim[at * d + col] = scored ? (float)a : nanf32;
            acc += a;
        }
        float score = (float)(wave_sum(acc) / (double)d);
        Closed closed = no_event();
        bool flag = false;
        double compared = __builtin_nan("");                    // SPOT: the threshold this row met
        if (scored) {
            const long i = k - g.W;                             // score index, as in anomaly_scores / anomaly_events
            if (hd.smooth) {
                sl.num = (double)score + hd.decay * sl.num;
                sl.den = 1.0 + hd.decay * sl.den;
                score = (float)(sl.num / sl.den);
            }
            if constexpr (SPOT) {
                compared = sc.z;
                flag = spot_step(sc, spot_ring, sp.max_peaks, spot_q, spot_adaptive, (double)score, lane);
            } else {
                flag = (double)score > thr;                     // NaN and equality are not flagged
            }
            if (flag) {
                if (!sl.ev_open) {
                    sl.ev_open = 1;
                    sl.ev_start = i;
                    sl.ev_peak = i;
                    sl.ev_peak_score = score;
                    sl.ev_sum = (double)score;
                } else {
                    sl.ev_sum += sl.ev_tail + (double)score;    // the gap belongs to the event
                    if (score > sl.ev_peak_score) { sl.ev_peak_score = score; sl.ev_peak = i; }
                }
                sl.ev_last = i;
                sl.ev_tail = 0.0;
            } else if (sl.ev_open) {
                if (i - sl.ev_last > hd.merge_gap) {            // i = ev_last + 1 + merge_gap: no later run can merge into it
                    closed = event_of(sl, hd.min_length);
                    sl.ev_open = 0;
                } else {
                    sl.ev_tail += (double)score;
                }
            }
        } else {
            score = nanf32;
        }
        if (lane == 0) {
            if (o.scores) o.scores[at] = score;
            if (o.flags) o.flags[at] = flag ? 1 : 0;
            put_closed(o, at, closed);
            if constexpr (SPOT)
                if (sp.thresholds_out) sp.thresholds_out[at] = compared;
        }
    }
    // the forecast of the row after this push's last one (a wave runs in lockstep: every read of the old values is done)
    for (int col = lane; col < d; col += 64) p.pending[s * d + col] = preds[(j * T + T - 1) * d + col];
    sl.count += T;
    if (lane == 0) p.slots[s] = sl;
    if constexpr (SPOT)
        if (lane == 0) spot_cols[s] = sc;
}

// grid (ceil(n / 4)) x 256 threads: one wave per selected stream; out arrays are (n)
__global__ void __launch_bounds__(256) k_stream_flush(StreamPtrs p, StreamGeom g, const long* __restrict__ streams, long n, int report,
                                                       int reset, StreamOut o) {
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= n) return;
    const long s = stream_of(streams, j);
    const bool ok = geom_matches(p.hd, g) && s >= 0 && s < g.S;
    if (report && lane == 0) put_closed(o, j, ok ? event_of(p.slots[s], p.hd->min_length) : no_event());
    if (!ok || !reset) return;
    if (lane == 0) {
        StreamSlot z;
        z.count = 0; z.num = 0.0; z.den = 0.0; z.ev_start = 0; z.ev_last = 0; z.ev_peak = 0; z.ev_sum = 0.0; z.ev_tail = 0.0;
        z.ev_peak_score = 0.f; z.ev_open = 0;
        p.slots[s] = z;
    }
    for (long c = lane; c < g.d; c += 64) p.pending[s * g.d + c] = 0.f;
    const long per = 2 * g.R * g.F;
    for (long i = lane; i < per; i += 64) p.ring[s * per + i] = 0.f;
}

int launch_stream_init(void* state, const StreamHeader& hd, const int* dims_host, const float* center_host, const float* spread_host,
                       hipStream_t s) {
    const StreamLayout l = stream_layout(hd.S, hd.max_block, hd.W, hd.F, hd.d);
    char* b = static_cast<char*>(state);
    hipError_t e = hipMemsetAsync(state, 0, l.bytes, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b, &hd, sizeof(hd), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b + l.dims, dims_host, 4 * (size_t)hd.d, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && hd.scaled) e = hipMemcpyAsync(b + l.center, center_host, 4 * (size_t)hd.d, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && hd.scaled) e = hipMemcpyAsync(b + l.spread, spread_host, 4 * (size_t)hd.d, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);            // the host buffers are the caller's again on return
    return (int)e;
}

int launch_stream_stage(void* state, const StreamGeom& g, const float* rows, const long* streams, long n, long T, long* starts, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_stage, dim3((unsigned)n), dim3(256), 0, s, stream_ptrs(state, g), g, rows, streams, T, starts);
    return (int)hipGetLastError();
}

int launch_stream_score(void* state, const StreamGeom& g, const float* rows, const long* streams, long n, long T, const float* preds,
                        const float* recons_last, double threshold, const double* thresholds, const StreamOut& out, hipStream_t s,
                        const StreamSpot* spot) {
    const dim3 grid((unsigned)((n + 3) / 4));
    if (spot)
        hipLaunchKernelGGL(k_stream_score<true>, grid, dim3(256), 0, s, stream_ptrs(state, g), g, rows, streams, n, T, preds, recons_last,
                           threshold, thresholds, out, *spot);
    else
        hipLaunchKernelGGL(k_stream_score<false>, grid, dim3(256), 0, s, stream_ptrs(state, g), g, rows, streams, n, T, preds, recons_last,
                           threshold, thresholds, out, StreamSpot{});
    return (int)hipGetLastError();
}

int launch_stream_flush(void* state, const StreamGeom& g, const long* streams, long n, int report, int reset, const StreamOut& out,
                        hipStream_t s) {
    hipLaunchKernelGGL(k_stream_flush, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, stream_ptrs(state, g), g, streams, n, report, reset, out);
    return (int)hipGetLastError();
}

}  // namespace mtadgat

extern "C" int64_t mtadgat_stream_window_start(int64_t count, int64_t t, int64_t W, int64_t R) {
    if (count < 0 || t < 0 || W < 1 || R < W) return -1;
    return (int64_t)mtadgat::stream_window_start((long)count, (long)t, (long)W, (long)R);
}
