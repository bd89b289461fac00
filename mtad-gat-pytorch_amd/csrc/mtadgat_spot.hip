// Peaks-over-threshold thresholds on the device (evaluation.spot_calibrate / spot_run / pot_eval; entry points mtadgat_spot_*).
// The fit and the per-score step are in mtadgat_spot.h, shared with k_stream_score<true> (mtadgat_stream.hip) and with the host
// hook mtadgat_spot_fit_host.  One state allocation holds a header, a SpotCol per column and a ring of the last max_peaks excesses
// per column.  The ring is this package's own bound: SPOT as published keeps every excess; here Nt counts every excess and the fit
// sees only the stored ones, so until a ring wraps this is the paper's Algorithm 1.
//
//   k_spot_calibrate: one workgroup per column of an (n_init, S) float32 score matrix.  t = sorted[int(level n_init)] comes from the
//       exact radix select of mtadgat_evalcol.hip (launch_column_rank).  The excesses x - t of the rows with x > t are compacted in
//       row order by a ballot scan, 256 rows per step, excess number e into ring slot e % P when it is among the last P; then the
//       first wave fits.  A column with fewer than 8 excesses, a NaN or a non-positive mean excess gets an error code the host raises on.
//   k_spot_run: one wave per column over an (n, S) float32 score matrix, rows in order; 64 rows are loaded and their thresholds
//       and flags stored at a time, one per lane.  The state is left advanced: a second call continues where the first stopped.
//   k_spot_copy: columns from one state to another (a clone of some columns, one column serving many streams, a reset).
// No atomics; nothing depends on the launch geometry; every store is an ordinary vector store.
#include "../../include/mtadgat.h"      // the entry points' declarations
#include "mtadgat_device.h"
#include "mtadgat_spot.h"

#include <string>
#include <vector>

namespace mtadgat {

namespace {

struct SpotPtrs {
    SpotHeader* hd;
    SpotCol* cols;
    double* ring;
};
__host__ __device__ inline SpotPtrs spot_ptrs(void* state, long S) {
    char* b = static_cast<char*>(state);
    return SpotPtrs{reinterpret_cast<SpotHeader*>(b), reinterpret_cast<SpotCol*>(b + spot_cols_offset()),
                    reinterpret_cast<double*>(b + spot_ring_offset(S))};
}

}  // namespace

// grid (S) x 256 threads
__global__ void __launch_bounds__(256) k_spot_calibrate(void* state, long S, long P, const float* __restrict__ init, long n, long ld,
                                                         const float* __restrict__ ord, double q, double level, int dynamic) {
    __shared__ long s_cnt[4];
    __shared__ int s_nan[4];
    const long col = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpotPtrs p = spot_ptrs(state, S);
    double* ring = p.ring + col * P;
    if (col == 0 && tid == 0) {
        SpotHeader hd;
        hd.magic = SPOT_MAGIC; hd.S = S; hd.P = P; hd.dynamic = dynamic; hd.n_init = n; hd.q = q; hd.level = level; hd.pad = 0;
        *p.hd = hd;
    }
    const double t = (double)ord[col];
    // the number of excesses, and whether the column holds a NaN
    long cnt = 0;
    int nan = 0;
    for (long row = tid; row < n; row += 256) {
        const float v = init[row * ld + col];
        nan |= (v != v) ? 1 : 0;
        cnt += ((double)v > t) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off);
        nan |= __shfl_xor(nan, off);
    }
    if (lane == 0) { s_cnt[wave] = cnt; s_nan[wave] = nan; }
    __syncthreads();
    const long Nt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    nan = s_nan[0] | s_nan[1] | s_nan[2] | s_nan[3];
    __syncthreads();
    SpotCol c;
    c.t = t; c.z = __builtin_nan(""); c.gamma = 0.0; c.sigma = 0.0; c.n = n; c.Nt = Nt; c.pad = 0;
    c.err = nan ? SPOT_ERR_NAN : (Nt < SPOT_MIN_PEAKS ? SPOT_ERR_FEW : 0);
    if (c.err) {                                              // uniform over the workgroup
        if (tid == 0) p.cols[col] = c;
        return;
    }
    // the excesses in row order: excess number e goes to slot e % P, the last P of them stay
    long base = 0;
    for (long row0 = 0; row0 < n; row0 += 256) {
        const long row = row0 + tid;
        const float v = row < n ? init[row * ld + col] : 0.f;
        const bool ex = row < n && (double)v > t;
        const unsigned long long b = __ballot(ex);
        if (lane == 0) s_cnt[wave] = __popcll(b);
        __syncthreads();
        long e = base + __popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) e += s_cnt[w];
        if (ex && e >= Nt - P) ring[e % P] = (double)v - t;
        base += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
    if (wave != 0) return;                                    // the ring is complete: the barrier above ordered its stores
    const RingPeaks pk = spot_ring_peaks(ring, P, Nt, lane);
    double ymin, ymax, ysum;
    pk.moments(&ymin, &ymax, &ysum);
    if (!(ysum > 0.0)) {
        c.err = SPOT_ERR_MEAN;
    } else {
        const SpotFit f = spot_fit(pk, c.n, c.Nt, c.t, q);
        c.gamma = f.gamma; c.sigma = f.sigma; c.z = f.z;
    }
    if (lane == 0) p.cols[col] = c;
}

// grid (ceil(S / 4)) x 256 threads: one wave per column
__global__ void __launch_bounds__(256) k_spot_run(void* state, long S, long P, const float* __restrict__ scores, long n, long ld,
                                                   double* __restrict__ thr, unsigned char* __restrict__ flags) {
    const long col = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (col >= S) return;
    const SpotPtrs p = spot_ptrs(state, S);
    const bool ok = spot_header_matches(p.hd, S, P);          // a state made for other sizes: nothing is read or advanced
    SpotCol c{};
    double q = 0.0;
    bool adaptive = false;
    if (ok) {
        c = p.cols[col];
        q = p.hd->q;
        adaptive = p.hd->dynamic != 0;
    }
    double* ring = p.ring + col * P;
    for (long base = 0; base < n; base += 64) {
        const long mine = base + lane;
        const float xv = mine < n ? scores[mine * ld + col] : 0.f;
        const int cnt = n - base < 64 ? (int)(n - base) : 64;
        double zt = __builtin_nan("");
        unsigned char fl = 0;
        for (int r = 0; ok && r < cnt; ++r) {
            const double x = (double)__shfl(xv, r);
            const double zb = c.z;
            const bool f = spot_step(c, ring, P, q, adaptive, x, lane);
            if (lane == r) { zt = zb; fl = f ? 1 : 0; }
        }
        if (mine < n) {
            if (thr) thr[mine * S + col] = zt;
            if (flags) flags[mine * S + col] = fl;
        }
    }
    if (ok && lane == 0) p.cols[col] = c;
}

// grid (n) x 256 threads: one workgroup per selected column of dst
__global__ void __launch_bounds__(256) k_spot_copy(void* dst, long dstS, const void* src, long srcS, long P, const long* __restrict__ columns,
                                                    int write_header) {
    const SpotPtrs d = spot_ptrs(dst, dstS);
    const SpotPtrs s = spot_ptrs(const_cast<void*>(src), srcS);
    if (!spot_header_matches(s.hd, srcS, P)) return;
    if (write_header) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            SpotHeader hd = *s.hd;
            hd.S = dstS;
            *d.hd = hd;
        }
    } else if (!spot_header_matches(d.hd, dstS, P)) {
        return;
    }
    const long col = columns ? columns[blockIdx.x] : (long)blockIdx.x;
    if (col < 0 || col >= dstS) return;
    const long from = srcS == 1 ? 0 : col;
    if (from >= srcS) return;
    if (threadIdx.x == 0) d.cols[col] = s.cols[from];
    for (long i = threadIdx.x; i < P; i += 256) d.ring[col * P + i] = s.ring[from * P + i];
}

int launch_spot_copy(void* dst, long dstS, const void* src, long srcS, long P, const long* columns, long n, hipStream_t s, int write_header) {
    hipLaunchKernelGGL(k_spot_copy, dim3((unsigned)n), dim3(256), 0, s, dst, dstS, src, srcS, P, columns, write_header);
    return (int)hipGetLastError();
}

}  // namespace mtadgat

using namespace mtadgat;

namespace {

constexpr int64_t SPOT_MAX_CALIBRATE_COLUMNS = 65536;

// what every call on a state checks on the host; 0 or the status
int spot_check_state(const void* state, int64_t S, int64_t P, const char* who) {
    const std::string w(who);
    if (S < 1 || S > 2147483647LL) return record_error(-1, (w + ": n_columns must lie in [1, 2^31 - 1]").c_str());
    if (P < SPOT_MIN_PEAKS || P > SPOT_MAX_PEAKS) return record_error(-1, (w + ": max_peaks must lie in [8, 4096]").c_str());
    if (!state) return record_error(-1, (w + ": state is NULL").c_str());
    if ((uintptr_t)state & 15) return record_error(-1, (w + ": state must be 16-byte aligned").c_str());
    return 0;
}

}  // namespace

extern "C" {

size_t mtadgat_spot_state_bytes(int64_t n_columns, int64_t max_peaks) {
    if (n_columns < 1 || n_columns > 2147483647LL || max_peaks < SPOT_MIN_PEAKS || max_peaks > SPOT_MAX_PEAKS) return 0;
    return spot_state_bytes((long)n_columns, (long)max_peaks);
}

size_t mtadgat_spot_calibrate_scratch(int64_t n_init, int64_t n_columns) {
    if (n_init < SPOT_MIN_INIT || n_columns < 1 || n_columns > SPOT_MAX_CALIBRATE_COLUMNS) return 0;
    return column_rank_scratch((int)n_columns);
}

int mtadgat_spot_calibrate(const float* init_dev, int64_t n_init, int64_t n_columns, int64_t ld, double q, double level, int64_t max_peaks,
                           int dynamic, void* state_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    if (!(q > 0.0 && q < 1.0)) return record_error(-1, "spot_calibrate: q must lie in (0, 1)");
    if (!(level > 0.0 && level < 1.0)) return record_error(-1, "spot_calibrate: level must lie in (0, 1)");
    if (n_init < SPOT_MIN_INIT || n_init > 2147483647LL) return record_error(-1, "spot_calibrate: n_init must lie in [16, 2^31 - 1]");
    if (n_columns > SPOT_MAX_CALIBRATE_COLUMNS) return record_error(-1, "spot_calibrate: at most 65536 columns are calibrated by one call");
    int rc = spot_check_state(state_dev, n_columns, max_peaks, "spot_calibrate");
    if (rc) return rc;
    if (!init_dev) return record_error(-1, "spot_calibrate: init scores are NULL");
    if (ld < n_columns) return record_error(-1, "spot_calibrate: ld < n_columns");
    if (!scratch_dev || ((uintptr_t)scratch_dev & 15)) return record_error(-5, "spot_calibrate: scratch is NULL or not 16-byte aligned");
    if (scratch_bytes < column_rank_scratch((int)n_columns))
        return record_error(-5, "spot_calibrate: scratch too small (see mtadgat_spot_calibrate_scratch)");
    hipStream_t s = (hipStream_t)stream;
    long rank = (long)(level * (double)n_init);                    // int(level * n_init)
    if (rank > n_init - 1) rank = (long)n_init - 1;
    const float* ord = nullptr;
    if (launch_column_rank(init_dev, (long)n_init, (int)n_columns, (long)ld, rank, scratch_dev, &ord, s) != 0)
        return record_error(-3, "spot_calibrate: kernel launch failed");
    hipLaunchKernelGGL(k_spot_calibrate, dim3((unsigned)n_columns), dim3(256), 0, s, state_dev, (long)n_columns, (long)max_peaks, init_dev,
                       (long)n_init, (long)ld, ord, q, level, dynamic ? 1 : 0);
    if (hipGetLastError() != hipSuccess) return record_error(-3, "spot_calibrate: kernel launch failed");
    std::vector<SpotCol> cols((size_t)n_columns);
    if (hipMemcpyAsync(cols.data(), static_cast<const char*>(state_dev) + spot_cols_offset(), sizeof(SpotCol) * cols.size(), hipMemcpyDeviceToHost,
                       s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return record_error(-3, "spot_calibrate: reading the columns back failed");
    for (int64_t c = 0; c < n_columns; ++c) {
        if (!cols[c].err) continue;
        const char* why = cols[c].err == SPOT_ERR_NAN ? "holds a NaN"
                          : cols[c].err == SPOT_ERR_FEW ? "has fewer than 8 excesses over its initial threshold"
                                                        : "has a non-positive mean excess";
        return record_error(-1, ("spot_calibrate: column " + std::to_string(c) + " " + why).c_str());
    }
    return 0;
}

int mtadgat_spot_run(void* state_dev, int64_t n_columns, int64_t max_peaks, const float* scores_dev, int64_t n, int64_t ld,
                     double* thresholds_dev, uint8_t* flags_dev, void* stream) {
    int rc = spot_check_state(state_dev, n_columns, max_peaks, "spot_run");
    if (rc) return rc;
    if (!scores_dev) return record_error(-1, "spot_run: scores are NULL");
    if (n < 1 || n > 2147483647LL) return record_error(-1, "spot_run: n must lie in [1, 2^31 - 1]");
    if (ld < n_columns) return record_error(-1, "spot_run: ld < n_columns");
    hipLaunchKernelGGL(k_spot_run, dim3((unsigned)((n_columns + 3) / 4)), dim3(256), 0, (hipStream_t)stream, state_dev, (long)n_columns,
                       (long)max_peaks, scores_dev, (long)n, (long)ld, thresholds_dev, flags_dev);
    return hipGetLastError() == hipSuccess ? 0 : record_error(-3, "spot_run: kernel launch failed");
}

int mtadgat_spot_read(const void* state_dev, int64_t n_columns, int64_t max_peaks, double* out_host, void* stream) {
    int rc = spot_check_state(state_dev, n_columns, max_peaks, "spot_read");
    if (rc) return rc;
    if (!out_host) return record_error(-1, "spot_read: out is NULL");
    hipStream_t s = (hipStream_t)stream;
    SpotHeader hd;
    std::vector<SpotCol> cols((size_t)n_columns);
    if (hipMemcpyAsync(&hd, state_dev, sizeof(hd), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(cols.data(), static_cast<const char*>(state_dev) + spot_cols_offset(), sizeof(SpotCol) * cols.size(), hipMemcpyDeviceToHost,
                       s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return record_error(-3, "spot_read: copy failed");
    if (hd.magic != SPOT_MAGIC || hd.S != n_columns || hd.P != max_peaks)
        return record_error(-1, "spot_read: the state was not calibrated for these sizes");
    for (int64_t c = 0; c < n_columns; ++c) {
        double* o = out_host + 6 * c;
        o[0] = cols[c].t; o[1] = cols[c].z; o[2] = (double)cols[c].n; o[3] = (double)cols[c].Nt; o[4] = cols[c].gamma; o[5] = cols[c].sigma;
    }
    return 0;
}

int mtadgat_spot_copy(void* dst_dev, int64_t dst_columns, const void* src_dev, int64_t src_columns, int64_t max_peaks,
                      const int64_t* columns_dev, int64_t n, int init, void* stream) {
    int rc = spot_check_state(dst_dev, dst_columns, max_peaks, "spot_copy");
    if (rc) return rc;
    if ((rc = spot_check_state(src_dev, src_columns, max_peaks, "spot_copy"))) return rc;
    if (src_columns != 1 && src_columns != dst_columns) return record_error(-1, "spot_copy: the source needs one column or as many as the destination");
    if (n < 1 || n > dst_columns) return record_error(-1, "spot_copy: n must lie in [1, dst_columns]");
    if (init && (columns_dev || n != dst_columns)) return record_error(-1, "spot_copy: a new state takes all its columns");
    if (launch_spot_copy(dst_dev, (long)dst_columns, src_dev, (long)src_columns, (long)max_peaks, reinterpret_cast<const long*>(columns_dev), (long)n,
                         (hipStream_t)stream, init ? 1 : 0) != 0)
        return record_error(-3, "spot_copy: kernel launch failed");
    return 0;
}

int mtadgat_spot_fit_host(const double* peaks, int64_t m, int64_t n, int64_t Nt, double t, double q, double* out) {
    if (!peaks || !out) return record_error(-1, "spot_fit_host: null pointer");
    if (m < 1) return record_error(-1, "spot_fit_host: m must be >= 1");
    if (Nt < 1 || n < 1) return record_error(-1, "spot_fit_host: n and Nt must be >= 1");
    if (!(q > 0.0 && q < 1.0)) return record_error(-1, "spot_fit_host: q must lie in (0, 1)");
    for (int64_t i = 0; i < m; ++i)
        if (!(peaks[i] > 0.0)) return record_error(-1, "spot_fit_host: the excesses must be positive");
    const SpotFit f = spot_fit(HostPeaks{peaks, (long)m}, (long)n, (long)Nt, t, q);
    out[0] = f.gamma; out[1] = f.sigma; out[2] = f.z;
    return 0;
}

}  // extern "C"
