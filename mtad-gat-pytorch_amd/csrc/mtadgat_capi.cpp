// C ABI (include/mtadgat.h) over the gfx950 kernels: handle lifetime, weight upload,
// the forward() launch sequence and the per-stage entry points.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "mtadgat_host.h"

using namespace mtadgat;

struct mtadgat_handle_s {
    Model m;
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return MTADGAT_ERR_HIP;
}
#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t e__ = (expr);                             \
        if (e__ != hipSuccess) return hip_fail(e__, #expr);  \
    } while (0)
#define K_TRY(expr, what)                                                                          \
    do {                                                                                           \
        int rc__ = (expr);                                                                         \
        if (rc__ == -2) return fail(MTADGAT_ERR_UNSUPPORTED, std::string(what) + ": unsupported shape"); \
        if (rc__ != 0) return hip_fail((hipError_t)rc__, what);                                    \
    } while (0)

enum Slot { S_CONV = 0, S_PROJ = 1, S_ATTEND = 2, S_GRU = 3, S_FC = 4, S_RECON = 5 };
const char* kSlotNames[MTADGAT_PROFILE_SLOTS] = {"conv", "proj", "attend", "gru", "fc", "recon"};

struct Scope {  // brackets a kernel family with events when profiling is on
    Model& m;
    int slot;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    Scope(Model& m_, int slot_, hipStream_t s_) : m(m_), slot(slot_), s(s_) {
        if (m.profile) {
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
            (void)hipEventRecord(a, s);
        }
    }
    ~Scope() {
        if (a && b) {
            (void)hipEventRecord(b, s);
            m.ev[slot].emplace_back(a, b);
        }
    }
};

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- stage launch helpers; all pointers device, n windows ------------------------------------
// where the windows come from: a materialised (n, W, F) tensor, or views of a device-resident series
struct XSource {
    int x_bf16 = 0;                  // x points at bfloat16 elements
    const float* x = nullptr;        // windows (n, W, F) -- or the series when gather != 0
    int gather = 0;
    const int64_t* starts = nullptr;
    int64_t start0 = 0, stride = 1;
};

// the facts of a call whose fused layers read node rows v (row stride ldv, `cols` node columns); hcat: where the convolution writes
FrontCall front_call(FrontKind kind, const XSource& src, const float* v, int ldv, int cols, const float* hcat) {
    FrontCall c;
    c.kind = kind;
    if (src.gather) c.source = (!src.starts && src.stride == 1) ? SRC_SERIES_UNIT : SRC_SERIES;
    else c.source = src.x_bf16 ? SRC_WINDOWS_BF16 : SRC_WINDOWS;
    c.rows_aligned = aligned16(v); c.ldv_fits = (ldv & 3) == 0 && round_up(cols, 4) <= ldv; c.hcat_aligned = aligned16(hcat);
    return c;
}

// Round 6: the split packs are derived LAZILY, by the first launch that reads them after an upload.  Rounds 2-5 re-derived all of
// them behind every upload -- ~30 launches of a few microseconds each (ranges, scales, splits) after every optimizer step, although a
// training step of the reference's batch size (256 windows) reads none of them: 0.15-0.2 ms of a 2.3 ms step.  An upload now only
// bumps weights_version; each consumer calls ensure() on the group it reads (SplitTable, mtadgat_host.h), which derives the group on
// the consumer's stream when it is stale.  A group that is current but was derived on another stream is waited for through the event
// recorded after its last step: a handle may be used from several streams one after another.  Calls that fork onto the second lane
// derive everything on the caller's stream first (ensure_all_split in forward_impl), so the lanes never race for a derivation.
int ensure(Model& m, int group, hipStream_t s) {
    SplitGroup& g = m.split.groups[group];
    if (g.version == m.weights_version) {
        if (s != g.stream) HIP_TRY(hipStreamWaitEvent(s, g.done, 0));
        return 0;
    }
    float* P = m.packed_dev;
    for (const SplitStep& t : g.steps) {
        float* sc = P + t.scale;
        switch (t.op) {
        case SplitStep::ZERO_SCALE: HIP_TRY(hipMemsetAsync(sc, 0, 4 * sizeof(float), s)); break;
        case SplitStep::ABSMAX: K_TRY(launch_absmax(P + t.src, t.n, sc, s), "weight range"); break;
        case SplitStep::SCALE_FROM_MAX: K_TRY(launch_scale_from_max(sc, s), "weight scale"); break;
        case SplitStep::SPLIT3: K_TRY(launch_split3(P + t.src, P + t.dst, t.n, t.Qs, t.Qd, 1, nullptr, s), "split-bf16 weights"); break;
        case SplitStep::SPLIT2H: K_TRY(launch_split2h(P + t.src, P + t.dst, t.n, t.Qs, t.Qd, t.arg, sc + 1, s), "split-fp16 weights"); break;
        case SplitStep::SPLIT2H_GATH:
            K_TRY(launch_split2h_gath(P + t.src, P + t.dst, (int)t.n, t.Qs, t.Qd, reinterpret_cast<const int*>(P + t.ord), t.arg, sc + 1, s), "split-fp16 weights"); break;
        case SplitStep::SPLIT_X: K_TRY(launch_split_x(P + t.src, P + t.dst, t.n, t.Qs, t.Qd, t.arg, sc + 1, s), "split input weights"); break;
        case SplitStep::REORDER_XQ: K_TRY(launch_reorder_xq(P + t.src, P + t.dst, (int)t.n, t.Qd, s), "chunk-major input weights"); break;
        }
    }
    HIP_TRY(hipEventRecord(g.done, s));
    g.version = m.weights_version;
    g.stream = s;
    return 0;
}
// everything an inference call may read, on ONE stream (no-ops while the weights are unchanged)
int ensure_all_split(Model& m, hipStream_t s) {
    for (int i = 0; i < m.split.n_infer; ++i)
        if (int rc = ensure(m, i, s)) return rc;
    return 0;
}
// where window c0 of the source starts, for the kernels that read the input themselves
template <class A> void fill_source(const Model& m, const XSource& src, int64_t c0, A& a) {
    if (src.gather) {
        a.X = src.x; a.gather = 1;
        a.starts = src.starts ? reinterpret_cast<const long*>(src.starts + c0) : nullptr;
        a.start0 = src.start0 + c0 * src.stride; a.stride = src.stride;
    } else if (src.x_bf16) {
        a.X = reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(src.x) + c0 * (int64_t)m.W * m.F);
    } else {
        a.X = src.x + c0 * (int64_t)m.W * m.F;
    }
    a.x_bf16 = src.x_bf16;
}
// launch_conv's fp32 arguments for n windows of Wk rows from window c0 on; the caller sets the outputs
ConvArgs conv_args(const Model& m, const XSource& src, int64_t c0, int64_t n, int64_t Wk) {
    ConvArgs a{};
    fill_source(m, src, c0, a);
    a.B = n; a.W = (int)Wk; a.F = m.F; a.Fp = m.Fp; a.taps = m.taps; a.pad = m.pad;
    a.Fq = m.Fp;
    a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + m.conv_w_off);
    a.bias = m.packed_dev + m.conv_b_off;
    a.NT = m.convNT; a.Wpad = m.Wp; a.Dp = m.Dp;
    return a;
}
// the convolution launch the route names (CONV_WIN, CONV_LAUNCH); vmax: where the range is recorded when the route says so; bad:
// where k_conv_win leaves the windows' non-finite flags (run_poison), or null
int run_conv(Model& m, const FrontRoute& r, const XSource& src, int64_t c0, int64_t n, float* xc, float* xct, float* hcat, float* y,
             hipStream_t s, unsigned* vmax = nullptr, unsigned char* bad = nullptr) {
    Scope sc(m, S_CONV, s);
    ConvArgs a = conv_args(m, src, c0, n, m.W);
    a.XC = xc; a.XCT = xct; a.HCAT = hcat; a.Y = y;
    if (r.range) {
        HIP_TRY(hipMemsetAsync(vmax, 0, sizeof(unsigned), s));
        a.vmax = vmax;
    }
    if (r.conv_split_pack)
        if (int rc_ = ensure(m, m.conv_split, s)) return rc_;
    if (r.conv == CONV_WIN) {
        a.Fq = m.Fp16;
        a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + m.conv_w2h_off);
        a.wscale = m.packed_dev + m.conv_scale_off + 1;
        a.bad = bad;
        K_TRY(launch_conv_win(a, s), "conv (window per workgroup)");
        return 0;
    }
    if (r.conv != CONV_LAUNCH) return fail(MTADGAT_ERR_INVALID, "internal: front route names no convolution launch");
    if (r.conv_build == FRONT_BF16) {
        a.bf16 = 1; a.Fq = m.Fp16;
        a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + m.conv_w16_off);
    } else if (r.conv_build == FRONT_X3) {
        a.Wp3 = reinterpret_cast<const f32x4*>(m.packed_dev + m.conv_w3_off);
        a.Fq = m.Fp16;
    }
    K_TRY(launch_conv(a, s), "conv");
    return 0;
}

// CONV_SHARED: the convolution of n stride-1 windows of a series without computing a shared row more than once (SURVEY section
// 8f row 3: interior rows are shared by up to W windows; the per-window zero padding, modules.py:14,20, makes the first / last
// `pad` rows of every window its own).  Three launches of the SAME kernel -- so every value equals the per-window launch's, bit
// for bit: the segment as one (n + W - 1)-row window, the windows' first and last 2 pad rows as 2 pad-row windows -- and a
// copy that places the rows into h_cat.
int run_conv_shared(Model& m, const XSource& src, int64_t c0, int64_t n, float* hcat, float* cf, float* el, float* er, hipStream_t s,
                    unsigned* vmax) {
    XSource seg = src;
    seg.start0 = src.start0 + c0; seg.stride = 1;
    const int64_t L = n + m.W - 1, EW = 2 * m.pad;
    HIP_TRY(hipMemsetAsync(vmax, 0, sizeof(unsigned), s));
    auto rows = [&](int64_t nwin, int64_t Wk, float* out) {
        Scope sc(m, S_CONV, s);
        ConvArgs a = conv_args(m, seg, 0, nwin, Wk);
        a.XC = out; a.vmax = vmax;
        K_TRY(launch_conv(a, s), "conv");
        return 0;
    };
    int rc;
    if ((rc = rows(1, L, cf))) return rc;
    if ((rc = rows(n, EW, el))) return rc;
    seg.start0 += m.W - EW;
    if ((rc = rows(n, EW, er))) return rc;
    Scope sc(m, S_CONV, s);
    K_TRY(launch_conv_scatter(cf, el, er, hcat, n, m.W, m.F, m.Fp, m.Dp, m.pad, s), "conv row placement");
    return 0;
}

// The sign-group boundaries handed to the attention kernels by VALUE: GATv2 layers keep the authoritative [P8, PT] in the packed image
// (the device-side re-pack moves them without telling the host), every kernel reads them through its `ord` pointer, and the by-value
// copies are poisoned so that a path that forgot `ord` fails its parity tests instead of using a stale order; GAT (v1) has no
// sign groups (0, 0).
static int pt_by_value(const Model& m, const GatPlan& g) { return m.cfg.use_gatv2 ? -1 : g.PT; }
static int p8_by_value(const Model& m, const GatPlan& g) { return m.cfg.use_gatv2 ? -1 : g.P8; }

int run_proj(Model& m, const GatPlan& g, const FrontLayerRoute& lr, const float* rows, long ld, int64_t nrows, float* lc, float* rt,
             hipStream_t s) {
    Scope sc(m, S_PROJ, s);
    RowGemmArgs a{};
    a.X = rows; a.ldx = ld; a.Kvalid = g.D; a.Q = g.Q;
    a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + g.w_off);
    a.bias = m.packed_dev + g.b_off;
    a.Y = lc; a.ldy = g.ldl; a.Nvalid = g.ldl; a.vec_store = 1;
    a.R = nrows; a.NT = g.NT; a.relu = 0;
    a.NT_rm = g.NT_L; a.YT = rt; a.group = g.K; a.YT_rows = g.rt_rows; a.YT_ld = g.Kp;
    if (lr.split_pack)
        if (int rc_ = ensure(m, g.split, s)) return rc_;
    if (lr.build == FRONT_X3) {       // the split row GEMM
        a.x3 = 1; a.Q16 = g.uQ16;
        a.Wp3 = reinterpret_cast<const f32x4*>(m.packed_dev + g.uw3_off);
    }
    K_TRY(launch_rowgemm(a, s), "gat projection");
    return 0;
}

int run_attend(Model& m, const GatPlan& g, const FrontLayerRoute& lr, const float* lc, const float* rt, const float* v, int ldv,
               int64_t n, float* out, long so_w, long so_i, long so_d, float* sc, hipStream_t s, float* att = nullptr,
               const DropArgs* drop = nullptr, unsigned drop_stream = 0) {
    Scope sc_(m, S_ATTEND, s);
    if (lr.kernel == LAYER_WIDE) {
        // LDS-tiled pair grid of the fused kernel over the HBM-resident projections (BASELINE config 4 shapes)
        K_TRY(launch_gat_wide(lc, rt, g.ldl, g.rt_rows, g.Kp, pt_by_value(m, g), p8_by_value(m, g), m.packed_dev + g.bias_off, v, ldv, g.D, g.K, out, so_w,
                              so_i, so_d, n, m.cfg.use_gatv2 ? 0 : 1, m.cfg.alpha, s, att, drop, drop_stream,
                              m.cfg.use_gatv2 ? reinterpret_cast<const int*>(m.packed_dev + g.ord_off) : nullptr),
              "wide gat attention");
        return 0;
    }
    if (att) sc = att;       // training forward: the softmax rows are built in the tape's attention matrix
    if (!sc) return fail(MTADGAT_ERR_INVALID, "internal: no score scratch for an attention layer with more than 512 nodes / features");
    AttendArgs a{};
    a.LC = lc; a.RT = rt; a.ldl = g.ldl; a.rt_rows = g.rt_rows; a.Kp = g.Kp; a.PT = pt_by_value(m, g); a.P8 = p8_by_value(m, g);
    a.ord = m.cfg.use_gatv2 ? reinterpret_cast<const int*>(m.packed_dev + g.ord_off) : nullptr;
    a.bias = m.packed_dev + g.bias_off;
    a.V = v; a.ldv = ldv; a.D = g.D;
    a.out = out; a.so_w = so_w; a.so_i = so_i; a.so_d = so_d;
    a.K = g.K;
    a.nwin = n;
    a.v1 = m.cfg.use_gatv2 ? 0 : 1;
    a.alpha = m.cfg.alpha;
    a.S = sc;
    K_TRY(launch_attend(a, drop, drop_stream, s), "gat attention (score matrix)");
    return 0;
}

// fused layer: V rows (n*K, ldv) -> out, nothing but V read from / out written to HBM
// vmax: the convolution's recorded range (the route's `range`); cv (temporal layer behind CONV_IN_GATH): the window convolution
// runs inside k_gath's workgroup
int run_gat_fused(Model& m, const GatPlan& g, const FrontLayerRoute& lr, const float* v, int ldv, int vt, int64_t n, float* out,
                  long so_w, long so_i, long so_d, hipStream_t s, float* att = nullptr, const DropArgs* drop = nullptr,
                  unsigned drop_stream = 0, const unsigned* vmax = nullptr, const GatConvIn* cv = nullptr) {
    Scope sc(m, S_ATTEND, s);
    if (cv && lr.kernel != LAYER_GATH) return fail(MTADGAT_ERR_INVALID, "internal: fused convolution without k_gath");
    GatArgs a{};
    a.V = v; a.ldv = ldv; a.vt = vt; a.D = g.D; a.K = g.K; a.vld = g.f_vld; a.lr_floats = g.f_lr;
    a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + g.w_off);
    a.pbias = m.packed_dev + g.b_off;
    a.NT_L = g.NT_L; a.Q = g.Q; a.PT = pt_by_value(m, g); a.P8 = p8_by_value(m, g);
    a.ord = m.cfg.use_gatv2 ? reinterpret_cast<const int*>(m.packed_dev + g.ord_off) : nullptr;
    if (lr.split_pack)
        if (int rc_ = ensure(m, g.split, s)) return rc_;
    if (lr.build == FRONT_BF16) {
        a.bf16 = 1; a.Q = g.Q16;
        a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + g.w16_off);
    } else if (lr.build == FRONT_X3) {
        a.bf16 = 2; a.Q = g.Q16;
        a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + g.w3_off);
    }
    if (lr.fp16) {       // two fp16 pieces instead when the convolution that produced the node values recorded a maximum below 2^15
        a.vmax = vmax;
        a.Wp2 = reinterpret_cast<const f32x4*>(m.packed_dev + g.w2h_off);
        a.scale2 = m.packed_dev + g.gscale_off + 1;
    }
    a.bias = m.packed_dev + g.bias_off;
    a.out = out; a.so_w = so_w; a.so_i = so_i; a.so_d = so_d;
    a.nwin = n;
    a.v1 = m.cfg.use_gatv2 ? 0 : 1;
    a.alpha = m.cfg.alpha;
    a.ATT = att;
    if (drop) a.drop = *drop;
    a.drop_stream = drop_stream;
    if (lr.kernel == LAYER_GATH) {
        GatArgs b = a;
        b.vld = g.fh_vld; b.lr_floats = g.fh_lr; b.n_full = g.fh_full; b.n_short = g.fh_short;
        b.lr_buf = g.fh_lr_buf;
        b.E = m.cfg.use_gatv2 ? g.E : 0;
        b.dbg = m.gath_dbg;              // (measurement hook: mtadgat_set_option "gath_dbg", profiles/gath_knockout.py)
        if (cv) b.cv = *cv;
        K_TRY(launch_gath(b, g.fh_IBL, g.fh_JPL, g.fh_RJ, g.f_nw, g.fh_lds_bytes, cv != nullptr, s), cv ? "fused convolution + gat (fp16 pieces)" : "fused gat (fp16 pieces)");
        a.skip_h = 1;
        if (cv) a.winflag = cv->flag;    // per-window range guard: k_gat serves exactly the windows k_gath flagged
    }
    K_TRY(launch_gat(a, g.f_IBL, g.f_JPL, g.f_RJ, g.f_nw, g.f_lds_bytes, s), "fused gat");
    return 0;
}

// k_gath's convolution input (CONV_IN_GATH) for the windows from c0 on
GatConvIn fused_conv_args(const Model& m, const XSource& src, int64_t c0, float* hcat, unsigned* vmax, unsigned char* flag) {
    GatConvIn cv{};
    fill_source(m, src, c0, cv);
    cv.taps = m.taps; cv.pad = m.pad; cv.Fq = m.Fp16; cv.NT = m.convNT; cv.Dp = m.Dp;
    cv.pvx = conv_win_pitch(m.F, m.Fp16);
    cv.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + m.conv_w2h_off);
    cv.bias = m.packed_dev + m.conv_b_off;
    cv.wscale = m.packed_dev + m.conv_scale_off + 1;
    cv.HCAT = hcat; cv.vmax = vmax; cv.flag = flag;
    return cv;
}

// One graph-attention layer as its route says.  Fused: from the node rows v (vt = 1: their columns are the nodes); un-fused: the
// projection through lc / rt, then the attention (sc: score scratch of k_attend).  att / drop: training forward and attention maps.
struct LayerIo {
    const float* v = nullptr; int ldv = 0, vt = 0;
    float* lc = nullptr; float* rt = nullptr; float* sc = nullptr;
    float* out = nullptr; long so_w = 0, so_i = 0, so_d = 0;
    float* att = nullptr; const DropArgs* drop = nullptr; unsigned drop_stream = 0;
    const unsigned* vmax = nullptr; const GatConvIn* cv = nullptr;
};
// a layer that writes its third of h_cat (forward, training forward, attention maps); node rows: those of h_cat[:, :F] -- a fused
// feature layer reads its nodes from their columns -- or, un-fused feature layer, of xc^T
LayerIo hcat_layer(const Model& m, bool temporal, bool fused, float* hcat, const float* xct, float* lc, float* rt) {
    LayerIo io;
    io.v = (temporal || fused) ? hcat : xct; io.ldv = (temporal || fused) ? m.Dp : m.Wp; io.vt = !temporal && fused;
    io.lc = lc; io.rt = rt; io.out = hcat + (temporal ? 2 : 1) * m.F;
    io.so_w = (long)m.W * m.Dp; io.so_i = temporal ? m.Dp : 1; io.so_d = temporal ? 1 : m.Dp;
    return io;
}
int run_gat_layer(Model& m, const GatPlan& g, const FrontLayerRoute& lr, const LayerIo& io, int64_t n, hipStream_t s) {
    if (lr.fused())
        return run_gat_fused(m, g, lr, io.v, io.ldv, io.vt, n, io.out, io.so_w, io.so_i, io.so_d, s, io.att, io.drop, io.drop_stream, io.vmax, io.cv);
    if (int rc = run_proj(m, g, lr, io.v, io.ldv, n * g.K, io.lc, io.rt, s)) return rc;
    return run_attend(m, g, lr, io.lc, io.rt, io.v, io.ldv, n, io.out, io.so_w, io.so_i, io.so_d, io.sc, s, io.att, io.drop, io.drop_stream);
}

// A Linear over (window, step) rows in the default fp32 arithmetic: from 65 536 rows on the products come from three bf16 pieces per
// operand on the 16-bit matrix pipe (k_rowgemm_x3 / _x3s: 2.7 x less matrix time than the fp32 MFMA, results <= 2e-7 apart), with the
// split pack derived on first use after an upload -- as the wide attention layers' projections and the backward's data gradients
// do.  Round 6: the GRU's hoisted input projection and recon_model.fc ran on the fp32 MFMA whatever the size (config 4: two 2.3 ms
// launches per 896-window chunk, 42 of its 268 ms per 8 192 windows).
int lin_split_operands(Model& m, const LinPlan& p, long rows, RowGemmArgs& a, hipStream_t s) {
    if (!rowgemm_split(m, p.w3_off && p.Q16 > 0, rows, false)) return 0;
    if (int rc_ = ensure(m, p.split, s)) return rc_;
    a.x3 = 1; a.Q16 = p.Q16;
    a.Wp3 = reinterpret_cast<const f32x4*>(m.packed_dev + p.w3_off);
    return 0;
}

// The k_rowgemm arguments of a Linear over rows: Y = X W^T + b for `rows` rows of X (row stride ldx).  ldy == 0: Y is the caller's
// dense (rows, out_dim) tensor, stored with vector stores when its rows are 16-byte aligned; otherwise an internal buffer with
// 16-byte aligned rows of ldy floats, all of them written.  The caller adds what its site needs: ReLU, dropout, lin_split_operands.
RowGemmArgs lin_rows(const Model& m, const LinPlan& p, const float* x, long ldx, long rows, float* y, long ldy = 0) {
    RowGemmArgs a{};
    a.X = x; a.ldx = ldx; a.Kvalid = p.in_dim; a.Q = p.Q;
    a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + p.w_off);
    a.bias = m.packed_dev + p.b_off;
    a.R = rows; a.NT = p.NT; a.NT_rm = p.NT; a.group = 1;
    a.Y = y;
    if (ldy) {
        a.ldy = ldy; a.Nvalid = (int)ldy; a.vec_store = 1;
    } else {
        a.ldy = p.out_dim; a.Nvalid = p.out_dim;
        a.vec_store = (p.out_dim % 4 == 0 && aligned16(y)) ? 1 : 0;
    }
    return a;
}

// the buffers of one recurrence layer's call
struct GruIo {
    const float* x = nullptr;        // rows (n*T, ldx) for xmode 0, hin (n, ldx) for xmode 1
    long ldx = 0;
    int kx = 0;
    float* hend = nullptr;           // (n, ldhe) last states, or null
    long ldhe = 0;
    float* seq = nullptr;            // (n*T, Hp) states of every step, or null
    const LinPlan* fc = nullptr;     // a per-step Linear to run inside the recurrence, into yfc (all steps) / ylast (last step)
    float* yfc = nullptr;
    float* ylast = nullptr;
    float* gates = nullptr;          // training forward: the gate activations of every step
    float* xp = nullptr;             // room for the input products of all steps (n*T, 3 Hp), or null
    const unsigned* vmax = nullptr;  // the convolution's recorded output range, or null
};

// The operand packs `k` reads, into a.  A split-operand kernel and the fallback behind it share one pack selection at inference
// (the tile-major kernel reads the three-piece input pack the others' two-piece packs were split beside); the training forward's
// fallback is the fp32 kernel.
void gru_select_packs(const Model& m, const GruPlan& g, const GruRoute& r, GruKernel k, int xmode, const GruIo& io, GruArgs& a) {
    auto at = [&](size_t off) { return reinterpret_cast<const f32x4*>(m.packed_dev + off); };
    const bool train_x3 = io.gates && k == GRU_SPLIT_X3, infer_x3 = !io.gates && r.split_packs;
    a.Wx = at(g.wx_off); a.Wh = at(g.wh_off); a.whs = 4 * g.NCG + 2; a.Qxp = g.Qxp;
    a.bf16 = 0; a.x3 = 0; a.scale = nullptr; a.qb3 = 0; a.vmax = nullptr; a.Wx2 = nullptr; a.Wxq = nullptr;
    if (m.precision == 1) {       // bf16 operand build: the same streams in 16-feature chunks (inference, and the bf16 training step)
        a.Wx = at(g.wx16_off); a.Wh = at(g.wh16_off);
    }
    if (m.precision == 1 || train_x3 || infer_x3) {
        a.whs = 2 * g.NCG + 2; a.Qxp = g.Qxp16; a.bf16 = 1;
    }
    if (train_x3) {
        a.Wh = at(g.wh3_off); a.x3 = 1; a.scale = m.packed_dev + g.scale_off + 1;
        a.vmax = r.guarded ? io.vmax : nullptr;                  // layer 0: the convolution's channels need the recorded range
        a.Wxq = at(r.guarded ? g.wx2_off : g.wx3_off);
    } else if (infer_x3) {
        a.Wx = at(g.wx3_off); a.Wh = at(g.wh3_off); a.x3 = 1; a.scale = m.packed_dev + g.scale_off + 1;
        a.qb3 = g.qb3;
        if (r.guarded) {
            a.vmax = io.vmax;
            a.Wx2 = at(g.wx2_off);
        }
        if (r.first == GRU_SPLIT_X3) a.Wxq = (xmode == 0 && a.Wx2) ? a.Wx2 : a.Wx;      // the two-piece input pack in [tile][chunk] order
        if (r.first == GRU_CM) a.Wxq = xmode == 1 ? a.Wx : at(g.wxq_off);
    } else if (io.gates && r.fallback != GRU_NONE) {
        a.vmax = io.vmax;                                        // the fp32 kernel serves the launch when the range is too large
    }
}

int launch_gru_kernel(const GruRoute& r, GruKernel k, const GruArgs& a, int ncg, int xmode, bool fc, hipStream_t s) {
    switch (k) {
        case GRU_SPLIT: K_TRY(launch_gru_split(a, ncg, xmode, fc, s), a.Gates ? "gru (training)" : "gru (hidden-tile split)"); return 0;
        case GRU_SPLIT_X3: K_TRY(launch_gru_split_x3(a, ncg, xmode, fc, s), a.Gates ? "gru (training, split operands)" : "gru (hidden-tile split, split operands)"); return 0;
        case GRU_CM: K_TRY(launch_gru_cm(a, ncg, xmode, fc, s), "gru (chunk-major)"); return 0;
        case GRU_TILE: K_TRY(launch_gru_tile(a, ncg, xmode, fc, r.build, r.two, s), "gru (tile-major)"); return 0;
        default: return fail(MTADGAT_ERR_INVALID, "internal: recurrence route names no throughput kernel");
    }
}

// one GRU layer of `stack`: the kernels gru_route names, in its order
int run_gru_layer(Model& m, int slot, const std::vector<GruPlan>& stack, int layer, const GruIo& io, int64_t n, hipStream_t s) {
    Scope sc(m, slot, s);
    const GruPlan& g = stack[layer];
    GruCall c;
    c.training = io.gates != nullptr;
    c.fc = io.fc != nullptr; c.fc_out_dim = io.fc ? io.fc->out_dim : 0;
    c.range = io.vmax != nullptr; c.xp = io.xp != nullptr;
    c.hend_fits = io.hend == nullptr || io.ldhe >= g.Hp;
    const GruRoute r = gru_route(m, stack, layer, n, cu_count(), c);
    const float* x = io.x;
    long ldx = io.ldx;
    int xmode = g.xmode;
    if (r.hoist) {
        if (g.xmode == 0) {
            RowGemmArgs p = lin_rows(m, g.xproj, x, ldx, n * m.W, io.xp, 3L * g.Hp);
            if (int rc_ = lin_split_operands(m, g.xproj, p.R, p, s)) return rc_;
            K_TRY(launch_rowgemm(p, s), "gru input projection");
        } else {
            K_TRY(launch_xproj_dec(x, ldx, io.kx, m.packed_dev + g.fold_off, reinterpret_cast<const int*>(m.packed_dev + g.m0_off),
                                   m.packed_dev + g.b_off, g.Hp, m.W, n, io.xp, s), "decoder input projection");
        }
        x = io.xp; ldx = 3L * g.Hp; xmode = 3;
    }
    if (r.small()) {
        if (!g.has16 || io.fc) return fail(MTADGAT_ERR_INVALID, "internal: k_gru16 without its buffers");
        Gru16Args a{};
        a.XP = x; a.W16 = m.packed_dev + (r.first == GRU_WINDOW ? g.g1_off : g.g16_off); a.bias = m.packed_dev + g.b_off;
        a.Hp = g.Hp; a.KS = g.KS16; a.NT16 = g.NT16; a.T = m.W; a.B = n;
        a.Hend = io.hend; a.ldhe = io.ldhe; a.ncol = (int)std::min<long>(io.ldhe, g.Hp); a.Seq = io.seq; a.Gates = io.gates; a.H = g.H;
        if (r.first == GRU_WINDOW) K_TRY(launch_gru1(a, s), "gru (window per workgroup)");
        else K_TRY(launch_gru16(a, s), "gru (16-window groups)");
        return 0;
    }
    if (r.split_packs) {
        if (int rc_ = ensure(m, g.split, s)) return rc_;
    }
    GruArgs a{};
    a.X = x; a.ldx = ldx; a.Kx = io.kx; a.Qx = g.Qx;
    a.m0 = xmode == 1 ? reinterpret_cast<const int*>(m.packed_dev + g.m0_off) : nullptr;
    a.bias = m.packed_dev + g.b_off;
    a.Hp = g.Hp; a.H = g.H; a.T = m.W; a.B = n;
    a.Hend = io.hend; a.ldhe = io.ldhe;
    a.Seq = io.seq; a.ldseq = g.Hp;
    if (r.fc_rides) {
        a.Wfc = reinterpret_cast<const f32x4*>(m.packed_dev + io.fc->w_off);
        a.bfc = m.packed_dev + io.fc->b_off;
        a.NTfc = io.fc->NT;
        a.Yfc = io.yfc;
        a.Ylast = io.ylast;
        a.out_dim = io.fc->out_dim;
    }
    a.Gates = io.gates;
    gru_select_packs(m, g, r, r.first, xmode, io, a);
    if (int rc_ = launch_gru_kernel(r, r.first, a, g.NCG, xmode, r.fc_rides, s)) return rc_;
    if (r.fallback == GRU_NONE) return 0;
    // both kernels are launched, each returns at once when the launch is the other's (the device reads the recorded range)
    gru_select_packs(m, g, r, r.fallback, xmode, io, a);
    a.skip_xh = 1;
    return launch_gru_kernel(r, r.fallback, a, g.NCG, xmode, r.fc_rides, s);
}

// hcat is the internal (n*W, Dp) buffer: 16-byte aligned rows whose pad columns are zero (the kernels read them unguarded)
int run_gru_stack(Model& m, const float* hcat, long ldx, int64_t n, float* hend, long ldhe, float* ws,
                  const Workspace& o, hipStream_t s, const unsigned* vmax = nullptr) {
    const int L = (int)m.gru.size();
    const float* x = hcat;
    long ld = ldx;
    int kx = 3 * m.F;
    for (int l = 0; l < L; ++l) {
        const bool last = (l == L - 1);
        float* seq = last ? nullptr : ws + ((l & 1) ? o.seq1 : o.seq0);
        GruIo io;
        io.x = x; io.ldx = ld; io.kx = kx; io.hend = last ? hend : nullptr; io.ldhe = ldhe; io.seq = seq;
        if (l == 0) { io.xp = o.has_xp ? ws + o.xp : nullptr; io.vmax = vmax; }
        if (int rc = run_gru_layer(m, S_GRU, m.gru, l, io, n, s)) return rc;
        x = seq; ld = m.gru[l].Hp; kx = m.gru[l].H;      // sequence buffers hold all Hp columns, padding lanes are exact zeros
    }
    return 0;
}

// hend is the internal (n, Hp) buffer with zero pad columns
int run_heads(Model& m, const float* hend, long ldh, int64_t n, float* preds, float* recons, float* recons_last,
              float* ws, const Workspace& o, hipStream_t s) {
    if (preds) {
        Scope sc(m, S_FC, s);
        const float* x = hend;
        long ld = ldh;
        const int nfc = (int)m.fc.size();
        for (int i = 0; i < nfc; ++i) {
            const LinPlan& p = m.fc[i];
            const bool last = (i == nfc - 1);
            RowGemmArgs a = last ? lin_rows(m, p, x, ld, n, preds) : lin_rows(m, p, x, ld, n, ws + ((i & 1) ? o.fc1 : o.fc0), p.NT * 32);
            a.relu = last ? 0 : 1;   // eval mode: dropout is the identity (reference modules.py:309-310)
            K_TRY(launch_rowgemm(a, s), "forecasting head");
            x = a.Y; ld = a.ldy;
        }
    }
    if (recons || recons_last) {
        const int L = (int)m.rec.size();
        const float* x = hend;
        long ld = ldh;
        int kx = m.cfg.gru_hid_dim;
        // decoder layer 0 reads hend[m0(t) .. m0(t) + 8*Qx), clamped to the (zero padded) row inside the kernel
        // recon_model.fc (modules.py:282): with few outputs (target dims of MSL / SMAP) it rides inside the recurrence;
        // otherwise the last layer's states go to memory and the Linear is one throughput GEMM over the b*W rows --
        // inside the step loop it would sit on the latency chain with 4 * Qh matrix instructions per 32 outputs
        if (gru_stack_small(m, m.rec, n, false) && o.rec16) {
            // small batch: k_gru16 keeps the states (or, when only the last step is wanted, the last state) and
            // recon_model.fc is a row GEMM over them
            Scope sc(m, S_RECON, s);
            const GruPlan& g = m.rec[0];
            const LinPlan& p = m.rec_fc;
            float* seq = ws + o.rseq0;
            GruIo io;
            io.x = x; io.ldx = ld; io.kx = kx; io.hend = recons ? nullptr : seq; io.ldhe = g.Hp; io.seq = recons ? seq : nullptr;
            io.xp = ws + o.xp;
            if (int rc = run_gru_layer(m, S_RECON, m.rec, 0, io, n, s)) return rc;
            RowGemmArgs a = lin_rows(m, p, seq, g.Hp, recons ? n * (int64_t)m.W : n, recons ? recons : recons_last);
            // (the arithmetic is chosen by the size of the whole reconstruction, also when only its last step is wanted: score_series
            // equals forward() on the same windows bit for bit)
            if (int rc_ = lin_split_operands(m, p, n * (int64_t)m.W, a, s)) return rc_;
            K_TRY(launch_rowgemm(a, s), "reconstruction Linear");
            if (recons && recons_last)
                K_TRY(launch_copy2d(recons + (int64_t)(m.W - 1) * p.out_dim, (long)m.W * p.out_dim, recons_last, p.out_dim, n, p.out_dim, s),
                      "last reconstruction step");
            return 0;
        }
        const bool hoist_fc = m.cfg.out_dim > 4 && recons != nullptr;
        for (int l = 0; l < L; ++l) {
            const bool last = (l == L - 1);
            const bool fc_in = last && !hoist_fc;
            float* seq = (last && !hoist_fc) ? nullptr : ws + ((l & 1) ? o.rseq1 : o.rseq0);
            GruIo io;
            io.x = x; io.ldx = ld; io.kx = kx; io.seq = seq;
            if (fc_in) { io.fc = &m.rec_fc; io.yfc = recons; io.ylast = recons_last; }
            if (int rc = run_gru_layer(m, S_RECON, m.rec, l, io, n, s)) return rc;
            x = seq; ld = m.rec[l].Hp; kx = m.rec[l].H;
        }
        if (hoist_fc) {
            Scope sc(m, S_RECON, s);
            const LinPlan& p = m.rec_fc;
            RowGemmArgs a = lin_rows(m, p, x, ld, n * (int64_t)m.W, recons);
            if (int rc_ = lin_split_operands(m, p, a.R, a, s)) return rc_;
            K_TRY(launch_rowgemm(a, s), "reconstruction Linear");
            if (recons_last)
                K_TRY(launch_copy2d(recons + (int64_t)(m.W - 1) * p.out_dim, (long)m.W * p.out_dim, recons_last, p.out_dim, n, p.out_dim, s),
                      "last reconstruction step");
        }
    }
    return 0;
}

// The non-finite contract (include/mtadgat.h): NaN over the outputs of the windows from c0 on that hold a NaN / inf sample, behind the
// heads that wrote them and on their stream.  The outputs are those of these n windows.  bad: the per-window flags the piece's
// convolution left (k_conv_win, k_gath's CONV build: the large-batch routes) -- one byte read per window.  bad == null (every other
// convolution, the training forward): the kernel reads the piece's input once more, n * W * F elements -- a third of h_cat, which is
// written once and read by every layer behind it; 1.4 GB per 65 536 flagship windows, which is why the large-batch routes carry flags.
int run_poison(const Model& m, const XSource& src, int64_t c0, int64_t n, const unsigned char* bad, float* preds, float* recons,
               float* recons_last, hipStream_t s) {
    NonFiniteArgs a{};
    fill_source(m, src, c0, a);
    a.bad = bad;
    a.n = n; a.W = m.W; a.F = m.F; a.od = m.cfg.out_dim;
    a.preds = preds; a.recons = recons; a.recons_last = recons_last;
    K_TRY(launch_poison_nonfinite(a, s), "non-finite windows");
    return 0;
}

// plan: the call's forward plan where the caller has made it (forward_impl)
int check_common(mtadgat_handle h, int64_t batch, void* ws, size_t ws_bytes, bool need_ws, const ForwardPlan* plan = nullptr) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    if (batch < 0) return fail(MTADGAT_ERR_INVALID, "negative batch");
    if (!h->m.have_weights) return fail(MTADGAT_ERR_NOWEIGHTS, "mtadgat_load_weights has not been called");
    if (h->m.precision == 1 && !h->m.bf16_packed)
        return fail(MTADGAT_ERR_NOWEIGHTS, "bf16 precision selected after the weights were loaded: call mtadgat_load_weights again");
    if (need_ws && batch > 0) {
        if (!ws) return fail(MTADGAT_ERR_WORKSPACE, "workspace is NULL");
        if (!aligned16(ws)) return fail(MTADGAT_ERR_WORKSPACE, "workspace must be 16-byte aligned");
        if (ws_bytes < (plan ? plan->total_floats : plan_forward(h->m, batch).total_floats) * sizeof(float))
            return fail(MTADGAT_ERR_WORKSPACE, "workspace too small");
    }
    return 0;
}

}  // namespace

int mtadgat::record_error(int code, const char* msg) { return fail(code, msg); }

extern "C" {

int mtadgat_abi_version(void) { return MTADGAT_ABI_VERSION; }
const char* mtadgat_last_error(void) { return g_err.c_str(); }

int mtadgat_create(const mtadgat_config* cfg, mtadgat_handle* out) {
    if (!cfg || !out) return fail(MTADGAT_ERR_INVALID, "null argument");
    mtadgat_handle h = new (std::nothrow) mtadgat_handle_s();
    if (!h) return fail(MTADGAT_ERR_INVALID, "out of host memory");
    h->m.cfg = *cfg;
    std::string err = validate_and_plan(h->m);
    if (!err.empty()) {
        delete h;
        return fail(MTADGAT_ERR_UNSUPPORTED, err);
    }
    size_t free_b = 0, total_b = 0;
    h->m.chunk = default_chunk(h->m, hipMemGetInfo(&free_b, &total_b) == hipSuccess ? (double)total_b : 0.0);
    *out = h;
    return 0;
}

static void free_device_tables(Model& m) {
    DevTables& t = m.dt;
    int cur = 0;
    const bool sw = t.device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != t.device;
    if (sw) (void)hipSetDevice(t.device);
    if (t.gidx_dev) (void)hipFree(t.gidx_dev);
    if (t.foldcode_dev) (void)hipFree(t.foldcode_dev);
    if (t.foldsum_dev) (void)hipFree(t.foldsum_dev);
    for (int i = 0; i < 2; ++i) {
        if (t.gatcode_dev[i]) (void)hipFree(t.gatcode_dev[i]);
        if (t.colk_dev[i]) (void)hipFree(t.colk_dev[i]);
        t.gatcode_dev[i] = t.colk_dev[i] = nullptr;
    }
    if (t.pin) (void)hipHostFree(t.pin);
    if (sw) (void)hipSetDevice(cur);
    t.gidx_dev = t.foldcode_dev = nullptr;
    t.foldsum_dev = nullptr;
    t.pin = nullptr;
    t.ready = false;
    t.device = -1;
}

// the second lane's stream and events belong to the device they were created on (a handle may move: mtadgat_load_weights)
static void free_lane(Model& m) {
    if (!m.lane_stream) return;
    int cur = 0;
    const bool sw = m.lane_device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != m.lane_device;
    if (sw) (void)hipSetDevice(m.lane_device);
    (void)hipStreamSynchronize(m.lane_stream);
    (void)hipStreamDestroy(m.lane_stream);
    (void)hipEventDestroy(m.lane_begin);
    (void)hipEventDestroy(m.lane_end);
    for (hipEvent_t& e : m.fork_ev)
        if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (sw) (void)hipSetDevice(cur);
    m.lane_stream = nullptr;
    m.lane_begin = m.lane_end = nullptr;
    m.lane_device = -1;
}

// the packed image and the split groups' events (created with it) belong to the device they were allocated on
static void free_image(Model& m) {
    if (!m.packed_dev) return;
    int cur = 0;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != m.packed_device;
    if (sw) (void)hipSetDevice(m.packed_device);
    for (SplitGroup& g : m.split.groups)
        if (g.done) { (void)hipEventDestroy(g.done); g.done = nullptr; }
    (void)hipFree(m.packed_dev);
    if (sw) (void)hipSetDevice(cur);
    m.packed_dev = nullptr;
    m.have_weights = false;
}

int mtadgat_destroy(mtadgat_handle h) {
    if (!h) return 0;
    free_device_tables(h->m);
    if (h->m.upload_ev) {
        (void)hipEventSynchronize(h->m.upload_ev);
        (void)hipEventDestroy(h->m.upload_ev);
    }
    free_lane(h->m);
    if (h->m.staging_pinned) (void)hipHostFree(h->m.staging_pinned);
    free_image(h->m);
    for (auto& v : h->m.ev)
        for (auto& p : v) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    delete h;
    return 0;
}

int mtadgat_load_weights(mtadgat_handle h, const mtadgat_params* p, void* stream) {
    if (!h || !p) return fail(MTADGAT_ERR_INVALID, "null argument");
    Model& m = h->m;
    std::vector<float> host;
    std::string err = pack_weights(m, *p, host);
    if (!err.empty()) return fail(MTADGAT_ERR_INVALID, err);
    // the packed weights live on the device that is current now (the caller's); a handle that moves to
    // another GPU gets a fresh allocation there
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (m.packed_dev && m.packed_device != dev) free_image(m);
    if (!m.packed_dev) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m.packed_dev), m.packed_floats * sizeof(float)));
        m.packed_device = dev;
        for (SplitGroup& g : m.split.groups)
            if (hipError_t e = hipEventCreateWithFlags(&g.done, hipEventDisableTiming)) {
                free_image(m);
                return hip_fail(e, "hipEventCreateWithFlags");
            }
    }
    hipStream_t s = (hipStream_t)stream;
    // Stream-ordered upload without a device synchronisation: the packed image goes through a pinned staging
    // buffer owned by the handle (an async copy from pageable memory is not reliably ordered with the kernels
    // that follow on the stream); the buffer is only rewritten after the previous upload's event has fired.
    if (m.upload_ev) HIP_TRY(hipEventSynchronize(m.upload_ev));
    else HIP_TRY(hipEventCreateWithFlags(&m.upload_ev, hipEventDisableTiming));
    if (m.staging_pinned && m.staging_floats < m.packed_floats) {
        (void)hipHostFree(m.staging_pinned);
        m.staging_pinned = nullptr;
    }
    if (!m.staging_pinned) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m.staging_pinned), m.packed_floats * sizeof(float), hipHostMallocDefault));
        m.staging_floats = m.packed_floats;
    }
    std::memcpy(m.staging_pinned, host.data(), m.packed_floats * sizeof(float));
    HIP_TRY(hipMemcpyAsync(m.packed_dev, m.staging_pinned, m.packed_floats * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(m.upload_ev, s));
    ++m.weights_version;                 // every split pack is stale from here on
    m.have_weights = true;
    return 0;
}

/* Re-packs the weight image from a flat device buffer of the parameters (mtadgat_params field order = the order of
 * the flat gradient buffer, see mtadgat_grad_offsets) without a round trip through the host: the training loop's
 * optimizer.step() -> forward.  Needs one previous mtadgat_load_weights on this device (it lays down the padding
 * and the index maps) and the fp32 image (precision 0 or 2).  No host involvement: the column order of the folded GATv2
 * projection (the sign pattern of the two attention vectors `a`) is derived by a kernel as well. */
int mtadgat_update_weights_device(mtadgat_handle h, const float* flat_dev, int64_t n_floats, void* stream) {
    if (!h || !flat_dev) return fail(MTADGAT_ERR_INVALID, "null argument");
    Model& m = h->m;
    if (!m.have_weights || !m.packed_dev) return fail(MTADGAT_ERR_NOWEIGHTS, "update_weights_device needs a previous load_weights");
    if (m.precision == 1) return fail(MTADGAT_ERR_UNSUPPORTED, "device-side re-packing covers the fp32 image only");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != m.packed_device) return fail(MTADGAT_ERR_INVALID, "the weights live on another device");
    DevTables& t = m.dt;
    hipStream_t s = (hipStream_t)stream;
    auto upload = [&](int*& dst, const std::vector<int>& v) -> int {
        if (v.empty()) return 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dst), v.size() * sizeof(int)));
        HIP_TRY(hipMemcpy(dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
        return 0;
    };
    if (!t.ready || t.device != dev) {
        free_device_tables(m);
        std::string err = build_device_tables(m);
        if (!err.empty()) return fail(MTADGAT_ERR_UNSUPPORTED, err);
        int rc;
        if ((rc = upload(t.gidx_dev, t.gidx)) || (rc = upload(t.gatcode_dev[0], t.gatcode[0])) || (rc = upload(t.gatcode_dev[1], t.gatcode[1])) ||
            (rc = upload(t.foldcode_dev, t.foldcode))) return rc;
        for (int which = 0; which < 2; ++which) {
            const GatPlan& g = which == 0 ? m.feat : m.temp;
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t.colk_dev[which]), (size_t)(g.ldl + 16) * sizeof(int)));
            t.colk[which].clear();
        }
        t.device = dev;
        t.ready = true;
    }
    if (n_floats != t.fo.total) return fail(MTADGAT_ERR_INVALID, "flat parameter buffer: wrong number of floats");
    // column order of the GATv2 projections: from the signs of `a`, on the device (round 5: rounds 3-4 read `a` back through pinned
    // memory and synchronised the stream here, once per optimizer step).  The kernels take [P8, PT] from the image from now on;
    // the host's copies keep the values of the last host-side load (they only steer heuristics).
    if (m.cfg.use_gatv2)
        for (int which = 0; which < 2; ++which) {
            const GatPlan& g = which == 0 ? m.feat : m.temp;
            K_TRY(launch_gat_colorder(flat_dev + t.fo.a[which], g.E, (double)m.cfg.alpha, t.colk_dev[which], g.ldl + 16,
                                      reinterpret_cast<int*>(m.packed_dev + g.ord_off), s), "projection column order");
        }
    K_TRY(launch_pack_gather(flat_dev, t.gidx_dev, m.packed_dev, (long)m.packed_floats, s), "weight gather");
    for (int which = 0; which < 2; ++which) {
        const GatPlan& g = which == 0 ? m.feat : m.temp;
        PackGatArgs a{};
        a.flat = flat_dev; a.lin_w = t.fo.lin_w[which]; a.lin_b = t.fo.lin_b[which]; a.a = t.fo.a[which];
        a.E = g.E; a.D = g.D; a.KS = g.ldl; a.ord = reinterpret_cast<const int*>(m.packed_dev + g.ord_off);
        a.v2 = m.cfg.use_gatv2 ? 1 : 0; a.fused = g.fused ? 1 : 0;
        a.alpha = m.cfg.alpha; a.colk = t.colk_dev[which]; a.code = t.gatcode_dev[which];
        a.n_code = g.NT * g.Q * 256; a.n_bias = g.NT * 32;
        a.w_out = m.packed_dev + g.w_off; a.b_out = m.packed_dev + g.b_off;
        K_TRY(launch_pack_gat(a, s), "graph-attention projection pack");
    }
    for (size_t l = 0; l < m.gru.size(); ++l) {
        const GruPlan& g = m.gru[l];
        K_TRY(launch_pack_gru_bias(flat_dev, t.fo.gru_bih[l], t.fo.gru_bhh[l], g.H, g.Hp, m.packed_dev + g.b_off,
                                   g.has_xproj ? m.packed_dev + g.xproj.b_off : nullptr, s), "gru bias pack");
    }
    for (size_t l = 0; l < m.rec.size(); ++l) {
        const GruPlan& g = m.rec[l];
        K_TRY(launch_pack_gru_bias(flat_dev, t.fo.rec_bih[l], t.fo.rec_bhh[l], g.H, g.Hp, m.packed_dev + g.b_off,
                                   g.has_xproj ? m.packed_dev + g.xproj.b_off : nullptr, s), "decoder bias pack");
    }
    if (m.rec[0].xmode == 1) {
        const GruPlan& g = m.rec[0];
        PackFoldArgs a{};
        a.flat = flat_dev; a.wih = t.fo.rec_wih[0]; a.Hin = g.in_dim; a.T = m.W; a.H = g.H; a.Hp = g.Hp; a.NMp = 8 * g.Qx;
        a.code = t.foldcode_dev; a.tile_floats = (long)g.NCG * g.Qxp * 3 * 256;
        a.tiles_out = m.packed_dev + g.wx_off; a.fold_out = g.has16 ? m.packed_dev + g.fold_off : nullptr;
        if (!t.foldsum_dev) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t.foldsum_dev), (size_t)3 * g.H * (g.in_dim + 1) * sizeof(double)));
        a.prefix = t.foldsum_dev;
        K_TRY(launch_pack_fold(a, s), "decoder input fold");
    }
    ++m.weights_version;                 // the split packs follow the fp32 packs they are derived from
    m.bf16_packed = false;
    return 0;
}

int mtadgat_params_fingerprint(const void* const* tensors_dev, const int64_t* n_elements, int n_tensors, uint64_t* out_dev, void* stream) {
    if (!tensors_dev || !n_elements || !out_dev || n_tensors < 0) return fail(MTADGAT_ERR_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(uint64_t), s));
    long base = 0;
    for (int t0 = 0; t0 < n_tensors; t0 += FINGERPRINT_MAX_TENSORS) {
        FingerprintArgs a{};
        const int nt = std::min(FINGERPRINT_MAX_TENSORS, n_tensors - t0);
        for (int t = 0; t < nt; ++t) {
            a.ptr[t] = tensors_dev[t0 + t];
            a.count[t] = (long)n_elements[t0 + t];
            a.base[t] = base;
            base += a.count[t];
        }
        K_TRY(launch_fingerprint(a, nt, reinterpret_cast<unsigned long long*>(out_dev), s), "parameter fingerprint");
    }
    return 0;
}

/* (offset, length) pairs, in floats, of the regions of the packed image reserved for split packs (derived on the device from
 * other regions); at most max_pairs are written, the number of regions is returned */
int mtadgat_derived_regions(mtadgat_handle h, int64_t* out, int max_pairs) {
    if (!h || (!out && max_pairs > 0)) return 0;
    const std::vector<std::pair<size_t, size_t>>& r = h->m.split.regions;
    for (int i = 0; i < max_pairs && i < (int)r.size(); ++i) {
        out[2 * i] = (int64_t)r[i].first;
        out[2 * i + 1] = (int64_t)r[i].second;
    }
    return (int)r.size();
}

/* Read-only test hook (no GPU, no weights): the steps that derive the split packs (SplitTable), over all groups in group order then
 * step order, 10 int64 per step: [group, op (SplitStep::Op), scale, src, dst, n, Qs, Qd, arg, ord]; at most max_steps records are
 * written, the number of steps is returned.  mtadgat_split_n_infer: the groups [0, n_infer) are the ones an inference call may read. */
int mtadgat_split_steps(mtadgat_handle h, int64_t* out, int max_steps) {
    if (!h || (!out && max_steps > 0)) return 0;
    int k = 0;
    const std::vector<SplitGroup>& groups = h->m.split.groups;
    for (size_t g = 0; g < groups.size(); ++g)
        for (const SplitStep& t : groups[g].steps) {
            if (k < max_steps) {
                const int64_t v[10] = {(int64_t)g, (int64_t)t.op, (int64_t)t.scale, (int64_t)t.src, (int64_t)t.dst, (int64_t)t.n, t.Qs, t.Qd, t.arg, (int64_t)t.ord};
                std::copy(v, v + 10, out + 10 * (size_t)k);
            }
            ++k;
        }
    return k;
}
int mtadgat_split_n_infer(mtadgat_handle h) { return h ? h->m.split.n_infer : 0; }

/* Test hook: derives every split group that is stale, the training backward's included, on `stream` (what the consumers do lazily,
 * group by group); mtadgat_read_packed then shows all of them */
int mtadgat_derive_split_packs(mtadgat_handle h, void* stream) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null argument");
    Model& m = h->m;
    if (!m.have_weights || !m.packed_dev) return fail(MTADGAT_ERR_NOWEIGHTS, "no weights loaded");
    for (int i = 0; i < (int)m.split.groups.size(); ++i)
        if (int rc_ = ensure(m, i, (hipStream_t)stream)) return rc_;
    return 0;
}

/* Read-only test hook (no GPU, no weights): the recurrence route (gru_route) of layer `layer` of the GRU stack (stack 0) or the decoder
 * (stack 1) for a whole forward() / training forward of n windows on a device of `compute_units` CUs, under the handle's current
 * precision and "gru_kernel" option: out[0 .. 8) = first kernel, fallback kernel (GruKernel), operand build (GruBuild), two groups
 * per wave, hoisted input products, split packs needed, per-step Linear inside, the stack takes the small-batch kernels */
int mtadgat_gru_route(mtadgat_handle h, int stack, int layer, int64_t n, int training, int compute_units, int* out) {
    if (!h || !out) return fail(MTADGAT_ERR_INVALID, "null argument");
    const Model& m = h->m;
    if (stack != 0 && stack != 1) return fail(MTADGAT_ERR_INVALID, "stack must be 0 (GRU) or 1 (decoder)");
    const std::vector<GruPlan>& st = stack ? m.rec : m.gru;
    if (layer < 0 || layer >= (int)st.size() || n < 1 || compute_units < 1) return fail(MTADGAT_ERR_INVALID, "layer, window count or compute units out of range");
    const GruRoute r = gru_route(m, st, layer, n, compute_units, gru_call_facts(m, stack == 1, layer, n, training != 0));
    const int v[8] = {r.first, r.fallback, r.build, r.two, r.hoist, r.split_packs, r.fc_rides, gru_stack_small(m, st, n, training != 0)};
    std::copy(v, v + 8, out);
    return 0;
}

/* Read-only test hook (no GPU, no weights): front_route of a call; include/mtadgat.h defines the arguments and the 14 ints */
int mtadgat_front_route(mtadgat_handle h, int kind, int source, int64_t n, int facts, int* out) {
    if (!h || !out) return fail(MTADGAT_ERR_INVALID, "null argument");
    if (kind < 0 || kind > FRONT_CONV || source < 0 || source > SRC_SERIES || n < 1 || facts < 0 || facts > 7)
        return fail(MTADGAT_ERR_INVALID, "call kind, source, window count or facts out of range");
    FrontCall c;
    c.kind = (FrontKind)kind; c.source = (FrontSource)source;
    c.rows_aligned = facts & 1; c.ldv_fits = facts & 2; c.hcat_aligned = facts & 4;
    const FrontRoute r = front_route(h->m, n, c);
    auto split_gemm = [](const FrontLayerRoute& l) { return !l.fused() && l.build == FRONT_X3; };
    const int v[14] = {r.conv, r.conv_build, r.conv_split_pack, r.range,
                       r.temp.kernel, r.temp.build, r.temp.fp16, split_gemm(r.temp), r.temp.split_pack,
                       r.feat.kernel, r.feat.build, r.feat.fp16, split_gemm(r.feat), r.feat.split_pack};
    std::copy(v, v + 14, out);
    return 0;
}

/* Read-only test hook (no GPU, no weights): plan_forward of a call of `batch` windows under the handle's chunk size, precision and
 * "lanes" option; include/mtadgat.h defines the values written.  Returns their count. */
int mtadgat_forward_plan(mtadgat_handle h, int64_t batch, int64_t* out, int max_n) {
    if (!h || !out) return fail(MTADGAT_ERR_INVALID, "null argument");
    if (batch < 1) return fail(MTADGAT_ERR_INVALID, "the plan needs at least one window");
    const ForwardPlan p = plan_forward(h->m, batch);
    std::vector<int64_t> v = {(int64_t)p.pieces.size(), p.fork, (int64_t)p.lane_floats[0], (int64_t)p.lane_floats[1], (int64_t)p.total_floats};
    for (const ForwardPiece& pc : p.pieces) v.insert(v.end(), {pc.c0, pc.n, pc.lane});
    if ((int64_t)v.size() > max_n) return fail(MTADGAT_ERR_INVALID, "plan array too small");
    std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}

/* Read-only test hook (no GPU, no weights): the recurrence and attention routes of a training step of n windows under the handle's
 * precision and "gru_kernel" option; include/mtadgat.h defines the values written.  Returns their count. */
int mtadgat_train_route(mtadgat_handle h, int64_t n, int* out, int max_n) {
    if (!h || !out) return fail(MTADGAT_ERR_INVALID, "null argument");
    if (n < 1) return fail(MTADGAT_ERR_INVALID, "the route needs at least one window");
    const Model& m = h->m;
    if (!m.bw.supported) return fail(MTADGAT_ERR_UNSUPPORTED, "no HIP backward for this configuration: " + m.bw.why);
    std::vector<int> v;
    bool fc_rides = false;
    for (int decoder = 0; decoder < 2; ++decoder) {
        const std::vector<GruPlan>& st = decoder ? m.rec : m.gru;
        for (int l = 0; l < (int)st.size(); ++l) {
            const GruRoute f = gru_route(m, st, l, n, XP_PLAN_CUS, gru_call_facts(m, decoder != 0, l, n, true));
            const GruBwdRoute r = gru_bwd_route(m, decoder != 0, l, n);
            v.insert(v.end(), {f.first, r.kernel, r.x3});
            fc_rides = f.fc_rides;          // (of the last decoder layer when the loops end)
        }
    }
    v.push_back(fc_rides);
    for (int which = 0; which < 2; ++which) v.insert(v.end(), {m.bw.gat[which].wide, !m.cfg.use_gatv2});
    if ((int64_t)v.size() > max_n) return fail(MTADGAT_ERR_INVALID, "route array too small");
    std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}

/* Read-only test hook (no GPU, no weights): the weight-gradient GEMMs of a training step of n windows (one chunk of the Python step)
 * in the order of include/mtadgat.h, ten values each; the slab plan is wgrad_slab_plan's, which run_wgrad launches, the rows and
 * loader modes are those backward_impl / walk_stack_backward hand to run_wgrad.  Returns the count of values written. */
int mtadgat_wgrad_plan(mtadgat_handle h, int64_t n, int64_t* out, int max_n) {
    if (!h || !out) return fail(MTADGAT_ERR_INVALID, "null argument");
    if (n < 1) return fail(MTADGAT_ERR_INVALID, "the plan needs at least one window");
    const Model& m = h->m;
    const BwdPlan& b = m.bw;
    if (!b.supported) return fail(MTADGAT_ERR_UNSUPPORTED, "no HIP backward for this configuration: " + b.why);
    std::vector<int64_t> v;
    auto site = [&](const WgradPlan& p, long R, int bmode, int bshift) {
        const WgradSlabPlan sp = wgrad_slab_plan(m, R, p.Mp, p.Np);
        v.insert(v.end(), {(int64_t)R, p.M, p.N, p.Mp, p.Np, sp.nslab, (int64_t)sp.rows_per_slab, bmode, bshift, sp.x3});
    };
    const long RW = (long)n * m.W;
    site(b.conv_wg, RW, 1, 0);
    if (m.cfg.use_gatv2) {
        site(b.gat[0].wg, (long)n * m.F, 0, 0);
        site(b.gat[1].wg, RW, 0, 0);
    }
    for (const std::vector<GruBwdPlan>* st : {&b.gru, &b.rec})
        for (const GruBwdPlan& gp : *st) { site(gp.wg_ih, RW, 0, 0); site(gp.wg_hh, RW, 0, 1); }
    site(b.recfc_wg, RW, 0, 0);
    for (const WgradPlan& p : b.fc_wg) site(p, (long)n, 0, 0);
    if ((int64_t)v.size() > max_n) return fail(MTADGAT_ERR_INVALID, "plan array too small");
    std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}

/* Read-only test hook: rowgemm_split under the handle's precision and "rowgemm_kernel" option (1 / 0, negative: error) */
int mtadgat_rowgemm_split(mtadgat_handle h, int has_pack, int64_t rows, int backward) {
    return h ? (int)rowgemm_split(h->m, has_pack != 0, rows, backward != 0) : fail(MTADGAT_ERR_INVALID, "null handle");
}

/* Host-only self check of the device-side re-pack's gather table (no GPU needed): packs `p` with the host packer, builds
 * the table and counts the image positions whose table entry does not reproduce the packed value from the flat
 * parameter buffer.  *n_gathered receives the number of positions the table covers.  Returns the mismatch count (0 =
 * consistent), or a negative error code. */
int64_t mtadgat_selfcheck_gather_table(mtadgat_handle h, const mtadgat_params* p, int64_t* n_gathered) {
    if (!h || !p) return fail(MTADGAT_ERR_INVALID, "null argument");
    Model& m = h->m;
    const int keep_prec = m.precision;
    m.precision = 0;
    std::vector<float> img;
    std::string err = pack_weights(m, *p, img);
    if (err.empty()) err = build_device_tables(m);
    m.precision = keep_prec;
    if (!err.empty()) return fail(MTADGAT_ERR_UNSUPPORTED, err);
    const DevTables& t = m.dt;
    // the flat parameter buffer in the field order of mtadgat_params
    std::vector<float> flat((size_t)t.fo.total);
    auto put = [&](int64_t off, const float* src, int64_t n) { std::memcpy(flat.data() + off, src, (size_t)n * sizeof(float)); };
    const mtadgat_config& c = m.cfg;
    put(t.fo.conv_w, p->conv_weight, (int64_t)m.F * m.F * m.taps); put(t.fo.conv_b, p->conv_bias, m.F);
    for (int which = 0; which < 2; ++which) {
        const GatPlan& g = which == 0 ? m.feat : m.temp;
        const int lin_in = c.use_gatv2 ? 2 * g.D : g.D;
        put(t.fo.lin_w[which], which == 0 ? p->feat_lin_weight : p->temp_lin_weight, (int64_t)g.E * lin_in);
        put(t.fo.lin_b[which], which == 0 ? p->feat_lin_bias : p->temp_lin_bias, g.E);
        put(t.fo.a[which], which == 0 ? p->feat_a : p->temp_a, c.use_gatv2 ? g.E : 2 * g.E);
        put(t.fo.bias[which], which == 0 ? p->feat_bias : p->temp_bias, (int64_t)g.K * g.K);
    }
    for (size_t l = 0; l < m.gru.size(); ++l) {
        const int in = m.gru[l].in_dim, H = m.gru[l].H;
        put(t.fo.gru_wih[l], p->gru_w_ih[l], (int64_t)3 * H * in); put(t.fo.gru_whh[l], p->gru_w_hh[l], (int64_t)3 * H * H);
        put(t.fo.gru_bih[l], p->gru_b_ih[l], 3 * H); put(t.fo.gru_bhh[l], p->gru_b_hh[l], 3 * H);
    }
    for (size_t i = 0; i < m.fc.size(); ++i) {
        put(t.fo.fc_w[i], p->fc_weight[i], (int64_t)m.fc[i].out_dim * m.fc[i].in_dim); put(t.fo.fc_b[i], p->fc_bias[i], m.fc[i].out_dim);
    }
    for (size_t l = 0; l < m.rec.size(); ++l) {
        const int in = m.rec[l].in_dim, H = m.rec[l].H;
        put(t.fo.rec_wih[l], p->rec_w_ih[l], (int64_t)3 * H * in); put(t.fo.rec_whh[l], p->rec_w_hh[l], (int64_t)3 * H * H);
        put(t.fo.rec_bih[l], p->rec_b_ih[l], 3 * H); put(t.fo.rec_bhh[l], p->rec_b_hh[l], 3 * H);
    }
    put(t.fo.rec_fc_w, p->rec_fc_weight, (int64_t)c.out_dim * c.recon_hid_dim); put(t.fo.rec_fc_b, p->rec_fc_bias, c.out_dim);
    int64_t bad = 0, cov = 0;
    for (size_t i = 0; i < m.packed_floats; ++i) {
        const int g = t.gidx[i];
        if (g < 0) continue;
        ++cov;
        if (std::memcmp(&img[i], &flat[(size_t)g], sizeof(float)) != 0) ++bad;
    }
    if (n_gathered) *n_gathered = cov;
    return bad;
}

int64_t mtadgat_packed_floats(mtadgat_handle h) { return h ? (int64_t)h->m.packed_floats : 0; }
int mtadgat_read_packed(mtadgat_handle h, float* dst_host, int64_t n_floats, void* stream) {
    if (!h || !dst_host) return fail(MTADGAT_ERR_INVALID, "null argument");
    Model& m = h->m;
    if (!m.have_weights || !m.packed_dev) return fail(MTADGAT_ERR_NOWEIGHTS, "no weights loaded");
    if (n_floats != (int64_t)m.packed_floats) return fail(MTADGAT_ERR_INVALID, "wrong size");
    if (int rc_ = ensure_all_split(m, (hipStream_t)stream)) return rc_;      // the image as the kernels would see it
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(dst_host, m.packed_dev, m.packed_floats * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int mtadgat_set_precision(mtadgat_handle h, int mode) {
    if (!h || mode < 0 || mode > 2)
        return fail(MTADGAT_ERR_INVALID, "precision mode must be 0 (fp32 MFMA), 1 (bf16 operands) or 2 (fp32 through split-bf16 operands)");
    h->m.precision = mode;
    return 0;
}

/* 1 when the bf16 weight streams are present in the packed image (they are packed by mtadgat_load_weights only
 * while precision 1 is selected: call set_precision before load_weights, or load again after switching) */
int mtadgat_bf16_ready(mtadgat_handle h) { return (h && h->m.have_weights && h->m.bf16_packed) ? 1 : 0; }

/* Testing / measurement hook: "gru_kernel" = 0 automatic choice of the large-batch recurrence kernel, 1 tile-major (k_gru),
 * 2 chunk-major (k_gru_cm) wherever it applies, 3 hidden-tile split on split operands (k_gru_split X3H) wherever it applies */
int mtadgat_set_option(mtadgat_handle h, const char* name, int value) {
    if (!h || !name) return fail(MTADGAT_ERR_INVALID, "null argument");
    if (std::strcmp(name, "gru_kernel") == 0 && value >= 0 && value <= 3) { h->m.gru_kernel = value; return 0; }
    if (std::strcmp(name, "gat_kernel") == 0 && (value == 0 || value == 1 || value == 3)) { h->m.gat_kernel = value; return 0; }
    if (std::strcmp(name, "wgrad_kernel") == 0 && value >= 0 && value <= 2) { h->m.wgrad_kernel = value; return 0; }
    if (std::strcmp(name, "conv_kernel") == 0 && value >= 0 && value <= 2) { h->m.conv_kernel = value; return 0; }
    if (std::strcmp(name, "rowgemm_kernel") == 0 && value >= 0 && value <= 2) { h->m.rowgemm_kernel = value; return 0; }
    if (std::strcmp(name, "gemm_lds") == 0 && value >= 0 && value <= 1) { set_gemm_lds_off(value); return 0; }      // process-wide; 1 = off
    if (std::strcmp(name, "conv_shared") == 0 && value >= 0 && value <= 1) { h->m.conv_shared = value; return 0; }
    if (std::strcmp(name, "conv_fused") == 0 && value >= 0 && value <= 1) { h->m.conv_fused = value; return 0; }
    if (std::strcmp(name, "lanes") == 0 && value >= 0 && value <= 1) { h->m.lanes = value; return 0; }
    if (std::strcmp(name, "gath_dbg") == 0 && value >= 0 && value <= 63) { h->m.gath_dbg = value; return 0; }
    return fail(MTADGAT_ERR_INVALID, "unknown option or value");
}

/* Largest value the convolution wrote during the last forward() on this workspace (of its last chunk), read back after
 * the stream has drained: below 2^15 the large-batch kernels formed their products from two fp16 pieces per operand, above
 * from three bf16 pieces (the device-side range guard).  0 when the forward did not record it (un-fused attention path). */
int mtadgat_last_conv_max(mtadgat_handle h, const void* ws, int64_t batch, float* out_host, void* stream) {
    if (!h || !ws || !out_host || batch <= 0) return fail(MTADGAT_ERR_INVALID, "null argument");
    const ForwardPlan p = plan_forward(h->m, batch);          // the layout of the call's last piece (each piece has its own plan, each lane its own workspace)
    const ForwardPiece& last = p.pieces.back();
    Workspace o;
    plan_workspace(h->m, last.n, o);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(out_host, static_cast<const float*>(ws) + p.lane_offset(last.lane) + o.vmax, sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int64_t mtadgat_chunk_windows(mtadgat_handle h) { return h ? h->m.chunk : 0; }
int mtadgat_set_chunk_windows(mtadgat_handle h, int64_t w) {
    if (!h || w < 1) return fail(MTADGAT_ERR_INVALID, "chunk must be >= 1");
    h->m.chunk = w;
    return 0;
}

size_t mtadgat_workspace_bytes(mtadgat_handle h, int64_t batch) {
    if (!h || batch <= 0) return 0;
    return plan_forward(h->m, batch).total_floats * sizeof(float);
}

static int forward_impl(mtadgat_handle h, const XSource& src, int64_t batch, float* preds, float* recons, float* recons_last,
                        float* hend_out, void* ws_, size_t ws_bytes, void* stream) {
    const ForwardPlan plan = h && batch > 0 ? plan_forward(h->m, batch) : ForwardPlan();
    int rc = check_common(h, batch, ws_, ws_bytes, true, &plan);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!src.x) return fail(MTADGAT_ERR_INVALID, "input is NULL");
    Model& m = h->m;
    hipStream_t s0 = (hipStream_t)stream;
    const int F = m.F, W = m.W;
    if ((rc = ensure_all_split(m, s0))) return rc;        // (no-ops while the weights are unchanged; before any lane forks off)
    const bool second = plan.second, fork = plan.fork;        // (a small call runs its independent stages side by side: plan_forward)
    const bool both_fused = m.temp.fused && m.feat.fused;
    if (second || fork) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        if (m.lane_stream && m.lane_device != dev) free_lane(m);        // the handle moved to another GPU since the lane was made
        if (!m.lane_stream) {
            m.lane_device = dev;
            HIP_TRY(hipStreamCreateWithFlags(&m.lane_stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&m.lane_begin, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&m.lane_end, hipEventDisableTiming));
            for (hipEvent_t& e : m.fork_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
    }
    if (second) {
        HIP_TRY(hipEventRecord(m.lane_begin, s0));            // the second lane starts after whatever the caller queued before this call
        HIP_TRY(hipStreamWaitEvent(m.lane_stream, m.lane_begin, 0));
    }
    struct Joiner {                                           // the caller's stream waits for the second lane on every way out
        Model& m; hipStream_t s0; bool on;
        ~Joiner() {
            if (on && hipEventRecord(m.lane_end, m.lane_stream) == hipSuccess) (void)hipStreamWaitEvent(s0, m.lane_end, 0);
        }
    } joiner{m, s0, second || fork};
    for (const ForwardPiece& pc : plan.pieces) {
        const int64_t c0 = pc.c0, n = pc.n;
        hipStream_t s = pc.lane ? m.lane_stream : s0;
        float* ws = static_cast<float*>(ws_) + plan.lane_offset(pc.lane);
        Workspace o;
        plan_workspace(m, n, o);
        float* xc = ws + o.xc;
        float* xct = ws + o.xct;
        float* hcat = ws + o.hcat;
        LayerIo temp = hcat_layer(m, true, true, hcat, nullptr, ws + o.lct, ws + o.rtt), feat = hcat_layer(m, false, true, hcat, nullptr, ws + o.lcf, ws + o.rtf);
        temp.sc = feat.sc = ws + o.sc;
        const unsigned char* bad = nullptr;                   // the windows' non-finite flags, where the convolution leaves them
        if (both_fused) {
            // fused front: conv writes only h_cat[:, :F]; each layer's workgroup stages its window from
            // there (the feature layer transposes on the way into LDS) -- no xc / xc^T / L' / R' in HBM
            const FrontRoute r = front_route(m, n, front_call(FRONT_FORWARD, src, hcat, m.Dp, F, hcat));
            unsigned* vmax = reinterpret_cast<unsigned*>(ws + o.vmax);
            temp.vmax = feat.vmax = vmax;
            GatConvIn cv{};
            const bool conv_in_gat = r.conv == CONV_IN_GATH;
            unsigned char* winflag = reinterpret_cast<unsigned char*>(ws + o.winflag);
            if (conv_in_gat || r.conv == CONV_WIN) bad = winflag;        // these two leave the windows' non-finite flags there
            if (r.conv == CONV_SHARED) {
                if ((rc = run_conv_shared(m, src, c0, n, hcat, ws + o.cf, ws + o.el, ws + o.er, s, vmax))) return rc;
            } else if (conv_in_gat) {
                if ((rc = ensure(m, m.conv_split, s))) return rc;
                cv = fused_conv_args(m, src, c0, hcat, vmax, winflag);
                temp.cv = &cv;
                HIP_TRY(hipMemsetAsync(vmax, 0, sizeof(unsigned), s));
            } else if ((rc = run_conv(m, r, src, c0, n, nullptr, nullptr, hcat, nullptr, s, vmax, winflag))) return rc;
            if (fork && !conv_in_gat) {                       // the feature layer on the second lane, beside the temporal one
                HIP_TRY(hipEventRecord(m.fork_ev[0], s));
                HIP_TRY(hipStreamWaitEvent(m.lane_stream, m.fork_ev[0], 0));
                if ((rc = run_gat_layer(m, m.feat, r.feat, feat, n, m.lane_stream))) return rc;
                HIP_TRY(hipEventRecord(m.fork_ev[1], m.lane_stream));
            }
            if ((rc = run_gat_layer(m, m.temp, r.temp, temp, n, s))) return rc;
            if (fork && !conv_in_gat) HIP_TRY(hipStreamWaitEvent(s, m.fork_ev[1], 0));
            else if ((rc = run_gat_layer(m, m.feat, r.feat, feat, n, s))) return rc;
        } else {
            const FrontRoute r = front_route(m, n, front_call(FRONT_FORWARD_UNFUSED, src, xc, m.Fp, F, hcat));
            if ((rc = run_conv(m, r, src, c0, n, xc, xct, hcat, nullptr, s))) return rc;
            temp.v = xc; temp.ldv = m.Fp;        // temporal layer: nodes = time steps, rows of xc
            feat.v = xct; feat.ldv = m.Wp; feat.vt = 0;      // feature layer: nodes = features, rows of xc^T
            if ((rc = run_gat_layer(m, m.temp, r.temp, temp, n, s))) return rc;
            if ((rc = run_gat_layer(m, m.feat, r.feat, feat, n, s))) return rc;
        }
        float* hend = ws + o.hend;
        const long ldh = m.gru.back().Hp;
        if ((rc = run_gru_stack(m, hcat, m.Dp, n, hend, ldh, ws, o, s,
                                both_fused ? reinterpret_cast<const unsigned*>(ws + o.vmax) : nullptr))) return rc;
        if (hend_out)
            K_TRY(launch_copy2d(hend, ldh, hend_out + c0 * m.cfg.gru_hid_dim, m.cfg.gru_hid_dim, n, m.cfg.gru_hid_dim, s),
                  "h_end copy");
        if (fork && preds && (recons || recons_last)) {
            // the forecasting head on the second lane, beside the reconstruction decoder (their scratch regions are disjoint)
            HIP_TRY(hipEventRecord(m.fork_ev[2], s));
            HIP_TRY(hipStreamWaitEvent(m.lane_stream, m.fork_ev[2], 0));
            float* pr = preds + c0 * m.cfg.out_dim;
            float* rc_ = recons ? recons + c0 * (int64_t)W * m.cfg.out_dim : nullptr;
            float* rl = recons_last ? recons_last + c0 * m.cfg.out_dim : nullptr;
            if ((rc = run_heads(m, hend, ldh, n, pr, nullptr, nullptr, ws, o, m.lane_stream))) return rc;
            if ((rc = run_poison(m, src, c0, n, bad, pr, nullptr, nullptr, m.lane_stream))) return rc;      // each lane behind its own head
            if ((rc = run_heads(m, hend, ldh, n, nullptr, rc_, rl, ws, o, s))) return rc;
            if ((rc = run_poison(m, src, c0, n, bad, nullptr, rc_, rl, s))) return rc;
        } else if (preds || recons || recons_last) {
            float* pr = preds ? preds + c0 * m.cfg.out_dim : nullptr;
            float* rc_ = recons ? recons + c0 * (int64_t)W * m.cfg.out_dim : nullptr;
            float* rl = recons_last ? recons_last + c0 * m.cfg.out_dim : nullptr;
            if ((rc = run_heads(m, hend, ldh, n, pr, rc_, rl, ws, o, s))) return rc;
            if ((rc = run_poison(m, src, c0, n, bad, pr, rc_, rl, s))) return rc;
        }
    }
    return 0;
}

int mtadgat_forward(mtadgat_handle h, const float* x, int64_t batch, float* preds, float* recons, float* hend_out,
                    void* ws_, size_t ws_bytes, void* stream) {
    XSource src;
    src.x = x;
    return forward_impl(h, src, batch, preds, recons, nullptr, hend_out, ws_, ws_bytes, stream);
}

int mtadgat_forward_xbf16(mtadgat_handle h, const void* x_bf16, int64_t batch, float* preds, float* recons, float* hend_out,
                          void* ws_, size_t ws_bytes, void* stream) {
    if (h && !conv_lds_staged(h->m.taps, std::max(h->m.Fp, h->m.Fp16)))
        return fail(MTADGAT_ERR_UNSUPPORTED, "bfloat16 input is read by the LDS-staged convolution only (n_features too large): pass float32");
    XSource src;
    src.x = static_cast<const float*>(x_bf16);
    src.x_bf16 = 1;
    return forward_impl(h, src, batch, preds, recons, nullptr, hend_out, ws_, ws_bytes, stream);
}

int mtadgat_forward_series(mtadgat_handle h, const float* series, int64_t n_rows, const int64_t* starts, int64_t start0,
                           int64_t stride, int64_t batch, float* preds, float* recons, float* recons_last, void* ws_,
                           size_t ws_bytes, void* stream) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    if (n_rows < h->m.W) return fail(MTADGAT_ERR_INVALID, "series shorter than one window");
    if (!starts) {   // starts_dev cannot be checked on the host; the arithmetic progression can
        if (stride < 0 || start0 < 0 || (batch > 0 && start0 + (batch - 1) * stride + h->m.W > n_rows))
            return fail(MTADGAT_ERR_INVALID, "windows start0 + w*stride .. +W do not lie inside the series");
    }
    XSource src;
    src.x = series; src.gather = 1; src.starts = starts; src.start0 = start0; src.stride = stride;
    return forward_impl(h, src, batch, preds, recons, recons_last, nullptr, ws_, ws_bytes, stream);
}

int mtadgat_conv(mtadgat_handle h, const float* x, int64_t batch, float* y, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_common(h, batch, ws, ws_bytes, false);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!x || !y) return fail(MTADGAT_ERR_INVALID, "null tensor");
    XSource src;
    src.x = x;
    const FrontRoute r = front_route(h->m, batch, front_call(FRONT_CONV, src, nullptr, 0, 0, nullptr));
    return run_conv(h->m, r, src, 0, batch, nullptr, nullptr, nullptr, y, (hipStream_t)stream);
}

int mtadgat_gat(mtadgat_handle h, int which, const float* xc_in, int64_t batch, float* out, void* ws_, size_t ws_bytes,
                void* stream) {
    int rc = check_common(h, batch, ws_, ws_bytes, true);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!xc_in || !out) return fail(MTADGAT_ERR_INVALID, "null tensor");
    if (which != 0 && which != 1) return fail(MTADGAT_ERR_INVALID, "which must be 0 (feature) or 1 (temporal)");
    Model& m = h->m;
    hipStream_t s = (hipStream_t)stream;
    float* ws = static_cast<float*>(ws_);
    const int F = m.F, W = m.W;
    Workspace o;
    plan_workspace(m, std::min<int64_t>(batch, m.chunk), o);
    for (int64_t c0 = 0; c0 < batch; c0 += m.chunk) {
        const int64_t n = std::min<int64_t>(m.chunk, batch - c0);
        const float* xin = xc_in + c0 * (int64_t)W * F;
        float* o_c = out + c0 * (int64_t)W * F;
        LayerIo io;
        io.out = o_c; io.so_w = (long)W * F; io.sc = ws + o.sc;
        if (which == 1) {
            K_TRY(launch_copy2d(xin, F, ws + o.xc, m.Fp, n * W, F, s), "pad copy");
            io.v = ws + o.xc; io.ldv = m.Fp; io.lc = ws + o.lct; io.rt = ws + o.rtt; io.so_i = F; io.so_d = 1;
        } else {
            K_TRY(launch_transpose_win(xin, F, ws + o.xct, m.Wp, n, W, F, s), "transpose");
            io.v = ws + o.xct; io.ldv = m.Wp; io.lc = ws + o.lcf; io.rt = ws + o.rtf; io.so_i = 1; io.so_d = F;
        }
        const FrontRoute r = front_route(m, n, front_call(FRONT_FORWARD_UNFUSED, XSource{}, io.v, io.ldv, which ? F : W, nullptr));
        if ((rc = run_gat_layer(m, which ? m.temp : m.feat, which ? r.temp : r.feat, io, n, s))) return rc;
    }
    return 0;
}

int mtadgat_gru(mtadgat_handle h, const float* hcat, int64_t batch, float* hend, void* ws_, size_t ws_bytes, void* stream) {
    int rc = check_common(h, batch, ws_, ws_bytes, true);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!hcat || !hend) return fail(MTADGAT_ERR_INVALID, "null tensor");
    Model& m = h->m;
    float* ws = static_cast<float*>(ws_);
    const int D = 3 * m.F, H = m.cfg.gru_hid_dim;
    Workspace o;
    plan_workspace(m, std::min<int64_t>(batch, m.chunk), o);
    for (int64_t c0 = 0; c0 < batch; c0 += m.chunk) {
        const int64_t n = std::min<int64_t>(m.chunk, batch - c0);
        // the kernel wants 16-byte aligned, zero padded rows: stage the caller's (b, W, 3F) tensor into the padded buffer
        hipStream_t s = (hipStream_t)stream;
        HIP_TRY(hipMemsetAsync(ws + o.hcat, 0, (size_t)n * m.W * m.Dp * sizeof(float), s));
        K_TRY(launch_copy2d(hcat + c0 * (int64_t)m.W * D, D, ws + o.hcat, m.Dp, n * m.W, D, s), "h_cat pad copy");
        if ((rc = run_gru_stack(m, ws + o.hcat, m.Dp, n, hend + c0 * H, H, ws, o, s))) return rc;
    }
    return 0;
}

int mtadgat_heads(mtadgat_handle h, const float* hend, int64_t batch, float* preds, float* recons, void* ws_, size_t ws_bytes,
                  void* stream) {
    int rc = check_common(h, batch, ws_, ws_bytes, true);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!hend) return fail(MTADGAT_ERR_INVALID, "null tensor");
    Model& m = h->m;
    float* ws = static_cast<float*>(ws_);
    const int H = m.cfg.gru_hid_dim;
    Workspace o;
    plan_workspace(m, std::min<int64_t>(batch, m.chunk), o);
    for (int64_t c0 = 0; c0 < batch; c0 += m.chunk) {
        const int64_t n = std::min<int64_t>(m.chunk, batch - c0);
        hipStream_t s = (hipStream_t)stream;
        const long ldh = m.gru.back().Hp;
        HIP_TRY(hipMemsetAsync(ws + o.hend, 0, (size_t)n * ldh * sizeof(float), s));
        K_TRY(launch_copy2d(hend + c0 * H, H, ws + o.hend, ldh, n, H, s), "h_end pad copy");
        if ((rc = run_heads(m, ws + o.hend, ldh, n, preds ? preds + c0 * m.cfg.out_dim : nullptr,
                            recons ? recons + c0 * (int64_t)m.W * m.cfg.out_dim : nullptr, nullptr, ws, o, s)))
            return rc;
    }
    return 0;
}

// ---- attention maps (the post-softmax `attention` of modules.py:85-89 / :184-188, eval mode; scratch: plan_attention) ------------
// The maps come from the fp32 builds the training forward keeps its softmax rows with (k_gat / k_gat_wide / k_attend, no
// dropout), whatever precision mode the handle is in (front_route, FRONT_ATTENTION); profiling is off for the call and restored.
static int attention_impl(mtadgat_handle h, const XSource& src, int64_t batch, bool reduce, float* att_f, float* att_t, void* ws_,
                          size_t ws_bytes, void* stream) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    if (batch < 1) return fail(MTADGAT_ERR_INVALID, "attention maps need at least one window");
    if (!h->m.have_weights) return fail(MTADGAT_ERR_NOWEIGHTS, "mtadgat_load_weights has not been called");
    if (!src.x) return fail(MTADGAT_ERR_INVALID, "input is NULL");
    if (!att_f && !att_t) return fail(MTADGAT_ERR_INVALID, "both attention outputs are NULL");
    if (!ws_) return fail(MTADGAT_ERR_WORKSPACE, "workspace is NULL");
    if (!aligned16(ws_)) return fail(MTADGAT_ERR_WORKSPACE, "workspace must be 16-byte aligned");
    Model& m = h->m;
    AttPlan p;
    plan_attention(m, batch, reduce, p);
    if (ws_bytes < p.total * sizeof(float)) return fail(MTADGAT_ERR_WORKSPACE, "workspace too small");
    struct Restore {
        Model& m; bool profile;
        ~Restore() { m.profile = profile; }
    } restore{m, m.profile};
    m.profile = false;
    hipStream_t s = (hipStream_t)stream;
    float* ws = static_cast<float*>(ws_);
    const int F = m.F, W = m.W;
    float* hcat = ws + p.hcat;
    int rc;
    for (int64_t c0 = 0; c0 < batch; c0 += p.chunk) {
        const int64_t n = std::min<int64_t>(p.chunk, batch - c0);
        const FrontRoute r = front_route(m, n, front_call(FRONT_ATTENTION, src, hcat, m.Dp, F, hcat));
        if ((rc = run_conv(m, r, src, c0, n, nullptr, (att_f && !r.feat.fused()) ? ws + p.xct : nullptr, hcat, nullptr, s))) return rc;
        // temporal layer: nodes = time steps, rows of h_cat[:, :F]
        if (att_t) {
            LayerIo io = hcat_layer(m, true, true, hcat, nullptr, ws + p.lct, ws + p.rtt);
            io.att = reduce ? ws + p.maps : att_t + c0 * (int64_t)W * W;
            if ((rc = run_gat_layer(m, m.temp, r.temp, io, n, s))) return rc;
            if (reduce) K_TRY(launch_att_mean_part(io.att, n, W, p.slabs_t, c0 == 0, ws + p.ps_t, ws + p.pc_t, s), "attention mean (temporal)");
        }
        // feature layer: nodes = features, columns of h_cat[:, :F] (fused) or rows of x_c^T
        if (att_f) {
            LayerIo io = hcat_layer(m, false, r.feat.fused(), hcat, ws + p.xct, ws + p.lcf, ws + p.rtf);
            io.att = reduce ? ws + p.maps : att_f + c0 * (int64_t)F * F;
            if ((rc = run_gat_layer(m, m.feat, r.feat, io, n, s))) return rc;
            if (reduce) K_TRY(launch_att_mean_part(io.att, n, F, p.slabs_f, c0 == 0, ws + p.ps_f, ws + p.pc_f, s), "attention mean (feature)");
        }
    }
    if (reduce && att_t) K_TRY(launch_att_mean_final(ws + p.ps_t, ws + p.pc_t, W, p.slabs_t, batch, att_t, s), "attention mean (temporal)");
    if (reduce && att_f) K_TRY(launch_att_mean_final(ws + p.ps_f, ws + p.pc_f, F, p.slabs_f, batch, att_f, s), "attention mean (feature)");
    return 0;
}

static int attention_series(mtadgat_handle h, const float* series, int64_t n_rows, const int64_t* starts, int64_t start0,
                            int64_t stride, int64_t batch, bool reduce, float* att_f, float* att_t, void* ws, size_t ws_bytes,
                            void* stream) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    if (n_rows < h->m.W) return fail(MTADGAT_ERR_INVALID, "series shorter than one window");
    if (!starts && (stride < 0 || start0 < 0 || (batch > 0 && start0 + (batch - 1) * stride + h->m.W > n_rows)))
        return fail(MTADGAT_ERR_INVALID, "windows start0 + w*stride .. +W do not lie inside the series");
    XSource src;
    src.x = series; src.gather = 1; src.starts = starts; src.start0 = start0; src.stride = stride;
    return attention_impl(h, src, batch, reduce, att_f, att_t, ws, ws_bytes, stream);
}

size_t mtadgat_attention_workspace_bytes(mtadgat_handle h, int64_t batch, int reduce) {
    if (!h || batch <= 0) return 0;
    AttPlan p;
    plan_attention(h->m, batch, reduce != 0, p);
    return p.total * sizeof(float);
}

int mtadgat_attention(mtadgat_handle h, const float* x, int64_t batch, float* att_feat, float* att_temp, void* ws, size_t ws_bytes,
                      void* stream) {
    XSource src;
    src.x = x;
    return attention_impl(h, src, batch, false, att_feat, att_temp, ws, ws_bytes, stream);
}

int mtadgat_attention_mean(mtadgat_handle h, const float* x, int64_t batch, float* mean_feat, float* mean_temp, void* ws,
                           size_t ws_bytes, void* stream) {
    XSource src;
    src.x = x;
    return attention_impl(h, src, batch, true, mean_feat, mean_temp, ws, ws_bytes, stream);
}

int mtadgat_attention_series(mtadgat_handle h, const float* series, int64_t n_rows, const int64_t* starts, int64_t start0,
                             int64_t stride, int64_t batch, float* att_feat, float* att_temp, void* ws, size_t ws_bytes,
                             void* stream) {
    return attention_series(h, series, n_rows, starts, start0, stride, batch, false, att_feat, att_temp, ws, ws_bytes, stream);
}

int mtadgat_attention_series_mean(mtadgat_handle h, const float* series, int64_t n_rows, const int64_t* starts, int64_t start0,
                                  int64_t stride, int64_t batch, float* mean_feat, float* mean_temp, void* ws, size_t ws_bytes,
                                  void* stream) {
    return attention_series(h, series, n_rows, starts, start0, stride, batch, true, mean_feat, mean_temp, ws, ws_bytes, stream);
}

// ---- forecast / reconstruction errors of a series (Trainer.evaluate, training.py:188-228; scratch: plan_losses) -------------------
// Chunk by chunk: the forward of that chunk's windows alone into the workspace, then mtadgat_eval_window_sse over them.
int64_t mtadgat_series_losses_chunk(mtadgat_handle h) {
    if (!h) return 0;
    LossPlan p;
    plan_losses(h->m, 1, p);
    return p.chunk;
}

size_t mtadgat_series_losses_workspace_bytes(mtadgat_handle h, int64_t batch) {
    if (!h || batch <= 0) return 0;
    LossPlan p;
    plan_losses(h->m, batch, p);
    return p.total * sizeof(float);
}

// age == nullptr: mtadgat_series_losses (two entries per window, two kinds per dimension); else the masked call (four)
static int series_losses_impl(mtadgat_handle h, const float* series, int64_t n_rows, const int64_t* starts, int64_t start0, int64_t stride,
                              int64_t batch, const int32_t* dims, const int32_t* age, int64_t ld_age, int32_t max_age, double* window_out,
                              double* dim_out, void* ws_, size_t ws_bytes, void* stream) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    if (batch < 1 || batch > 2147483647LL) return fail(MTADGAT_ERR_INVALID, "series losses need between 1 and 2^31 - 1 windows");
    if (!h->m.have_weights) return fail(MTADGAT_ERR_NOWEIGHTS, "mtadgat_load_weights has not been called");
    if (!series || !window_out) return fail(MTADGAT_ERR_INVALID, "null tensor");
    Model& m = h->m;
    const int W = m.W, od = m.cfg.out_dim;
    if (n_rows < (int64_t)W + 1) return fail(MTADGAT_ERR_INVALID, "series shorter than one window and its target row");
    if (!dims && od > m.F) return fail(MTADGAT_ERR_INVALID, "out_dim > n_features needs dims_dev");
    if (age && ld_age < m.F) return fail(MTADGAT_ERR_INVALID, "ld_age < n_features");
    if (!starts && (stride < 0 || start0 < 0 || start0 + W > n_rows - 1 || (stride > 0 && batch - 1 > (n_rows - 1 - W - start0) / stride)))
        return fail(MTADGAT_ERR_INVALID, "windows start0 + w*stride .. +W and their target rows do not lie inside the series");
    if (!ws_) return fail(MTADGAT_ERR_WORKSPACE, "workspace is NULL");
    if (!aligned16(ws_)) return fail(MTADGAT_ERR_WORKSPACE, "workspace must be 16-byte aligned");
    LossPlan p;
    plan_losses(m, batch, p, age != nullptr);
    if (ws_bytes < p.total * sizeof(float)) return fail(MTADGAT_ERR_WORKSPACE, "workspace too small");
    float* ws = static_cast<float*>(ws_);
    for (int64_t c0 = 0; c0 < batch; c0 += p.chunk) {
        const int64_t n = std::min<int64_t>(p.chunk, batch - c0);
        XSource src;
        src.x = series; src.gather = 1; src.stride = stride;
        src.starts = starts ? starts + c0 : nullptr;
        src.start0 = start0 + c0 * stride;
        int rc = forward_impl(h, src, n, ws + p.preds, ws + p.recons, nullptr, nullptr, ws, p.fwd_floats * sizeof(float), stream);
        if (rc) return rc;
        if (age)
            rc = mtadgat_fit_masked_sse(ws + p.preds, ws + p.recons, n, W, od, series, n_rows, m.F, m.F, src.starts, src.start0, stride, dims,
                                        age, ld_age, max_age, c0 > 0, window_out + 4 * c0, dim_out, ws + p.scratch, p.scratch_bytes, stream);
        else
            rc = mtadgat_eval_window_sse(ws + p.preds, ws + p.recons, n, W, od, series, n_rows, m.F, m.F, src.starts, src.start0, stride, dims,
                                         c0 > 0, window_out + 2 * c0, dim_out, ws + p.scratch, p.scratch_bytes, stream);
        if (rc) return rc;
    }
    return 0;
}

int mtadgat_series_losses(mtadgat_handle h, const float* series, int64_t n_rows, const int64_t* starts, int64_t start0, int64_t stride,
                          int64_t batch, const int32_t* dims, double* window_sse, double* dim_sse, void* ws_, size_t ws_bytes,
                          void* stream) {
    return series_losses_impl(h, series, n_rows, starts, start0, stride, batch, dims, nullptr, 0, 0, window_sse, dim_sse, ws_, ws_bytes, stream);
}

size_t mtadgat_series_losses_masked_workspace_bytes(mtadgat_handle h, int64_t batch) {
    if (!h || batch <= 0) return 0;
    LossPlan p;
    plan_losses(h->m, batch, p, true);
    return p.total * sizeof(float);
}

int mtadgat_series_losses_masked(mtadgat_handle h, const float* series, int64_t n_rows, const int64_t* starts, int64_t start0,
                                 int64_t stride, int64_t batch, const int32_t* dims, const int32_t* age, int64_t ld_age, int32_t max_age,
                                 double* window_out, double* dim_out, void* ws_, size_t ws_bytes, void* stream) {
    if (!age) return fail(MTADGAT_ERR_INVALID, "null tensor");
    return series_losses_impl(h, series, n_rows, starts, start0, stride, batch, dims, age, ld_age, max_age, window_out, dim_out, ws_, ws_bytes,
                              stream);
}

int mtadgat_profile_enable(mtadgat_handle h, int on) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    h->m.profile = on != 0;
    return 0;
}

int mtadgat_profile_read(mtadgat_handle h, double ms[MTADGAT_PROFILE_SLOTS], int64_t launches[MTADGAT_PROFILE_SLOTS]) {
    if (!h || !ms || !launches) return fail(MTADGAT_ERR_INVALID, "null argument");
    for (int i = 0; i < MTADGAT_PROFILE_SLOTS; ++i) {
        ms[i] = 0.0;
        launches[i] = 0;
        for (auto& p : h->m.ev[i]) {
            HIP_TRY(hipEventSynchronize(p.second));
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, p.first, p.second));
            ms[i] += t;
            launches[i] += 1;
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        h->m.ev[i].clear();
    }
    return 0;
}

const char* mtadgat_profile_name(int slot) {
    return (slot >= 0 && slot < MTADGAT_PROFILE_SLOTS) ? kSlotNames[slot] : "";
}

}  // extern "C"

// =====================================================================================================
// training step: forward that keeps the activations ("tape") + backward  (reference training.py:106-127)
// =====================================================================================================
namespace {

DropArgs make_drop(float p, uint64_t seed, int64_t win0) {
    DropArgs d{};
    if (p > 0.f) {
        double t = (double)p * 4294967296.0;
        d.thresh = t >= 4294967295.0 ? 4294967295u : (unsigned)t;
        if (d.thresh == 0) d.thresh = 1;
        d.keep_scale = 1.0f / (1.0f - p);
    } else {
        d.thresh = 0;
        d.keep_scale = 1.0f;
    }
    d.seed_lo = (unsigned)(seed & 0xffffffffu);
    d.seed_hi = (unsigned)(seed >> 32);
    d.win0 = win0;
    return d;
}

int check_train(mtadgat_handle h, int64_t batch, float p) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    if (batch < 0) return fail(MTADGAT_ERR_INVALID, "negative batch");
    if (!h->m.have_weights) return fail(MTADGAT_ERR_NOWEIGHTS, "mtadgat_load_weights has not been called");
    if (!h->m.bw.supported) return fail(MTADGAT_ERR_UNSUPPORTED, "no HIP backward for this configuration: " + h->m.bw.why);
    if (!(p >= 0.f && p < 1.f)) return fail(MTADGAT_ERR_INVALID, "dropout probability must be in [0, 1)");
    if (h->m.precision == 1)
        return fail(MTADGAT_ERR_UNSUPPORTED, "the training step computes in fp32 (mtadgat_set_precision 0 or 2): the bf16-operand recurrences of "
                                             "rounds 2-5 were slower than it at every batch size and are gone");
    return 0;
}

// d X = d Y W through k_rowgemm with the transposed pack
int run_rowgemm_T(Model& m, const LinTPlan& p, const float* X, long ldx, long R, float* Y, long ldy, int nvalid, bool accumulate,
                  const float* gate, long ldg, float gate_scale, hipStream_t s) {
    RowGemmArgs a{};
    a.X = X; a.ldx = ldx; a.Kvalid = p.in_dim; a.Q = p.Q;
    a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + p.w_off);
    a.bias = m.packed_dev + m.bw.zero_off;
    a.Y = Y; a.ldy = ldy; a.Nvalid = nvalid;
    a.vec_store = ((ldy & 3) == 0 && aligned16(Y)) ? 1 : 0;
    a.R = R; a.NT = p.NT; a.NT_rm = p.NT; a.group = 1; a.relu = 0;
    a.accumulate = accumulate ? 1 : 0;
    a.gate = gate; a.ldg = ldg; a.gate_scale = gate_scale;
    if (rowgemm_split(m, p.w3_off != 0, R, true)) {
        if (int rc_ = ensure(m, p.split, s)) return rc_;
        a.x3 = 1; a.Q16 = p.Q16;
        a.Wp3 = reinterpret_cast<const f32x4*>(m.packed_dev + p.w3_off);
    }
    K_TRY(launch_rowgemm(a, s), "data-gradient rowgemm");
    return 0;
}

// the un-scaled projections [L | R] = V [W_l ; W_r]^T + [b | 0] of the node rows (GATv2 score backward): one row GEMM over the backward
// plan's pack, on three bf16 pieces per operand from 65 536 rows (as the data-gradient GEMMs; the pack is split on first use after an upload)
int run_bwd_projection(Model& m, const GatPlan& gp, const GatBwdPlan& gb, const float* Vn, long ldv, long rows, float* LR, hipStream_t s) {
    RowGemmArgs r{};
    r.X = Vn; r.ldx = ldv; r.Kvalid = gp.D; r.Q = gp.Q;
    r.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + gb.wu_off);
    r.bias = m.packed_dev + gb.bu_off;
    r.Y = LR; r.ldy = 2L * gb.Ep; r.Nvalid = 2 * gb.Ep; r.vec_store = 1;
    r.R = rows; r.NT = 2 * gb.NTu; r.NT_rm = 2 * gb.NTu; r.group = 1; r.relu = 0;
    if (rowgemm_split(m, gb.wu3_off != 0, rows, true)) {
        if (int rc_ = ensure(m, gb.split, s)) return rc_;
        r.x3 = 1; r.Q16 = (gp.Q + 1) / 2;
        r.Wp3 = reinterpret_cast<const f32x4*>(m.packed_dev + gb.wu3_off);
    }
    K_TRY(launch_rowgemm(r, s), "attention backward (projection)");
    return 0;
}

struct WgradIn {
    const float* A = nullptr; long lda = 0;
    const float* B = nullptr; long ldb = 0; int bmode = 0; int bshift = 0;
    long R = 0; int T = 1;
};
// The weight-gradient GEMMs of a backward leave their slab partials in consecutive regions of `base`; the reductions into the flat
// gradient buffer are queued and run as ONE launch (flush) -- at the end of the backward, or earlier when the region is full.
struct WgradQueue {
    float* base = nullptr;
    size_t cap = 0, used = 0;
    WgradReduceArgs pend[WGRAD_BATCH_MAX];
    int n = 0;
    hipStream_t s = nullptr;
    int flush() {
        if (n == 0) return 0;
        K_TRY(launch_wgrad_reduce_batch(pend, n, s), "weight-gradient reductions");
        n = 0; used = 0;
        return 0;
    }
};
int run_wgrad(Model& m, const WgradPlan& p, const WgradIn& in, WgradQueue& wq, float* outW, float* outB, hipStream_t s) {
    const WgradSlabPlan sp = wgrad_slab_plan(m, in.R, p.Mp, p.Np);
    const int nslab = sp.nslab;
    const size_t need_ = ((size_t)nslab * p.Mp * p.Np + 63) & ~(size_t)63;
    if (need_ > wq.cap) return fail(MTADGAT_ERR_WORKSPACE, "internal: weight-gradient partial region too small");
    if (wq.used + need_ > wq.cap || wq.n == WGRAD_BATCH_MAX)
        if (int rc_ = wq.flush()) return rc_;
    float* wpart = wq.base + wq.used;
    wq.used += need_;
    WgradArgs a{};
    a.A = in.A; a.lda = in.lda; a.M = p.M;
    a.B = in.B; a.ldb = in.ldb; a.N = p.N; a.bmode = in.bmode; a.bshift = in.bshift;
    a.T = in.T; a.F = m.F; a.taps = m.taps; a.pad = m.pad;
    a.R = in.R;
    a.nslab = nslab;
    a.rows_per_slab = sp.rows_per_slab;
    a.P = wpart; a.Mp = p.Mp; a.Np = p.Np;
    a.x3 = sp.x3;
    K_TRY(launch_wgrad(a, s), "weight-gradient GEMM");
    WgradReduceArgs r{};
    r.P = wpart; r.nslab = a.nslab; r.Mp = p.Mp; r.Np = p.Np; r.M = p.M; r.N = p.N;
    r.rowmapW = reinterpret_cast<const int*>(m.packed_dev + p.rowW_off);
    r.colmap = reinterpret_cast<const int*>(m.packed_dev + p.col_off);
    r.rowmapB = p.has_bias && outB ? reinterpret_cast<const int*>(m.packed_dev + p.rowB_off) : nullptr;
    r.outW = outW; r.outB = outB;
    wq.pend[wq.n++] = r;
    return 0;
}
// column sums over the windows (d bias / d a of a GATv2 layer): the first stage now, the reduction in the step's batched launch
int run_sum_rows_queued(const float* src, long ld, long R, int N, float* scratch, float* dst, WgradQueue& wq, hipStream_t s) {
    if (wq.n == WGRAD_BATCH_MAX)
        if (int rc_ = wq.flush()) return rc_;
    int nslab = 0;
    K_TRY(launch_sum_rows_part(src, ld, R, N, scratch, &nslab, s), "column sums");
    if (nslab == 0) return 0;
    WgradReduceArgs r{};
    r.P = scratch; r.nslab = nslab; r.Mp = 1; r.Np = N; r.M = 1; r.N = N;
    r.outW = dst;
    wq.pend[wq.n++] = r;
    return 0;
}

// The training forward of one recurrence stack (modules.py:235-238 / :276-283): every layer keeps its gates and states; between
// stacked layers nn.GRU's dropout (training only; modules.py:232-233 / :253) -- the dropped sequence is what the next layer reads
// and is kept as well.  What the two stacks differ in:
struct StackFwd {
    int slot; const char* name; unsigned drop0;     // profile slot, "gru" / "decoder", dropout stream of layer 0's states
    const float* x; long ldx; int kx;               // what layer 0 reads
    float* xp = nullptr;                            // layer 0: room for hoisted input products (the small-batch kernels need it) ...
    const unsigned* vmax = nullptr;                 // ... and the convolution's recorded range
    float* hend = nullptr;                          // the top layer's last states
    const LinPlan* fc = nullptr;                    // a per-step Linear on the top layer's states into yfc: inside its recurrence
    bool rides = false;                             // (rides), otherwise a row GEMM over the kept states
    float* yfc = nullptr;
};
int walk_stack_forward(Model& m, const std::vector<GruPlan>& stack, const std::vector<TapeLayer>& tl, float* T, StackFwd f,
                       const DropArgs& drop, int64_t n, hipStream_t s) {
    const int L = (int)stack.size();
    const std::string drop_what = std::string(f.name) + " inter-layer dropout";
    for (int l = 0; l < L; ++l) {
        const GruPlan& g = stack[l];
        const bool top = l == L - 1;
        float* seq = T + tl[l].seq;
        GruIo io;
        io.x = f.x; io.ldx = f.ldx; io.kx = f.kx; io.seq = seq; io.gates = T + tl[l].gates;
        io.hend = top ? f.hend : nullptr; io.ldhe = f.hend ? g.Hp : 0;
        if (l == 0) { io.xp = f.xp; io.vmax = f.vmax; }
        if (top && f.rides) { io.fc = f.fc; io.yfc = f.yfc; }
        if (int rc = run_gru_layer(m, f.slot, stack, l, io, n, s)) return rc;
        if (!top) {
            float* dr = T + tl[l].drop;
            K_TRY(launch_seq_dropout(seq, dr, n, m.W, g.H, g.Hp, drop, f.drop0 + (unsigned)l, s), drop_what.c_str());
            f.x = dr; f.ldx = g.Hp; f.kx = g.H;
        } else if (f.fc && !f.rides) {
            Scope sc(m, f.slot, s);
            K_TRY(launch_rowgemm(lin_rows(m, *f.fc, seq, g.Hp, n * (int64_t)m.W, f.yfc), s), "reconstruction Linear (training)");
        }
    }
    return 0;
}

// What the steps of one backward call share.  grads == nullptr: the data path only.
struct BwdCall {
    Model& m; const float* T; int64_t n; const DropArgs& drop; float* grads; WgradQueue& wq;
    float* da;        // gate gradients of every step of the layer at hand
    float* dhdec;     // gradient of every state of the layer below it
    hipStream_t s;
};
// The backward of one recurrence stack from the top layer down.  Per layer: BPTT with the kernel gru_bwd_route names (gate
// gradients of every step into `da`), the layer's weight gradients, and d (rows the layer read) = d a W_ih -- above layer 0 into
// dhdec and through the dropout's adjoint: the gradient of the states of the layer below.  What the two stacks differ in:
struct StackBwd {
    bool decoder; const char* name; unsigned drop0;
    const float* x0; float* d0; long ld0;           // layer 0: the rows it read, where their gradient goes, the row stride of both
    const float* dh_seq; const float* dh_end;       // top layer: gradient of every state / of the last state only (nullptr: none)
};
int walk_stack_backward(const BwdCall& c, const std::vector<TapeLayer>& tl, const StackBwd& sb) {
    Model& m = c.m;
    const std::vector<GruPlan>& stack = sb.decoder ? m.rec : m.gru;
    const std::vector<GruBwdPlan>& plans = sb.decoder ? m.bw.rec : m.bw.gru;
    const GradLayout& gl = m.bw.gl;
    const std::vector<int64_t>&o_wih = sb.decoder ? gl.rec_wih : gl.gru_wih, &o_whh = sb.decoder ? gl.rec_whh : gl.gru_whh,
                              &o_bih = sb.decoder ? gl.rec_bih : gl.gru_bih, &o_bhh = sb.decoder ? gl.rec_bhh : gl.gru_bhh;
    const int W = m.W, L = (int)stack.size();
    const int64_t n = c.n;
    const long RW = (long)n * W;
    const std::string what = std::string(sb.name) + " backward", drop_what = std::string(sb.name) + " inter-layer dropout (adjoint)";
    hipStream_t s = c.s;
    float* da = c.da;
    for (int l = L - 1; l >= 0; --l) {
        const GruPlan& q = stack[l];
        const GruBwdPlan& qb = plans[l];
        const bool top = l == L - 1;
        const float* gates = c.T + tl[l].gates;
        const float* seq = c.T + tl[l].seq;
        const float* xin = l == 0 ? sb.x0 : c.T + tl[l - 1].drop;
        const long ldxin = l == 0 ? sb.ld0 : stack[l - 1].Hp;
        const float* dhseq = top ? sb.dh_seq : c.dhdec;
        const float* dhend = top ? sb.dh_end : nullptr;
        const GruBwdRoute r = gru_bwd_route(m, sb.decoder, l, n);
        if (r.kernel != GRU_BWD_SPLIT) {
            Gru16BwdArgs ga{};
            ga.Gates = gates; ga.Seq = seq; ga.DHseq = dhseq; ga.lddh = q.Hp; ga.DHend = dhend; ga.ldde = q.Hp;
            ga.W16T = m.packed_dev + (r.kernel == GRU_BWD_WINDOW ? q.g1T_off : q.g16T_off);
            ga.DA = da; ga.Hp = q.Hp; ga.KS = q.KS16; ga.NT16 = q.NT16; ga.T = W; ga.B = n; ga.H = q.H;
            if (r.kernel == GRU_BWD_WINDOW) K_TRY(launch_gru1_bwd(ga, s), what.c_str());
            else K_TRY(launch_gru16_bwd(ga, s), what.c_str());
        } else {
            GruBwdArgs ga{};
            ga.Gates = gates; ga.Seq = seq; ga.DHseq = dhseq; ga.lddh = q.Hp; ga.DHend = dhend; ga.ldde = q.Hp;
            if (r.split_pack)
                if (int rc_ = ensure(m, qb.split, s)) return rc_;
            ga.WhT = reinterpret_cast<const f32x4*>(m.packed_dev + (r.x3 ? qb.whT3_off : qb.whT_off));
            ga.x3 = r.x3 ? 1 : 0;
            ga.DA = da; ga.Hp = q.Hp; ga.H = q.H; ga.T = W; ga.NCG = q.NCG; ga.B = n;
            K_TRY(launch_gru_bwd(ga, s), what.c_str());
        }
        if (c.grads) {
            WgradIn hh;
            hh.A = da + q.Hp; hh.lda = 4L * q.Hp; hh.bshift = 1; hh.B = seq; hh.ldb = q.Hp; hh.R = RW; hh.T = W;
            if (int rc = run_wgrad(m, qb.wg_hh, hh, c.wq, c.grads + o_whh[l], c.grads + o_bhh[l], s)) return rc;
            WgradIn ih;
            ih.A = da; ih.lda = 4L * q.Hp; ih.B = xin; ih.ldb = ldxin; ih.R = RW; ih.T = W;
            if (int rc = run_wgrad(m, qb.wg_ih, ih, c.wq, c.grads + o_wih[l], c.grads + o_bih[l], s)) return rc;
        }
        if (l > 0) {
            const GruPlan& lo = stack[l - 1];
            if (int rc = run_rowgemm_T(m, qb.wihT, da, 4L * q.Hp, RW, c.dhdec, lo.Hp, lo.Hp, false, nullptr, 0, 1.f, s)) return rc;
            K_TRY(launch_seq_dropout(c.dhdec, c.dhdec, n, W, lo.H, lo.Hp, c.drop, sb.drop0 + (unsigned)(l - 1), s), drop_what.c_str());
        } else if (int rc = run_rowgemm_T(m, qb.wihT, da, 4L * q.Hp, RW, sb.d0, sb.ld0, (int)sb.ld0, false, nullptr, 0, 1.f, s))
            return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

int mtadgat_backward_supported(mtadgat_handle h) {
    if (!h) return 0;
    if (!h->m.bw.supported) g_err = "no HIP backward for this configuration: " + h->m.bw.why;
    return h->m.bw.supported ? 1 : 0;
}

size_t mtadgat_tape_bytes(mtadgat_handle h, int64_t batch) {
    if (!h || batch <= 0 || !h->m.bw.supported) return 0;
    Tape t;
    plan_tape(h->m, batch, t);
    return t.total * sizeof(float);
}

size_t mtadgat_backward_workspace_bytes(mtadgat_handle h, int64_t batch) {
    if (!h || batch <= 0 || !h->m.bw.supported) return 0;
    BwdWorkspace w;
    plan_bwd_workspace(h->m, batch, w);
    return w.total * sizeof(float);
}

int64_t mtadgat_grad_floats(mtadgat_handle h) { return h ? h->m.bw.gl.total : 0; }

int mtadgat_grad_offsets(mtadgat_handle h, int64_t* out, int max_n) {
    if (!h || !out) return fail(MTADGAT_ERR_INVALID, "null argument");
    const GradLayout& g = h->m.bw.gl;
    std::vector<int64_t> v = {g.conv_w, g.conv_b, g.lin_w[0], g.lin_b[0], g.a[0], g.bias[0], g.lin_w[1], g.lin_b[1], g.a[1], g.bias[1]};
    for (size_t l = 0; l < g.gru_wih.size(); ++l) v.insert(v.end(), {g.gru_wih[l], g.gru_whh[l], g.gru_bih[l], g.gru_bhh[l]});
    for (size_t i = 0; i < g.fc_w.size(); ++i) { v.push_back(g.fc_w[i]); v.push_back(g.fc_b[i]); }
    for (size_t l = 0; l < g.rec_wih.size(); ++l) v.insert(v.end(), {g.rec_wih[l], g.rec_whh[l], g.rec_bih[l], g.rec_bhh[l]});
    v.insert(v.end(), {g.rec_fc_w, g.rec_fc_b});
    if ((int)v.size() > max_n) return fail(MTADGAT_ERR_INVALID, "offset array too small");
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    return (int)v.size();
}

int mtadgat_train_layout(mtadgat_handle h, int64_t batch, int64_t* out, int max_n) {
    if (!h || !out || batch <= 0 || !h->m.bw.supported) return fail(MTADGAT_ERR_INVALID, "bad argument");
    Tape t;
    plan_tape(h->m, batch, t);
    BwdWorkspace w;
    plan_bwd_workspace(h->m, batch, w);
    std::vector<int64_t> v = {(int64_t)t.hcat, (int64_t)t.xct, (int64_t)t.att_f, (int64_t)t.att_t, (int64_t)t.hend, (int64_t)t.gru[0].gates,
                              (int64_t)t.gru[0].seq, (int64_t)t.rec[0].gates, (int64_t)t.rec[0].seq, (int64_t)t.xdec,
                              (int64_t)w.da, (int64_t)w.dhcat, (int64_t)w.dhdec, (int64_t)w.dhend, (int64_t)w.dz0, (int64_t)w.dz1,
                              (int64_t)w.de_f, (int64_t)w.de_t, (int64_t)w.dv_f, (int64_t)w.dv_t, (int64_t)w.dlr_f, (int64_t)w.dlr_t,
                              (int64_t)w.dap_f, (int64_t)w.dap_t, (int64_t)w.dpre};
    if ((int)v.size() > max_n) return fail(MTADGAT_ERR_INVALID, "layout array too small");
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    return (int)v.size();
}

int mtadgat_forward_train(mtadgat_handle h, const float* x, int64_t batch, int64_t window0, float dropout_p, uint64_t seed,
                          float* preds, float* recons, void* tape_, size_t tape_bytes, void* stream) {
    int rc = check_train(h, batch, dropout_p);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!x || !preds || !recons || !tape_) return fail(MTADGAT_ERR_INVALID, "null tensor");
    Model& m = h->m;
    Tape t;
    plan_tape(m, batch, t);
    if (!aligned16(tape_) || tape_bytes < t.total * sizeof(float)) return fail(MTADGAT_ERR_WORKSPACE, "tape too small or misaligned");
    hipStream_t s = (hipStream_t)stream;
    float* T = static_cast<float*>(tape_);
    const int F = m.F, W = m.W;
    const int64_t n = batch;
    const DropArgs drop = make_drop(dropout_p, seed, window0);
    float* hcat = T + t.hcat;
    XSource src;
    src.x = x;
    unsigned* vmax = reinterpret_cast<unsigned*>(T + t.vmax);
    const FrontRoute fr = front_route(m, n, front_call(FRONT_TRAIN, src, hcat, m.Dp, F, hcat));
    if ((rc = run_conv(m, fr, src, 0, n, nullptr, T + t.xct, hcat, nullptr, s, vmax))) return rc;
    // the two attention layers: fused per-window kernels, or -- wide layers -- projection through memory + k_gat_wide; either way
    // the softmax rows are kept and the dropout of modules.py:90 / :189 is applied inside the kernel
    LayerIo temp = hcat_layer(m, true, true, hcat, nullptr, T + t.lct, T + t.rtt), feat = hcat_layer(m, false, fr.feat.fused(), hcat, T + t.xct, T + t.lcf, T + t.rtf);
    temp.att = T + t.att_t; temp.drop = &drop; temp.drop_stream = DROP_TEMP; temp.vmax = vmax;
    feat.att = T + t.att_f; feat.drop = &drop; feat.drop_stream = DROP_FEAT; feat.vmax = vmax;
    if ((rc = run_gat_layer(m, m.temp, fr.temp, temp, n, s))) return rc;
    if ((rc = run_gat_layer(m, m.feat, fr.feat, feat, n, s))) return rc;
    // GRU stack (modules.py:235-238): layer 0 behind the convolution's recorded range, the top layer produces h_end
    const GruPlan& g = m.gru.back();
    float* hend = T + t.hend;
    StackFwd gs{S_GRU, "gru", DROP_GRU0, hcat, m.Dp, 3 * F};
    gs.xp = T + t.xp; gs.vmax = vmax; gs.hend = hend;
    if ((rc = walk_stack_forward(m, m.gru, t.gru, T, gs, drop, n, s))) return rc;
    // forecasting head: ReLU + dropout on the hidden layers (modules.py:307-311), activations kept
    {
        Scope sc(m, S_FC, s);
        const float* xin = hend;
        long ld = g.Hp;
        const int nfc = (int)m.fc.size();
        for (int i = 0; i < nfc; ++i) {
            const LinPlan& p = m.fc[i];
            const bool last = (i == nfc - 1);
            RowGemmArgs a = last ? lin_rows(m, p, xin, ld, n, preds) : lin_rows(m, p, xin, ld, n, T + t.fc_act[i], p.NT * 32);
            if (!last) {
                a.relu = 1;
                a.drop_thresh = drop.thresh; a.seed_lo = drop.seed_lo; a.seed_hi = drop.seed_hi; a.keep_scale = drop.keep_scale;
                a.drop_stream = DROP_FC0 + (unsigned)i; a.row0 = window0;
            }
            K_TRY(launch_rowgemm(a, s), "forecasting head (training)");
            xin = a.Y; ld = a.ldy;
        }
    }
    // reconstruction decoder, all steps kept: layer 0 reads the repeated h_end (modules.py:279).  Small batches: one layer on the
    // small-batch kernels behind its hoisted input products.  Otherwise the per-step Linear (modules.py:282) rides in the last layer
    // while its weights fit beside the state in 64 KB of LDS (launch_gru_split); where it does not ride it is a row GEMM over the
    // kept states
    const bool dec_small = gru_stack_small(m, m.rec, n, true);
    StackFwd ds{S_RECON, "decoder", DROP_REC0, hend, g.Hp, m.cfg.gru_hid_dim};
    ds.xp = dec_small ? T + t.xp : nullptr;
    ds.fc = &m.rec_fc; ds.rides = !dec_small && rec_fc_rides_train(m); ds.yfc = recons;
    if ((rc = walk_stack_forward(m, m.rec, t.rec, T, ds, drop, n, s))) return rc;
    K_TRY(launch_xdec(hend, g.Hp, m.cfg.gru_hid_dim, W, n, T + t.xdec, g.Hp, s), "decoder input");
    // a window with a non-finite sample answers NaN, so that the loss a caller forms from it is NaN (its gradients are unspecified)
    return run_poison(m, src, 0, n, nullptr, preds, recons, nullptr, s);
}

}  // extern "C"

namespace {

// The backward of one chunk.  grads == nullptr: the data path only (mtadgat_backward_data) -- the same kernels in the same order
// produce every data gradient, so the convolution's pre-activation gradients (and the input gradient from them) are those of
// the full backward bit for bit; no weight-gradient GEMM, column sum or reduction is issued and no gradient buffer is touched.
// (Kernels that produce a weight-only partial beside their data output -- k_bw_pair's d a', k_gat_bwd_v1 / k_bw_v1's per-window
// sums -- still run: their data outputs are what the layer below reads; the partials stay in the workspace.)
int backward_impl(mtadgat_handle h, const float* x, int64_t batch, int64_t window0, float dropout_p, uint64_t seed,
                  const float* d_preds, const float* d_recons, const void* tape_, size_t tape_bytes, float* grads,
                  void* ws_, size_t ws_bytes, void* stream) {
    int rc = check_train(h, batch, dropout_p);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!d_preds || !d_recons || !tape_ || !ws_ || (grads && !x)) return fail(MTADGAT_ERR_INVALID, "null tensor");
    const bool wg = grads != nullptr;
    Model& m = h->m;
    const BwdPlan& b = m.bw;
    const GradLayout& gl = b.gl;
    Tape t;
    plan_tape(m, batch, t);
    BwdWorkspace w;
    plan_bwd_workspace(m, batch, w);
    if (!aligned16(tape_) || tape_bytes < t.total * sizeof(float)) return fail(MTADGAT_ERR_WORKSPACE, "tape too small or misaligned");
    if (!aligned16(ws_) || ws_bytes < w.total * sizeof(float)) return fail(MTADGAT_ERR_WORKSPACE, "backward workspace too small or misaligned");
    hipStream_t s = (hipStream_t)stream;
    const float* T = static_cast<const float*>(tape_);
    float* ws = static_cast<float*>(ws_);
    const int F = m.F, W = m.W, od = m.cfg.out_dim;
    const int64_t n = batch;
    const long RW = (long)n * W;
    const DropArgs drop = make_drop(dropout_p, seed, window0);
    const GruPlan& g = m.gru.back();                 // the layer that produced h_end (all GRU layers share the hidden size)
    const GruPlan& r = m.rec.back();                 // the decoder layer under the per-step Linear
    const float* hcat = T + t.hcat;
    const float* hend = T + t.hend;
    WgradQueue wpart;
    wpart.base = ws + w.wpart; wpart.cap = w.wpart_floats; wpart.s = s;
    float* dhend = ws + w.dhend;

    // ---- 1. forecasting head (modules.py:307-311)
    {
        const int nfc = (int)m.fc.size();
        const float* dy = d_preds;
        long lddy = od;
        for (int i = nfc - 1; i >= 0; --i) {
            const LinPlan& p = m.fc[i];
            const float* act = i > 0 ? T + t.fc_act[i - 1] : hend;
            const long lda = i > 0 ? (long)m.fc[i - 1].NT * 32 : g.Hp;
            WgradIn in;
            in.A = dy; in.lda = lddy; in.B = act; in.ldb = lda; in.R = n; in.T = 1;
            if (wg && (rc = run_wgrad(m, b.fc_wg[i], in, wpart, grads + gl.fc_w[i], grads + gl.fc_b[i], s))) return rc;
            float* y = i > 0 ? ws + ((i & 1) ? w.dz1 : w.dz0) : dhend;
            const long ldy = i > 0 ? (long)b.fcT[i].NT * 32 : g.Hp;
            if ((rc = run_rowgemm_T(m, b.fcT[i], dy, lddy, n, y, ldy, (int)ldy, false, i > 0 ? act : nullptr, lda, drop.keep_scale, s))) return rc;
            dy = y; lddy = ldy;
        }
    }
    float* dhdec = ws + w.dhdec;
    const BwdCall call{m, T, n, drop, grads, wpart, ws + w.da, dhdec, s};
    // ---- 2. reconstruction model (modules.py:276-283): per-step Linear, decoder layers from the top, decoder input
    {
        if ((rc = run_rowgemm_T(m, b.recfcT, d_recons, od, RW, dhdec, r.Hp, r.Hp, false, nullptr, 0, 1.f, s))) return rc;
        WgradIn in;
        in.A = d_recons; in.lda = od; in.B = T + t.rec.back().seq; in.ldb = r.Hp; in.R = RW; in.T = W;
        if (wg && (rc = run_wgrad(m, b.recfc_wg, in, wpart, grads + gl.rec_fc_w, grads + gl.rec_fc_b, s))) return rc;
        // layer 0: d (decoder input) -> d h_end through the repeat_interleave / view of modules.py:279
        if ((rc = walk_stack_backward(call, t.rec, {true, "decoder", DROP_REC0, T + t.xdec, dhdec, g.Hp, dhdec, nullptr}))) return rc;
        K_TRY(launch_xdec_bwd(dhdec, g.Hp, m.cfg.gru_hid_dim, W, n, dhend, g.Hp, s), "decoder input adjoint");
    }
    // ---- 3. GRU layers from the top (modules.py:235-238): the last one receives d h_end, the others the gradient of their states
    float* dhcat = ws + w.dhcat;
    if ((rc = walk_stack_backward(call, t.gru, {false, "gru", DROP_GRU0, hcat, dhcat, m.Dp, nullptr, dhend}))) return rc;
    // ---- 4. the two graph-attention layers (modules.py:65-95, :166-193)
    for (int which = 1; which >= 0; --which) {
        const GatPlan& gp = which == 0 ? m.feat : m.temp;
        const GatBwdPlan& gb = b.gat[which];
        const int K = gp.K, D = gp.D, Ep = gb.Ep;
        float* de = ws + (which == 0 ? w.de_f : w.de_t);
        float* dv = ws + (which == 0 ? w.dv_f : w.dv_t);
        float* dlr = ws + (which == 0 ? w.dlr_f : w.dlr_t);
        float* dap = ws + (which == 0 ? w.dap_f : w.dap_t);
        const int lddv = which == 0 ? m.Wp : m.Fp;
        const int colofs = which == 0 ? F : 2 * F;
        const long so_w = (long)W * m.Dp, so_i = which == 0 ? 1 : m.Dp, so_d = which == 0 ? m.Dp : 1;
        const float* att = T + (which == 0 ? t.att_f : t.att_t);
        const unsigned dstream = which == 0 ? DROP_FEAT : DROP_TEMP;
        const float* Vn = which == 0 ? T + t.xct : hcat;          // node rows: xc^T rows (feature layer) / h_cat rows (temporal layer)
        const long ldv = which == 0 ? m.Wp : m.Dp;
        const int vt = which == 0 ? 1 : 0;                        // fused kernels read the nodes from h_cat: the feature layer's from its columns
        // scores and aggregation: d e (through the softmax and the dropout of the attention rows) and the aggregation's share of d V
        if (gb.wide) {
            // wide layer (mtadgat_bwdw.hip): every matrix through memory, generic in K and D
            const int ldS = round_up(D, 4);
            float* dS = ws + w.wds;
            K_TRY(launch_bw_ds(hcat + colofs, dhcat + colofs, so_w, so_i, so_d, n, K, D, dS, ldS, s), "attention backward (d S)");
            // d V (aggregation path) = att'^T d S, att' = dropout(att)
            K_TRY(launch_bgemm(att, (long)K * K, 1, K, dS, (long)K * ldS, ldS, 1, dv, (long)K * lddv, lddv, K, D, K, n, &drop, dstream, K, s),
                  "attention backward (aggregation d V)");
            // d att' = d S V^T, then the softmax backward in place -> d e
            K_TRY(launch_bgemm(dS, (long)K * ldS, ldS, 1, Vn, (long)K * ldv, 1, ldv, de, (long)K * K, K, K, K, D, n, nullptr, 0, 0, s),
                  "attention backward (d att)");
            K_TRY(launch_bw_softmax(att, de, n, K, drop, dstream, s), "attention backward (softmax)");
        } else {
            GatBwdAttArgs aa{};
            aa.V = hcat; aa.ldv = m.Dp; aa.D = D; aa.K = K; aa.vt = vt; aa.vld = gp.f_vld;
            aa.H = hcat + colofs; aa.dH = dhcat + colofs;
            aa.so_w = so_w; aa.so_i = so_i; aa.so_d = so_d;
            aa.ATT = att;
            aa.DE = de; aa.DV = dv; aa.lddv = lddv; aa.nwin = n;
            aa.drop = drop; aa.drop_stream = dstream;
            K_TRY(launch_gat_bwd_att(aa, gp.f_IBL, gp.f_JPL, gp.f_RJ, gp.f_nw, gb.att_lds, s), "attention backward (scores)");
        }
        if (!m.cfg.use_gatv2) {
            // GAT (v1) scores: linear in the node vectors below d s -- the fused layers' kernel reads them from h_cat
            // (k_gat_bwd_v1, mtadgat_bwd.hip), the wide layers' the same algebra from the node rows in memory (k_bw_v1)
            const int E = gp.E, PV = 2 * D + 2;
            float* u = ws + w.v1s + (size_t)which * 2 * (2 * std::max(m.F, m.W) + 2);
            float* P = u + (2 * std::max(m.F, m.W) + 2);
            const float* Wm = m.packed_dev + gb.w1_off;
            const float* bv = m.packed_dev + gb.b1_off;
            const float* av = m.packed_dev + gb.a_off;
            K_TRY(launch_gat_v1_prep(Wm, bv, av, E, D, u, s), "attention backward (v1 vectors)");
            if (gb.wide) K_TRY(launch_bw_v1(Vn, ldv, D, K, u, de, m.cfg.alpha, dv, lddv, dlr, n, s), "attention backward (v1 scores, wide)");
            else K_TRY(launch_gat_bwd_v1(hcat, m.Dp, D, K, vt, u, de, m.cfg.alpha, dv, lddv, dlr, n, s), "attention backward (v1 scores)");
            if (!wg) continue;
            HIP_TRY(hipMemsetAsync(P, 0, (size_t)PV * sizeof(float), s));
            K_TRY(launch_sum_rows(dlr, PV, n, PV, ws + w.sums, P, s), "attention backward (v1 sums)");
            K_TRY(launch_gat_v1_finish(P, Wm, bv, av, E, D, grads + gl.lin_w[which], grads + gl.lin_b[which], grads + gl.a[which], s),
                  "attention parameter gradients (v1)");
            K_TRY(launch_sum_rows(de, (long)K * K, n, K * K, ws + w.sums, grads + gl.bias[which], s), "attention bias gradient");
            continue;
        }
        // GATv2: the un-scaled projections [L | R] of the node rows as one row GEMM, then the one-pass score backward (k_bw_pair,
        // mtadgat_bwdw.hip) -- for fused layers too
        float* LR = ws + w.wlr;
        const long RK = (long)n * K;
        if ((rc = run_bwd_projection(m, gp, gb, Vn, ldv, RK, LR, s))) return rc;
        K_TRY(launch_bw_pair(LR, 2 * Ep, Ep, m.packed_dev + gb.a_off, de, K, m.cfg.alpha, dlr, dap, n, s), "attention backward (pairs)");
        if ((rc = run_rowgemm_T(m, gb.lrT, dlr, 2L * Ep, RK, dv, lddv, D, true, nullptr, 0, 1.f, s))) return rc;
        WgradIn in;
        in.A = dlr; in.lda = 2L * Ep; in.R = RK; in.T = 1; in.B = Vn; in.ldb = ldv;
        if (wg && (rc = run_wgrad(m, gb.wg, in, wpart, grads + gl.lin_w[which], grads + gl.lin_b[which], s))) return rc;
        if (wg && (rc = run_sum_rows_queued(de, (long)K * K, n, K * K, ws + w.sums_q[2 * which], grads + gl.bias[which], wpart, s))) return rc;
        if (wg && (rc = run_sum_rows_queued(dap, Ep, n, gp.E, ws + w.sums_q[2 * which + 1], grads + gl.a[which], wpart, s))) return rc;
    }
    // ---- 5. convolution (modules.py:18-22)
    {
        float* dpre = ws + w.dpre;
        K_TRY(launch_dxc(hcat, dhcat, m.Dp, ws + w.dv_t, m.Fp, ws + w.dv_f, m.Wp, n, W, F, dpre, m.Fp, s), "conv pre-activation gradient");
        WgradIn in;
        in.A = dpre; in.lda = m.Fp; in.B = x; in.bmode = 1; in.R = RW; in.T = W;
        if (wg && (rc = run_wgrad(m, b.conv_wg, in, wpart, grads + gl.conv_w, grads + gl.conv_b, s))) return rc;
    }
    return wpart.flush();            // every weight-gradient reduction of the step, one launch
}

// d x of the chunk whose backward left its convolution pre-activation gradients in `ws`: k_conv_dx (the window in LDS) up to
// 64 KB per window, above that the convolution of d pre with the flipped, transposed kernel (conv_wT_off) on k_conv
int input_gradient(Model& m, int64_t batch, const float* ws, const BwdWorkspace& w, float* dx, hipStream_t s) {
    if (!conv_dx_wide(m)) {
        K_TRY(launch_conv_dx(ws + w.dpre, m.Fp, m.packed_dev + m.conv_wraw_off, batch, m.W, m.F, m.taps, m.pad, dx, s), "input gradient");
        return 0;
    }
    if (m.taps != 2 * m.pad + 1 || !m.conv_wT_off) return fail(MTADGAT_ERR_UNSUPPORTED, "input gradient of wide windows needs an odd kernel size");
    ConvArgs a{};
    a.X = ws + w.dpre; a.ldx = m.Fp;
    a.B = batch; a.W = m.W; a.F = m.F; a.Fp = m.Fp; a.Fq = m.Fp; a.taps = m.taps; a.pad = m.pad;
    a.Wp = reinterpret_cast<const f32x4*>(m.packed_dev + m.conv_wT_off);
    a.NT = m.convNT;
    a.Y = dx; a.linear = 1;
    K_TRY(launch_conv_dx_gemm(a, s), "input gradient (wide windows)");
    return 0;
}

}  // namespace

extern "C" {

int mtadgat_backward(mtadgat_handle h, const float* x, int64_t batch, int64_t window0, float dropout_p, uint64_t seed,
                     const float* d_preds, const float* d_recons, const void* tape_, size_t tape_bytes, float* grads,
                     void* ws_, size_t ws_bytes, void* stream) {
    if (int rc = check_train(h, batch, dropout_p)) return rc;
    if (batch > 0 && (!x || !grads)) return fail(MTADGAT_ERR_INVALID, "null tensor");
    return backward_impl(h, x, batch, window0, dropout_p, seed, d_preds, d_recons, tape_, tape_bytes, grads, ws_, ws_bytes, stream);
}

int mtadgat_backward_data(mtadgat_handle h, const float* x, int64_t batch, int64_t window0, float dropout_p, uint64_t seed,
                          const float* d_preds, const float* d_recons, const void* tape_, size_t tape_bytes, float* dx,
                          void* ws_, size_t ws_bytes, void* stream) {
    int rc = check_train(h, batch, dropout_p);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!dx) return fail(MTADGAT_ERR_INVALID, "null tensor");
    if ((rc = backward_impl(h, x, batch, window0, dropout_p, seed, d_preds, d_recons, tape_, tape_bytes, nullptr, ws_, ws_bytes, stream)))
        return rc;
    BwdWorkspace w;
    plan_bwd_workspace(h->m, batch, w);
    return input_gradient(h->m, batch, static_cast<const float*>(ws_), w, dx, (hipStream_t)stream);
}

/* d x of the chunk whose mtadgat_backward left its convolution pre-activation gradients in `ws` */
int mtadgat_backward_input(mtadgat_handle h, int64_t batch, const void* ws_, size_t ws_bytes, float* dx, void* stream) {
    int rc = check_train(h, batch, 0.f);
    if (rc) return rc;
    if (batch == 0) return 0;
    if (!ws_ || !dx) return fail(MTADGAT_ERR_INVALID, "null tensor");
    Model& m = h->m;
    BwdWorkspace w;
    plan_bwd_workspace(m, batch, w);
    if (!aligned16(ws_) || ws_bytes < w.total * sizeof(float)) return fail(MTADGAT_ERR_WORKSPACE, "backward workspace too small or misaligned");
    return input_gradient(m, batch, static_cast<const float*>(ws_), w, dx, (hipStream_t)stream);
}

/* ---- score attribution (scratch: plan_attribution) ------------------------------------------------------------------------- */
size_t mtadgat_score_attribution_workspace_bytes(mtadgat_handle h, int64_t count, int steps) {
    if (!h || count < 1 || steps < 0 || !h->m.bw.supported) return 0;
    AttrPlan p;
    plan_attribution(h->m, count, steps, p);
    return p.total * sizeof(float);
}

int mtadgat_score_attribution(mtadgat_handle h, const float* series, int64_t n_rows, const int64_t* idx, int64_t count,
                              const int32_t* dims, int n_dims, const float* dim_w, float gamma, int steps, const float* baseline,
                              int baseline_kind, float* out, void* ws_, size_t ws_bytes, void* stream) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    Model& m = h->m;
    if (!m.have_weights) return fail(MTADGAT_ERR_NOWEIGHTS, "mtadgat_load_weights has not been called");
    if (!m.bw.supported) return fail(MTADGAT_ERR_UNSUPPORTED, "score attribution needs the HIP backward, which this configuration lacks: " + m.bw.why);
    if (count < 0) return fail(MTADGAT_ERR_INVALID, "negative index count");
    if (steps < 0) return fail(MTADGAT_ERR_INVALID, "steps must be >= 0 (0 = gradient)");
    if (n_dims != m.cfg.out_dim) return fail(MTADGAT_ERR_INVALID, "n_dims must equal out_dim (one series column per output dimension)");
    if (baseline_kind < 0 || baseline_kind > 2) return fail(MTADGAT_ERR_INVALID, "baseline_kind must be 0 (zeros), 1 (F) or 2 (W+1, F)");
    if (baseline_kind != 0 && !baseline) return fail(MTADGAT_ERR_INVALID, "baseline is NULL");
    if (!(std::isfinite(gamma))) return fail(MTADGAT_ERR_INVALID, "gamma must be finite");
    if (count == 0) return 0;
    if (n_rows < (int64_t)m.W + 1) return fail(MTADGAT_ERR_INVALID, "series shorter than window_size + 1");
    if (!series || !idx || !dims || !dim_w || !out) return fail(MTADGAT_ERR_INVALID, "null tensor");
    if (!ws_) return fail(MTADGAT_ERR_WORKSPACE, "workspace is NULL");
    if (!aligned16(ws_)) return fail(MTADGAT_ERR_WORKSPACE, "workspace must be 16-byte aligned");
    AttrPlan p;
    plan_attribution(m, count, steps, p);
    if (ws_bytes < p.total * sizeof(float)) return fail(MTADGAT_ERR_WORKSPACE, "workspace too small");
    // fp32 arithmetic of the training step: mode 0 stays 0, modes 1 and 2 run as 2; restored (with profiling) on return
    struct Restore {
        Model& m; int precision; bool profile;
        ~Restore() { m.precision = precision; m.profile = profile; }
    } restore{m, m.precision, m.profile};
    m.precision = m.precision == 0 ? 0 : 2;
    m.profile = false;
    hipStream_t s = (hipStream_t)stream;
    float* ws = static_cast<float*>(ws_);
    AttrArgs a{};
    a.series = series; a.idx = reinterpret_cast<const long*>(idx); a.dims = dims; a.dim_w = dim_w;
    a.base = baseline; a.base_kind = baseline_kind;
    a.W = m.W; a.F = m.F; a.od = m.cfg.out_dim; a.steps = steps; a.gamma = gamma;
    a.X = ws + p.x; a.Y = ws + p.y; a.preds = ws + p.preds; a.recons = ws + p.recons; a.dpreds = ws + p.dpreds; a.drecons = ws + p.drecons;
    a.gy = ws + p.gy; a.dx = ws + p.dx; a.out = out;
    const int64_t U = count * std::max(steps, 1);
    int rc;
    for (int64_t u0 = 0; u0 < U; u0 += p.units) {
        const int64_t nu = std::min<int64_t>(p.units, U - u0);
        a.u0 = u0; a.nu = nu;
        K_TRY(launch_attr_gather(a, s), "attribution (gather)");
        if ((rc = mtadgat_forward_train(h, a.X, 2 * nu, 0, 0.f, 0, ws + p.preds, ws + p.recons, ws + p.tape, p.tape_floats * sizeof(float), stream)))
            return rc;
        K_TRY(launch_attr_seed(a, s), "attribution (seed)");
        if ((rc = mtadgat_backward_data(h, a.X, 2 * nu, 0, 0.f, 0, ws + p.dpreds, ws + p.drecons, ws + p.tape, p.tape_floats * sizeof(float),
                                        ws + p.dx, ws + p.bws, p.bws_floats * sizeof(float), stream)))
            return rc;
        K_TRY(launch_attr_combine(a, s), "attribution (combine)");
    }
    return 0;
}

/* The keep-masks of nn.GRU's dropout between stacked layers (reference modules.py:233 / :253): mask_gru (gru_n_layers - 1, batch, W, H),
 * mask_rec (recon_n_layers - 1, batch, W, recon_hid_dim); either may be NULL */
int mtadgat_dropout_masks_rnn(mtadgat_handle h, int64_t batch, int64_t window0, float dropout_p, uint64_t seed, float* mask_gru,
                              float* mask_rec, void* stream) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    if (batch <= 0) return 0;
    Model& m = h->m;
    hipStream_t s = (hipStream_t)stream;
    const DropArgs drop = make_drop(dropout_p, seed, window0);
    if (mask_gru)
        for (size_t l = 0; l + 1 < m.gru.size(); ++l)
            K_TRY(launch_dropmask(drop, DROP_GRU0 + (unsigned)l, batch, (long)m.W * m.gru[l].H, mask_gru + l * (size_t)batch * m.W * m.gru[l].H, s), "dropout mask");
    if (mask_rec)
        for (size_t l = 0; l + 1 < m.rec.size(); ++l)
            K_TRY(launch_dropmask(drop, DROP_REC0 + (unsigned)l, batch, (long)m.W * m.rec[l].H, mask_rec + l * (size_t)batch * m.W * m.rec[l].H, s), "dropout mask");
    return 0;
}

int mtadgat_dropout_masks(mtadgat_handle h, int64_t batch, int64_t window0, float dropout_p, uint64_t seed, float* mask_feat,
                          float* mask_temp, float* mask_fc, void* stream) {
    if (!h) return fail(MTADGAT_ERR_INVALID, "null handle");
    if (batch <= 0) return 0;
    Model& m = h->m;
    hipStream_t s = (hipStream_t)stream;
    const DropArgs drop = make_drop(dropout_p, seed, window0);
    if (mask_feat) K_TRY(launch_dropmask(drop, DROP_FEAT, batch, (long)m.F * m.F, mask_feat, s), "dropout mask");
    if (mask_temp) K_TRY(launch_dropmask(drop, DROP_TEMP, batch, (long)m.W * m.W, mask_temp, s), "dropout mask");
    if (mask_fc) {
        const int hid = m.cfg.forecast_hid_dim;
        for (size_t i = 0; i + 1 < m.fc.size(); ++i)
            K_TRY(launch_dropmask(drop, DROP_FC0 + (unsigned)i, batch, hid, mask_fc + i * (size_t)batch * hid, s), "dropout mask");
    }
    return 0;
}

}  // extern "C"

// ---- scoring live streams row by row (kernels: mtadgat_stream.hip) -----------------------------------------------------------
namespace {

constexpr int64_t STREAM_MAX_BLOCK = 65536;

bool stream_sizes_ok(int64_t n_streams, int64_t max_block) {
    return n_streams >= 1 && n_streams <= 2147483647LL && max_block >= 1 && max_block <= STREAM_MAX_BLOCK;
}
StreamGeom stream_geom(const Model& m, int64_t n_streams, int64_t max_block) {
    return StreamGeom{(long)n_streams, (long)(m.W + max_block - 1), (long)m.W, (long)m.F, (long)m.cfg.out_dim};
}
// what every call on an initialised state checks on the host
int stream_check(mtadgat_handle h, const void* state, int64_t n_streams, int64_t max_block, int64_t n, int64_t T, const char* who) {
    if (!h) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": null handle");
    if (!state) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": state is NULL");
    if (!aligned16(state)) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": state must be 16-byte aligned");
    if (!stream_sizes_ok(n_streams, max_block))
        return fail(MTADGAT_ERR_INVALID, std::string(who) + ": needs 1 <= n_streams < 2^31 and 1 <= max_block <= 65536");
    if (n < 1 || n > n_streams) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": n must lie in [1, n_streams]");
    if (T < 1 || T > max_block) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": T must lie in [1, max_block]");
    return 0;
}
StreamOut stream_out(const mtadgat_stream_outputs* o) {
    StreamOut r{};
    if (!o) return r;
    r.scores = o->scores; r.flags = o->flags; r.per_dim = o->per_dim;
    r.closed_start = reinterpret_cast<long*>(o->closed_start); r.closed_end = reinterpret_cast<long*>(o->closed_end);
    r.closed_peak = reinterpret_cast<long*>(o->closed_peak); r.closed_peak_score = o->closed_peak_score; r.closed_mean = o->closed_mean;
    return r;
}

}  // namespace

extern "C" {

size_t mtadgat_stream_state_bytes(mtadgat_handle h, int64_t n_streams, int64_t max_block) {
    if (!h || !stream_sizes_ok(n_streams, max_block)) return 0;
    return stream_layout((long)n_streams, (long)max_block, h->m.W, h->m.F, h->m.cfg.out_dim).bytes;
}

int mtadgat_stream_init(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, double gamma, double alpha, int64_t merge_gap,
                        int64_t min_length, const int32_t* dims_host, const float* center_host, const float* spread_host, void* stream) {
    int rc = stream_check(h, state, n_streams, max_block, 1, 1, "stream_init");
    if (rc) return rc;
    const Model& m = h->m;
    const int d = m.cfg.out_dim;
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(MTADGAT_ERR_INVALID, "stream_init: alpha outside [0, 1]");
    if (!(gamma == gamma)) return fail(MTADGAT_ERR_INVALID, "stream_init: gamma is NaN");
    if (merge_gap < 0) return fail(MTADGAT_ERR_INVALID, "stream_init: merge_gap must be >= 0");
    if (min_length < 1) return fail(MTADGAT_ERR_INVALID, "stream_init: min_length must be >= 1");
    if ((center_host == nullptr) != (spread_host == nullptr)) return fail(MTADGAT_ERR_INVALID, "stream_init: give center and spread, or neither");
    std::vector<int> dims(d);
    for (int c = 0; c < d; ++c) {
        dims[c] = dims_host ? dims_host[c] : c;
        if (dims[c] < 0 || dims[c] >= m.F) return fail(MTADGAT_ERR_INVALID, "stream_init: a target dimension lies outside [0, n_features)");
    }
    StreamHeader hd{};
    hd.S = n_streams; hd.R = m.W + max_block - 1; hd.W = m.W; hd.F = m.F; hd.d = d; hd.max_block = max_block;
    hd.merge_gap = merge_gap; hd.min_length = min_length; hd.gamma = gamma; hd.decay = 1.0 - alpha;
    hd.smooth = alpha > 0.0 ? 1 : 0; hd.scaled = center_host ? 1 : 0;
    HIP_TRY((hipError_t)launch_stream_init(state, hd, dims.data(), center_host, spread_host, (hipStream_t)stream));
    return 0;
}

size_t mtadgat_stream_workspace_bytes(mtadgat_handle h, int64_t windows) {
    if (!h || windows < 1 || windows > 2147483647LL) return 0;
    return stream_ws(h->m, windows).total * sizeof(float);
}

}  // extern "C"

namespace {

// the SPOT state of the *_spot entry points, checked on the host like the stream state
int stream_spot_check(const void* spot, int64_t max_peaks, const char* who) {
    if (max_peaks < 8 || max_peaks > 4096) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": max_peaks must lie in [8, 4096]");
    if (!spot) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": the SPOT state is NULL");
    if (!aligned16(spot)) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": the SPOT state must be 16-byte aligned");
    return 0;
}

// mtadgat_stream_update and mtadgat_stream_update_spot (spot non-null)
int stream_update(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, const float* preds, const float* recons_last,
                  const float* rows, const int64_t* streams, int64_t n, int64_t T, int staged, double threshold, const double* thresholds,
                  const StreamSpot* spot, const mtadgat_stream_outputs* out, void* stream, const char* who) {
    int rc = stream_check(h, state, n_streams, max_block, n, T, who);
    if (rc) return rc;
    if (spot && (rc = stream_spot_check(spot->state, spot->max_peaks, who))) return rc;
    if (!preds || !recons_last || !rows) return fail(MTADGAT_ERR_INVALID, std::string(who) + ": null tensor");
    const StreamGeom g = stream_geom(h->m, n_streams, max_block);
    const long* st = reinterpret_cast<const long*>(streams);
    hipStream_t s = (hipStream_t)stream;
    if (!staged) K_TRY(launch_stream_stage(state, g, rows, st, n, T, nullptr, s), "stream stage");
    K_TRY(launch_stream_score(state, g, rows, st, n, T, preds, recons_last, threshold, thresholds, stream_out(out), s, spot), "stream score");
    return 0;
}

int stream_push(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, const float* rows, const int64_t* streams, int64_t n,
                int64_t T, double threshold, const double* thresholds, const StreamSpot* spot, const mtadgat_stream_outputs* out, void* ws_,
                size_t ws_bytes, void* stream, const char* who);

}  // namespace

extern "C" {

int mtadgat_stream_update(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, const float* preds, const float* recons_last,
                          const float* rows, const int64_t* streams, int64_t n, int64_t T, int staged, double threshold,
                          const double* thresholds, const mtadgat_stream_outputs* out, void* stream) {
    return stream_update(h, state, n_streams, max_block, preds, recons_last, rows, streams, n, T, staged, threshold, thresholds, nullptr, out,
                         stream, "stream_update");
}

int mtadgat_stream_update_spot(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, const float* preds,
                               const float* recons_last, const float* rows, const int64_t* streams, int64_t n, int64_t T, int staged,
                               void* spot, int64_t max_peaks, double* thresholds_out, const mtadgat_stream_outputs* out, void* stream) {
    const StreamSpot sp{spot, (long)max_peaks, thresholds_out};
    return stream_update(h, state, n_streams, max_block, preds, recons_last, rows, streams, n, T, staged, 0.0, nullptr, &sp, out, stream,
                         "stream_update_spot");
}

int mtadgat_stream_push(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, const float* rows, const int64_t* streams,
                        int64_t n, int64_t T, double threshold, const double* thresholds, const mtadgat_stream_outputs* out, void* ws_,
                        size_t ws_bytes, void* stream) {
    return stream_push(h, state, n_streams, max_block, rows, streams, n, T, threshold, thresholds, nullptr, out, ws_, ws_bytes, stream,
                       "stream_push");
}

int mtadgat_stream_push_spot(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, const float* rows, const int64_t* streams,
                             int64_t n, int64_t T, void* spot, int64_t max_peaks, double* thresholds_out, const mtadgat_stream_outputs* out,
                             void* ws_, size_t ws_bytes, void* stream) {
    const StreamSpot sp{spot, (long)max_peaks, thresholds_out};
    return stream_push(h, state, n_streams, max_block, rows, streams, n, T, 0.0, nullptr, &sp, out, ws_, ws_bytes, stream, "stream_push_spot");
}

int mtadgat_stream_reset_spot(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, void* spot, const void* spot_calibrated,
                              int64_t calibrated_columns, int64_t max_peaks, const int64_t* streams, int64_t n, void* stream) {
    int rc = stream_check(h, state, n_streams, max_block, n, 1, "stream_reset_spot");
    if (rc) return rc;
    if ((rc = stream_spot_check(spot, max_peaks, "stream_reset_spot")) || (rc = stream_spot_check(spot_calibrated, max_peaks, "stream_reset_spot")))
        return rc;
    if (calibrated_columns != 1 && calibrated_columns != n_streams)
        return fail(MTADGAT_ERR_INVALID, "stream_reset_spot: the calibrated state needs one column or n_streams columns");
    const long* st = reinterpret_cast<const long*>(streams);
    K_TRY(launch_stream_flush(state, stream_geom(h->m, n_streams, max_block), st, n, 0, 1, StreamOut{}, (hipStream_t)stream), "stream flush");
    K_TRY(launch_spot_copy(spot, (long)n_streams, spot_calibrated, (long)calibrated_columns, (long)max_peaks, st, (long)n, (hipStream_t)stream),
          "spot copy");
    return 0;
}

}  // extern "C"

namespace {

int stream_push(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, const float* rows, const int64_t* streams, int64_t n,
                int64_t T, double threshold, const double* thresholds, const StreamSpot* spot, const mtadgat_stream_outputs* out, void* ws_,
                size_t ws_bytes, void* stream, const char* who_) {
    const std::string who(who_);
    int rc = stream_check(h, state, n_streams, max_block, n, T, who_);
    if (rc) return rc;
    if (spot && (rc = stream_spot_check(spot->state, spot->max_peaks, who_))) return rc;
    if (!rows) return fail(MTADGAT_ERR_INVALID, who + ": null tensor");
    const Model& m = h->m;
    const int64_t windows = n * T;
    if (windows > 2147483647LL) return fail(MTADGAT_ERR_INVALID, who + ": n * T must stay below 2^31");
    const StreamWs w = stream_ws(m, windows);
    if (!ws_) return fail(MTADGAT_ERR_WORKSPACE, who + ": workspace is NULL");
    if (!aligned16(ws_)) return fail(MTADGAT_ERR_WORKSPACE, who + ": workspace must be 16-byte aligned");
    if (ws_bytes < w.total * sizeof(float)) return fail(MTADGAT_ERR_WORKSPACE, who + ": workspace too small (see mtadgat_stream_workspace_bytes)");
    if ((rc = check_common(h, windows, nullptr, 0, false))) return rc;
    const StreamGeom g = stream_geom(m, n_streams, max_block);
    const StreamLayout l = stream_layout(g.S, (long)max_block, g.W, g.F, g.d);
    float* ws = static_cast<float*>(ws_);
    int64_t* starts = reinterpret_cast<int64_t*>(ws + w.starts);
    const long* st = reinterpret_cast<const long*>(streams);
    hipStream_t s = (hipStream_t)stream;
    K_TRY(launch_stream_stage(state, g, rows, st, n, T, reinterpret_cast<long*>(starts), s), "stream stage");
    const float* history = reinterpret_cast<const float*>(static_cast<const char*>(state) + l.ring);
    if ((rc = mtadgat_forward_series(h, history, g.S * 2 * g.R, starts, 0, 1, windows, ws + w.preds, nullptr, ws + w.last, ws + w.fwd,
                                     (w.total - w.fwd) * sizeof(float), stream)))
        return rc;
    if (!out) return 0;
    K_TRY(launch_stream_score(state, g, rows, st, n, T, ws + w.preds, ws + w.last, threshold, thresholds, stream_out(out), s, spot), "stream score");
    return 0;
}

}  // namespace

extern "C" {

int mtadgat_stream_flush(mtadgat_handle h, void* state, int64_t n_streams, int64_t max_block, const int64_t* streams, int64_t n, int reset,
                         const mtadgat_stream_outputs* out, void* stream) {
    int rc = stream_check(h, state, n_streams, max_block, n, 1, "stream_flush");
    if (rc) return rc;
    if (!out && !reset) return fail(MTADGAT_ERR_INVALID, "stream_flush: neither outputs nor reset asked for");
    K_TRY(launch_stream_flush(state, stream_geom(h->m, n_streams, max_block), reinterpret_cast<const long*>(streams), n, out ? 1 : 0,
                              reset ? 1 : 0, stream_out(out), (hipStream_t)stream), "stream flush");
    return 0;
}

}  // extern "C"
