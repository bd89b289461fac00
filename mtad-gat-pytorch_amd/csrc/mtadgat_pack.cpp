// Host-side planning and weight packing: reference-format parameters -> the tile
// streams the gfx950 kernels consume (mtadgat_kernels.hip).  Pure host C++.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include "mtadgat_host.h"

namespace mtadgat {

namespace {

// tile format: [NT][Q][64 lanes][4]; lane (j = lane&31, g = lane>>5), element s holds
// M[32n + j][8q + 4g + s] (zero outside the matrix)
template <class T, class Get>
void pack_tiles(T* out, int NT, int Q, Get get) {
    for (int n = 0; n < NT; ++n)
        for (int q = 0; q < Q; ++q) {
            T* o = out + ((size_t)n * Q + q) * 256;
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s) o[lane * 4 + s] = get(32 * n + (lane & 31), 8 * q + 4 * (lane >> 5) + s);
        }
}

// GRU stream format: [NCG][Q][3 gates][64 lanes][4]
template <class Get>
void pack_gru_tiles(float* out, int NCG, int Q, Get get /*(gate,row,k)*/) {
    for (int c = 0; c < NCG; ++c)
        for (int q = 0; q < Q; ++q)
            for (int st = 0; st < 3; ++st) {
                float* o = out + (((size_t)c * Q + q) * 3 + st) * 256;
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s) o[lane * 4 + s] = get(st, 32 * c + (lane & 31), 8 * q + 4 * (lane >> 5) + s);
            }
}

inline uint16_t f2bf(float f) {                      // round to nearest even, as v_cvt_pk_bf16_f32
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// feature index of element e of lane-half g inside a 16-feature bf16 chunk (mtadgat_device.h)
inline int bf_k(int g, int e) { return e < 4 ? 4 * g + e : 8 + 4 * g + (e - 4); }

// bf16 tile format: [NT][Q16][64 lanes][8 bf16]; lane (j, g) element e holds M[32n + j][16q + bf_k(g, e)]
template <class Get>
void pack_tiles_bf16(float* out, int NT, int Q, Get get) {
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out);
    for (int n = 0; n < NT; ++n)
        for (int q = 0; q < Q; ++q) {
            uint16_t* o = o16 + ((size_t)n * Q + q) * 512;
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) o[lane * 8 + e] = f2bf(get(32 * n + (lane & 31), 16 * q + bf_k(lane >> 5, e)));
        }
}

// bf16 GRU stream: [NCG][Q16][3 gates][64 lanes][8 bf16]
template <class Get>
void pack_gru_tiles_bf16(float* out, int NCG, int Q, Get get /*(gate,row,k)*/) {
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out);
    for (int c = 0; c < NCG; ++c)
        for (int q = 0; q < Q; ++q)
            for (int st = 0; st < 3; ++st) {
                uint16_t* o = o16 + (((size_t)c * Q + q) * 3 + st) * 512;
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) o[lane * 8 + e] = f2bf(get(st, 32 * c + (lane & 31), 16 * q + bf_k(lane >> 5, e)));
            }
}

}  // namespace

std::string validate_and_plan(Model& m) {
    const mtadgat_config& c = m.cfg;
    if (c.n_features < 1 || c.window_size < 1 || c.out_dim < 1) return "n_features, window_size and out_dim must be >= 1";
    if (c.kernel_size < 1 || (c.kernel_size & 1) == 0) return "kernel_size must be odd (the reference's ConvLayer shortens the window otherwise)";
    if (c.feat_embed < 1 || c.time_embed < 1) return "embedding dims must be >= 1";
    if (c.n_features > 2048) return "n_features up to 2048 are supported";
    if (c.window_size > 512) return "window_size up to 512 nodes is supported";
    if (c.gru_n_layers < 1 || c.gru_n_layers > MTADGAT_MAX_LAYERS) return "gru_n_layers out of range";
    if (c.recon_n_layers < 1 || c.recon_n_layers > MTADGAT_MAX_LAYERS) return "recon_n_layers out of range";
    if (c.forecast_n_linear < 1 || c.forecast_n_linear > MTADGAT_MAX_LAYERS) return "forecast_n_linear out of range";
    if (c.gru_hid_dim < 1 || c.gru_hid_dim > 256 || c.recon_hid_dim < 1 || c.recon_hid_dim > 256)
        return "GRU hidden sizes 1..256 are supported";
    if (c.forecast_hid_dim < 1) return "forecast_hid_dim must be >= 1";

    m.F = c.n_features;
    m.W = c.window_size;
    m.Fp = round_up(m.F, 8);
    m.Wp = round_up(m.W, 8);
    m.Dp = round_up(3 * m.F, 8);
    m.taps = c.kernel_size;
    m.pad = (c.kernel_size - 1) / 2;

    Carver img;          // the packed image
    // split packs (SplitTable): take_split reserves a region for one, split_group records the steps that derive a group of them
    using S = SplitStep;
    m.split = SplitTable();
    auto take_split = [&](size_t n) { const size_t o = img.take(n); m.split.regions.emplace_back(o, n); return o; };
    auto split_group = [&](std::vector<SplitStep> st) { m.split.groups.push_back(SplitGroup{std::move(st)}); return (int)m.split.groups.size() - 1; };
    auto lin_split = [&](auto& p) { p.split = split_group({{S::SPLIT3, 0, p.w_off, p.w3_off, p.NT, p.Q, p.Q16}}); };
    // conv
    m.convNT = (m.F + 31) / 32;
    {
        const int Q = m.taps * m.Fp / 8;
        m.conv_w_off = img.take((size_t)m.convNT * Q * 256);
        m.conv_b_off = img.take((size_t)m.convNT * 32);
        m.conv_wraw_off = img.take((size_t)m.F * m.F * m.taps);
        m.Fp16 = round_up(m.F, 16);
        m.conv_w16_off = img.take((size_t)m.convNT * (m.taps * m.Fp16 / 16) * 256);
        m.conv_wf16_off = img.take((size_t)m.convNT * (m.taps * m.Fp16 / 8) * 256);
        m.conv_w3_off = take_split((size_t)m.convNT * (m.taps * m.Fp16 / 16) * 3 * 256);
        m.conv_w2h_off = take_split((size_t)m.convNT * (m.taps * m.Fp16 / 16) * 2 * 256);
        m.conv_scale_off = take_split(4);
        m.conv_wT_off = conv_dx_wide(m) ? img.take((size_t)m.convNT * Q * 256) : 0;
        // k_conv_win's two fp16 pieces of S * W in the 16-channel geometry; three bf16 pieces for the wide models' k_conv_x3
        const int q8 = m.taps * m.Fp16 / 8;
        const size_t sc = m.conv_scale_off;
        m.conv_split = split_group({{S::ZERO_SCALE, sc},
                                    {S::ABSMAX, sc, m.conv_wf16_off, 0, (long)m.convNT * q8 * 256},
                                    {S::SCALE_FROM_MAX, sc},
                                    {S::SPLIT2H, sc, m.conv_wf16_off, m.conv_w2h_off, m.convNT, q8, q8 / 2, 1},
                                    {S::SPLIT3, 0, m.conv_wf16_off, m.conv_w3_off, m.convNT, q8, q8 / 2}});
    }
    // GAT layers
    auto plan_gat = [&](GatPlan& g, int K, int D, int E) {
        g.K = K; g.D = D; g.E = E;
        const int ptcap = c.use_gatv2 ? round_up(E, 8) + 8 : 0;
        g.ldl = round_up(ptcap + 1, 32);
        g.rt_rows = g.ldl;
        g.Kp = round_up(K, 4);
        g.NT_L = g.ldl / 32;
        g.NT = 2 * g.NT_L;
        g.PT = g.P8 = 0;
        // fused plan: one workgroup (f_nw waves) per window, tiles of the layer resident in LDS.
        // A wave owns 4*IBL query rows, a lane JPL key nodes (16*JPL >= K); see k_gat.
        g.fused = false;
        g.Q = (D + 7) / 8;
        if (K <= 128 && D <= 128) {
            const int ibl = 4, ibw = 4 * ibl;
            const int nwa = (K + ibw - 1) / ibw;                 // waves that own query rows
            const int ntask = 2 * ((K + 31) / 32);               // projection tiles per part
            int nw = nwa;
            if (ntask > nwa) nw = std::min(8, std::max(nwa, std::min(ntask, round_up(nwa, 4))));   // extra waves only project
            const int rows = nwa * ibw;
            const int qf = (D + 8) / 8;                          // chunks incl. the bias row D (times the ones column of Vs)
            const int vld = 8 * qf + 4;
            const size_t lr = round_up((int)std::max((size_t)(rows + K) * 34, (size_t)rows * 68), 4);
            const size_t bytes = ((size_t)round_up(K, 16) * vld + lr) * sizeof(float);
            if (bytes <= 80 * 1024) {
                g.fused = true; g.f_nw = nw; g.f_IBL = ibl; g.f_JPL = (K + 15) / 16; g.f_RJ = 16; g.f_vld = vld; g.f_lr = (int)lr;
                // 8 lanes along the key axis when that pads the keys less (K = 55: 56 instead of 64)
                if (K <= 56 && ((K + 7) / 8) % 2 == 1) { g.f_RJ = 8; g.f_IBL = 2; g.f_JPL = (K + 7) / 8; }
                g.f_lds_bytes = bytes;
                g.Q = qf;
            }
        }
        g.w_off = img.take((size_t)g.NT * g.Q * 256);
        g.b_off = img.take((size_t)g.NT * 32);
        g.bias_off = img.take((size_t)K * K);
        g.ord_off = img.take(16);
        g.PTcap = ptcap;
        g.Q16 = g.fused ? (D + 1 + 15) / 16 : 0;
        if (g.fused) {      // fp16-piece build: pitch 4 x odd halfs (conflict-free 8-byte operand reads of 32 consecutive nodes)
            g.fh_IBL = g.f_IBL; g.fh_JPL = g.f_JPL; g.fh_RJ = g.f_RJ;
            // (8 lanes along the keys also where that pads them less than 16 -- K = 100: 104 instead of 112 keys -- costs as much in
            // LDS operand reads as it saves in pair instructions: 10.15 vs 10.05 ms for the two layers; measurement hook)
            if (const char* e_ = getenv("MTADGAT_GATH_RJ8"))
                if (atoi(e_) && g.f_RJ == 16 && round_up(K, 8) < round_up(K, 16) && (K + 7) / 8 <= 15) { g.fh_RJ = 8; g.fh_IBL = 2; g.fh_JPL = (K + 7) / 8; }
            {   // row blocks of the owning waves: as few padded rows as 16-row and short (12- / 8-row) blocks allow
                const int shortrows = 16 - 64 / g.fh_RJ;
                int best_rows = 1 << 30, bf = 0, bs = 0;
                for (int nf = 0; nf <= g.f_nw; ++nf)
                    for (int ns = 0; nf + ns <= g.f_nw; ++ns) {
                        const int rows = 16 * nf + shortrows * ns;
                        if (rows >= K && (rows < best_rows || (rows == best_rows && nf + ns < bf + bs))) { best_rows = rows; bf = nf; bs = ns; }
                    }
                g.fh_full = bf; g.fh_short = bs;
            }
            // piece pitch: the smallest 4 x odd halfs that holds the D + 1 features (conflict-free 8-byte operand reads of 32
            // consecutive nodes; the last chunk of a row may read on into the next row: finite values against zero weights)
            g.fh_vld = (D + 1 + 3) & ~3;
            if ((g.fh_vld >> 2) % 2 == 0) g.fh_vld += 4;
            if (g.fh_vld > 16 * g.Q16 + 4) g.fh_vld = 16 * g.Q16 + 4;
            const int orows = (g.fh_full + g.fh_short) * 16;     // rows of L' the owning waves address
            g.fh_lr = (int)round_up((int)std::max((size_t)(orows + K) * 34, (size_t)orows * 36), 4);
            g.fh_lds_bytes = (size_t)g.fh_lr * sizeof(float) + (size_t)2 * ((K + 1) * g.fh_vld + 16) * 2;
            {   // run-ahead projection (k_gath): a second L' / R' buffer when the workgroup has a wave that owns no query rows, the
                // part's weight words fit the projector's registers (Q <= 4) and the LDS does not cost a resident workgroup
                // (160 KB per CU; 16 waves per CU at the kernel's 128 registers).  Two buffers only fit with K rows of L' each.
                g.fh_lr_buf = 0;
                const size_t buf = (size_t)round_up((K + K) * 34, 4);
                const size_t pieces = (size_t)2 * ((K + 1) * g.fh_vld + 16) * 2;
                const size_t total = 2 * buf * sizeof(float) + pieces;
                auto resident = [&](size_t bytes) { return std::min<size_t>((size_t)160 * 1024 / bytes, (size_t)16 / g.f_nw); };
                if (g.f_nw == 8 && g.fh_full + g.fh_short <= 7 && g.Q16 <= 4 && ptcap >= 32 && (size_t)orows * 36 <= 2 * buf &&
                    total <= 160 * 1024 && resident(total) == resident(g.fh_lds_bytes) && !getenv("MTADGAT_GATH_NOAHEAD")) {
                    g.fh_lr_buf = (int)buf; g.fh_lr = (int)(2 * buf); g.fh_lds_bytes = total;
                }
            }
            // measurement hook (profiles/gath_timeline.py): more LDS per workgroup = fewer resident workgroups per CU
            if (const char* e_ = getenv("MTADGAT_GATH_PADLDS")) g.fh_lds_bytes = std::max<size_t>(g.fh_lds_bytes, (size_t)atoi(e_) * 1024);
        }
        g.w16_off = img.take((size_t)g.NT * g.Q16 * 256);
        g.w3_off = take_split((size_t)g.NT * g.Q16 * 3 * 256);
        g.w2h_off = take_split((size_t)g.NT * g.Q16 * 2 * 256);
        g.gscale_off = take_split(4);
        g.uQ16 = g.fused ? 0 : (g.Q + 1) / 2;
        g.uw3_off = take_split((size_t)g.NT * g.uQ16 * 3 * 256);
        const size_t sc = g.gscale_off;
        if (g.fused)        // k_gat's bf16 pieces; the scale and k_gath's fp16 pieces (GATv2: compact column order, non-negative group padded to 2, not 8)
            g.split = split_group({{S::SPLIT3, 0, g.w_off, g.w3_off, g.NT, g.Q, g.Q16},
                                   {S::ZERO_SCALE, sc},
                                   {S::ABSMAX, sc, g.w_off, 0, (long)g.NT * g.Q * 256},
                                   {S::SCALE_FROM_MAX, sc},
                                   c.use_gatv2 ? S{S::SPLIT2H_GATH, sc, g.w_off, g.w2h_off, g.NT_L, g.Q, g.Q16, g.E, g.ord_off}
                                               : S{S::SPLIT2H, sc, g.w_off, g.w2h_off, g.NT, g.Q, g.Q16, 1}});
        else if (g.uQ16 > 0)   // the row GEMM's pack (k_rowgemm_x3)
            g.split = split_group({{S::SPLIT3, 0, g.w_off, g.uw3_off, g.NT, g.Q, g.uQ16}});
    };
    // a recurrence layer: the power-of-two scale from its largest weight, the input pack on three bf16 pieces (and on two fp16 pieces),
    // the recurrent pack on two fp16 pieces, the chunk-major copy of the two-piece input pack (k_gru_cm)
    auto gru_split = [&](GruPlan& g) {
        const long outer_x = (long)(g.xmode == 1 ? m.W : 1) * g.NCG;
        const size_t sc = g.scale_off;
        const bool x2 = g.wx2_off && g.qb3 > 0;
        std::vector<SplitStep> st = {{S::ZERO_SCALE, sc},
                                     {S::ABSMAX, sc, g.wx_off, 0, outer_x * g.Qxp * 3 * 256},
                                     {S::ABSMAX, sc, g.wh_off, 0, (long)g.NCG * (4 * g.NCG + 2) * 3 * 256},
                                     {S::SCALE_FROM_MAX, sc},
                                     {S::SPLIT_X, sc, g.wx_off, g.wx3_off, outer_x, g.Qxp, g.Qxp16, g.qb3}};
        if (x2) st.push_back({S::SPLIT_X, sc, g.wx_off, g.wx2_off, outer_x, g.Qxp, g.Qxp16, 0});
        st.push_back({S::SPLIT2H, sc, g.wh_off, g.wh3_off, g.NCG, 4 * g.NCG + 2, 2 * g.NCG + 2, 3});
        if (g.wxq_off) st.push_back({S::REORDER_XQ, 0, x2 ? g.wx2_off : g.wx3_off, g.wxq_off, g.NCG, 0, g.Qxp16});
        g.split = split_group(std::move(st));
    };
    plan_gat(m.feat, m.F, m.W, c.feat_embed);
    plan_gat(m.temp, m.W, m.F, c.time_embed);
    auto plan16 = [&](GruPlan& g) {
        const int Hp16 = round_up(g.H, 16);
        if (Hp16 > 160 || (g.xmode == 1 && g.Qx != 1)) return;       // weights must fit the wave's registers; 8 folded columns
        g.has16 = true; g.KS16 = (g.H + 3) / 4; g.NT16 = Hp16 / 16;
        g.g16_off = img.take((size_t)g.NT16 * 3 * g.KS16 * 64);
        g.g16T_off = img.take((size_t)g.NT16 * 3 * g.KS16 * 64);
        if (g.xmode == 1) g.fold_off = img.take((size_t)m.W * 3 * g.Hp * 8);
        g.g1_off = img.take((size_t)g1_waves(g.H, g.Hp, false) * 16 * g1_ksm(g.H) * 64);
        g.g1T_off = img.take((size_t)g1_waves(g.H, g.Hp, true) * 16 * g1_ksm(g.H) * 64);
    };
    // GRU stack
    m.gru.assign(c.gru_n_layers, GruPlan());
    for (int l = 0; l < c.gru_n_layers; ++l) {
        GruPlan& g = m.gru[l];
        g.in_dim = (l == 0) ? 3 * m.F : c.gru_hid_dim;
        g.H = c.gru_hid_dim;
        g.Hp = round_up(g.H, 32);
        g.NCG = g.Hp / 32;
        g.Qx = (g.in_dim + 7) / 8;
        g.Qxp = round_up(g.Qx, 3);
        g.xmode = 0;
        g.wx_off = img.take((size_t)g.NCG * g.Qxp * 3 * 256);
        g.wh_off = img.take((size_t)g.NCG * (4 * g.NCG + 2) * 3 * 256);   // 2 zero chunks per tile: k_gru_split's ring padding
        g.b_off = img.take((size_t)4 * g.Hp);
        g.Qxp16 = round_up((g.Qx + 1) / 2, 6);       // whole turns of the bf16 weight ring (6 stages; k_gru_split: 3)
        g.wx16_off = img.take((size_t)g.NCG * g.Qxp16 * 3 * 256);
        g.wh16_off = img.take((size_t)g.NCG * (2 * g.NCG + 2) * 3 * 256);
        g.wx3_off = take_split((size_t)g.NCG * g.Qxp16 * 9 * 256);
        g.wh3_off = take_split((size_t)g.NCG * (2 * g.NCG + 2) * 6 * 256 + 3 * 256);
        g.scale_off = take_split(4);
        // layer 0 reads h_cat = [conv output (relu: unbounded) | h_feat | h_temp (sigmoids)]: the chunks that touch the
        // first F features keep three bf16 pieces; later layers read a previous layer's state, |h| <= 1
        g.qb3 = l == 0 ? std::min(g.Qxp16, round_up((m.F + 15) / 16, 2)) : 0;
        if (l == 0) g.wx2_off = take_split((size_t)g.NCG * g.Qxp16 * 6 * 256 + 3 * 256);
        g.wxq_off = take_split((size_t)g.NCG * g.Qxp16 * 6 * 256 + 3 * 256);
        gru_split(g);
        if (l == 0) {
            g.has_xproj = true;
            g.xproj.in_dim = g.in_dim; g.xproj.out_dim = 3 * g.Hp;
            g.xproj.NT = 3 * g.Hp / 32; g.xproj.Q = (g.in_dim + 7) / 8;
            g.xproj.w_off = img.take((size_t)g.xproj.NT * g.xproj.Q * 256);
            g.xproj.b_off = img.take((size_t)3 * g.Hp);
            g.xproj.Q16 = (g.in_dim + 15) / 16;
            g.xproj.w3_off = take_split((size_t)g.xproj.NT * g.xproj.Q16 * 3 * 256);
            lin_split(g.xproj);
            plan16(g);
        }
    }
    // forecasting head
    m.fc.assign(c.forecast_n_linear, LinPlan());
    for (int i = 0; i < c.forecast_n_linear; ++i) {
        LinPlan& p = m.fc[i];
        p.in_dim = (i == 0) ? c.gru_hid_dim : c.forecast_hid_dim;
        p.out_dim = (i == c.forecast_n_linear - 1) ? c.out_dim : c.forecast_hid_dim;
        p.NT = (p.out_dim + 31) / 32;
        p.Q = (p.in_dim + 7) / 8;
        p.w_off = img.take((size_t)p.NT * p.Q * 256);
        p.b_off = img.take((size_t)p.NT * 32);
    }
    // reconstruction decoder
    m.rec.assign(c.recon_n_layers, GruPlan());
    for (int l = 0; l < c.recon_n_layers; ++l) {
        GruPlan& g = m.rec[l];
        g.H = c.recon_hid_dim;
        g.Hp = round_up(g.H, 32);
        g.NCG = g.Hp / 32;
        if (l == 0) {
            // decoder input (t, j) = h_end[(t*H + j) / W]  (reference modules.py:279)
            const int Hin = c.gru_hid_dim, T = m.W;
            int nm = 1;
            for (int t = 0; t < T; ++t) {
                const int lo = (int)(((long)t * Hin) / T), hi = (int)(((long)t * Hin + Hin - 1) / T);
                if (hi - lo + 1 > nm) nm = hi - lo + 1;
            }
            g.in_dim = Hin;
            g.xmode = 1;
            g.Qx = (nm + 7) / 8;
            g.Qxp = g.Qx == 1 ? 1 : round_up(g.Qx, 3);
            g.wx_off = img.take((size_t)T * g.NCG * g.Qxp * 3 * 256);
            g.m0_off = img.take((size_t)T);
        } else {
            g.in_dim = c.recon_hid_dim;
            g.xmode = 0;
            g.Qx = (g.in_dim + 7) / 8;
            g.Qxp = round_up(g.Qx, 3);
            g.wx_off = img.take((size_t)g.NCG * g.Qxp * 3 * 256);
        }
        g.wh_off = img.take((size_t)g.NCG * (4 * g.NCG + 2) * 3 * 256);   // 2 zero chunks per tile: k_gru_split's ring padding
        g.b_off = img.take((size_t)4 * g.Hp);
        g.Qxp16 = g.xmode == 1 ? (g.Qx == 1 ? 1 : round_up((g.Qx + 1) / 2, 6)) : round_up((g.Qx + 1) / 2, 6);
        g.wx16_off = img.take((size_t)(g.xmode == 1 ? m.W : 1) * g.NCG * g.Qxp16 * 3 * 256);
        g.wh16_off = img.take((size_t)g.NCG * (2 * g.NCG + 2) * 3 * 256);
        g.wx3_off = take_split((size_t)(g.xmode == 1 ? m.W : 1) * g.NCG * g.Qxp16 * 9 * 256);
        g.wh3_off = take_split((size_t)g.NCG * (2 * g.NCG + 2) * 6 * 256 + 3 * 256);
        g.scale_off = take_split(4);
        if (g.xmode == 0) g.wxq_off = take_split((size_t)g.NCG * g.Qxp16 * 6 * 256 + 3 * 256);
        gru_split(g);
        if (l == 0) plan16(g);
    }
    {
        LinPlan& p = m.rec_fc;
        p.in_dim = c.recon_hid_dim;
        p.out_dim = c.out_dim;
        p.NT = (p.out_dim + 31) / 32;
        p.Q = m.rec.back().Hp / 8;
        p.w_off = img.take((size_t)p.NT * p.Q * 256);
        p.b_off = img.take((size_t)p.NT * 32);
        p.Q16 = (p.Q + 1) / 2;
        p.w3_off = take_split((size_t)p.NT * p.Q16 * 3 * 256);
        lin_split(p);
    }
    m.split.n_infer = (int)m.split.groups.size();

    // ---- backward (training) plans: transposed packs, un-scaled attention projections, gradient index maps
    {
        BwdPlan& b = m.bw;
        b = BwdPlan();
        auto lint = [&](LinTPlan& p, int kdim, int outdim) {
            p.in_dim = kdim; p.out_dim = outdim;
            p.NT = (outdim + 31) / 32; p.Q = (kdim + 7) / 8;
            p.w_off = img.take((size_t)p.NT * p.Q * 256);
            p.Q16 = (kdim + 15) / 16;
            p.w3_off = take_split((size_t)p.NT * p.Q16 * 3 * 256);
            lin_split(p);
        };
        auto wg = [&](WgradPlan& p, int M, int N, bool bias) {
            p.M = M; p.N = N; p.has_bias = bias;
            p.Mp = round_up(M, 32); p.Np = round_up(N + 1, 32);
            p.rowW_off = img.take((size_t)p.Mp);
            p.col_off = img.take((size_t)p.Np);
            p.rowB_off = img.take((size_t)p.Mp);
        };
        // flat gradient layout: the reference's parameters in the order of mtadgat_params
        GradLayout& gl = b.gl;
        int64_t go = 0;
        auto gtake = [&](int64_t n) { int64_t o = go; go += n; return o; };
        gl.conv_w = gtake((int64_t)m.F * m.F * m.taps); gl.conv_b = gtake(m.F);
        for (int which = 0; which < 2; ++which) {       // 0 feature, 1 temporal  (mtadgat_params order)
            const GatPlan& g = which == 0 ? m.feat : m.temp;
            const int lin_in = c.use_gatv2 ? 2 * g.D : g.D;
            gl.lin_w[which] = gtake((int64_t)g.E * lin_in); gl.lin_b[which] = gtake(g.E);
            gl.a[which] = gtake(c.use_gatv2 ? g.E : 2 * g.E); gl.bias[which] = gtake((int64_t)g.K * g.K);
        }
        gl.gru_wih.clear(); gl.gru_whh.clear(); gl.gru_bih.clear(); gl.gru_bhh.clear();
        for (int l = 0; l < c.gru_n_layers; ++l) {
            const int in = m.gru[l].in_dim, H = m.gru[l].H;
            gl.gru_wih.push_back(gtake((int64_t)3 * H * in)); gl.gru_whh.push_back(gtake((int64_t)3 * H * H));
            gl.gru_bih.push_back(gtake(3 * H)); gl.gru_bhh.push_back(gtake(3 * H));
        }
        gl.fc_w.clear(); gl.fc_b.clear();
        for (const LinPlan& p : m.fc) { gl.fc_w.push_back(gtake((int64_t)p.out_dim * p.in_dim)); gl.fc_b.push_back(gtake(p.out_dim)); }
        gl.rec_wih.clear(); gl.rec_whh.clear(); gl.rec_bih.clear(); gl.rec_bhh.clear();
        for (int l = 0; l < c.recon_n_layers; ++l) {
            const int in = m.rec[l].in_dim, H = m.rec[l].H;
            gl.rec_wih.push_back(gtake((int64_t)3 * H * in)); gl.rec_whh.push_back(gtake((int64_t)3 * H * H));
            gl.rec_bih.push_back(gtake(3 * H)); gl.rec_bhh.push_back(gtake(3 * H));
        }
        gl.rec_fc_w = gtake((int64_t)c.out_dim * c.recon_hid_dim); gl.rec_fc_b = gtake(c.out_dim);
        gl.total = go;

        // GATv2: the un-scaled projection pack (and its three bf16 pieces), its bias, `a`, the transposed pack of d V, the weight gradient
        // (round 6: the score backward's projections are a row GEMM for fused layers too)
        auto gat_wu = [&](GatBwdPlan& gb, const GatPlan& g) {
            gb.wu_off = img.take((size_t)2 * gb.NTu * g.Q * 256);
            gb.wu3_off = take_split((size_t)2 * gb.NTu * ((g.Q + 1) / 2) * 3 * 256);
            gb.split = split_group({{S::SPLIT3, 0, gb.wu_off, gb.wu3_off, 2 * gb.NTu, g.Q, (g.Q + 1) / 2}});
            gb.bu_off = img.take((size_t)2 * gb.Ep);
            gb.a_off = img.take((size_t)gb.Ep);
            lint(gb.lrT, 2 * gb.Ep, g.D);
            wg(gb.wg, 2 * gb.Ep, g.D, true);
        };
        // wide layers go through the generic kernels of mtadgat_bwdw.hip: GATv2 and (round 6) GAT v1, up to 2048 nodes / node dimensions
        b.supported = true;
        if (b.supported) {
            for (int which = 0; which < 2; ++which) {
                const GatPlan& g = which == 0 ? m.feat : m.temp;
                GatBwdPlan& gb = b.gat[which];
                gb.Ep = round_up(g.E, 32); gb.NTu = gb.Ep / 32;
                gb.wide = !g.fused;
                if (gb.wide && !c.use_gatv2) {       // GAT (v1), wide: plain parameter copies for k_gat_v1_prep / k_bw_v1 / k_gat_v1_finish
                    gb.w1_off = img.take((size_t)g.E * g.D);
                    gb.b1_off = img.take((size_t)g.E);
                    gb.a_off = img.take((size_t)2 * g.E);
                    continue;
                }
                if (gb.wide) {
                    gat_wu(gb, g);
                    continue;
                }
                gb.att_lds = gat_bwd_att_lds(g.K, g.D, g.f_vld, (g.K + 15) / 16);
                if (!c.use_gatv2) {
                    // GAT (v1): the score backward is linear in the node vectors (mtadgat_bwd.hip): plain parameter copies
                    gb.w1_off = img.take((size_t)g.E * g.D);
                    gb.b1_off = img.take((size_t)g.E);
                    gb.a_off = img.take((size_t)2 * g.E);
                    gb.pair_lds = gat_bwd_v1_lds(g.K, g.D);
                    if (gb.att_lds > 160 * 1024 || gb.pair_lds > 160 * 1024) { b.supported = false; b.why = "attention backward tiles exceed the LDS"; }
                    continue;
                }
                gat_wu(gb, g);
                if (gb.att_lds > 160 * 1024) { b.supported = false; b.why = "attention backward tiles exceed the LDS"; }
            }
            auto gru_b = [&](GruBwdPlan& gb, const GruPlan& g) {
                gb.whT_off = img.take((size_t)g.NCG * 12 * g.NCG * 256);
                gb.whT3_off = take_split((size_t)g.NCG * 6 * g.NCG * 3 * 256);
                gb.split = split_group({{S::SPLIT3, 0, gb.whT_off, gb.whT3_off, g.NCG, 12 * g.NCG, 6 * g.NCG}});
                lint(gb.wihT, 3 * g.Hp, g.in_dim);
                wg(gb.wg_ih, 3 * g.Hp, g.in_dim, true);
                wg(gb.wg_hh, 3 * g.Hp, g.H, true);
            };
            b.gru.assign(m.gru.size(), GruBwdPlan());
            b.rec.assign(m.rec.size(), GruBwdPlan());
            for (size_t l = 0; l < m.gru.size(); ++l) gru_b(b.gru[l], m.gru[l]);
            for (size_t l = 0; l < m.rec.size(); ++l) gru_b(b.rec[l], m.rec[l]);
            b.fcT.assign(m.fc.size(), LinTPlan());
            b.fc_wg.assign(m.fc.size(), WgradPlan());
            for (size_t i = 0; i < m.fc.size(); ++i) {
                lint(b.fcT[i], m.fc[i].out_dim, m.fc[i].in_dim);
                wg(b.fc_wg[i], m.fc[i].out_dim, m.fc[i].in_dim, true);
            }
            lint(b.recfcT, c.out_dim, m.rec.back().Hp);
            wg(b.recfc_wg, c.out_dim, c.recon_hid_dim, true);
            wg(b.conv_wg, m.F, m.taps * m.F, true);
            b.zero_off = img.take(1024);
        }
    }
    m.packed_floats = img.off;
    return "";
}

// ---- recurrence routes (mtadgat_host.h) -----------------------------------------------------------------------------------------
namespace {

// The split-operand kernels read 16-feature input chunks on two fp16 pieces.  Layer 0 of the GRU stack reads the convolution's
// (unbounded) output in its first qb3 chunks: those may go onto fp16 pieces only when the convolution recorded its output range --
// both kernels are launched then and the device picks (GruRoute::fallback); every other layer reads states and sigmoids, |x| <= 1.
bool gru_range_guarded(const GruPlan& g, const GruCall& c) { return c.range && g.wx2_off && g.qb3 > 0; }
bool gru_pieces_apply(const GruPlan& g, const GruCall& c) {
    if (g.xmode == 1) return g.Qxp16 == 1;                    // the decoder's folded input: one chunk per step
    return gru_range_guarded(g, c) || g.qb3 == 0;
}
// whole turns of the weight ring: of two stages (inference builds) or of the six that keep the gates (training)
bool gru_ring_turns(const GruPlan& g, int stages) { return g.Qxp16 == 1 || g.Qxp16 % stages == 0; }

// Can k_gru_cm / the split-operand build of k_gru_split serve this layer in this call?  (hidden sizes above 160, windows of more than
// 512 steps, a per-step Linear of more than 4 outputs, layer-0 packs that need the range guard without a recorded range cannot)
bool gru_split_operands_fit(const Model& m, const GruPlan& g, const GruCall& c) {
    return gru_cm_supported(g.NCG, g.xmode, c.fc, c.fc ? c.fc_out_dim : 0) && gru_ring_turns(g, 2) &&
           (g.xmode == 1 || (g.wxq_off != 0 && g.Qx >= 3)) && gru_pieces_apply(g, c) && c.hend_fits && m.W <= 512;
}

}  // namespace

// The small-batch fp32 recurrences (k_gru1 up to G1_MAX_WINDOWS, then k_gru16; mtadgat_gru16.hip) apply to a single-layer stack whose
// weights fit a wave's registers, up to G16_MAX_WINDOWS.  Inference in the bf16 mode uses them up to 1024 windows -- faster there
// than the bf16 build of the throughput kernels, and exact; inference in the split-operand arithmetic leaves them from
// SPLIT3_MIN_WINDOWS on where the hidden-tile-split kernel's split-operand build applies (it is the faster one there; gru_kernel = 3
// forces it at any size).  Layers the split-operand kernels cannot serve keep k_gru16 up to G16_MAX_WINDOWS.  The question is asked
// before the call's buffers are known: the range counts as recorded when the front end is fused (the convolution records it only
// there), the last-state rows as wide enough.
bool gru_stack_small(const Model& m, const std::vector<GruPlan>& stack, int64_t n, bool training) {
    if (stack.size() != 1 || !stack[0].has16) return false;
    if (m.precision == 1) return !training && n <= 1024;
    GruCall c;
    c.range = m.temp.fused && m.feat.fused;
    if (m.precision == 2 && !training && stack[0].NCG >= 2 && gru_split_operands_fit(m, stack[0], c) &&
        (m.gru_kernel == 3 || (m.gru_kernel == 0 && n >= SPLIT3_MIN_WINDOWS))) return false;
    return n <= G16_MAX_WINDOWS;
}

GruRoute gru_route(const Model& m, const std::vector<GruPlan>& stack, int layer, int64_t n, int cu, const GruCall& c) {
    const GruPlan& g = stack[layer];
    GruRoute r;
    if (layer == 0 && c.xp && gru_stack_small(m, stack, n, c.training)) {
        // input products of all steps ahead of the recurrence, register-resident weights; a per-step Linear is the caller's row GEMM
        r.first = n <= G1_MAX_WINDOWS ? GRU_WINDOW : GRU_GROUP16;
        r.hoist = true;
        return r;
    }
    r.fc_rides = c.fc;
    const bool p2 = m.precision == 2;
    const bool lds_fits = gru_split_lds_bytes(g.NCG, c.fc ? c.fc_out_dim : 0) <= GRU_SPLIT_LDS_MAX;
    const GruBuild plain = m.precision == 1 ? GRU_BF16 : GRU_F32;
    if (c.training) {
        // The hidden-tile-split kernel at every size (it is the one that keeps the gates): from SPLIT3_MIN_WINDOWS on its
        // split-operand build -- the input part in the kernel (no pre-projection GEMM on the fp32 pipe), any per-step Linear --
        // with the fp32 build behind it where layer 0's range guard may refuse; below, on fp32 packs behind the hoisted projection.
        const bool sp = p2 && g.NCG >= 2 && m.gru_kernel != 1 && n >= SPLIT3_MIN_WINDOWS && gru_ring_turns(g, 6) &&
                        gru_pieces_apply(g, c) && c.hend_fits && lds_fits;
        r.first = sp ? GRU_SPLIT_X3 : GRU_SPLIT;
        r.guarded = sp && g.xmode == 0 && g.qb3 > 0;
        r.fallback = r.guarded ? GRU_SPLIT : GRU_NONE;
        r.build = plain;
        r.split_packs = sp;
        r.hoist = !sp && c.xp && g.has_xproj && g.xmode == 0;
        return r;
    }
    // Chunk-major recurrence (k_gru_cm): 32 windows per wave, the weight stream shared by a workgroup's waves through LDS, from
    // CM_MIN_WINDOWS on.  Measured against the kernels it replaces (MSL shape, GRU layer + decoder): 12 288 windows 5.9 -> 4.0 ms,
    // 32 768: 7.3 -> 4.4, 65 536: 12.0 -> 9.1.  Between SPLIT3_MIN_WINDOWS and SPLIT3_MAX_WINDOWS the split-operand build of the
    // hidden-tile-split kernel instead (same packs, same range guard): there a 32-window wave per SIMD is a latency chain, five waves
    // per 32 windows are not.
    const bool fit = p2 && gru_split_operands_fit(m, g, c);
    const bool sp = fit && g.NCG >= 2 && (m.gru_kernel == 3 || (m.gru_kernel == 0 && n >= SPLIT3_MIN_WINDOWS && n <= SPLIT3_MAX_WINDOWS));
    const bool cm = fit && !sp && (m.gru_kernel == 2 || (m.gru_kernel == 0 && n >= CM_MIN_WINDOWS));
    // Split-bf16 operands (fp32-class results from the bf16 matrix pipe) for the tile-major kernel from 1.25 32-window groups per CU
    // on (measured: 12 320 windows 10.5 ms against 13.1 ms for the hidden-tile-split kernel at 12 288; 8 192 windows 7.4 ms there),
    // and wherever a split-operand kernel runs in front of it.
    const long groups = (long)((n + 31) / 32);
    const bool x3 = p2 && gru_ring_turns(g, 2) && (groups > 5L * cu / 4 || cm || sp);
    r.split_packs = x3;
    r.guarded = x3 && gru_range_guarded(g, c);
    // small batch: all steps' input products as one throughput GEMM, the recurrence keeps only its h part
    r.hoist = !x3 && c.xp && g.has_xproj && g.xmode == 0 && gru_xp_serves(n, cu);
    // The kernel on un-split (or three-piece) operands.  Up to two groups per CU the 32-window groups are spread over NCG waves each
    // (k_gru_split) -- k_gru needs ~2 groups per SIMD to fill the machine and leaves it mostly idle below that.  Measured on MI355X
    // (W=100, F=55, H=150, GRU + decoder): 256 windows 12.0 -> 4.9 ms, 16 k windows 12.2 -> 9.9 ms, 32 k windows 12.2 vs 19.6 (the 5
    // waves of a group land 2/1/1/1 on the SIMDs, so the split form loses once the machine is full).  Pre-projected input: only the
    // split kernel takes it.  k_gru takes two groups per wave once that still gives every SIMD a wave.
    GruKernel tail = GRU_TILE;
    if (r.hoist || (!x3 && g.NCG >= 2 && groups <= 2L * cu && lds_fits)) tail = GRU_SPLIT;
    if (tail == GRU_TILE) r.two = groups >= 8L * cu;
    r.build = x3 ? (g.NCG >= 5 ? GRU_X3_HI : GRU_X3_LO) : plain;
    if ((sp && lds_fits) || cm) {
        r.first = sp ? GRU_SPLIT_X3 : GRU_CM;
        r.fallback = r.guarded ? tail : GRU_NONE;
        if (r.fallback == GRU_NONE) { r.build = GRU_F32; r.two = false; }
    } else {
        r.first = tail;
    }
    return r;
}

GruCall gru_call_facts(const Model& m, bool decoder, int layer, int64_t n, bool training) {
    GruCall c;
    c.training = training;
    if (!decoder) {
        c.range = layer == 0 && (training || (m.temp.fused && m.feat.fused));
        c.xp = layer == 0 && (training || (m.gru[0].has_xproj && gru_xp_serves(n, XP_PLAN_CUS)));
        return c;
    }
    const bool last = layer == (int)m.rec.size() - 1;
    c.fc = last && (training ? rec_fc_rides_train(m) : m.cfg.out_dim <= 4);
    c.fc_out_dim = m.rec_fc.out_dim;
    c.xp = layer == 0 && m.rec.size() == 1 && m.rec[0].has16 && n <= G16_MAX_WINDOWS;
    return c;
}

// The forward's kernel decides the backward's: k_gru1 / k_gru16 keep the tape k_gru1_bwd / k_gru16_bwd read, every other training
// route is the hidden-tile-split kernel's, read by k_gru_bwd.  A training route's small / large answer does not depend on the
// compute-unit count -- gru_route returns from its small-batch and training branches before `cu` is read -- so any count serves.
GruBwdRoute gru_bwd_route(const Model& m, bool decoder, int layer, int64_t n) {
    const GruKernel fwd = gru_route(m, decoder ? m.rec : m.gru, layer, n, XP_PLAN_CUS, gru_call_facts(m, decoder, layer, n, true)).first;
    GruBwdRoute r;
    r.kernel = fwd == GRU_WINDOW ? GRU_BWD_WINDOW : fwd == GRU_GROUP16 ? GRU_BWD_GROUP16 : GRU_BWD_SPLIT;
    // default arithmetic: three bf16 pieces per operand (split on first use after an upload)
    r.x3 = r.split_pack = r.kernel == GRU_BWD_SPLIT && m.precision == 2 && (decoder ? m.bw.rec : m.bw.gru)[layer].whT3_off != 0;
    return r;
}

// The one rule "this row GEMM takes split-bf16 operands": the split-operand arithmetic (mode 2) from 65 536 rows on (below that the
// product is a few tens of microseconds either way and the pack would be re-split after every optimizer step for nothing);
// "rowgemm_kernel" = 1 keeps the fp32 MFMA, 2 takes the split pack at any size.  The forward and the backward sites differ and
// always have: rowgemm_kernel = 2 forces the split pack in the backward (data gradients, the GATv2 score backward's projection)
// whatever the precision mode, in the forward (attention projections, hoisted GRU input, recon_model.fc) only in mode 2.
bool rowgemm_split(const Model& m, bool has_pack, int64_t rows, bool backward) {
    if (!has_pack) return false;
    if (backward) return (m.precision == 2 && m.rowgemm_kernel != 1 && rows >= 65536) || m.rowgemm_kernel == 2;
    return m.precision == 2 && m.rowgemm_kernel != 1 && (rows >= 65536 || m.rowgemm_kernel == 2);
}

namespace {

// One attention layer.  att: the softmax rows are kept (training forward, attention maps); range: the convolution recorded its
// output range for this call; scols: the node columns of the rows the fused kernel stages.
FrontLayerRoute front_layer(const Model& m, const GatPlan& g, int64_t n, const FrontCall& c, int prec, bool split_front, bool att,
                            bool range) {
    FrontLayerRoute r;
    if (!g.fused) {
        r.kernel = (g.K <= 512 && g.D <= 512) ? LAYER_WIDE : LAYER_ATTEND;
        // wide layers: three bf16 pieces per operand for the projection's row GEMM
        if (prec == 2 && rowgemm_split(m, g.uw3_off && g.uQ16 > 0, n * g.K, false)) { r.build = FRONT_X3; r.split_pack = true; }
        return r;
    }
    r.kernel = LAYER_GAT;
    if (prec == 1 && !att && !(split_front && range)) {
        r.build = FRONT_BF16;            // bf16 operand build of the projection (inference)
    } else if ((prec == 2 || (split_front && !att)) && (n >= 4096 || (m.gat_kernel == 3 && !att))) {
        // large batches: split-bf16 operands for the projection -- fp32-class L' / R' on the bf16 matrix pipe, which runs beside the
        // pair grid of the other waves (the fp32 MFMA does not: profiles/r02_mfma_valu_overlap.txt).  Measured at (W=100, F=55):
        // feature layer 5.90 -> 5.09 ms, temporal layer 7.40 -> 6.94 ms (two weight chunks in registers; with four the temporal
        // layer's larger pair-grid block spilled and lost)
        r.build = FRONT_X3;
        r.split_pack = true;
        // k_gath, the fp16-piece build of the row-split kernel (node vectors split once per window), serves the two-fp16-piece
        // arithmetic: node values below 2^15, decided on the device from the recorded range -- of its launch and k_gat's behind it
        // exactly one does the work.  The training forward takes it from 4096 windows as well: it keeps the softmax rows and
        // applies the dropout.
        if (range && (!att || n >= 4096) && (m.gat_kernel == 0 || m.gat_kernel == 3) && g.fh_lds_bytes <= 160 * 1024 &&
            c.rows_aligned && c.ldv_fits)
            r.kernel = LAYER_GATH;
        // Without k_gath in front k_gat would take the fp16 pieces itself -- but a GATv2 layer's fp16-piece pack is in k_gath's
        // compact column order (launch_split2h_gath), not the 8-padded one k_gat's tiles walk: there k_gat keeps the bf16 pieces.
        r.fp16 = r.kernel == LAYER_GATH || !m.cfg.use_gatv2;
    }
    return r;
}

}  // namespace

// The front end of one call: window convolution, temporal layer, feature layer.
FrontRoute front_route(const Model& m, int64_t n, const FrontCall& c) {
    FrontRoute r;
    const bool both_fused = m.temp.fused && m.feat.fused;
    const FrontKind kind = (c.kind == FRONT_FORWARD && !both_fused) ? FRONT_FORWARD_UNFUSED : c.kind;
    const int prec = kind == FRONT_ATTENTION ? 0 : m.precision;      // the maps come from the fp32 builds that keep the softmax rows
    const bool att = kind == FRONT_TRAIN || kind == FRONT_ATTENTION;
    const bool x_bf16 = c.source == SRC_WINDOWS_BF16;
    r.range = kind == FRONT_FORWARD || kind == FRONT_TRAIN;
    // The batch sizes / options at which the fused front end's convolution is the window-per-workgroup kernel on fp16 pieces.  The
    // bf16 operand mode takes the same front end from 4096 windows: its fp16-piece kernels are faster than the bf16 builds of
    // k_conv_lds / k_gat, 10.5 against 12.3 ms per 65 536 windows, and closer to the fp32 results; the recurrences stay bf16.
    const bool split_front = prec == 1 && n >= 4096 && m.conv_kernel == 0 && m.gat_kernel == 0;
    const bool win_selected = (prec == 2 || split_front) && m.conv_kernel != 1 && (n >= 4096 || m.conv_kernel == 2);
    const bool win = kind == FRONT_FORWARD && win_selected && conv_win_fits(m.W, m.F, m.Fp16, m.taps, m.pad, m.convNT, m.Dp);
    if (kind != FRONT_CONV) {
        r.temp = front_layer(m, m.temp, n, c, prec, split_front, att, r.range);
        r.feat = front_layer(m, m.feat, n, c, prec, split_front, att, r.range);
    }
    // Shared rows, for stride-1 windows of a series (run_conv_shared) where the LDS-staged kernel applies (it records the range;
    // its bf16 build writes h_cat only).  Not where the window-per-workgroup kernel runs: that reads its window out of the series
    // itself (the rows it re-reads are L2 hits) and is the faster of the two; taking it also keeps forward_series == forward on
    // the stacked windows bit for bit.  "conv_shared" = 1 keeps the shared rows there.
    if (kind == FRONT_FORWARD && c.source == SRC_SERIES_UNIT && n >= 1024 && prec != 1 && !(win && m.conv_shared != 1) &&
        m.taps == 2 * m.pad + 1 && m.pad >= 1 && m.W >= 4 * m.pad && conv_lds_staged(m.taps, m.Fp)) {
        r.conv = CONV_SHARED;
        return r;
    }
    // Inside the temporal layer's k_gath workgroup: wherever k_conv_win is selected, k_gath runs and the staged input fits its
    // L' / R' region -- no convolution launch, h_cat[:, :F] is written once and not read back by that layer.
    if (kind == FRONT_FORWARD && m.conv_fused != 1 && win_selected && r.temp.kernel == LAYER_GATH && c.hcat_aligned &&
        gath_conv_fits(m.W, m.F, m.Fp16, m.taps, m.pad, m.convNT, m.Dp, m.temp.f_nw, m.temp.K, m.temp.D, m.temp.fh_lr)) {
        r.conv = CONV_IN_GATH;
        r.conv_split_pack = true;
        return r;
    }
    if (win) {
        r.conv = CONV_WIN;
        r.conv_split_pack = true;
        return r;
    }
    r.conv = CONV_LAUNCH;
    const bool h_cat_only = kind == FRONT_FORWARD || kind == FRONT_CONV;      // (mtadgat_conv's y counts: one plain output)
    if (prec == 1 && h_cat_only && conv_lds_staged(m.taps, m.Fp16) && !(kind == FRONT_FORWARD && win_selected)) {
        r.conv_build = FRONT_BF16;       // bf16 operand build: where the LDS-staged kernel applies
    } else if (prec == 2 && !x_bf16 && m.conv_kernel != 1 && (n * m.W >= 65536 || m.conv_kernel == 2) && !conv_lds_staged(m.taps, m.Fp)) {
        // wide models (rows too long for the LDS-staged kernels): the straight-from-memory kernel on three bf16 pieces per operand.
        // (Split operands were tried for the LDS-staged convolution as well: 3.36 vs 3.37 ms at the flagship shape -- it is bound
        // by its staging and stores, not by the matrix pipe; the fp32 MFMA build stays.)
        r.conv_build = FRONT_X3;
        r.conv_split_pack = true;
    }
    return r;
}

void plan_workspace(const Model& m, int64_t n, Workspace& ws) {
    Carver cv;
    const size_t N = (size_t)n;
    // un-fused path intermediates (also used by the stage entry point mtadgat_gat, which copies its input
    // into xc / xcT): the projected L'/R'^T only exist when a layer's tiles do not fit in LDS
    const bool both_fused = m.temp.fused && m.feat.fused;
    const size_t xc_n = N * m.W * m.Fp, xct_n = N * m.F * m.Wp;
    if (!both_fused) {
        ws.xc = cv.take(xc_n);
        ws.xct = cv.take(xct_n);
    }
    ws.lct = cv.take(m.temp.fused ? 0 : N * m.W * m.temp.ldl);
    ws.rtt = cv.take(m.temp.fused ? 0 : N * m.temp.rt_rows * m.temp.Kp);
    ws.lcf = cv.take(m.feat.fused ? 0 : N * m.F * m.feat.ldl);
    ws.rtf = cv.take(m.feat.fused ? 0 : N * m.feat.rt_rows * m.feat.Kp);
    if (both_fused) {
        // forward() never materialises xc / xc^T then; the stage entry point mtadgat_gat stages its input
        // there, and does not use h_cat: the two share the space
        const size_t hc = N * m.W * m.Dp;
        ws.hcat = cv.take(std::max(hc, align64(xc_n) + xct_n));
        ws.xc = ws.hcat;
        ws.xct = ws.hcat + align64(xc_n);
    } else {
        ws.hcat = cv.take(N * m.W * m.Dp);
    }
    ws.hend = cv.take(N * m.gru.back().Hp);
    const bool gseq = m.gru.size() > 1;
    ws.seq0 = cv.take(gseq ? N * m.W * m.gru[0].Hp : 0);
    ws.seq1 = cv.take(m.gru.size() > 2 ? N * m.W * m.gru[0].Hp : 0);
    size_t fcw = 0;
    for (const LinPlan& p : m.fc) fcw = std::max(fcw, (size_t)p.NT * 32);
    ws.fc0 = cv.take(N * fcw);
    ws.fc1 = cv.take(N * fcw);
    // decoder state sequences: between stacked decoder layers, and -- when the per-step Linear has more than a
    // few outputs -- of the last layer, so that recon_model.fc runs as one row GEMM after the recurrence
    const bool rec16 = m.rec.size() == 1 && m.rec[0].has16 && n <= G16_MAX_WINDOWS;
    ws.rec16 = rec16;
    const bool rseq = m.rec.size() > 1 || m.cfg.out_dim > 4 || rec16;
    ws.rseq0 = cv.take(rseq ? N * m.W * m.rec[0].Hp : 0);
    ws.rseq1 = cv.take((m.rec.size() > 2 || (m.rec.size() > 1 && m.cfg.out_dim > 4)) ? N * m.W * m.rec[0].Hp : 0);
    ws.has_xp = m.gru[0].has_xproj && gru_xp_serves(n, XP_PLAN_CUS);
    ws.xp = cv.take((ws.has_xp || rec16) ? N * m.W * 3 * std::max(m.gru[0].Hp, m.rec[0].Hp) : 0);
    ws.vmax = cv.take(64);
    ws.winflag = cv.take(both_fused ? (N + 3) / 4 + 16 : 0);
    // series path with stride-1 windows: the convolution of the segment (n + W - 1 rows) and of the windows' edge rows
    ws.cf = cv.take(both_fused ? (N + m.W) * m.Fp : 0);
    ws.el = cv.take(both_fused ? N * 2 * m.pad * m.Fp : 0);
    ws.er = cv.take(both_fused ? N * 2 * m.pad * m.Fp : 0);
    size_t kk = 0;       // layers beyond k_gat_wide (more than 512 nodes / node dimensions) run through a score matrix, one at a time
    for (const GatPlan* g : {&m.feat, &m.temp})
        if (!g->fused && (g->K > 512 || g->D > 512)) kk = std::max(kk, (size_t)g->K * g->K);
    ws.sc = cv.take(N * kk);
    ws.total = cv.off;
}

// How forward() walks a call of `batch` windows: chunks of at most m.chunk windows one after the other (each planned for its own
// size: a short last chunk gets the small-batch kernels and their buffers), and -- fused front end, split-operand arithmetic --
// a chunk in PIECES that alternate between two lanes (the caller's stream and the handle's own), each lane with its own
// workspace.  Why: the large-batch recurrence (k_gru_cm) is a 100-step latency chain on one 4-wave workgroup per 128 windows
// and per CU, so its time is the same for any chunk up to 32 768 windows and doubles at 32 769; and while it runs it owns the
// register file but not the vector ALU.  Two lanes let one piece's convolution / attention fill the other's recurrence:
// measured (MSL shape, profiles/r04_overlap_experiment.txt) 10 240 windows 6.0 -> 5.4 ms, 12 288: 6.3 -> 5.7, 36 864:
// 15.9 -> 12.4, 40 960: 16.7 -> 14.1, 49 152: 18.0 -> 16.4; no gain at 16 384 .. 32 768 (one piece) and at whole multiples of
// 32 768.  The pieces' results are those of forward() called on each piece (the kernels are chosen by the piece's size).
ForwardPlan plan_forward(const Model& m, int64_t batch) {
    ForwardPlan p;
    const char* hook = getenv("MTADGAT_PIECES");                                           // measurement hook: "a,b,c": piece sizes, alternating lanes
    const bool both_fused = m.temp.fused && m.feat.fused;
    const bool two = m.lanes == 0 && m.precision == 2 && both_fused;
    // Round 6: models on the un-fused (wide) attention path walk a call of several chunks with the chunks ALTERNATING between the
    // lanes.  Their chunks are a few hundred windows (projections through HBM: ~7 MB of scratch per window at F = 512, W = 256), so the
    // recurrences of a chunk are small-batch latency chains on a quarter of the CUs (896 windows: ~56 workgroups; GRU layer + decoder
    // 68.7 of config 4's 273 ms in round 5, strictly behind the chunk's front end) -- on the other lane the next chunk's convolution,
    // projections and attention fill the rest of the machine meanwhile.  Each lane has its own workspace (lane_floats).
    const bool alt = m.lanes == 0 && !both_fused && batch > m.chunk && !hook;
    if (alt) {
        // the first piece is HALF a chunk: with equal pieces the lanes run in lock step (both front ends side by side, then both
        // recurrences on 2 x 56 CUs: 258 vs 268 ms for one lane); offset by half a chunk, one lane's recurrences sit under the other's
        // front end
        int64_t c0 = 0, ci = 0;
        const int64_t half = std::max<int64_t>(32, m.chunk / 2 / 32 * 32);
        while (c0 < batch) {
            const int64_t n = std::min<int64_t>(ci == 0 ? half : m.chunk, batch - c0);
            p.pieces.push_back({c0, n, (int)(ci & 1)});
            c0 += n; ++ci;
        }
    }
    for (int64_t c0 = 0; !alt && c0 < batch; c0 += m.chunk) {
        const int64_t n = std::min<int64_t>(m.chunk, batch - c0);
        int64_t k = 1, base = n;
        if (two && n > SPLIT3_MAX_WINDOWS && n <= 2 * SPLIT3_MAX_WINDOWS) {                // two halves for the hidden-tile-split kernel
            k = 2;
            base = n / 2 / 32 * 32;                                                        // (whole 32-window groups, the last piece takes the rest)
            // a short tail rides beside a full piece instead (9 216 windows: 5.15 -> 4.77 ms; from 10 240 on the halves are as fast)
            if (n - SPLIT3_MAX_WINDOWS <= 1536) base = SPLIT3_MAX_WINDOWS;
        } else if (two && n > 32768 && n % 32768 != 0) {                                   // full k_gru_cm rounds (256 workgroups of 128 windows), then the rest
            // (whole multiples of 32 768 gain nothing from the second lane -- every round is full -- and stay one piece on the caller's stream)
            k = (n + 32767) / 32768;
            base = 32768;
        }
        if (hook) {
            int64_t at = 0;
            int lane = 0;
            for (const char* q = hook; *q && at < n;) {
                int64_t len = std::min<int64_t>(n - at, strtoll(q, const_cast<char**>(&q), 10));
                if (*q == ',') ++q;
                if (len <= 0) break;
                p.pieces.push_back({c0 + at, len, lane});
                lane ^= 1; at += len;
            }
            if (at < n) p.pieces.push_back({c0 + at, n - at, lane});
            continue;
        }
        for (int64_t i = 0, at = 0; i < k; ++i) {
            const int64_t len = i + 1 < k ? base : n - at;
            p.pieces.push_back({c0 + at, len, (int)(i & 1)});
            at += len;
        }
    }
    // workspace: per lane the largest plan of the pieces it runs; lane 1 starts behind lane 0 (ForwardPlan::lane_offset)
    Workspace o;
    int64_t seen[2][2] = {{0, 0}, {0, 0}};                    // (plans repeat: sizes seen last per lane)
    for (const ForwardPiece& pc : p.pieces) {
        p.second = p.second || pc.lane == 1;
        if (pc.n == seen[pc.lane][0] || pc.n == seen[pc.lane][1]) continue;
        seen[pc.lane][1] = seen[pc.lane][0]; seen[pc.lane][0] = pc.n;
        plan_workspace(m, pc.n, o);
        p.lane_floats[pc.lane] = std::max(p.lane_floats[pc.lane], o.total);
    }
    plan_workspace(m, std::min<int64_t>(batch, m.chunk), o);  // (the stage entry points plan one chunk on one lane)
    p.total_floats = std::max(p.lane_floats[0] + p.lane_floats[1], o.total);
    // Small calls (the reference Predictor's 256 windows, prediction.py:31): no launch fills the machine, the forward is a chain of
    // latencies -- so the stages that do not depend on each other run side by side: the feature layer next to the temporal one
    // (both read the convolution, mtad_gat.py:68-69), the forecasting head next to the reconstruction decoder (both read h_end,
    // mtad_gat.py:76-77).  Same kernels, same results; the second stream joins before the call returns.
    // (large calls gain nothing from it: with the convolution as its own launch and both attention layers side by side, 65 536
    // windows take 21.0-21.2 ms against 21.1-21.3 one after the other -- the layers compete for the same vector ALUs)
    p.fork = !p.second && p.pieces.size() == 1 && m.lanes == 0 && p.pieces[0].n <= FORK_MAX_WINDOWS && both_fused;
    return p;
}

// Default chunk of a new handle: up to 65 536 windows, fewer when a window needs a lot of scratch (wide models on the
// un-fused attention path: ~8 MB per window at F=512, W=256), so that the workspace stays within a
// quarter of the device memory (device_bytes; 0 = no device can be queried: within 16 GB)
int64_t default_chunk(const Model& m, double device_bytes) {
    Workspace o;
    plan_workspace(m, 65536, o);       // large batches: without the small-batch extras (pre-projected inputs, decoder states)
    const double per_window = (double)o.total * sizeof(float) / 65536.0;
    double budget = device_bytes > 0 ? device_bytes / 4 : 16.0 * 1024 * 1024 * 1024;
    const bool unfused = !(m.temp.fused && m.feat.fused);
    if (unfused) budget = std::min(budget, 6.0 * 1024 * 1024 * 1024);   // projections through HBM: a few hundred windows fill the machine
    int64_t c = (int64_t)(budget / per_window);
    // (more than 512 features: score matrices of up to 16 MB and projections of up to 4 096 columns per window, ~70 MB of
    // scratch per window at F = 2048, W = 512 -- fewer than 128 windows fit the budget)
    const int64_t gran = unfused ? (m.F > 512 ? 8 : 128) : 2048;
    c = c / gran * gran;
    return c < gran ? gran : (c > 65536 ? 65536 : c);
}

int wgrad_slabs(long R, int Mp, int Np) {
    // 128 x 128 output blocks (one workgroup of 4 waves each); enough row slabs for ~4 workgroups per CU
    const long tiles = (long)((Mp + 127) / 128) * ((Np + 127) / 128);
    long s = 1024 / (tiles > 0 ? tiles : 1);
    // ... of at least MTADGAT_WGRAD_ROWS rows.  Measured (SMD shape, ms per training step at 256 / 1 024 / 8 192 windows): 128 rows
    // 2.84 / 7.79 / 33.5, 384 rows 2.80 / 6.91 / 33.6, 768 rows 3.16 / 7.12 / 34.0, 1 536 rows 3.99 / 8.49 / 34.2 -- a workgroup walks
    // its rows serially (a latency chain of staged 16-row steps), so short slabs win until the partial blocks (Mp x Np floats per
    // slab, written here and read back by k_wgrad_reduce) cost more than the parallelism buys
    static const long min_rows = getenv("MTADGAT_WGRAD_ROWS") ? atol(getenv("MTADGAT_WGRAD_ROWS")) : 384;
    const long rmax = (R + min_rows - 1) / min_rows;
    if (s > rmax) s = rmax;
    if (s > 512) s = 512;
    if (s >= 8) s = s / 8 * 8;                 // whole groups of 8 slabs: the kernel's XCD-aware block map (k_wgrad_lds)
    return (int)(s < 1 ? 1 : s);
}

WgradSlabPlan wgrad_slab_plan(const Model& m, long R, int Mp, int Np) {
    WgradSlabPlan p;
    p.nslab = wgrad_slabs(R, Mp, Np);
    long rps = (R + p.nslab - 1) / p.nslab;
    rps = (rps + 15) / 16 * 16;
    p.rows_per_slab = rps;
    // default fp32 arithmetic: the products from three bf16 pieces per operand (the fp32 MFMA is 2.7x the matrix time)
    p.x3 = (m.precision == 2 && m.wgrad_kernel != 1) || m.wgrad_kernel == 2;
    return p;
}

void plan_tape(const Model& m, int64_t n, Tape& t) {
    Carver cv;
    const size_t N = (size_t)n;
    const GruPlan& g = m.gru[0];
    const GruPlan& r = m.rec[0];
    t.hcat = cv.take(N * m.W * m.Dp);
    t.xct = cv.take(N * m.F * m.Wp);
    t.att_f = cv.take(N * m.F * m.F);
    t.att_t = cv.take(N * m.W * m.W);
    t.hend = cv.take(N * g.Hp);
    // layer 0 of each stack first, the layers above (the dropped-out states below them, their gates, their states) at the end
    t.gru.assign(m.gru.size(), TapeLayer{});
    t.rec.assign(m.rec.size(), TapeLayer{});
    t.gru[0].gates = cv.take(N * m.W * 4 * g.Hp);
    t.gru[0].seq = cv.take(N * m.W * g.Hp);
    t.rec[0].gates = cv.take(N * m.W * 4 * r.Hp);
    t.rec[0].seq = cv.take(N * m.W * r.Hp);
    t.xdec = cv.take(N * m.W * g.Hp);
    t.xp = cv.take(N * m.W * 3 * std::max(g.Hp, r.Hp));
    t.fc_act.clear();
    for (size_t i = 0; i + 1 < m.fc.size(); ++i) t.fc_act.push_back(cv.take(N * (size_t)m.fc[i].NT * 32));
    t.vmax = cv.take(64);
    t.lct = cv.take(m.temp.fused ? 0 : N * m.W * m.temp.ldl);
    t.rtt = cv.take(m.temp.fused ? 0 : N * m.temp.rt_rows * m.temp.Kp);
    t.lcf = cv.take(m.feat.fused ? 0 : N * m.F * m.feat.ldl);
    t.rtf = cv.take(m.feat.fused ? 0 : N * m.feat.rt_rows * m.feat.Kp);
    auto upper = [&](const std::vector<GruPlan>& stack, std::vector<TapeLayer>& tl) {
        for (size_t l = 1; l < stack.size(); ++l) {
            tl[l - 1].drop = cv.take(N * m.W * stack[l - 1].Hp);
            tl[l].gates = cv.take(N * m.W * 4 * stack[l].Hp);
            tl[l].seq = cv.take(N * m.W * stack[l].Hp);
        }
    };
    upper(m.gru, t.gru);
    upper(m.rec, t.rec);
    t.total = cv.off;
}

void plan_bwd_workspace(const Model& m, int64_t n, BwdWorkspace& w) {
    Carver cv;
    const size_t N = (size_t)n;
    const GruPlan& g = m.gru[0];
    const GruPlan& r = m.rec[0];
    const BwdPlan& b = m.bw;
    size_t hpmax = std::max(g.Hp, r.Hp);
    for (const GruPlan& q : m.gru) hpmax = std::max(hpmax, (size_t)q.Hp);
    for (const GruPlan& q : m.rec) hpmax = std::max(hpmax, (size_t)q.Hp);
    w.da = cv.take(N * m.W * 4 * hpmax);
    w.dhcat = cv.take(N * m.W * m.Dp);
    w.dhdec = cv.take(N * m.W * hpmax);
    w.dhend = cv.take(N * g.Hp);
    size_t fcw = 32;
    for (const LinPlan& p : m.fc) fcw = std::max(fcw, (size_t)std::max(p.NT * 32, round_up(p.in_dim, 32)));
    w.dz0 = cv.take(N * fcw);
    w.dz1 = cv.take(N * fcw);
    w.de_f = cv.take(N * m.F * m.F);
    w.de_t = cv.take(N * m.W * m.W);
    w.dv_f = cv.take(N * m.F * m.Wp);
    w.dv_t = cv.take(N * m.W * m.Fp);
    // (GAT v1 reuses these regions for its per-window partials [sum dc_i v_i | sum dd_j v_j | sc sd]: 2 D + 2 floats per window)
    w.dlr_f = cv.take(std::max(N * m.F * 2 * b.gat[0].Ep, m.cfg.use_gatv2 ? (size_t)0 : N * (2 * (size_t)m.W + 2)));
    w.dlr_t = cv.take(std::max(N * m.W * 2 * b.gat[1].Ep, m.cfg.use_gatv2 ? (size_t)0 : N * (2 * (size_t)m.F + 2)));
    w.dap_f = cv.take(N * b.gat[0].Ep);
    w.dap_t = cv.take(N * b.gat[1].Ep);
    w.dpre = cv.take(N * m.W * m.Fp);
    {   // wide attention layers (mtadgat_bwdw.hip), one layer at a time
        size_t ds = 0, lr = 0;
        for (int which = 0; which < 2; ++which) {
            const GatPlan& gp = which == 0 ? m.feat : m.temp;
            // (round 6: the un-scaled projections [L | R] go through memory for EVERY GATv2 layer -- the one-pass score backward
            // k_bw_pair serves the fused layers too)
            if (m.cfg.use_gatv2 || b.gat[which].wide) lr = std::max(lr, N * gp.K * 2 * (size_t)b.gat[which].Ep);
            if (!b.gat[which].wide) continue;
            ds = std::max(ds, N * gp.K * (size_t)round_up(gp.D, 4));
        }
        w.wds = cv.take(ds); w.wlr = cv.take(lr);          // (no transposed copy of d e since round 6: the score backward is one pass)
    }
    // partial sums of the weight-gradient GEMMs: one region each (round 6), so that their reductions can wait for ONE batched launch
    // at the end of the backward (the GEMMs used to share a region, each followed by its own reduction launch: twelve per step)
    size_t wp = 0;
    auto need = [&](const WgradPlan& p, long R) { wp += align64((size_t)wgrad_slabs(R, p.Mp, p.Np) * p.Mp * p.Np); };
    const long RW = (long)n * m.W;
    need(b.conv_wg, RW);
    if (m.cfg.use_gatv2) {
        need(b.gat[0].wg, (long)n * m.F);
        need(b.gat[1].wg, RW);
    }
    for (const GruBwdPlan& gp : b.gru) { need(gp.wg_ih, RW); need(gp.wg_hh, RW); }
    for (const GruBwdPlan& gp : b.rec) { need(gp.wg_ih, RW); need(gp.wg_hh, RW); }
    need(b.recfc_wg, RW);
    for (const WgradPlan& p : b.fc_wg) need(p, (long)n);
    w.wpart_floats = wp;
    w.wpart = cv.take(wp);
    const size_t pv = 2 * (size_t)std::max(m.F, m.W) + 2;             // GAT (v1): per-window partials [p1 | p2 | sc sd]
    w.v1s = cv.take(4 * pv);
    const size_t smax = std::max(std::max((size_t)m.W * m.W, pv), std::max((size_t)m.F * m.F, (size_t)std::max(b.gat[0].Ep, b.gat[1].Ep)));
    w.sums = cv.take(sum_rows_scratch(n, (int)smax));
    for (int which = 0; which < 2; ++which) {
        const size_t K = which == 0 ? (size_t)m.F : (size_t)m.W;
        w.sums_q[2 * which] = m.cfg.use_gatv2 ? cv.take(sum_rows_scratch(n, (int)(K * K))) : 0;
        w.sums_q[2 * which + 1] = m.cfg.use_gatv2 ? cv.take(sum_rows_scratch(n, b.gat[which].Ep)) : 0;
    }
    w.total = cv.off;
}

// mean mode: at most 2^26 floats (256 MB) of per-window maps per chunk (MSL's temporal layer: 6 710 windows of 100 x 100)
static constexpr int64_t ATT_MAPS_FLOATS = int64_t(1) << 26;
void plan_attention(const Model& m, int64_t batch, bool reduce, AttPlan& p) {
    Carver cv;
    const int64_t kk = std::max<int64_t>((int64_t)m.F * m.F, (int64_t)m.W * m.W);
    p.chunk = reduce ? std::min<int64_t>(m.chunk, std::max<int64_t>(1, ATT_MAPS_FLOATS / kk)) : m.chunk;
    const int64_t n = std::min<int64_t>(batch, p.chunk);
    const size_t N = (size_t)n;
    p.hcat = cv.take(N * m.W * m.Dp);
    p.xct = cv.take(m.feat.fused ? 0 : N * m.F * m.Wp);
    p.lct = cv.take(m.temp.fused ? 0 : N * m.W * m.temp.ldl);
    p.rtt = cv.take(m.temp.fused ? 0 : N * m.temp.rt_rows * m.temp.Kp);
    p.lcf = cv.take(m.feat.fused ? 0 : N * m.F * m.feat.ldl);
    p.rtf = cv.take(m.feat.fused ? 0 : N * m.feat.rt_rows * m.feat.Kp);
    p.slabs_f = reduce ? att_mean_slabs(n, m.F) : 0;
    p.slabs_t = reduce ? att_mean_slabs(n, m.W) : 0;
    p.maps = cv.take(reduce ? N * (size_t)kk : 0);
    p.ps_f = cv.take((size_t)p.slabs_f * m.F * m.F);
    p.pc_f = cv.take((size_t)p.slabs_f * m.F * m.F);
    p.ps_t = cv.take((size_t)p.slabs_t * m.W * m.W);
    p.pc_t = cv.take((size_t)p.slabs_t * m.W * m.W);
    p.total = cv.off;
}

// At most 2^26 floats of reconstructions per chunk, the bound of the attention mean's maps (MSL: 12 201 windows of 100 x 55), in whole
// 128-window workgroups of the large-batch recurrence where a chunk holds several.  The regions do not grow with batch beyond a chunk.
void plan_losses(const Model& m, int64_t batch, LossPlan& p, bool masked) {
    const int64_t per_window = (int64_t)m.W * m.cfg.out_dim;
    p.chunk = std::min<int64_t>(m.chunk, std::max<int64_t>(1, ATT_MAPS_FLOATS / per_window));
    if (p.chunk > 128) p.chunk = p.chunk / 128 * 128;
    const int64_t n = std::min<int64_t>(batch, p.chunk), rest = batch % p.chunk;
    p.fwd_floats = plan_forward(m, n).total_floats;
    if (batch > p.chunk && rest) p.fwd_floats = std::max(p.fwd_floats, plan_forward(m, rest).total_floats);
    Carver cv;
    cv.take(p.fwd_floats);
    p.preds = cv.take((size_t)n * m.cfg.out_dim);
    p.recons = cv.take((size_t)n * per_window);
    p.scratch_bytes = masked ? mtadgat_fit_masked_sse_scratch(n, m.cfg.out_dim) : mtadgat_eval_window_sse_scratch(n, m.cfg.out_dim);
    p.scratch = cv.take((p.scratch_bytes + sizeof(float) - 1) / sizeof(float));
    p.total = cv.off;
}

// the chunk's scratch stays below 4 GiB (MSL shape: ~2 300 windows; BASELINE config 4: ~190), and below mtadgat_chunk_windows()
static constexpr double ATTR_WS_BYTES = 4.0 * 1024 * 1024 * 1024;
void plan_attribution(const Model& m, int64_t count, int steps, AttrPlan& p) {
    const int W = m.W, F = m.F, od = m.cfg.out_dim;
    const int64_t U = count * std::max(steps, 1);
    Tape t;
    plan_tape(m, 64, t);
    BwdWorkspace w;
    plan_bwd_workspace(m, 64, w);
    const double per_window = ((double)(t.total + w.total) / 64 + 2.0 * W * F + 2.0 * (W + 1) * od + 2.0 * od) * sizeof(float);
    int64_t win = std::min<int64_t>(m.chunk, (int64_t)(ATTR_WS_BYTES / per_window));
    win = std::max<int64_t>(2, win / 2 * 2);
    p.units = std::max<int64_t>(1, std::min<int64_t>(U, win / 2));
    const size_t n = (size_t)(2 * p.units), nu = (size_t)p.units;
    Carver cv;
    p.x = cv.take(n * W * F);
    p.y = cv.take(nu * od);
    p.preds = cv.take(n * od);
    p.recons = cv.take(n * W * od);
    p.dpreds = cv.take(n * od);
    p.drecons = cv.take(n * W * od);
    p.gy = cv.take(nu * od);
    p.dx = cv.take(n * W * F);
    plan_tape(m, (int64_t)n, t);
    plan_bwd_workspace(m, (int64_t)n, w);
    p.tape_floats = t.total;
    p.bws_floats = w.total;
    p.tape = cv.take(t.total);
    p.bws = cv.take(w.total);
    p.total = cv.off;
}

// the push workspace of the streaming scorer: its own regions (rounded to 4 floats), the forward's workspace behind them
StreamWs stream_ws(const Model& m, int64_t windows) {
    const size_t od = ((size_t)windows * m.cfg.out_dim + 3) / 4 * 4;
    StreamWs w;
    w.preds = 0;
    w.last = od;
    w.starts = 2 * od;
    w.fwd = w.starts + ((size_t)windows * 2 + 3) / 4 * 4;          // (an int64 per window)
    w.total = w.fwd + plan_forward(m, windows).total_floats;
    return w;
}

// embedding columns with a'_k = (1 - alpha)/2 a_k >= 0 first (padded to a multiple of 8), then the negative ones
void gat_column_order(const float* a, int E, double alpha, std::vector<int>& colk, int& P8, int& PT, int* npos) {
    std::vector<int> pos, neg;
    for (int k = 0; k < E; ++k) (((1.0 - alpha) * 0.5 * (double)a[k]) >= 0.0 ? pos : neg).push_back(k);
    if (npos) *npos = (int)pos.size();
    P8 = round_up((int)pos.size(), 8);
    const int N8 = round_up((int)neg.size(), 8);
    PT = P8 + N8;
    colk.assign(PT, -1);
    for (size_t n = 0; n < pos.size(); ++n) colk[n] = pos[n];
    for (size_t n = 0; n < neg.size(); ++n) colk[P8 + n] = neg[n];
}

static void pack_gat(Model& m, GatPlan& g, const float* lin_w, const float* lin_b, const float* a, const float* bias,
                     std::vector<float>& out) {
    const int E = g.E, D = g.D;
    const double alpha = m.cfg.alpha;
    // projected columns: query side [0, ldl) = [L'(PT) | c | 0..], key side [ldl, 2 ldl) = [R'(PT) | d | 0..]
    const int NC = 2 * g.ldl, KS = g.ldl;
    std::vector<double> rows((size_t)NC * D, 0.0), bvec(NC, 0.0);
    if (m.cfg.use_gatv2) {
        // e_ij = a . LeakyReLU(W_l v_i + W_r v_j + b)          (reference modules.py:74-77, :174-177)
        //      = c_i + d_j + sum_k a'_k |L_ik + R_jk|,  LeakyReLU(u) = (1+alpha)/2 u + (1-alpha)/2 |u|
        const int lin_in = 2 * D;
        std::vector<int> colk;
        gat_column_order(a, E, alpha, colk, g.P8, g.PT, &g.npos);
        for (int n = 0; n < g.PT; ++n) {
            const int k = colk[n];
            if (k < 0) continue;
            const double s = std::fabs((1.0 - alpha) * 0.5 * (double)a[k]);
            for (int cidx = 0; cidx < D; ++cidx) {
                rows[(size_t)n * D + cidx] = s * (double)lin_w[(size_t)k * lin_in + cidx];
                rows[(size_t)(KS + n) * D + cidx] = s * (double)lin_w[(size_t)k * lin_in + D + cidx];
            }
            bvec[n] = s * (double)lin_b[k];
        }
        const double hl = (1.0 + alpha) * 0.5;
        for (int k = 0; k < E; ++k) {
            for (int cidx = 0; cidx < D; ++cidx) {
                rows[(size_t)(g.PT) * D + cidx] += hl * (double)a[k] * (double)lin_w[(size_t)k * lin_in + cidx];
                rows[(size_t)(KS + g.PT) * D + cidx] += hl * (double)a[k] * (double)lin_w[(size_t)k * lin_in + D + cidx];
            }
            bvec[g.PT] += hl * (double)a[k] * (double)lin_b[k];
        }
    } else {
        // e_ij = LeakyReLU(a1 . (W v_i + b) + a2 . (W v_j + b))   (reference modules.py:80-83, :180-183)
        g.PT = g.P8 = 0;
        for (int k = 0; k < E; ++k) {
            for (int cidx = 0; cidx < D; ++cidx) {
                rows[(size_t)0 * D + cidx] += (double)a[k] * (double)lin_w[(size_t)k * D + cidx];
                rows[(size_t)KS * D + cidx] += (double)a[E + k] * (double)lin_w[(size_t)k * D + cidx];
            }
            bvec[0] += (double)a[k] * (double)lin_b[k];
            bvec[KS] += (double)a[E + k] * (double)lin_b[k];
        }
    }
    pack_tiles(out.data() + g.w_off, g.NT, g.Q, [&](int n, int k) -> float {
        if (n >= NC) return 0.f;
        if (k < D) return (float)rows[(size_t)n * D + k];
        return (g.fused && k == D) ? (float)bvec[n] : 0.f;       // fused kernel: bias = weight row D
    });
    if (g.fused && m.precision == 1)
        pack_tiles_bf16(out.data() + g.w16_off, g.NT, g.Q16, [&](int n, int k) -> float {
            if (n >= NC) return 0.f;
            if (k < D) return (float)rows[(size_t)n * D + k];
            return k == D ? (float)bvec[n] : 0.f;
        });
    for (int n = 0; n < NC; ++n) out[g.b_off + n] = (float)bvec[n];
    std::memcpy(out.data() + g.bias_off, bias, sizeof(float) * (size_t)g.K * g.K);
    {   // the sign-group boundaries the kernels read (ints in the float image)
        int* ord = reinterpret_cast<int*>(out.data() + g.ord_off);
        ord[0] = g.P8; ord[1] = g.PT; ord[2] = g.npos; ord[3] = 0;
    }
}

static void pack_gru_layer(const GruPlan& g, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                           std::vector<float>& out, bool bf16) {
    const int H = g.H, in = g.in_dim;
    if (g.xmode == 0) {
        pack_gru_tiles(out.data() + g.wx_off, g.NCG, g.Qxp, [&](int st, int r, int k) -> float {
            return (r < H && k < in) ? w_ih[((size_t)st * H + r) * in + k] : 0.f;
        });
    }
    pack_gru_tiles(out.data() + g.wh_off, g.NCG, 4 * g.NCG + 2, [&](int st, int r, int k) -> float {
        return (r < H && k < H) ? w_hh[((size_t)st * H + r) * H + k] : 0.f;
    });
    if (g.xmode == 0 && bf16) {
        pack_gru_tiles_bf16(out.data() + g.wx16_off, g.NCG, g.Qxp16, [&](int st, int r, int k) -> float {
            return (r < H && k < in) ? w_ih[((size_t)st * H + r) * in + k] : 0.f;
        });
    }
    if (bf16)
        pack_gru_tiles_bf16(out.data() + g.wh16_off, g.NCG, 2 * g.NCG + 2, [&](int st, int r, int k) -> float {
            return (r < H && k < H) ? w_hh[((size_t)st * H + r) * H + k] : 0.f;
        });
    float* b = out.data() + g.b_off;
    for (int j = 0; j < g.Hp; ++j) {
        b[0 * g.Hp + j] = j < H ? b_ih[j] + b_hh[j] : 0.f;
        b[1 * g.Hp + j] = j < H ? b_ih[H + j] + b_hh[H + j] : 0.f;
        b[2 * g.Hp + j] = j < H ? b_ih[2 * H + j] : 0.f;
        b[3 * g.Hp + j] = j < H ? b_hh[2 * H + j] : 0.f;
    }
    if (g.has16) {
        float* w = out.data() + g.g16_off;
        float* wT = out.data() + g.g16T_off;
        for (int tile = 0; tile < g.NT16; ++tile)
            for (int gate = 0; gate < 3; ++gate)
                for (int s = 0; s < g.KS16; ++s)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int unit = 16 * tile + (lane & 15), k = 4 * s + (lane >> 4);
                        const bool ok = unit < H && k < H;
                        const size_t o = (((size_t)tile * 3 + gate) * g.KS16 + s) * 64 + lane;
                        w[o] = ok ? w_hh[((size_t)gate * H + unit) * H + k] : 0.f;
                        wT[o] = ok ? w_hh[((size_t)gate * H + k) * H + unit] : 0.f;
                    }
    }
    if (g.has16) {
        const int HK = 16 * g1_ksm(H), nwf = g1_waves(H, g.Hp, false), nwb = g1_waves(H, g.Hp, true), jbs = (H + 15) / 16;
        float* w = out.data() + g.g1_off;
        for (int wv = 0; wv < nwf; ++wv)
            for (int k = 0; k < HK; ++k)
                for (int lane = 0; lane < 64; ++lane) {
                    const int R = wv * 64 + lane;
                    w[((size_t)wv * HK + k) * 64 + lane] = (R < 3 * H && k < H) ? w_hh[(size_t)R * H + k] : 0.f;
                }
        float* wT = out.data() + g.g1T_off;
        for (int wv = 0; wv < nwb; ++wv)
            for (int k = 0; k < HK; ++k)
                for (int lane = 0; lane < 64; ++lane) {
                    const int rr = (wv * 64 + lane) >> 4, p = rr % 3, jb = rr / 3, j = 16 * jb + (lane & 15);
                    wT[((size_t)wv * HK + k) * 64 + lane] = (jb < jbs && j < H && k < H) ? w_hh[((size_t)p * H + k) * H + j] : 0.f;
                }
    }
    if (g.has_xproj) {
        const int Hp = g.Hp;
        pack_tiles(out.data() + g.xproj.w_off, g.xproj.NT, g.xproj.Q, [&](int n, int k) -> float {
            const int blk = n / Hp, u = n % Hp;
            return (blk < 3 && u < H && k < in) ? w_ih[((size_t)blk * H + u) * in + k] : 0.f;
        });
        std::memcpy(out.data() + g.xproj.b_off, b, sizeof(float) * 3 * Hp);
    }
}

std::string pack_weights(Model& m, const mtadgat_params& p, std::vector<float>& out) {
    const mtadgat_config& c = m.cfg;
    out.assign(m.packed_floats, 0.f);
    if (!p.conv_weight || !p.conv_bias || !p.feat_lin_weight || !p.feat_lin_bias || !p.feat_a || !p.feat_bias ||
        !p.temp_lin_weight || !p.temp_lin_bias || !p.temp_a || !p.temp_bias || !p.rec_fc_weight || !p.rec_fc_bias)
        return "null parameter pointer";
    for (int l = 0; l < c.gru_n_layers; ++l)
        if (!p.gru_w_ih[l] || !p.gru_w_hh[l] || !p.gru_b_ih[l] || !p.gru_b_hh[l]) return "null GRU parameter pointer";
    for (int i = 0; i < c.forecast_n_linear; ++i)
        if (!p.fc_weight[i] || !p.fc_bias[i]) return "null forecasting parameter pointer";
    for (int l = 0; l < c.recon_n_layers; ++l)
        if (!p.rec_w_ih[l] || !p.rec_w_hh[l] || !p.rec_b_ih[l] || !p.rec_b_hh[l]) return "null decoder parameter pointer";
    // The regions of the packed image are independent: five host threads fill them concurrently (the image is
    // re-packed after every optimizer step, so this sits on the training step's critical path).
    // conv: K index = tap*Fp + channel   (reference weight (F_out, F_in, k), modules.py:15)
    auto job_conv_feat = [&]() {
        const int F = m.F, Fp = m.Fp, taps = m.taps;
        pack_tiles(out.data() + m.conv_w_off, m.convNT, taps * Fp / 8, [&](int n, int k) -> float {
            const int tap = k / Fp, ch = k % Fp;
            return (n < F && ch < F && tap < taps) ? p.conv_weight[((size_t)n * F + ch) * taps + tap] : 0.f;
        });
        for (int n = 0; n < F; ++n) out[m.conv_b_off + n] = p.conv_bias[n];
        for (size_t k = 0; k < (size_t)F * F * taps; ++k) out[m.conv_wraw_off + k] = p.conv_weight[k];
        if (m.conv_wT_off)           // input gradient of wide windows: dx[t][i] = sum_{o,j} w[o][i][taps-1-j] dpre[t+j-pad][o] (odd taps)
            pack_tiles(out.data() + m.conv_wT_off, m.convNT, taps * Fp / 8, [&](int n, int k) -> float {
                const int tap = k / Fp, ch = k % Fp;
                return (n < F && ch < F && tap < taps) ? p.conv_weight[((size_t)ch * F + n) * taps + (taps - 1 - tap)] : 0.f;
            });
        const int Fp16 = m.Fp16;
        pack_tiles(out.data() + m.conv_wf16_off, m.convNT, taps * Fp16 / 8, [&](int n, int k) -> float {
            const int tap = k / Fp16, ch = k % Fp16;
            return (n < F && ch < F && tap < taps) ? p.conv_weight[((size_t)n * F + ch) * taps + tap] : 0.f;
        });
        if (m.precision == 1) pack_tiles_bf16(out.data() + m.conv_w16_off, m.convNT, taps * Fp16 / 16, [&](int n, int k) -> float {
            const int tap = k / Fp16, ch = k % Fp16;
            return (n < F && ch < F && tap < taps) ? p.conv_weight[((size_t)n * F + ch) * taps + tap] : 0.f;
        });
        pack_gat(m, m.feat, p.feat_lin_weight, p.feat_lin_bias, p.feat_a, p.feat_bias, out);
    };
    auto job_temp_gru = [&]() {
        pack_gat(m, m.temp, p.temp_lin_weight, p.temp_lin_bias, p.temp_a, p.temp_bias, out);
        for (int l = 0; l < c.gru_n_layers; ++l) pack_gru_layer(m.gru[l], p.gru_w_ih[l], p.gru_w_hh[l], p.gru_b_ih[l], p.gru_b_hh[l], out, m.precision == 1);
    };
    auto job_heads = [&]() {
    for (int i = 0; i < c.forecast_n_linear; ++i) {
        const LinPlan& lp = m.fc[i];
        const float* w = p.fc_weight[i];
        pack_tiles(out.data() + lp.w_off, lp.NT, lp.Q, [&](int n, int k) -> float {
            return (n < lp.out_dim && k < lp.in_dim) ? w[(size_t)n * lp.in_dim + k] : 0.f;
        });
        for (int n = 0; n < lp.out_dim; ++n) out[lp.b_off + n] = p.fc_bias[i][n];
    }
    for (int l = 0; l < c.recon_n_layers; ++l) {
        const GruPlan& g = m.rec[l];
        if (g.xmode == 1) {
            // x_t[j] = h_end[(t*Hin + j) / T]: fold W_ih over the j that share an h_end entry.  The j of one entry
            // are consecutive, so every folded weight is a difference of two prefix sums over j (double)
            const int Hin = g.in_dim, T = m.W, H = g.H;
            const int NMp = 8 * g.Qx;
            std::vector<double> pre((size_t)3 * H * (Hin + 1));
            for (int r = 0; r < 3 * H; ++r) {
                double acc = 0.0;
                pre[(size_t)r * (Hin + 1)] = 0.0;
                for (int j = 0; j < Hin; ++j) {
                    acc += (double)p.rec_w_ih[l][(size_t)r * Hin + j];
                    pre[(size_t)r * (Hin + 1) + j + 1] = acc;
                }
            }
            int* m0 = reinterpret_cast<int*>(out.data() + g.m0_off);
            std::vector<float> fw((size_t)3 * H * NMp);          // folded weights of one step: [gate*H + r][k]
            auto steps = [&](int t_lo, int t_hi, std::vector<float>& f) {
                for (int t = t_lo; t < t_hi; ++t) {
                    const int lo = (int)(((long)t * Hin) / T);
                    m0[t] = lo;
                    for (int k = 0; k < NMp; ++k) {
                        // j with (t*Hin + j) / T == lo + k:  j in [(lo+k)*T - t*Hin, (lo+k+1)*T - t*Hin)
                        long j0 = (long)(lo + k) * T - (long)t * Hin, j1 = j0 + T;
                        j0 = j0 < 0 ? 0 : j0;
                        j1 = j1 > Hin ? Hin : j1;
                        for (int r = 0; r < 3 * H; ++r)
                            f[(size_t)r * NMp + k] = j1 > j0 ? (float)(pre[(size_t)r * (Hin + 1) + j1] - pre[(size_t)r * (Hin + 1) + j0]) : 0.f;
                    }
                    auto fold = [&](int st, int r, int k) -> float { return (r < H && k < NMp) ? f[((size_t)st * H + r) * NMp + k] : 0.f; };
                    pack_gru_tiles(out.data() + g.wx_off + (size_t)t * g.NCG * g.Qxp * 3 * 256, g.NCG, g.Qxp, fold);
                    if (m.precision == 1) pack_gru_tiles_bf16(out.data() + g.wx16_off + (size_t)t * g.NCG * g.Qxp16 * 3 * 256, g.NCG, g.Qxp16, fold);
                    if (g.has16) {
                        float* fo = out.data() + g.fold_off + (size_t)t * 3 * g.Hp * 8;
                        for (int st = 0; st < 3; ++st)
                            for (int r = 0; r < H; ++r)
                                for (int k = 0; k < 8; ++k) fo[((size_t)st * g.Hp + r) * 8 + k] = f[((size_t)st * H + r) * NMp + k];
                    }
                }
            };
            std::vector<float> fw2(fw.size());
            std::thread th(steps, T / 2, T, std::ref(fw2));
            steps(0, T / 2, fw);
            th.join();
        }
        pack_gru_layer(g, p.rec_w_ih[l], p.rec_w_hh[l], p.rec_b_ih[l], p.rec_b_hh[l], out, m.precision == 1);
    }
    {
        const LinPlan& lp = m.rec_fc;
        pack_tiles(out.data() + lp.w_off, lp.NT, lp.Q, [&](int n, int k) -> float {
            return (n < lp.out_dim && k < lp.in_dim) ? p.rec_fc_weight[(size_t)n * lp.in_dim + k] : 0.f;
        });
        for (int n = 0; n < lp.out_dim; ++n) out[lp.b_off + n] = p.rec_fc_bias[n];
    }
    };

    // ---- backward packs (transposed weights, un-scaled attention projections, gradient index maps)
    auto job_bwd = [&]() {
    if (m.bw.supported) {
        const BwdPlan& b = m.bw;
        auto maps = [&](const WgradPlan& wp, auto rowW, auto col, auto rowB) {
            int* rw = reinterpret_cast<int*>(out.data() + wp.rowW_off);
            int* cm = reinterpret_cast<int*>(out.data() + wp.col_off);
            int* rb = reinterpret_cast<int*>(out.data() + wp.rowB_off);
            for (int i = 0; i < wp.Mp; ++i) { rw[i] = i < wp.M ? rowW(i) : -1; rb[i] = i < wp.M ? rowB(i) : -1; }
            for (int i = 0; i < wp.Np; ++i) cm[i] = i < wp.N ? col(i) : -1;
        };
        auto ident = [](int n) { return n; };
        for (int which = 0; which < 2; ++which) {
            const GatPlan& g = which == 0 ? m.feat : m.temp;
            const GatBwdPlan& gb = b.gat[which];
            const float* lw = which == 0 ? p.feat_lin_weight : p.temp_lin_weight;
            const float* lb = which == 0 ? p.feat_lin_bias : p.temp_lin_bias;
            const float* av = which == 0 ? p.feat_a : p.temp_a;
            const int E = g.E, D = g.D, Ep = gb.Ep;
            if (!c.use_gatv2) {
                for (size_t i = 0; i < (size_t)E * D; ++i) out[gb.w1_off + i] = lw[i];
                for (int e = 0; e < E; ++e) out[gb.b1_off + e] = lb[e];
                for (int e = 0; e < 2 * E; ++e) out[gb.a_off + e] = av[e];
                continue;
            }
            pack_tiles(out.data() + gb.wu_off, 2 * gb.NTu, g.Q, [&](int n, int k) -> float {
                const int side = n / Ep, e = n % Ep;
                if (e >= E) return 0.f;
                if (k < D) return lw[(size_t)e * 2 * D + (size_t)side * D + k];
                return (k == D && side == 0) ? lb[e] : 0.f;
            });
            for (int e = 0; e < E; ++e) out[gb.a_off + e] = av[e];
            for (int e = 0; e < E; ++e) out[gb.bu_off + e] = lb[e];      // (the row GEMM takes the projection bias as a vector)
            pack_tiles(out.data() + gb.lrT.w_off, gb.lrT.NT, gb.lrT.Q, [&](int n, int k) -> float {
                const int side = k / Ep, e = k % Ep;
                return (n < D && e < E && side < 2) ? lw[(size_t)e * 2 * D + (size_t)side * D + n] : 0.f;
            });
            maps(gb.wg, [&](int r) { const int side = r / Ep, e = r % Ep; return e < E ? e * 2 * D + side * D : -1; }, ident,
                 [&](int r) { const int side = r / Ep, e = r % Ep; return (side == 0 && e < E) ? e : -1; });
        }
        auto gru_pack = [&](const GruBwdPlan& gb, const GruPlan& g, const float* w_ih, const float* w_hh) {
            const int H = g.H, Hp = g.Hp, in = g.in_dim;
            pack_tiles(out.data() + gb.whT_off, g.NCG, 12 * g.NCG, [&](int n, int k) -> float {      // blocks r | z | nh
                const int blk = k / Hp, u = k % Hp;
                return (n < H && u < H && blk < 3) ? w_hh[((size_t)blk * H + u) * H + n] : 0.f;
            });
            auto gate_ih = [](int blk) { return blk == 0 ? 2 : blk - 1; };                            // blocks n | r | z
            pack_tiles(out.data() + gb.wihT.w_off, gb.wihT.NT, gb.wihT.Q, [&](int n, int k) -> float {
                const int blk = k / Hp, u = k % Hp;
                return (n < in && u < H && blk < 3) ? w_ih[((size_t)gate_ih(blk) * H + u) * in + n] : 0.f;
            });
            maps(gb.wg_ih, [&](int r) { const int blk = r / Hp, u = r % Hp; return u < H ? (gate_ih(blk) * H + u) * in : -1; }, ident,
                 [&](int r) { const int blk = r / Hp, u = r % Hp; return u < H ? gate_ih(blk) * H + u : -1; });
            maps(gb.wg_hh, [&](int r) { const int blk = r / Hp, u = r % Hp; return u < H ? (blk * H + u) * H : -1; }, ident,
                 [&](int r) { const int blk = r / Hp, u = r % Hp; return u < H ? blk * H + u : -1; });
        };
        for (size_t l = 0; l < m.gru.size(); ++l) gru_pack(b.gru[l], m.gru[l], p.gru_w_ih[l], p.gru_w_hh[l]);
        for (size_t l = 0; l < m.rec.size(); ++l) gru_pack(b.rec[l], m.rec[l], p.rec_w_ih[l], p.rec_w_hh[l]);
        for (size_t i = 0; i < m.fc.size(); ++i) {
            const LinPlan& lp = m.fc[i];
            const float* w = p.fc_weight[i];
            pack_tiles(out.data() + b.fcT[i].w_off, b.fcT[i].NT, b.fcT[i].Q, [&](int n, int k) -> float {
                return (n < lp.in_dim && k < lp.out_dim) ? w[(size_t)k * lp.in_dim + n] : 0.f;
            });
            maps(b.fc_wg[i], [&](int r) { return r * lp.in_dim; }, ident, ident);
        }
        {
            const int Hr = c.recon_hid_dim, od = c.out_dim;
            pack_tiles(out.data() + b.recfcT.w_off, b.recfcT.NT, b.recfcT.Q, [&](int n, int k) -> float {
                return (n < Hr && k < od) ? p.rec_fc_weight[(size_t)k * Hr + n] : 0.f;
            });
            maps(b.recfc_wg, [&](int r) { return r * Hr; }, ident, ident);
        }
        {
            const int F = m.F, taps = m.taps;
            maps(b.conv_wg, [&](int r) { return r * F * taps; }, [&](int n) { const int tap = n / F, ch = n % F; return ch * taps + tap; }, ident);
        }
    }
    };
    std::thread t1(job_conv_feat), t2(job_temp_gru), t3(job_heads);
    job_bwd();
    t1.join(); t2.join(); t3.join();
    m.bf16_packed = (m.precision == 1);
    return "";
}


// ---- device-side re-packing: host tables ---------------------------------------------------------------
FlatOffsets flat_offsets(const Model& m) {
    const mtadgat_config& c = m.cfg;
    FlatOffsets f;
    int64_t go = 0;
    auto take = [&](int64_t n) { int64_t o = go; go += n; return o; };
    f.conv_w = take((int64_t)m.F * m.F * m.taps); f.conv_b = take(m.F);
    for (int which = 0; which < 2; ++which) {
        const GatPlan& g = which == 0 ? m.feat : m.temp;
        const int lin_in = c.use_gatv2 ? 2 * g.D : g.D;
        f.lin_w[which] = take((int64_t)g.E * lin_in); f.lin_b[which] = take(g.E);
        f.a[which] = take(c.use_gatv2 ? g.E : 2 * g.E); f.bias[which] = take((int64_t)g.K * g.K);
    }
    for (int l = 0; l < c.gru_n_layers; ++l) {
        const int in = m.gru[l].in_dim, H = m.gru[l].H;
        f.gru_wih.push_back(take((int64_t)3 * H * in)); f.gru_whh.push_back(take((int64_t)3 * H * H));
        f.gru_bih.push_back(take(3 * H)); f.gru_bhh.push_back(take(3 * H));
    }
    for (const LinPlan& p : m.fc) { f.fc_w.push_back(take((int64_t)p.out_dim * p.in_dim)); f.fc_b.push_back(take(p.out_dim)); }
    for (int l = 0; l < c.recon_n_layers; ++l) {
        const int in = m.rec[l].in_dim, H = m.rec[l].H;
        f.rec_wih.push_back(take((int64_t)3 * H * in)); f.rec_whh.push_back(take((int64_t)3 * H * H));
        f.rec_bih.push_back(take(3 * H)); f.rec_bhh.push_back(take(3 * H));
    }
    f.rec_fc_w = take((int64_t)c.out_dim * c.recon_hid_dim); f.rec_fc_b = take(c.out_dim);
    f.total = go;
    return f;
}

void params_from_flat(const Model& m, const FlatOffsets& f, const float* flat, mtadgat_params& p) {
    std::memset(&p, 0, sizeof(p));
    p.conv_weight = flat + f.conv_w; p.conv_bias = flat + f.conv_b;
    p.feat_lin_weight = flat + f.lin_w[0]; p.feat_lin_bias = flat + f.lin_b[0]; p.feat_a = flat + f.a[0]; p.feat_bias = flat + f.bias[0];
    p.temp_lin_weight = flat + f.lin_w[1]; p.temp_lin_bias = flat + f.lin_b[1]; p.temp_a = flat + f.a[1]; p.temp_bias = flat + f.bias[1];
    for (size_t l = 0; l < m.gru.size(); ++l) {
        p.gru_w_ih[l] = flat + f.gru_wih[l]; p.gru_w_hh[l] = flat + f.gru_whh[l];
        p.gru_b_ih[l] = flat + f.gru_bih[l]; p.gru_b_hh[l] = flat + f.gru_bhh[l];
    }
    for (size_t i = 0; i < m.fc.size(); ++i) { p.fc_weight[i] = flat + f.fc_w[i]; p.fc_bias[i] = flat + f.fc_b[i]; }
    for (size_t l = 0; l < m.rec.size(); ++l) {
        p.rec_w_ih[l] = flat + f.rec_wih[l]; p.rec_w_hh[l] = flat + f.rec_whh[l];
        p.rec_b_ih[l] = flat + f.rec_bih[l]; p.rec_b_hh[l] = flat + f.rec_bhh[l];
    }
    p.rec_fc_weight = flat + f.rec_fc_w; p.rec_fc_bias = flat + f.rec_fc_b;
}

// The gather table is obtained from the host packer itself: it is run over parameters whose value is their flat index
// + 1 (exact in fp32 below 2^24), so every position of the image that is a plain copy of a parameter names its
// source, whatever tile format it sits in.  Regions whose content is computed (scaled / sorted / summed / folded) are
// excluded -- the kernels of mtadgat_packdev.hip fill them -- and everything else (zero padding, index maps) is left
// as the first host-side load wrote it.
std::string build_device_tables(Model& m) {
    DevTables& t = m.dt;
    if (m.precision == 1) return "device-side re-packing covers the fp32 image only";
    t.fo = flat_offsets(m);
    if (t.fo.total != m.bw.gl.total) return "internal: flat parameter layout mismatch";
    if (t.fo.total >= ((int64_t)1 << 31)) return "model too large for the index-encoded gather table";
    // fp32 holds integers exactly below 2^24 only: models of more than 2^24 parameters (F > 512) are encoded in two runs of the
    // packer, the low 22 bits of the index and the rest
    const int64_t LOW = (int64_t)1 << 22;
    const int runs = t.fo.total < ((int64_t)1 << 24) ? 1 : 2;
    std::vector<float> img[2];
    for (int r = 0; r < runs; ++r) {
        std::vector<float> synth((size_t)t.fo.total);
        for (int64_t i = 0; i < t.fo.total; ++i) synth[(size_t)i] = (float)(runs == 1 ? i + 1 : (r == 0 ? (i & (LOW - 1)) : (i >> 22)) + 1);
        mtadgat_params p;
        params_from_flat(m, t.fo, synth.data(), p);
        const int keep[4] = {m.feat.PT, m.feat.P8, m.temp.PT, m.temp.P8};
        const int keep_np[2] = {m.feat.npos, m.temp.npos};
        const bool keep_bf = m.bf16_packed;
        std::string err = pack_weights(m, p, img[r]);
        m.feat.PT = keep[0]; m.feat.P8 = keep[1]; m.temp.PT = keep[2]; m.temp.P8 = keep[3];
        m.feat.npos = keep_np[0]; m.temp.npos = keep_np[1];
        m.bf16_packed = keep_bf;
        if (!err.empty()) return err;
    }
    t.gidx.assign(m.packed_floats, -1);
    auto code = [](float v, int64_t hi) -> int64_t { return (v >= 1.f && v <= (float)hi && v == std::floor(v)) ? (int64_t)v - 1 : -1; };
    for (size_t i = 0; i < m.packed_floats; ++i) {
        if (runs == 1) {
            t.gidx[i] = (int)code(img[0][i], t.fo.total);
        } else {
            const int64_t lo = code(img[0][i], LOW), hi = code(img[1][i], (t.fo.total >> 22) + 1);
            const int64_t idx = hi * LOW + lo;
            if (lo >= 0 && hi >= 0 && idx < t.fo.total) t.gidx[i] = (int)idx;
        }
    }
    auto exclude = [&](size_t off, size_t n) { std::fill(t.gidx.begin() + off, t.gidx.begin() + off + n, -1); };
    for (int which = 0; which < 2; ++which) {
        const GatPlan& g = which == 0 ? m.feat : m.temp;
        exclude(g.w_off, (size_t)g.NT * g.Q * 256);
        exclude(g.b_off, (size_t)g.NT * 32);
        const int D = g.D, NC = 2 * g.ldl;
        t.gatcode[which].assign((size_t)g.NT * g.Q * 256, 0);
        pack_tiles(t.gatcode[which].data(), g.NT, g.Q, [&](int n, int k) -> int { return (n < NC && k <= D) ? n * (D + 1) + k + 1 : 0; });
    }
    auto gru_excl = [&](const GruPlan& g) {
        exclude(g.b_off, (size_t)4 * g.Hp);
        if (g.has_xproj) exclude(g.xproj.b_off, (size_t)3 * g.Hp);
    };
    for (const GruPlan& g : m.gru) gru_excl(g);
    for (const GruPlan& g : m.rec) gru_excl(g);
    t.foldcode.clear();
    {
        const GruPlan& g = m.rec[0];
        if (g.xmode == 1) {
            exclude(g.wx_off, (size_t)m.W * g.NCG * g.Qxp * 3 * 256);
            if (g.has16) exclude(g.fold_off, (size_t)m.W * 3 * g.Hp * 8);
            const int NMp = 8 * g.Qx, H = g.H;
            std::vector<float> code((size_t)g.NCG * g.Qxp * 3 * 256, 0.f);
            pack_gru_tiles(code.data(), g.NCG, g.Qxp, [&](int st, int r, int k) -> float {
                return (r < H && k < NMp) ? (float)(((size_t)st * H + r) * NMp + k + 1) : 0.f;
            });
            t.foldcode.assign(code.size(), 0);
            for (size_t i = 0; i < code.size(); ++i) t.foldcode[i] = (int)code[i];
        }
    }
    return "";
}

}  // namespace mtadgat
