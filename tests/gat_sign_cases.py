"""Cases and specification for the sign-sorted column order of the GATv2 attention layers (tests/test_host_gat_sign_cases.py on the
CPU, tests/test_gpu_gat_sign_order.py on the GPU).

The packers rewrite a . LeakyReLU(u) as c_i + d_j + sum_k a'_k |L_ik + R_jk| with a'_k = (1 - alpha) / 2 * a_k and sort the embedding
columns by the sign of a'_k (gat_column_order, csrc/mtadgat_pack.cpp; k_gat_colorder, csrc/mtadgat_packdev.hip).  Every attention
kernel walks that order; the shapes and sign patterns below put its group boundaries where the walks degenerate: an empty group, a
group of one column, a boundary on a tile edge, the c / d column opening a 32-column part of its own, exact (signed) zeros, and more
than 256 embedding columns.

This file is the specification in plain Python: it imports nothing, uses no GPU and makes no library call.  The models and the oracle
references of the cases are built by the helpers at the top of tests/test_host_gat_sign_cases.py, for both test files."""

# ---- shapes: MTAD_GAT kwargs.  The recurrences and heads are small: they are not under test. ------------------------------------
_SMALL_HEADS = dict(gru_hid_dim=16, forecast_n_layers=1, forecast_hid_dim=8, recon_hid_dim=16)
SHAPES = {
    # smallest order: E = 2 / 2, one column per sign
    "e2": dict(n_features=5, window_size=10, out_dim=2, kernel_size=3, feat_gat_embed_dim=1, time_gat_embed_dim=1, **_SMALL_HEADS),
    # E = 32 / 8: PT % 32 == 0 in the feature layer, a single-tile temporal layer
    "small": dict(n_features=9, window_size=16, out_dim=3, kernel_size=5, feat_gat_embed_dim=16, time_gat_embed_dim=4, **_SMALL_HEADS),
    # E = 200 / 110: seven 32-column parts at the flagship node counts
    "msl_like": dict(n_features=55, window_size=100, out_dim=1, kernel_size=7, **_SMALL_HEADS),
    # E = 64 / 32: more than 128 nodes / node dimensions, the un-fused route (row GEMM + k_gat_wide)
    "wide": dict(n_features=12, window_size=136, out_dim=2, kernel_size=3, feat_gat_embed_dim=32, time_gat_embed_dim=16, **_SMALL_HEADS),
    # E = 24 / 1026: more than 512 features, the score-matrix route (row GEMM + k_attend)
    "attend": dict(n_features=513, window_size=12, out_dim=3, kernel_size=3, **_SMALL_HEADS),
    # E = 600 / 8: three chunks of k_gat_colorder's ballot ranks, the last one partial
    "long_embedding": dict(n_features=4, window_size=300, out_dim=4, kernel_size=3, **_SMALL_HEADS),
}
MODEL_SEED = 5
WINDOWS = 3
GRAD_SHAPES = ("e2", "small")
GRAD_PATTERNS = ("all_neg", "one_pos", "zeros", "all_zero")
GRAD_WINDOWS, GRAD_SEED = 9, 11
ALPHA_CASE = ("small", "alternating")
ALPHAS = (0.0, 1.0, 1.5)                       # 1.0: every a' is +-0; 1.5: the sign sense is reversed
SEQUENCE = ("all_pos", "all_neg", "one_pos", "all_zero", "alternating")     # walked on one handle of `small`


def embed_dims(kw):
    """(E_feat, E_temp) of a GATv2 model: twice the embedding dimension, which defaults to the layer's node dimension."""
    return 2 * (kw.get("feat_gat_embed_dim") or kw["window_size"]), 2 * (kw.get("time_gat_embed_dim") or kw["n_features"])


# ---- sign patterns: factors 0 / +-1 on |a_init|, so the magnitudes stay those of the initialisation -----------------------------
def _alternating(k):
    return 1.0 if k % 2 == 0 else -1.0


def _zeros(k):
    if k % 3 == 0:
        return 0.0 if k % 6 == 0 else -0.0      # both zeros count as non-negative and get scale 0
    return _alternating(k)


PATTERNS = {
    "all_pos": lambda k, E: 1.0,
    "all_neg": lambda k, E: -1.0,
    "one_pos": lambda k, E: 1.0 if k == E // 2 else -1.0,          # only the middle column non-negative
    "one_neg": lambda k, E: -1.0 if k == E // 2 else 1.0,
    "last_pos": lambda k, E: 1.0 if k == E - 1 else -1.0,
    "alternating": lambda k, E: _alternating(k),
    "first7_pos": lambda k, E: 1.0 if k < 7 else -1.0,
    "first8_pos": lambda k, E: 1.0 if k < 8 else -1.0,
    "halves_neg_first": lambda k, E: -1.0 if k < E // 2 else 1.0,
    "zeros": lambda k, E: _zeros(k),
    "all_zero": lambda k, E: 0.0,
    "chunk_neg_first": lambda k, E: -1.0 if k < 256 else 1.0,      # the first chunk of k_gat_colorder holds no non-negative column
}
LONG_ONLY = ("chunk_neg_first",)               # only where a layer has more than 256 embedding columns


def factors(pattern, E):
    return [PATTERNS[pattern](k, E) for k in range(E)]


def patterns_of(shape):
    long = max(embed_dims(SHAPES[shape])) > 256
    return [p for p in PATTERNS if long or p not in LONG_ONLY]


CASES = [(s, p) for s in SHAPES for p in patterns_of(s)]


# ---- the specification of the order ---------------------------------------------------------------------------------------------
def _round_up(n, m):
    return (n + m - 1) // m * m


def column_order(a, alpha):
    """The sorted column order of one layer for the attention vector a (E numbers): ((colk, P8, PT, npos), (colk2, P2, PT2)).

    Non-negative columns -- (1 - alpha) / 2 * a_k >= 0, which +0.0 and -0.0 satisfy -- come first, then the negative ones, each group
    in ascending embedding order.  8-padded order (gat_column_order): the groups are padded to multiples of 8, P8 = round_up(npos, 8),
    PT = P8 + round_up(nneg, 8); colk[n] is the embedding column of sorted column n, -1 for a pad.  Compact order (gath_compact_src):
    the non-negative group is padded to 2 only, P2 = round_up(npos, 2), PT2 = round_up(P2 + nneg, 8).  The rank-1 terms c / d sit in
    column PT (compact: PT2)."""
    half = (1.0 - float(alpha)) * 0.5
    pos = [k for k, v in enumerate(a) if half * float(v) >= 0.0]
    neg = [k for k, v in enumerate(a) if not half * float(v) >= 0.0]
    npos, nneg = len(pos), len(neg)
    P8 = _round_up(npos, 8)
    PT = P8 + _round_up(nneg, 8)
    colk = [-1] * PT
    colk[:npos] = pos
    colk[P8:P8 + nneg] = neg
    P2 = _round_up(npos, 2)
    PT2 = _round_up(P2 + nneg, 8)
    colk2 = [-1] * PT2
    colk2[:npos] = pos
    colk2[P2:P2 + nneg] = neg
    return (colk, P8, PT, npos), (colk2, P2, PT2)


def case_orders(shape, pattern, alpha=0.2):
    """[("feature" | "temporal", E, column_order(...))] of a case; the order depends on the signs alone, so the factors stand for a."""
    return [(name, E, column_order(factors(pattern, E), alpha)) for name, E in zip(("feature", "temporal"), embed_dims(SHAPES[shape]))]
