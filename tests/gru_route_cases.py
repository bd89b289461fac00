"""Cases and specification for the recurrence routes (tests/test_host_gru_route_cases.py on the CPU, tests/test_gpu_gru_routes.py on
the GPU): tiny models at batch sizes that reach every kernel gru_route (csrc/mtadgat_pack.cpp) can name for an inference call -- the
window-per-workgroup and 16-window-group kernels, the hidden-tile-split kernel on fp32 / bf16 / split operands, the chunk-major
kernel, the tile-major kernel on its four operand builds with one and two 32-window groups per wave, as a first kernel and as the
range guard's fallback, with and without the per-step Linear riding inside.

Every case carries its HAND-WRITTEN pieces and routes: what forward_plan and gru_route answer on 256 compute units, spelled as
tests/test_host_gru_route.py's `_describe` spells a route ("+" joins a first kernel to its fallback), layers "GRU ... | decoder ...".
The CPU test holds the library's answers against these strings, the GPU test asks the device's own compute-unit count: a call that
leaves its route fails there, it is not skipped.

This file is the specification in plain Python: it imports nothing but `random`, uses no GPU and makes no library call.  The models,
inputs and float32 / float64 oracle references are built by the helpers at the top of tests/test_host_gru_route_cases.py, for both
test files."""
import random

CU = 256
MODEL_SEED, X_SEED, PICK_SEED = 29, 31, 37

# ---- shapes: MTAD_GAT kwargs -------------------------------------------------------------------------------------------------------
BASE = dict(n_features=6, window_size=8, out_dim=2, kernel_size=3, gru_hid_dim=40, recon_hid_dim=33)
SHAPES = {
    "A": dict(BASE),                                                             # 2 hidden tiles / 2 hidden tiles, Linear of 2 outputs
    "B": dict(BASE, gru_n_layers=2, recon_n_layers=2),                           # stacked layers
    "C": dict(BASE, gru_hid_dim=150, recon_hid_dim=150),                         # 5 hidden tiles: the x3_hi build
    "D": dict(BASE, gru_hid_dim=161, recon_hid_dim=200),                         # 6 / 7 hidden tiles: beyond the split-operand kernels
    "E": dict(BASE, out_dim=6, recon_n_layers=2),                                # a Linear of 6 outputs does not ride
    "G": dict(BASE, window_size=5, gru_hid_dim=96, recon_hid_dim=40),            # decoder input folded over more than 8 entries
    "H": dict(BASE, gru_hid_dim=32, recon_hid_dim=17),                           # one hidden tile
    "B128": dict(BASE, gru_n_layers=2, recon_n_layers=2, gru_hid_dim=128, recon_hid_dim=97),
    "L": dict(BASE, window_size=100),                                            # 100 steps: a carried state has time to build up
}
MODES = {2: "fp32", 0: "fp32_strict", 1: "bf16"}                 # mtadgat_set_precision mode -> MTAD_GAT.precision

# ---- input variants ----------------------------------------------------------------------------------------------------------------
# plain:    x ~ U[0, 1), seeded.
# spike:    window n // 2 times 2^17: the convolution's recorded range reaches 2^15, so the launch-wide range guard turns a guarded
#           route to its fallback kernel and the tile-major kernel on split operands to its three-piece input pack -- for every
#           ordinary window of the call.  The spiked window itself is only required to be finite: at 2^17 float32 resolves 2^-7, a
#           pre-activation that cancels to O(1) there is a property of the input, not of a kernel.
# saturate: every recurrence weight matrix (weight_ih / weight_hh of every GRU and decoder layer) times SATURATE_FACTOR: gate
#           arguments far into the clamped ends of gate_sigmoid / gate_tanh.
#           Only on W <= 8 shapes (at W = 100 the scaled recurrence is chaotic: float32 against float64 6.8e-4, not a test).
# carry:    + 5 on the update-gate rows of every bias_ih: z ~ 1, the state is carried over all steps.  From h0 = 0 it takes in
#           (1 - z) n ~ 0.007 n per step: after the 8 steps of the base shapes |h| <= 0.03 and the recurrent product hardly
#           matters (its weights rounded to fp16 move h_end by 5.6e-8), after the 100 steps of shape L |h| reaches 0.28 and the same
#           rounding moves h_end by 4.5e-6 in every window.  So carry runs on both: W = 8 for the gates' ends, L for a carried
#           state that the recurrent product's low piece shows in.
SPIKE_SCALE = 2.0 ** 17
RANGE_EDGE = 2.0 ** 15
# Measured, float32 oracle against float64 over the picked windows of every case using the variant (h_end, preds, recons;
# tests/test_host_gru_route_cases.py prints and bounds them): plain 9.7e-8, spike (its ordinary windows) 9.7e-8 (8.4e-8 on the W <= 8
# shapes alone), carry 1.1e-7 at W = 8 and 3.1e-7 at W = 100, saturate at factor 4: 4.9e-7 -- under the 5e-6 asked of it, so the factor stays at 4.
SATURATE_FACTOR = 4.0
CARRY_SHIFT = 5.0
REF_CAP = 1e-5                                                   # helpers.FP32_TOL: the float32 oracle's distance to float64
SATURATE_CAP = 5e-6

FP32_REL_TOL = 2e-6                                              # modes 0 and 2: times max(1, |ref64|max); the bound the suite holds between any two routes
BF16_TOL = 2e-2                                                  # mode 1: the project's bf16 gate

# ---- the cases ---------------------------------------------------------------------------------------------------------------------
PICK_OFFSETS = (0, 1, 15, 16, 31, 32, 63, 64, 127, 128)
N_RANDOM_PICKS = 8
P, S, SC = ("plain",), ("plain", "spike"), ("plain", "saturate", "carry")
SSC = ("plain", "spike", "saturate", "carry")
C, CS = ("plain", "carry"), ("plain", "spike", "carry")


def _case(shape, mode, gk, lanes, chunk, n, routes, variants, pieces=None):
    """routes: one string per piece, layers "GRU 0 | GRU 1 | ... | decoder 0 | ..."; pieces: window counts (one piece of n by default)."""
    routes = [routes] if isinstance(routes, str) else list(routes)
    return dict(shape=shape, mode=mode, gru_kernel=gk, lanes=lanes, chunk=chunk, n=n, pieces=list(pieces or [n]), routes=routes,
                variants=variants)


CASES = [
    # shape A: one GRU layer of 2 hidden tiles, one decoder layer with the Linear inside
    _case("A", 2, 0, 0, None, 33, "gru1 | gru1", SC),
    _case("A", 2, 0, 0, None, 1793, "gru16 | gru16", SC),
    _case("A", 2, 3, 0, None, 45, "splitx3+tile:x3_lo | splitx3:fc", SSC),
    _case("A", 2, 0, 0, None, 2561, "splitx3+tile:x3_lo | splitx3:fc", S),
    _case("A", 2, 2, 0, None, 4127, "cm+tile:x3_lo | cm:fc", SSC),
    _case("A", 2, 0, 1, None, 9001, "cm+tile:x3_lo | cm:fc", S),
    _case("A", 2, 1, 1, None, 10273, "tile:x3_lo | tile:x3_lo:fc", SSC),
    _case("A", 2, 1, 1, None, 65505, "tile:x3_lo:2 | tile:x3_lo:2:fc", S),
    _case("A", 2, 0, 1, 1 << 17, 65540, "cm+tile:x3_lo:2 | cm:fc", S),
    _case("A", 0, 0, 0, None, 4097, "split:fp32:xp | split:fp32:fc", SC),
    _case("A", 0, 0, 0, None, 16417, "tile:fp32 | tile:fp32:fc", SC),
    _case("A", 0, 0, 0, 1 << 17, 65540, "tile:fp32:2 | tile:fp32:2:fc", P),
    _case("A", 1, 0, 0, None, 1025, "split:bf16:xp | split:bf16:fc", P),
    _case("A", 1, 0, 0, None, 16417, "tile:bf16 | tile:bf16:fc", P),
    _case("A", 1, 0, 0, 1 << 17, 65540, "tile:bf16:2 | tile:bf16:2:fc", P),
    # a piece boundary: 8192 windows on the hidden-tile split, the 809 behind them on the window-per-workgroup kernel
    _case("A", 2, 0, 0, None, 9001, ["splitx3+tile:x3_lo | splitx3:fc", "gru1 | gru1"], S, pieces=[8192, 809]),
    # shape B: two layers per stack
    _case("B", 2, 0, 0, None, 45, "split:fp32:xp | split:fp32 | split:fp32 | split:fp32:fc", P),
    _case("B", 2, 2, 0, None, 45, "cm+tile:x3_lo | cm | cm | split:fp32:fc", S),
    _case("B", 2, 2, 0, None, 129, "cm+tile:x3_lo | cm | cm | split:fp32:fc", S),
    _case("B", 2, 3, 0, None, 45, "splitx3+tile:x3_lo | splitx3 | splitx3 | split:fp32:fc", S),
    _case("B", 2, 1, 1, None, 10273, "tile:x3_lo | tile:x3_lo | tile:x3_lo | tile:x3_lo:fc", S),
    _case("B", 0, 0, 0, None, 16417, "tile:fp32 | tile:fp32 | tile:fp32 | tile:fp32:fc", P),
    _case("B", 1, 0, 0, None, 45, "split:bf16:xp | split:bf16 | split:bf16 | split:bf16:fc", P),
    _case("B", 1, 0, 0, None, 16417, "tile:bf16 | tile:bf16 | tile:bf16 | tile:bf16:fc", P),
    # shape C: five hidden tiles
    _case("C", 2, 0, 0, None, 45, "gru1 | split:fp32:fc", P),
    _case("C", 2, 3, 0, None, 45, "splitx3+tile:x3_hi | split:fp32:fc", S),
    _case("C", 2, 2, 0, None, 4127, "cm+tile:x3_hi | split:fp32:fc", S),
    _case("C", 2, 1, 1, None, 10273, "tile:x3_hi | tile:x3_hi:fc", S),
    _case("C", 2, 0, 1, None, 10273, "cm+tile:x3_hi | tile:x3_hi:fc", S),
    # shape D: hidden sizes only the hidden-tile-split and tile-major kernels take
    _case("D", 2, 0, 0, None, 45, "split:fp32:xp | split:fp32:fc", P),
    _case("D", 2, 0, 1, None, 10273, "tile:x3_hi | tile:x3_hi:fc", S),
    _case("D", 0, 0, 0, None, 16417, "tile:fp32 | tile:fp32:fc", P),
    # shape E: the decoder's Linear as a row GEMM of its own
    _case("E", 2, 0, 0, None, 45, "gru1 | split:fp32 | split:fp32", P),
    _case("E", 2, 2, 0, None, 45, "gru1 | cm | cm", P),
    _case("E", 2, 3, 0, None, 45, "splitx3+tile:x3_lo | splitx3 | splitx3", S),
    _case("E", 2, 0, 1, None, 10273, "cm+tile:x3_lo | cm | cm", S),
    # shape G: the decoder's folded input in three chunks
    _case("G", 2, 0, 0, None, 45, "gru1 | split:fp32:fc", P),
    _case("G", 2, 3, 0, None, 45, "splitx3+tile:x3_lo | split:fp32:fc", S),
    _case("G", 2, 0, 1, None, 10273, "cm+tile:x3_lo | tile:x3_lo:fc", S),
    # shape H: one hidden tile
    _case("H", 2, 0, 0, None, 4097, "split:fp32:xp | tile:fp32:fc", P),
    _case("H", 2, 0, 1, None, 10273, "tile:x3_lo | tile:x3_lo:fc", S),
    # shape B128: a second GRU layer the chunk-major kernel takes, a decoder it does not
    _case("B128", 2, 2, 0, None, 45, "cm+tile:x3_lo | cm | split:fp32 | split:fp32:fc", S),
    _case("B128", 2, 3, 0, None, 45, "splitx3+tile:x3_lo | splitx3 | split:fp32 | split:fp32:fc", S),
    # shape L: shape A over 100 steps, each kernel with a state that is carried long enough to be there
    _case("L", 2, 0, 0, None, 33, "gru1 | gru1", C),
    _case("L", 2, 0, 0, None, 1793, "gru16 | gru16", C),
    _case("L", 2, 3, 0, None, 45, "splitx3+tile:x3_lo | splitx3:fc", CS),
    _case("L", 2, 2, 0, None, 4127, "cm+tile:x3_lo | cm:fc", CS),
    _case("L", 2, 1, 1, None, 10273, "tile:x3_lo | tile:x3_lo:fc", CS),
    _case("L", 0, 0, 0, None, 4097, "split:fp32:xp | split:fp32:fc", C),
]


def case_id(c, variant=None):
    s = f"{c['shape']}-{MODES[c['mode']]}-gk{c['gru_kernel']}-l{c['lanes']}-n{c['n']}" + ("-c%d" % c["chunk"] if c["chunk"] else "")
    return s if variant is None else s + "-" + variant


RUNS = [(c, v) for c in CASES for v in c["variants"]]            # one GPU test id each
RUN_IDS = [case_id(c, v) for c, v in RUNS]


def layers_of(c):
    """(GRU layers, decoder layers) of a case's shape."""
    kw = SHAPES[c["shape"]]
    return kw.get("gru_n_layers", 1), kw.get("recon_n_layers", 1)


def piece_routes(c):
    """Per piece: [route string per layer], GRU layers first."""
    return [[s.strip() for s in r.split("|")] for r in c["routes"]]


def needs_spike(c):
    """Layer 0 of the GRU stack is range-guarded (has a fallback) or is the tile-major kernel on split operands, in any piece."""
    return any("+" in r[0] or r[0].startswith("tile:x3") for r in piece_routes(c))


def spike_window(c):
    return c["n"] // 2


def picks(c):
    """The windows of a case that are held against the oracle, sorted: per piece the offsets PICK_OFFSETS, its last window, the first
    window of its last 32-window group and the window before that one, all clipped to the piece; then N_RANDOM_PICKS seeded random
    windows of the call."""
    out, at = set(), 0
    for n in c["pieces"]:
        last_group = (n - 1) // 32 * 32
        for off in PICK_OFFSETS + (n - 1, last_group, last_group - 1):
            out.add(at + min(max(off, 0), n - 1))
        at += n
    rnd = random.Random(PICK_SEED * 100003 + c["n"])
    out.update(rnd.randrange(c["n"]) for _ in range(N_RANDOM_PICKS))
    return sorted(out)


# ---- the ledger: (layer kind, route) pairs the table must keep reaching --------------------------------------------------------------
LEDGER = {
    "gru0": ["gru1", "gru16", "split:fp32:xp", "split:bf16:xp", "splitx3+tile:x3_lo", "splitx3+tile:x3_hi", "cm+tile:x3_lo",
             "cm+tile:x3_hi", "cm+tile:x3_lo:2", "tile:fp32", "tile:fp32:2", "tile:bf16", "tile:bf16:2", "tile:x3_lo", "tile:x3_lo:2",
             "tile:x3_hi"],
    "gru1+": ["split:fp32", "split:bf16", "splitx3", "cm", "tile:fp32", "tile:bf16", "tile:x3_lo"],
    "dec0": ["gru1", "gru16", "split:fp32", "split:fp32:fc", "split:bf16", "split:bf16:fc", "splitx3", "splitx3:fc", "cm", "cm:fc",
             "tile:fp32", "tile:fp32:fc", "tile:fp32:2:fc", "tile:bf16", "tile:bf16:fc", "tile:bf16:2:fc", "tile:x3_lo", "tile:x3_lo:fc",
             "tile:x3_lo:2:fc", "tile:x3_hi:fc"],
    "dec1+": ["split:fp32", "split:fp32:fc", "split:bf16:fc", "splitx3", "cm", "tile:fp32:fc", "tile:bf16:fc", "tile:x3_lo:fc"],
}
assert sum(len(v) for v in LEDGER.values()) == 51


def ledger_of(cases):
    """{layer kind: set of routes} the given cases reach, from their hand-written strings."""
    got = {k: set() for k in LEDGER}
    for c in cases:
        lg, ld = layers_of(c)
        for routes in piece_routes(c):
            assert len(routes) == lg + ld, (case_id(c), routes)
            for i, r in enumerate(routes):
                kind = ("gru0" if i == 0 else "gru1+") if i < lg else ("dec0" if i == lg else "dec1+")
                got[kind].add(r)
    return got
