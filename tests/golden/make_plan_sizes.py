#!/usr/bin/env python3
"""Known-answer fixture for the host-side layout planners: what every workspace / tape / scratch size query of the C ABI answered
at the commit BEFORE the forward plan, the region carver and the planners' move into mtadgat_pack.cpp (plan_sizes.json was
written there and is not regenerated when the planners change: tests/test_host_forward_plan.py holds them to it).  No GPU and no
weights are needed; every handle gets an explicit chunk size, because the default one depends on the device memory found.

    python -B tests/golden/make_plan_sizes.py          # rewrites tests/golden/plan_sizes.json
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (os.path.join(ROOT, "mtad-gat-pytorch_amd"), ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, "plan_sizes.json")

MODES = (0, 1, 2)                       # mtadgat_set_precision
LANES = (0, 1)                          # option "lanes"
CHUNKS = (65536, 10000, 9000, 2048)
CONFIG4 = "config4"                     # BASELINE config 4: the un-fused wide attention path, chunks of a few hundred windows
CONFIG4_CHUNKS = (896, 24)
BATCHES = (1, 64, 256, 1024, 1025, 4096, 4097, 8192, 8193, 9728, 9729, 10240, 16384, 16385, 32768, 32769, 36864, 65536, 65537,
           98304, 100000)
N_LAYOUT = 25                           # entries of mtadgat_train_layout


def shapes():
    from helpers import Case
    from test_host_derived_regions import SHAPES
    s = {"msl": Case("msl").kwargs, "smd_1_1": Case("smd_1_1").kwargs}
    s.update(SHAPES)
    s[CONFIG4] = dict(n_features=512, window_size=256, out_dim=512, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3,
                      forecast_hid_dim=150, recon_hid_dim=150)
    return s


def chunks_of(name):
    return CONFIG4_CHUNKS if name == CONFIG4 else CHUNKS


def create(kw):
    import _native
    from mtad_gat import MTAD_GAT
    lib = _native.load_library()
    h = ctypes.c_void_p()
    assert lib.mtadgat_create(ctypes.byref(_native.Config(**MTAD_GAT(**kw)._native_cfg)), ctypes.byref(h)) == 0, lib.mtadgat_last_error()
    return lib, h


def key(mode, lanes, chunk):
    return f"mode{mode}/lanes{lanes}/chunk{chunk}"


def collect_shape(name, kw):
    """The answers of one shape.  `workspace` and `stream` depend on the precision mode, the lanes option and the chunk: one list over
    BATCHES per combination.  The attention and attribution sizes depend on the chunk only and the training sizes on neither: they are
    queried under every mode and lanes value all the same, and recorded once after checking that the answers agree."""
    lib, h = create(kw)
    out = {"kwargs": kw, "backward_supported": int(lib.mtadgat_backward_supported(h)), "workspace": {}, "stream": {}, "attention": {},
           "attribution": {}}
    bwd = out["backward_supported"] == 1

    def once(store, k, v):
        assert store.setdefault(k, v) == v, (name, k)

    try:
        for mode in MODES:
            assert lib.mtadgat_set_precision(h, mode) == 0
            for lanes in LANES:
                assert lib.mtadgat_set_option(h, b"lanes", lanes) == 0
                for chunk in chunks_of(name):
                    assert lib.mtadgat_set_chunk_windows(h, chunk) == 0
                    k = key(mode, lanes, chunk)
                    out["workspace"][k] = [lib.mtadgat_workspace_bytes(h, b) for b in BATCHES]
                    out["stream"][k] = [lib.mtadgat_stream_workspace_bytes(h, b) for b in BATCHES]
                    once(out["attention"], f"chunk{chunk}", [[lib.mtadgat_attention_workspace_bytes(h, b, r) for r in (0, 1)] for b in BATCHES])
                    if bwd:
                        once(out["attribution"], f"chunk{chunk}",
                             [[lib.mtadgat_score_attribution_workspace_bytes(h, b, s) for s in (0, 8)] for b in BATCHES])
                if bwd:
                    once(out, "tape", [lib.mtadgat_tape_bytes(h, b) for b in BATCHES])
                    once(out, "backward_workspace", [lib.mtadgat_backward_workspace_bytes(h, b) for b in BATCHES])
                    layouts = []
                    for b in BATCHES:
                        buf = (ctypes.c_int64 * N_LAYOUT)()
                        assert lib.mtadgat_train_layout(h, b, buf, N_LAYOUT) == N_LAYOUT, lib.mtadgat_last_error()
                        layouts.append(list(buf))
                    once(out, "train_layout", layouts)
    finally:
        lib.mtadgat_destroy(h)
    return out


def main():
    s = shapes()
    rec = {name: collect_shape(name, kw) for name, kw in s.items()}
    with open(PATH, "w") as f:                                   # one line per shape
        f.write('{"batches":' + json.dumps(list(BATCHES), separators=(",", ":")) + ',\n"shapes":{\n')
        f.write(",\n".join(json.dumps(n) + ":" + json.dumps(r, separators=(",", ":")) for n, r in rec.items()))
        f.write("\n}}\n")
    no_bwd = [n for n, r in rec.items() if not r["backward_supported"]]
    print(PATH, os.path.getsize(PATH), "bytes;", len(rec), "shapes; without a HIP backward (training / attribution sizes skipped):", no_bwd or "none")


if __name__ == "__main__":
    main()
