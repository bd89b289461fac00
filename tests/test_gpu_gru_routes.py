"""Every recurrence route of an inference call against the float64 oracle, at batch sizes that reach it (tests/gru_route_cases.py; the
models, references and the gate from tests/test_host_gru_route_cases.py, which checks on the CPU that the table reaches every route
and that the gate can fail).

Per run: the engine is asked for its plan and its routes with the device's own compute-unit count -- they must equal the hand-written
table, a call that leaves its route fails --, one forward returns the GRU stack's last state, the predictions and the reconstructions,
and the picked windows of every piece (its first groups, both sides of its ragged last group, its last window, seeded random windows)
are held per window against the float64 oracle:  |ours - ref64|(w) <= |ref32 - ref64|(w) + tol,  tol = 2e-6 max(1, |ref64|max) in the
fp32 arithmetics, 2e-2 in the bf16 mode.  The whole output is then held against the same call walked in chunks of 1024 windows (the
small-batch routes): finite and within the same tol, so a row that no kernel wrote is seen wherever it lies."""
import pytest
import torch

import gru_route_cases as rc
from helpers import call_routes, device_compute_units
from test_host_gru_route_cases import case_input, new_model, ordinary_rows, reference, route_gate

pytestmark = pytest.mark.gpu


def test_the_device_has_the_compute_units_the_table_is_written_for(gpu_device):
    assert device_compute_units(gpu_device) == rc.CU


@pytest.mark.parametrize("run", rc.RUNS, ids=rc.RUN_IDS)
def test_route_against_float64(run, gpu_device):
    c, variant = run
    what = rc.case_id(c, variant)
    ref = reference(c, variant)
    model = new_model(c["shape"], variant).to(gpu_device)
    model.precision = rc.MODES[c["mode"]]
    x = case_input(c, variant).to(gpu_device)
    eng = model._sync_engine(gpu_device, bf16=c["mode"] == 1)
    keep_chunk = eng.chunk_windows()
    try:
        eng.set_precision(c["mode"])
        eng.set_option("gru_kernel", c["gru_kernel"])
        eng.set_option("lanes", c["lanes"])
        if c["chunk"]:
            eng.set_chunk_windows(c["chunk"])
        pieces, routes = call_routes(eng, c["n"], device_compute_units(gpu_device))
        assert pieces == c["pieces"] and routes == c["routes"], (what, pieces, routes)
        preds, recons, hend = eng.forward(x, want_hend=True)
        conv_max = eng.last_conv_max(c["n"], gpu_device)
        # spike: the same call without the spiked window, i.e. on the other side of the range guard
        hend_plain = eng.forward(case_input(c, "plain").to(gpu_device), want_hend=True)[2] if variant == "spike" else None
        eng.set_chunk_windows(1024)
        assert max(n for _, n, _ in eng.forward_plan(c["n"])["pieces"]) <= 1024
        preds_s, recons_s, hend_s = eng.forward(x, want_hend=True)
    finally:
        eng.set_option("gru_kernel", 0)
        eng.set_option("lanes", 0)
        eng.set_chunk_windows(keep_chunk)
        eng.set_precision(2)
        model._finish_weight_check()
    # the side of the range guard the variant means: what the convolution recorded (last_conv_max reads the call's last piece, so
    # only one-piece calls are asked; the CPU test holds the oracle's convolution of every case on its side of the edge)
    if rc.needs_spike(c) and len(pieces) == 1:
        assert (conv_max >= rc.RANGE_EDGE) == (variant == "spike"), (what, conv_max)
    pk = torch.tensor(ref["picks"], device=gpu_device)
    ours = {"h_end": hend[pk], "preds": preds[pk], "recons": recons[pk]}
    rows = ordinary_rows(c, variant, ref["picks"])
    worst = route_gate(ours, ref[32], ref[64], c["mode"], rows=rows, what=what)
    print(f"{what}: {' || '.join(routes)}: |ours - ref64| h_end {worst['h_end']:.2e} preds {worst['preds']:.2e} "
          f"recons {worst['recons']:.2e}")
    # every row of the call, against the small-batch routes
    held = torch.ones(c["n"], dtype=torch.bool, device=gpu_device)
    if variant == "spike":
        held[rc.spike_window(c)] = False
        # the guard acts on the whole launch: the ordinary windows took another kernel / another input pack than in the plain call,
        # a different arithmetic that agrees within tol but not bit for bit
        assert not torch.equal(hend[held], hend_plain[held]), f"{what}: the range guard did not change what ran"
        assert (hend[held] - hend_plain[held]).abs().max().item() <= rc.FP32_REL_TOL, what
    for name, a, b in (("h_end", hend, hend_s), ("preds", preds, preds_s), ("recons", recons, recons_s)):
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (what, name)
        tol = rc.BF16_TOL if c["mode"] == 1 else rc.FP32_REL_TOL * max(1.0, ref[64][name][rows].abs().max().item())
        d = (a - b).flatten(1).abs().amax(1)
        over = (held & (d > tol)).nonzero().flatten()
        assert over.numel() == 0, (what, name, f"{over.numel()} windows beyond {tol:.2e} of the 1024-window chunks' result, the first "
                                   f"{over[:6].tolist()}, the largest difference {d[held].max().item():.3e}")
