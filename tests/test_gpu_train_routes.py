"""Every parameter gradient of the HIP training step against float64, route by route and slab plan by slab plan
(tests/train_route_cases.py; the models, picked windows, references and gates from tests/test_host_train_route_cases.py, which checks
on the CPU that the table reaches every ledger entry and that the gate can fail).

Per run (case, precision mode, "wgrad_kernel") and for p = 0 and p = P_DROP: the engine's train route, training-forward front route,
weight-gradient slab plans and row-GEMM arithmetic of every chunk must equal the hand-written table BEFORE the call -- a call that
leaves its route fails --; then model(x) on all n windows with grad_path == "hip" and  ((preds * cp).sum() + (recons * cr).sum()).backward()
with cp, cr zero everywhere but at the K picked windows.  Windows are independent, so every parameter gradient of the n-window call is
the sum over the picked windows, which the float64 torch-op route evaluates on the CPU; one wrong (window, step) row is 1 / (K W) of
the terms.  Gate per parameter tensor p, s_p = max |ref64_p|:

    max |ours_p - ref64_p| <= max |ref32_p - ref64_p| + c s_p + 1e-30        (c = train_route_cases.GATE_C, derived from the reference; ROUTE_C: a route's own)

and preds / recons of the picked windows under the forward route gate's rule.  Run with -s for the worst ratio per ledger entry.
Under MTADGAT_POISON_SCRATCH=1 the partial blocks of empty trailing slabs start out poisoned: the run shows that they are written."""
import copy

import pytest
import torch

import helpers
import train_route_cases as tc
from test_host_train_route_cases import assert_case_routes, base_model, case_input, forward_gate, gate_constants, grad_gate, reference

pytestmark = pytest.mark.gpu

_models = {}
_worst = {}                                      # ledger entry -> largest |ours - ref64| / s_p seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\nlargest max|ours - ref64| / max|ref64| per ledger entry:")
        for entry, r in sorted(_worst.items(), key=lambda kv: str(kv[0])):
            print(f"  {str(entry):50s} {r:.2e}")


def _site_of(name, v2):
    """The ledger's site kind of a parameter (None: a column sum or GAT (v1)'s finish kernel, no weight-gradient GEMM)."""
    if name.startswith("conv."):
        return "conv"
    if ".lin." in name:
        return "gat_lin" if v2 else None
    if "_ih_l" in name:
        return "ih"
    if "_hh_l" in name:
        return "hh"
    if name.startswith("recon_model.fc."):
        return "rec_fc"
    return "fc" if name.startswith("forecasting_model.") else None


def _record(c, mode, wk, ratios):
    v2 = tc.SHAPES[c["shape"]]["use_gatv2"]
    slabs, recs, fcs, atts = tc.ledger_of([(c, mode, wk)])
    rec_worst = max(r for n, r in ratios.items() if _site_of(n, v2) in ("ih", "hh"))
    att_worst = max(r for n, r in ratios.items() if "_gat." in n)
    for kind, a, cls in slabs:
        r = max(r for n, r in ratios.items() if _site_of(n, v2) == kind)
        _worst[(kind, a, cls)] = max(_worst.get((kind, a, cls), 0.0), r)
    for e, r in [(e, rec_worst) for e in recs | fcs] + [(e, att_worst) for e in atts]:
        _worst[e] = max(_worst.get(e, 0.0), r)
    return max(ratios.values())


def _model(shape, device):
    if shape not in _models:
        _models[shape] = copy.deepcopy(base_model(shape)).to(device)
    return _models[shape]


def _step(c, mode, wk, p, device):
    """One HIP training step of a case on all its windows with sparse cotangents; returns (ratios per parameter, forward errors)."""
    import _hipgrad
    kw = tc.SHAPES[c["shape"]]
    what = f"{tc.case_id(c)} {mode} wk={wk} p={p}"
    ref = reference(c, p)
    model = _model(c["shape"], device)
    model.train(p > 0)
    model.precision = mode
    eng = model._sync_engine(device)
    model._finish_weight_check()
    try:
        eng.set_option("wgrad_kernel", wk)
        assert _hipgrad._chunk_windows(eng, device) == tc.TRAIN_CHUNK, what
        assert_case_routes(eng, c, mode, wk, what=what)                       # before the call
        n, picks = c["n"], torch.tensor(ref["picks"], device=device)
        x = case_input(c).to(device)
        cp = torch.zeros(n, kw["out_dim"], device=device)
        cr = torch.zeros(n, kw["window_size"], kw["out_dim"], device=device)
        cp[picks], cr[picks] = ref["cp"].to(device), ref["cr"].to(device)
        for q in model.parameters():
            q.grad = None
        torch.manual_seed(tc.DROP_TORCH_SEED)                                 # p > 0: _hipgrad draws ref["seed"]
        pr, rc = model(x)
        assert model.grad_path == "hip", model.grad_path
        ((pr * cp).sum() + (rc * cr).sum()).backward()
        ours = {name: q.grad.detach().cpu() for name, q in model.named_parameters()}
        outs = {"preds": pr.detach()[picks].cpu(), "recons": rc.detach()[picks].cpu()}
        if p > 0:                                                             # the library's masks of the picked GLOBAL windows
            masks = helpers.masks_at(eng, ref["picks"], p, ref["seed"], device)
            for key, v in ref["masks"].items():
                for a, b in zip(v if isinstance(v, list) else [v], masks[key] if isinstance(v, list) else [masks[key]]):
                    assert torch.equal(a, b), (what, key, "the restated masks differ from the library's")
    finally:
        eng.set_option("wgrad_kernel", 0)
        for q in model.parameters():
            q.grad = None
        model.eval()
        model.precision = "auto"
    fwd = forward_gate(outs, ref[32], ref[64], what=what)
    ratios = grad_gate(ours, ref[32]["grads"], ref[64]["grads"], c=gate_constants(c, ref), what=what)
    return ratios, fwd


@pytest.mark.parametrize("run", tc.RUNS, ids=tc.RUN_IDS)
def test_parameter_gradients_against_float64(run, gpu_device):
    c, mode, wk = run
    for p in (0.0, tc.P_DROP):
        ratios, fwd = _step(c, mode, wk, p, gpu_device)
        worst = _record(c, mode, wk, ratios)
        top = max(ratios, key=ratios.get)
        print(f"{tc.case_id(c)} {mode} wk={wk} p={p}: {' || '.join(ch['route'][mode] for ch in c['chunks'])}: largest |ours - ref64| / s "
              f"{worst:.2e} ({top}); forward preds {fwd['preds']:.2e} recons {fwd['recons']:.2e}")


@pytest.mark.parametrize("c", tc.UNNORMALISED_CASES, ids=[tc.case_id(c) for c in tc.UNNORMALISED_CASES])
@pytest.mark.parametrize("mode", tc.MODES)
def test_unnormalised_inputs_hold_the_same_gate(c, mode, gpu_device):
    """Inputs x 4e5 at 2 600 windows: the convolution records outputs beyond 2^15.  "stacked" is then on the range guard's fallback
    (k_gru_split on fp32 operands instead of split operands, mode fp32); the base shape has no guarded recurrence, its hoisted input
    products read the recorded range.  The gate is the sparse gate scaled by the reference: per tensor c_p = 4 x the float32 route's
    own max |ref32_p - ref64_p| / s_p on this run, between GATE_C and 1e-4 (test_host_train_route_cases.gate_constants)."""
    model = _model(c["shape"], gpu_device)
    with torch.no_grad():
        assert model.conv(case_input(c)[:64].to(gpu_device)).max().item() >= 32768.0
    if c["shape"] == "stacked":
        model.precision = mode
        eng = model._sync_engine(gpu_device)
        model._finish_weight_check()
        model.precision = "auto"
        r = eng.gru_route(0, 0, c["n"], training=True, compute_units=helpers.device_compute_units(gpu_device))
        assert (r["first"], r["fallback"]) == ((4, 3) if mode == "fp32" else (3, 0)), r          # k_gru_split_x3 guarded by k_gru_split
    for p in (0.0, tc.P_DROP):
        ratios, fwd = _step(c, mode, 0, p, gpu_device)
        # (behind the saturated first GRU layer the gradients vanish -- 1e-38 and less, where only the gate's 1e-30 speaks)
        live = {n: r for n, r in ratios.items() if reference(c, p)[64]["grads"][n].abs().max().item() >= 1e-6}
        top = max(live, key=live.get)
        print(f"{tc.case_id(c)} {mode} p={p}: largest |ours - ref64| / s {live[top]:.2e} ({top}; {len(ratios) - len(live)} of {len(ratios)} "
              f"tensors vanish); forward preds {fwd['preds']:.2e} recons {fwd['recons']:.2e}")
