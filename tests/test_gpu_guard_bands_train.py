"""The training step stays inside the buffers it is handed: every case of train_route_cases in both precision modes (p = P_DROP,
the default "wgrad_kernel") takes the Python step of tests/test_gpu_train_routes.py -- model(x) with x.requires_grad, sparse cotangents,
backward() -- four times (tests/guard_rows.py): on allocator buffers, then with x, preds, recons, every chunk's tape and backward
workspace, dx and the flat gradient buffer carved from a guard-banded arena (tests/arena.py) under the NaN pattern, the huge finite
pattern, and the NaN pattern with the data buffers 4, 8 or 12 bytes past a 16-byte boundary.  The train route, front route and slab
plans are asserted before every call (assert_case_routes).  One mtadgat_backward_data call per shape runs the same way, its
cotangents in the arena too.

In the Python step the cotangents come from autograd, outside the seam; test_backward therefore calls forward_train, backward and
backward_input through the engine with d_preds and d_recons in the arena and skewed like x, once per shape and at two ragged slab
plans, so that the weight-gradient GEMM (k_wgrad_lds) takes its scalar loader on them, and holds grads bit for bit.

Bit equality: the ordinary step runs twice first and must reproduce every tensor bit for bit (it does, on every case),
so every tensor of the arena runs is held by bit equality against the ordinary step."""
import copy

import pytest
import torch

import _native
import train_route_cases as tc
from guard_rows import four_calls, same_bits
from test_host_train_route_cases import assert_case_routes, base_model, case_input, dropout_seed, reference

pytestmark = pytest.mark.gpu

_models = {}
ROWS = [(c, m, 0) for c in tc.CASES for m in tc.MODES]


def _model(shape, device):
    if shape not in _models:
        _models[shape] = copy.deepcopy(base_model(shape)).to(device)
    return _models[shape]


def test_the_training_rows_reach_every_ledger_entry():
    """Every case in both modes: the rows reach every slab class, recurrence pair, Linear placement and attention backward of the
    table's ledgers (tests/test_host_train_route_cases.py holds the table to them with the same function)."""
    slabs, recs, fcs, atts = tc.ledger_of(ROWS)
    assert not [e for e in tc.SLAB_LEDGER if e not in slabs]
    assert set(tc.RECURRENCE_LEDGER) == recs and set(tc.FC_LEDGER) == fcs and set(tc.ATTENTION_LEDGER) == atts


@pytest.mark.parametrize("run", ROWS, ids=[tc.case_id(c) + "-" + m for c, m, _ in ROWS])
def test_training_step(run, gpu_device, monkeypatch):
    import _hipgrad
    c, mode, wk = run
    p = tc.P_DROP
    kw = tc.SHAPES[c["shape"]]
    what = f"{tc.case_id(c)} {mode} wk={wk} p={p}"
    ref = reference(c, p)
    model = _model(c["shape"], gpu_device)
    model.train(True)
    model.precision = mode
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    n, picks = c["n"], torch.tensor(ref["picks"], device=gpu_device)
    cp = torch.zeros(n, kw["out_dim"], device=gpu_device)
    cr = torch.zeros(n, kw["window_size"], kw["out_dim"], device=gpu_device)
    cp[picks], cr[picks] = ref["cp"].to(gpu_device), ref["cr"].to(gpu_device)

    def before():
        assert _hipgrad._chunk_windows(eng, gpu_device) == tc.TRAIN_CHUNK, what
        assert_case_routes(eng, c, mode, wk, what=what)

    def step(ins):
        x = ins["x"].detach().requires_grad_(True)
        for q in model.parameters():
            q.grad = None
        torch.manual_seed(tc.DROP_TORCH_SEED)
        pr, rc = model(x)
        assert model.grad_path == "hip", model.grad_path
        ((pr * cp).sum() + (rc * cr).sum()).backward()
        out = {"preds": pr.detach(), "recons": rc.detach(), "dx": x.grad, "grads": eng._flat_grads[0]}
        out.update({"grad:" + name: q.grad.detach() for name, q in model.named_parameters()})
        return {k: v.clone() for k, v in out.items()}

    try:
        eng.set_option("wgrad_kernel", wk)
        x = case_input(c).to(gpu_device)
        before()
        first = step({"x": x})
        torch.cuda.synchronize()

        def second(out):                                             # the step reproduces itself bit for bit, so bit equality holds everything
            loose = [k for k in first if not same_bits(first[k], out[k])]
            assert loose == [], (what, "not bit-equal between two ordinary steps", loose)
        _, names = four_calls(monkeypatch, gpu_device, [eng], {"x": x}, step, what, before=before, on_ordinary=second)
        # what the seam routed into the arena: both outputs, a tape and a backward workspace per chunk, dx, the gradient buffer
        taken = names["A"]
        for need in ("x", "forward_train.preds", "forward_train.recons", "forward_train.tape", "_bws", "backward_input.dx", "backward.grads"):
            assert need in taken, (what, need, taken)
        assert sum(t.startswith("_bws") for t in taken) == len(c["chunks"]), taken
    finally:
        eng.set_option("wgrad_kernel", 0)
        for q in model.parameters():
            q.grad = None
        model.eval()
        model.precision = "auto"


SHAPE_CASES = {}
for _c in tc.CASES:
    SHAPE_CASES.setdefault(_c["shape"], _c)                          # the smallest case of every shape


@pytest.mark.parametrize("shape", list(SHAPE_CASES))
def test_backward_data(shape, gpu_device, monkeypatch):
    """mtadgat_forward_train + mtadgat_backward_data through the engine, x and both cotangents in the arena (skewed in the last call)."""
    c = SHAPE_CASES[shape]
    kw = tc.SHAPES[shape]
    model = _model(shape, gpu_device)
    model.precision = "fp32"
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    n, W, od = c["n"], kw["window_size"], kw["out_dim"]
    g = torch.Generator().manual_seed(23)
    inputs = {"x": case_input(c).to(gpu_device), "d_preds": torch.randn(n, od, generator=g).to(gpu_device),
              "d_recons": torch.randn(n, W, od, generator=g).to(gpu_device)}
    seed = dropout_seed()

    def call(ins):
        preds, recons, tape = eng.forward_train(ins["x"], tc.P_DROP, seed)
        dx = eng.backward_data(ins["x"], tc.P_DROP, seed, ins["d_preds"], ins["d_recons"], tape)
        return {"preds": preds, "recons": recons, "dx": dx}
    try:
        four_calls(monkeypatch, gpu_device, [eng], inputs, call, f"backward_data {tc.case_id(c)}",
                   before=lambda: assert_case_routes(eng, c, "fp32", 0, what=shape))
    finally:
        model.precision = "auto"


BACKWARD_CASES = dict({shape: c for shape, c in SHAPE_CASES.items()},
                      **{tc.case_id(c): c for c in tc.CASES if tc.case_id(c) in ("base-n1793", "base-n4097")})   # empty trailing slabs; k_gru_bwd


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_backward(name, mode, gpu_device, monkeypatch):
    """mtadgat_forward_train + mtadgat_backward + mtadgat_backward_input through the engine: x, d_preds and d_recons in the arena (4, 8
    or 12 bytes past a 16-byte boundary in the last call: the weight-gradient GEMM's loader is chosen from their low bits), the
    gradient buffer from the seam and zeroed; preds, recons, dx and every parameter gradient bit-equal to the ordinary call's.
    fc_in / fc_out: d_recons rows of 96 / 97 floats -- whole 16-byte words the float4 loader takes when aligned."""
    c = BACKWARD_CASES[name]
    shape = c["shape"]
    kw = tc.SHAPES[shape]
    model = _model(shape, gpu_device)
    model.precision = mode
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    n, W, od = c["n"], kw["window_size"], kw["out_dim"]
    total = eng.grad_layout()[1]
    g = torch.Generator().manual_seed(29)
    inputs = {"x": case_input(c).to(gpu_device), "d_preds": torch.randn(n, od, generator=g).to(gpu_device),
              "d_recons": torch.randn(n, W, od, generator=g).to(gpu_device)}
    seed = dropout_seed()

    def call(ins):
        preds, recons, tape = eng.forward_train(ins["x"], tc.P_DROP, seed)
        grads = _native._empty(total, dtype=torch.float32, device=gpu_device).zero_()
        eng.backward(ins["x"], tc.P_DROP, seed, ins["d_preds"], ins["d_recons"], tape, grads)
        return {"preds": preds, "recons": recons, "grads": grads, "dx": eng.backward_input(ins["x"])}
    try:
        ref, names = four_calls(monkeypatch, gpu_device, [eng], inputs, call, f"backward {tc.case_id(c)} {mode}",
                                before=lambda: assert_case_routes(eng, c, mode, 0, what=name))
        assert "call.grads" in names["A skewed"] and bool(ref["grads"].any())
    finally:
        model.precision = "auto"
