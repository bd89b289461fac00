"""The row GEMM and the implicit-GEMM convolution share their one-wave GEMM cores (csrc/mtadgat_kernels.hip: gemm_core_f32, gemm_core_x3),
fed by a row source or a convolution source; the workgroup kernels k_rowgemm_x3s / k_conv_x3s are the same pipeline written twice.  Each
is run here from both sources through the stage entry points (Engine.conv, Engine.heads) at the smallest shapes that reach what it can
get wrong -- a partly masked last K chunk, a pass of a four-tile group with one live tile, a last row tile partly out of range, both
window edges, the scalar loader of rows that are not whole 16-byte words, a half-empty last workgroup -- against float64 torch on the
CPU through helpers.gate at its default tolerance.  The route is asserted from front_route / mtadgat_rowgemm_split, and the two
arithmetics of a pair must differ, so no case passes on the wrong kernel.  (k_rowgemm_x3s:
test_gpu_shapes.py::test_many_row_gemms_share_weight_words_through_lds; the epilogue's gate / accumulate / transposed branches and the
linear convolution: test_gpu_backward.py, test_gpu_large_batch_gradients.py.)"""
import pytest
import torch

import _native
import _torchpath as tp
from helpers import gate, model64

pytestmark = pytest.mark.gpu

CONV_KIND = _native.FRONT_KINDS.index("conv")
WINDOWS = _native.FRONT_SOURCES.index("windows")


def _model(seed, **kw):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(seed)
    return MTAD_GAT(**kw).eval()


def _conv_build(eng, n):
    r = eng.front_route(CONV_KIND, WINDOWS, n)
    assert _native.FRONT_CONVS[r["conv"]] == "launch_conv", r
    return _native.FRONT_BUILDS[r["conv_build"]]


def _close_not_equal(a, b, what):
    """Two arithmetics of the same product: not the same kernel, and within the 2e-6 of the output scale test_gpu_shapes.py holds the pair to."""
    assert not torch.equal(a, b), f"{what}: the split-bf16 kernel did not run"
    assert (a - b).abs().max().item() <= 2e-6 * max(1.0, b.abs().max().item()), what


@pytest.mark.parametrize("F", [136, 134])
def test_convolution_straight_from_memory(F, gpu_device):
    """k_conv<2> (conv_kernel = 1) and k_conv_x3<4> (conv_kernel = 2): rows too long for the LDS-staged kernel (kernel_size 7: F >= 132).
    Fq = 144: the last 16-channel chunk is partly masked; NT = 5: the second pass of a four-tile group has one live tile; 3 windows of
    21 steps = 63 rows: the last row tile is partly out of range, and pad = 3 reaches both window edges.  F = 134 takes the scalar loader."""
    model = _model(41, n_features=F, window_size=21, out_dim=2, kernel_size=7, gru_hid_dim=8, forecast_hid_dim=8, recon_hid_dim=8)
    x = torch.randn(3, 21, F, generator=torch.Generator().manual_seed(42))
    with torch.no_grad():
        ref32, ref64 = tp.conv_stage(model, x), tp.conv_stage(model64(model), x.double())
        m = model.to(gpu_device)
        eng = m._sync_engine(gpu_device)
        xd = x.to(gpu_device)
        out = {}
        try:
            for option, build in ((1, "fp32"), (2, "x3")):
                eng.set_option("conv_kernel", option)
                assert _conv_build(eng, 3) == build
                out[build] = eng.conv(xd)
        finally:
            eng.set_option("conv_kernel", 0)
    for build, y in out.items():
        gate(y, ref32, ref64, what=f"convolution F={F}, {build} operands")
    _close_not_equal(out["x3"], out["fp32"], f"convolution F={F}")


def test_workgroup_convolution(gpu_device):
    """k_conv_x3s: 1 025 windows of 128 steps = 131 200 rows, past the 131 072 rows it starts at, the last 256-row workgroup half
    empty.  Bit-equal to k_conv_x3 (engine option "gemm_lds" = 1); the first and last two windows against float64."""
    n, W, F = 1025, 128, 136
    assert n * W >= 64 * 2048 and (n * W) % 256 == 128
    model = _model(43, n_features=F, window_size=W, out_dim=2, kernel_size=7, gru_hid_dim=8, forecast_hid_dim=8, recon_hid_dim=8)
    x = torch.randn(n, W, F, generator=torch.Generator().manual_seed(44))
    pick = torch.tensor([0, 1, n - 2, n - 1])
    with torch.no_grad():
        ref32, ref64 = tp.conv_stage(model, x[pick]), tp.conv_stage(model64(model), x[pick].double())
        m = model.to(gpu_device)
        eng = m._sync_engine(gpu_device)
        xd = x.to(gpu_device)
        assert _conv_build(eng, n) == "x3"
        y = eng.conv(xd)
        eng.set_option("gemm_lds", 1)
        try:
            assert _conv_build(eng, n) == "x3"
            y1 = eng.conv(xd)
        finally:
            eng.set_option("gemm_lds", 0)
    assert torch.equal(y, y1)
    gate(y[pick.to(gpu_device)], ref32, ref64, what="workgroup convolution, first and last windows")


@pytest.mark.parametrize("hid", [41, 3], ids=["K41", "K3"])
def test_row_gemm_of_the_heads(hid, gpu_device):
    """recon_model.fc over the decoder's states (Engine.heads): 401 windows of 41 steps = 16 441 rows (not a multiple of 32), out_dim
    130 (NT = 5: neither 1 nor a multiple of 4, the second pass of a four-tile group has one live tile), on k_rowgemm<2>
    (rowgemm_kernel = 1) and k_rowgemm_x3<4> (rowgemm_kernel = 2).  K = 41 is no multiple of 16 and no multiple of 4: 16-byte row
    loads with a straddling group; K = 3 < 4 takes the 4-byte loader (XV = false) -- the stage entries pad every row stride to whole
    16-byte words, so that is the one way to it."""
    n, W = 401, 41
    model = _model(45, n_features=6, window_size=W, out_dim=130, kernel_size=3, gru_hid_dim=35, forecast_hid_dim=33, recon_hid_dim=hid)
    hend = torch.rand(n, 35, generator=torch.Generator().manual_seed(46)) * 2 - 1
    with torch.no_grad():
        m64 = model64(model)
        p32, r32 = tp.forecast_stage(model, hend), tp.recon_stage(model, hend)
        p64, r64 = tp.forecast_stage(m64, hend.double()), tp.recon_stage(m64, hend.double())
        m = model.to(gpu_device)
        eng = m._sync_engine(gpu_device)
        hd = hend.to(gpu_device)
        out = {}
        try:
            for option, split in ((1, 0), (2, 1)):
                eng.set_option("rowgemm_kernel", option)
                assert eng.lib.mtadgat_rowgemm_split(eng.handle, 1, n * W, 0) == split
                out[split] = eng.heads(hd)
        finally:
            eng.set_option("rowgemm_kernel", 0)
    for split, (p, r) in out.items():
        gate(p, p32, p64, what=f"preds, K={hid}, split={split}")
        gate(r, r32, r64, what=f"recons, K={hid}, split={split}")
    assert torch.equal(out[0][0], out[1][0])                 # (the forecasting head's Linears are never split)
    _close_not_equal(out[1][1], out[0][1], f"recon_model.fc, K={hid}")
