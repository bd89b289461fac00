"""What the split-pack kernels write (k_absmax, k_scale_from_max, k_split3, k_split2h, k_split2h_gath, k_split_x, k_reorder_xq),
read back from the device and compared bit for bit with the numpy replay of the same table on the same image's fp32 part
(tests/split_refs.py; the table itself is checked by tests/test_host_split_table.py).  Every other image comparison of the suite masks
these regions out, and the end-to-end gates do not see a dropped low piece, a scale one power of two off or a stale pack.

Gates, all derived: bit identity with the replay (the operation is a pure function of the fp32 image, the table and RNE conversions);
independent of the replay, hi + mid + lo == S v exactly for three bf16 pieces and |S v - hi - lo| <= max(2^-22 |S v|, 2^-25) for two
fp16 pieces (csrc/mtadgat_device.h), all-zero bits in padding chunks and padding columns; zero bits in the floats of a region
beyond its step's footprint (the ring slack of wh3 / wx2 / wxq: the image starts zeroed, the device re-pack leaves derived regions
alone and nothing else writes there)."""
import copy

import numpy as np
import pytest
import torch

import gat_sign_cases as gc
import split_refs as sr
from test_gpu_device_pack import CONFIGS, _perturb
from test_host_derived_regions import SHAPES as REGION_SHAPES

pytestmark = pytest.mark.gpu

SHAPES = dict(CONFIGS)
SHAPES["wide_features"] = REGION_SHAPES["wide_features"]
SHAPES["e2"] = gc.SHAPES["e2"]
SHAPES["small"] = gc.SHAPES["small"]

GRU0 = ("gru.gru.weight_ih_l0", "gru.gru.weight_hh_l0")
GRU1 = ("gru.gru.weight_ih_l1", "gru.gru.weight_hh_l1")
REC0 = ("recon_model.decoder.rnn.weight_ih_l0", "recon_model.decoder.rnn.weight_hh_l0")
CONV = ("conv.conv.weight",)
EDGE = float(2.0 ** -3)
BELOW_EDGE = float(np.nextafter(np.float32(EDGE), np.float32(0)))


# ---- models ---------------------------------------------------------------------------------------------------------------------
def _model(shape, seed=0, perturb=10):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(seed)
    model = MTAD_GAT(**SHAPES[shape]).eval()
    if perturb is not None:
        _perturb(model, perturb)
    return model


def _scale_keys(model, keys, factors):
    with torch.no_grad():
        sd = model.state_dict()
        for k, f in zip(keys, factors):
            sd[k].mul_(f)


def _set_largest(model, keys, value):
    """every weight of the group below 0.1 in magnitude, one of them exactly `value`"""
    with torch.no_grad():
        sd = model.state_dict()
        top = max(sd[k].abs().max().item() for k in keys)
        for k in keys:
            sd[k].mul_(0.1 / top)
        sd[keys[-1]].view(-1)[3] = -value


def _zero(model, keys):
    with torch.no_grad():
        sd = model.state_dict()
        for k in keys:
            sd[k].zero_()


def _engine(model, gpu_device):
    for p in model.parameters():                                    # the cases promise: 0, or within [2^-60, 2^60] (no fp32 denormal)
        a = p.detach().abs()
        a = a[a > 0]
        assert a.numel() == 0 or (a.min().item() >= 2.0 ** -60 and a.max().item() <= 2.0 ** 60)
    model = model.to(gpu_device).eval()
    return model, model._sync_engine(gpu_device)


# ---- the checks -----------------------------------------------------------------------------------------------------------------
def _read(eng, gpu_device):
    eng.derive_split_packs(gpu_device)
    return eng.read_packed(gpu_device).numpy().copy()


def _reference(img, eng):
    """the replay of the table on the image's fp32 part: derived regions zeroed first, as after an upload"""
    base = img.copy()
    for off, n in eng.derived_regions():
        base.view(np.int32)[off:off + n] = 0
    return sr.replay(base, eng.split_steps())


def _check_bits(img, ref, eng, what):
    gi, ri = img.view(np.int32), ref.view(np.int32)
    for k, s in enumerate(eng.split_steps()):
        off, n = sr.dst_span(s)
        bad = np.flatnonzero(gi[off:off + n] != ri[off:off + n])
        if bad.size:
            i = int(bad[0])
            raise AssertionError("%s: step %d %s (group %d) differs from the reference in %d of %d floats, first at %s: device %08x, "
                                 "reference %08x" % (what, k, s["op"], s["group"], bad.size, n, sr.locate(s, i),
                                                     int(gi[off + i]) & 0xFFFFFFFF, int(ri[off + i]) & 0xFFFFFFFF))
    # what is left: the fp32 part (the reference's own input) and the floats of the regions beyond the footprints, zero in both
    bad = np.flatnonzero(gi != ri)
    if bad.size:
        i = int(bad[0])
        region = [r for r in eng.derived_regions() if r[0] <= i < r[0] + r[1]]
        raise AssertionError("%s: float %d of the image (region %s) is %08x beyond every footprint, not zero" % (what, i, region, int(gi[i]) & 0xFFFFFFFF))


def _check(eng, gpu_device, what):
    img = _read(eng, gpu_device)
    _check_bits(img, _reference(img, eng), eng, what)
    sr.check_contract(img, eng.split_steps(), what)
    return img


def _group_of(eng, which):
    """the steps of the recurrence groups in image order (GRU layers, then decoder layers), or of the convolution"""
    steps = eng.split_steps()
    groups = {}
    for s in steps:
        groups.setdefault(s["group"], []).append(s)
    if which == "conv":
        return groups[0]
    rec = [g for g in groups.values() if any(t["op"] == "SPLIT_X" for t in g)]
    return rec[which]


# ---- (a) initialisation plus a perturbation, every shape ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_packs_of_perturbed_initial_weights(shape, gpu_device):
    _, eng = _engine(_model(shape), gpu_device)
    img = _check(eng, gpu_device, shape)
    assert eng.split_n_infer() < len({s["group"] for s in eng.split_steps()}) or not SHAPES[shape].get("use_gatv2", True)
    for s in eng.split_steps():                                     # nothing trivially zero: every pack holds weights
        if s["op"] in sr.SPLIT_OPS:
            off, n = sr.dst_span(s)
            assert img.view(np.int32)[off:off + n].any(), (shape, s)


def test_fp16_subnormal_low_pieces_are_kept(gpu_device):
    """At initialisation-sized weights some low pieces are fp16 subnormals (below 2^-14 after the scale): the device keeps them, as
    the 2^-25 term of the contract needs."""
    _, eng = _engine(_model("msl_shape"), gpu_device)
    img = _check(eng, gpu_device, "msl_shape")
    sub = 0
    for s in eng.split_steps():
        if s["op"] in ("SPLIT2H", "SPLIT2H_GATH", "SPLIT_X"):
            for part in sr.decode(img, s):
                if part["kind"] == "f16":
                    lo = part["bits"][1]
                    sub += int(((lo & 0x7C00) == 0).sum() - ((lo & 0x7FFF) == 0).sum())
    assert sub > 0


# ---- (b) one side of a recurrence layer in fp16's subnormal range ---------------------------------------------------------------
@pytest.mark.parametrize("layer,keys", [("gru0", GRU0), ("gru1", GRU1), ("rec0", REC0)])
@pytest.mark.parametrize("factors", [(1e-6, 3e4), (3e4, 1e-6)], ids=["ih_small", "hh_small"])
def test_recurrence_weights_of_very_different_ranges_share_a_scale(layer, keys, factors, gpu_device):
    model = _model("stacked")
    _scale_keys(model, keys, factors)
    _, eng = _engine(model, gpu_device)
    img = _check(eng, gpu_device, (layer, factors))
    g = _group_of(eng, dict(gru0=0, gru1=1, rec0=2)[layer])
    slot = img.view(np.uint32)[g[0]["scale"]:g[0]["scale"] + 4]
    assert slot[1:2].view(np.float32)[0] <= 2.0 ** 4                # the large side sets the scale: max |W| >= 3e4 * 0.03


# ---- (c) the two ends of [2^13, 2^14) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,keys", [("gru0", GRU0), ("conv", CONV)])
@pytest.mark.parametrize("value,S", [(EDGE, 2.0 ** 16), (BELOW_EDGE, 2.0 ** 17)], ids=["2^-3", "below_2^-3"])
def test_largest_weight_at_a_power_of_two(which, keys, value, S, gpu_device):
    model = _model("odd_shapes")
    _set_largest(model, keys, value)
    _, eng = _engine(model, gpu_device)
    img = _check(eng, gpu_device, (which, value))
    g = _group_of(eng, 0 if which == "gru0" else "conv")
    slot = img.view(np.uint32)[g[0]["scale"]:g[0]["scale"] + 4]
    assert slot[0] == np.float32(value).view(np.uint32) and list(slot[1:].view(np.float32)) == [S, 1.0 / S, 0.0]
    top = float(value) * S
    assert 2.0 ** 13 <= top < 2.0 ** 14 and (top == 2.0 ** 13 or top == float(np.nextafter(np.float32(2.0 ** 14), np.float32(0))))


# ---- (d) a layer of zeros -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,keys", [("gru0", GRU0), ("conv", CONV)])
def test_all_zero_weights_give_zero_pieces(which, keys, gpu_device):
    model = _model("odd_shapes")
    _zero(model, keys)
    _, eng = _engine(model, gpu_device)
    img = _check(eng, gpu_device, which)
    g = _group_of(eng, 0 if which == "gru0" else "conv")
    slot = img.view(np.uint32)[g[0]["scale"]:g[0]["scale"] + 4]
    assert slot[0] == 0 and list(slot[1:].view(np.float32)) == [2.0 ** 14, 2.0 ** -14, 0.0]
    for s in g:
        if s["op"] not in sr.SCALE_OPS:
            off, n = sr.dst_span(s)
            assert not img.view(np.int32)[off:off + n].any(), (which, s)


# ---- (e) the convolution's range ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1e-6, 3e4])
@pytest.mark.parametrize("shape", ["odd_shapes", "wide_features"])
def test_convolution_weights_of_other_ranges(shape, factor, gpu_device):
    model = _model(shape)
    _scale_keys(model, CONV, (factor,))
    _, eng = _engine(model, gpu_device)
    img = _check(eng, gpu_device, (shape, factor))
    g = _group_of(eng, "conv")
    S = img[g[0]["scale"] + 1]
    assert (S >= 2.0 ** 30) if factor < 1 else (S <= 2.0 ** 4)


# ---- (f) degenerate sign groups of the compact column order ---------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["all_pos", "all_neg", "one_pos", "first7_pos", "zeros", "all_zero"])
@pytest.mark.parametrize("shape", ["e2", "small"])
def test_compact_order_at_degenerate_sign_groups(shape, pattern, gpu_device):
    from test_host_gat_sign_cases import apply_pattern, new_model
    model, _, mags = new_model(shape)
    apply_pattern(model, mags, pattern)
    _, eng = _engine(model, gpu_device)
    img = _check(eng, gpu_device, (shape, pattern))
    gath = [s for s in eng.split_steps() if s["op"] == "SPLIT2H_GATH"]
    assert len(gath) == 2
    for s, (_, E, ((_, P8, PT, npos), _)) in zip(gath, gc.case_orders(shape, pattern)):
        assert s["arg"] == E and [int(v) for v in img.view(np.int32)[s["ord"]:s["ord"] + 3]] == [P8, PT, npos], (shape, pattern, s)


# ---- freshness and determinism --------------------------------------------------------------------------------------------------
def _packs_differ(a, b, eng, what):
    ai, bi = a.view(np.int32), b.view(np.int32)
    n_infer, seen = eng.split_n_infer(), set()
    for s in eng.split_steps():
        if s["op"] in sr.SCALE_OPS:
            continue
        off, n = sr.dst_span(s)
        assert not np.array_equal(ai[off:off + n], bi[off:off + n]), (what, "a pack kept the earlier weights", s)
        seen.add(s["group"] >= n_infer)
    assert seen == {False, True}                                    # the backward's groups too


def test_packs_follow_every_kind_of_upload(gpu_device):
    model, eng = _engine(_model("stacked"), gpu_device)
    first = _check(eng, gpu_device, "first load")
    _perturb(model, 21)
    assert eng.update_weights_device(model.state_dict(), gpu_device)
    second = _check(eng, gpu_device, "device re-pack")
    _packs_differ(first, second, eng, "device re-pack")
    _perturb(model, 22)
    eng.load_weights(model.state_dict(), gpu_device, allow_device_pack=False)
    third = _check(eng, gpu_device, "host re-pack")
    _packs_differ(second, third, eng, "host re-pack")


def test_two_derivations_of_the_same_weights_are_identical(gpu_device):
    model, eng = _engine(_model("odd_shapes"), gpu_device)
    first = _read(eng, gpu_device)
    eng.load_weights(copy.deepcopy(model.state_dict()), gpu_device, allow_device_pack=False)    # every group stale again
    second = _read(eng, gpu_device)
    assert np.array_equal(first.view(np.int32), second.view(np.int32))
    assert eng.update_weights_device(model.state_dict(), gpu_device)      # (its fp32 part may differ in the decoder's fold: no bit gate)
    _check(eng, gpu_device, "device re-pack of the same weights")
