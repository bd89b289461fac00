"""The deterministic evaluation kernels against the bits of the commit before they were merged: moving_average and
moving_average(parts=) are two instantiations of one scan (csrc/mtadgat_evalcol.hip), the per-part epsilon table runs the tile
routine it shares with the plain one (csrc/mtadgat_scan.h).  None of them uses atomics, so the SHA-256 of their output bytes, recorded
on the MI355X by tests/golden/make_eval_bits.py before the change (tests/golden/eval_bits.json), has to come out again: a different
hash is a change of arithmetic -- a contraction or an order of operations -- to be found and restored, not tolerated."""
import json
import sys

import pytest

from helpers import GOLDEN_DIR

if GOLDEN_DIR not in sys.path:
    sys.path.insert(0, GOLDEN_DIR)
import make_eval_bits as rec  # noqa: E402


def _golden():
    with open(rec.PATH) as f:
        return json.load(f)["sha256"]


def _assert_same(got, want):
    assert got, "no case was computed"
    differ = [k for k, v in got.items() if want.get(k) != v]
    assert not differ, differ


def test_the_recorded_cases_are_the_ones_computed():
    keys = {f"ewm/n{n}/span{s}/{w}" for n in rec.EWM_SIZES for s in rec.EWM_SPANS for w in ("plain",) + rec.EWM_LAYOUTS}
    keys |= {f"parts/W{W}/{t}" for W in rec.TABLE_WINDOWS for t in ("moments", "table")}
    assert set(_golden()) == keys


@pytest.mark.gpu
@pytest.mark.parametrize("n", rec.EWM_SIZES)
def test_moving_average_bits(n, gpu_device):
    _assert_same(rec.ewm_hashes(n, gpu_device), _golden())


@pytest.mark.gpu
@pytest.mark.parametrize("W", rec.TABLE_WINDOWS)
def test_part_table_bits(W, gpu_device):
    _assert_same(rec.table_hashes(W, gpu_device), _golden())
