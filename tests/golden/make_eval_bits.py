#!/usr/bin/env python3
"""Known-answer fixture for the deterministic evaluation kernels: the SHA-256 of the bytes that moving_average, moving_average(parts=)
and the raw per-part tables of mtadgat_eval_part_epsilon_moments / _table returned on an MI355X at commit fa198ba, the commit BEFORE
the plain and the segmented exponentially weighted mean became two instantiations of one scan and the plain and per-part epsilon
kernels came to share one tile routine (eval_bits.json was written there and is not regenerated when the kernels change:
tests/test_gpu_eval_bits.py holds them to it).  All three are free of atomics, so a different hash is a change of arithmetic.

    python -B tests/golden/make_eval_bits.py [--commit ID] [--out FILE]      # rewrites tests/golden/eval_bits.json; needs the GPU
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (os.path.join(ROOT, "mtad-gat-pytorch_amd"), ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, "eval_bits.json")

EWM_SIZES = (1, 5, 1023, 1024, 1025, 4097, 66601)       # 66601: more than 65 chunks of 1024, a second step of the carry wave
EWM_SPANS = (1, 2, 7, 1280)                              # test_gpu_parts.SPANS
EWM_LAYOUTS = ("one", "mid_chunk", "every_element")
TABLE_WINDOWS = (1, 100)                                 # test_gpu_parts.WINDOWS
TABLE_SEED = 31
_dp = ctypes.POINTER(ctypes.c_double)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ewm_input(n):
    """(n,) float32: uniform noise, the second half a factor 1e-6 below the first."""
    x = np.random.default_rng([21, n]).random(n) + 0.5
    x[n // 2:] *= 1e-6
    return x.astype(np.float32)


def ewm_lengths(n, layout):
    """Part lengths for n scores at window 1: one part; one seam in the middle of a chunk; a seam on every element of one chunk (the
    second chunk where there is one, else the first)."""
    import part_refs
    at = {"one": [], "mid_chunk": [min(n // 2, 1024 + 500)],
          "every_element": range(1024, 2049) if n > 2049 else range(1, n)}[layout]
    return part_refs.lengths_from_seams(n, 1, at)


def ewm_hashes(n, device):
    """{case: sha256} of the float32 output bytes for every span, plain and with each layout of parts."""
    import torch
    import evaluation as ev
    t = torch.from_numpy(ewm_input(n)).to(device)
    out = {}
    for span in EWM_SPANS:
        out[f"ewm/n{n}/span{span}/plain"] = _sha(ev.moving_average(t, span).cpu().numpy())
        for layout in EWM_LAYOUTS:
            sp = ev.score_parts(ewm_lengths(n, layout), 1, device=device)
            out[f"ewm/n{n}/span{span}/{layout}"] = _sha(ev.moving_average(t, span, parts=sp).cpu().numpy())
    return out


def part_tables(W, device):
    """The raw (P, 3) moments and (P, 4 nz) table of test_gpu_parts._bursty_parts(W, 31), with the thresholds that
    evaluation.find_epsilon_parts forms from the moments (an empty part: a NaN row)."""
    import torch
    import evaluation as ev
    from test_gpu_parts import _bursty_parts
    lib = ev._lib()
    x, lengths = _bursty_parts(W, TABLE_SEED)
    t = torch.from_numpy(x).to(device)
    sp = ev.score_parts(lengths, W, device=device)
    P, zs, halo = sp.n_parts, ev._EPSILON_ZS, ev._EPSILON_HALO
    nz = len(zs)
    scratch = ev._scratch(lib.mtadgat_eval_part_epsilon_scratch(t.numel(), P, nz), device)
    mom = np.empty((P, 3), dtype=np.float64)
    with torch.cuda.device(device):
        rc = lib.mtadgat_eval_part_epsilon_moments(t.data_ptr(), t.numel(), sp.start.data_ptr(), sp.end.data_ptr(), P, nz, scratch.data_ptr(),
                                                   scratch.numel() * 8, mom.ctypes.data_as(_dp), ev._stream(t))
    assert rc == 0, lib.mtadgat_last_error()
    count = sp.end_host - sp.start_host
    eps = np.full((P, nz), np.nan)
    for p in range(P):
        if count[p] > 0:
            mean = mom[p, 0] / count[p]
            eps[p] = mean + np.sqrt(max(mom[p, 1] / count[p] - mean * mean, 0.0)) * zs
    tab = np.empty((P, 4 * nz), dtype=np.float64)
    with torch.cuda.device(device):
        rc = lib.mtadgat_eval_part_epsilon_table(t.data_ptr(), t.numel(), sp.start.data_ptr(), sp.end.data_ptr(), P, eps.ctypes.data_as(_dp),
                                                 nz, halo, scratch.data_ptr(), scratch.numel() * 8, tab.ctypes.data_as(_dp), ev._stream(t))
    assert rc == 0, lib.mtadgat_last_error()
    return mom, tab


def table_hashes(W, device):
    mom, tab = part_tables(W, device)
    return {f"parts/W{W}/moments": _sha(mom), f"parts/W{W}/table": _sha(tab)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit of the tree this runs on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=PATH)
    args = ap.parse_args()
    import torch
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dev = torch.device("cuda:0")
    rec = {}
    for n in EWM_SIZES:
        rec.update(ewm_hashes(n, dev))
    for W in TABLE_WINDOWS:
        rec.update(table_hashes(W, dev))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"commit": commit, "device": torch.cuda.get_device_properties(dev).name, "sha256": rec}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(args.out, len(rec), "hashes at commit", commit)


if __name__ == "__main__":
    main()
