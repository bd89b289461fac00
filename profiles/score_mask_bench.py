"""Time of the calls that score a gappy series beside their plain counterparts, and of the plain calls alone for a comparison between
two builds of the library.
  method    HIP events around ONE call, WARMUP calls at the timed shape first, then ROUNDS rounds of RUNS timed calls, the masked call
            and its plain counterpart alternately; reported is the median over all calls with the smallest and largest round median
  sizes     (73 729 x 55) -- the MSL test series -- and (2^20 x 38) float32 per-dimension scores, 15 % of the samples missing (iid)
  calls     scored_rows (no plain counterpart: beside fitting.training_windows, which adds the host read of the count);
            anomaly_scores(age=) / anomaly_scores; column_quantiles(skip_nan) / column_quantiles for q = 0.25, 0.5, 0.75;
            moving_average(skip_nan) / moving_average, span 1280, on the (n,) global score; find_epsilon_columns(skip_nan) /
            find_epsilon_columns (whose moments are moments_valid / mtadgat_eval_moments_columns); MTAD_GAT.anomaly_scores(age=,
            scale_scores=True, use_mov_av=True) / the same without age, on a (MODEL_ROWS x 38) series
  --plain   only the plain calls, and moving_average(skip_nan) and moving_average(parts=) (PARTS equal parts) beside the plain moving
            average, one line of medians as JSON: run once per process with the package of either build first on sys.path
            (--package DIR), the two builds alternately, to see whether a call changed
Usage: python profiles/score_mask_bench.py [--out FILE] [--cases N:D ...] [--plain] [--package DIR]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WARMUP, RUNS, ROUNDS, MODEL_ROWS, PARTS = 3, 10, 3, 1 << 16, 27


def one_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def compare(*fns):
    """(median over all calls, smallest round median, largest round median) ms per function, the functions called alternately"""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    rounds = [[[] for _ in range(ROUNDS)] for _ in fns]
    for r in range(ROUNDS):
        for _ in range(RUNS):
            for k, fn in enumerate(fns):
                rounds[k][r].append(one_ms(fn))
    out = []
    for per_round in rounds:
        meds = [statistics.median(v) for v in per_round]
        out.append((statistics.median([t for v in per_round for t in v]), min(meds), max(meds)))
    return out


def moments_columns(ev, a):
    """mtadgat_eval_moments_columns as find_epsilon_columns calls it"""
    import ctypes
    n, d = a.shape
    scratch = torch.empty(2 * d, dtype=torch.float64, device=a.device)
    mom = np.empty((d, 2), dtype=np.float64)
    rc = ev._lib().mtadgat_eval_moments_columns(a.data_ptr(), n, d, a.stride(0), scratch.data_ptr(), mom.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                ev._stream(a))
    assert rc == 0
    return mom


def model_for(dev, F):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(0)
    return MTAD_GAT(n_features=F, window_size=100, out_dim=F, kernel_size=7, gru_hid_dim=150, forecast_hid_dim=150, recon_hid_dim=150).to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", nargs="*", default=["73729:55", f"{1 << 20}:38"])
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--package", default=os.path.join(ROOT, "mtad-gat-pytorch_amd"))
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.package), os.path.dirname(os.path.abspath(args.package))]
    import evaluation as ev
    if not torch.cuda.is_available():
        raise SystemExit("score_mask_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    lines = [f"device: {props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} compute units; {ROUNDS} rounds of "
             f"{RUNS} single calls per entry after {WARMUP} warm-up calls, HIP events: median [smallest, largest round median] ms per call"]
    plain = {}
    W = 100
    for case in args.cases:
        n, d = (int(v) for v in case.split(":"))
        rng = np.random.default_rng(n % 1000)
        a = torch.from_numpy((rng.random((n, d), dtype=np.float32) * 3.0)).to(dev)
        glob = a[:, 0].contiguous()
        if args.plain:
            gappy = torch.where(torch.from_numpy(rng.random(n) < 0.15).to(dev), torch.full_like(glob, float("nan")), glob)
            lengths = np.full(PARTS, (n + W) // PARTS, dtype=np.int64)
            lengths[0] += (n + W) % PARTS
            parts = ev.score_parts(lengths, W, device=dev)
            res = compare(lambda: ev.column_quantiles(a, [0.25, 0.5, 0.75]), lambda: ev.moving_average(glob, 1280),
                          lambda: ev.moving_average(gappy, 1280, skip_nan=True), lambda: ev.moving_average(glob, 1280, parts=parts),
                          lambda: ev.find_epsilon_columns(a))
            names = ("column_quantiles", "moving_average", "moving_average(skip_nan)", "moving_average(parts=)", "find_epsilon_columns")
            for name, r in zip(names, res):
                plain[f"{name} {n}x{d}"] = r[0]
            continue
        import fitting
        gaps = torch.from_numpy(rng.random((n, d)) < 0.15).to(dev)
        g = torch.where(gaps, torch.full_like(a, float("nan")), a)
        gg = g[:, 0].contiguous()
        age = torch.zeros((n + W, d), dtype=torch.int32, device=dev)
        age[W:] = gaps.to(torch.int32)
        values = torch.rand((n + W, d), device=dev)
        preds, recons = torch.rand((n, d), device=dev), torch.rand((n, d), device=dev)
        keep = ev.scored_rows(n + W, W, d, age)
        entries = [
            ("scored_rows", lambda: ev.scored_rows(n + W, W, d, age), "fitting.training_windows", lambda: fitting.training_windows(n + W, W, d, age=age)),
            ("anomaly_scores(age=, keep=)", lambda: ev.anomaly_scores(preds, recons, values, W, age=age, keep=keep),
             "anomaly_scores", lambda: ev.anomaly_scores(preds, recons, values, W)),
            ("column_quantiles(skip_nan)", lambda: ev.column_quantiles(g, [0.25, 0.5, 0.75], skip_nan=True),
             "column_quantiles", lambda: ev.column_quantiles(a, [0.25, 0.5, 0.75])),
            ("moving_average(skip_nan)", lambda: ev.moving_average(gg, 1280, skip_nan=True), "moving_average", lambda: ev.moving_average(glob, 1280)),
            ("moments_valid", lambda: ev.moments_valid(g), "mtadgat_eval_moments_columns", lambda: moments_columns(ev, a)),
            ("find_epsilon_columns(skip_nan)", lambda: ev.find_epsilon_columns(g, skip_nan=True), "find_epsilon_columns", lambda: ev.find_epsilon_columns(a)),
        ]
        lines.append(f"n = {n}, d = {d} ({n * d * 4 / 2 ** 20:.0f} MiB), 15 % missing")
        for name, masked, pname, stock in entries:
            (med, lo, hi), (smed, slo, shi) = compare(masked, stock)
            lines.append(f"  {name:<34s} {med:9.4f} [{lo:.4f}, {hi:.4f}]")
            lines.append(f"  {'  ' + pname:<34s} {smed:9.4f} [{slo:.4f}, {shi:.4f}]   masked / plain = {med / smed:.2f}")
        a = g = gaps = age = values = preds = recons = None
        torch.cuda.empty_cache()
    # the whole model call
    F = 38
    model = model_for(dev, F)
    series = torch.rand((MODEL_ROWS, F), device=dev)
    with torch.no_grad():
        if args.plain:
            plain[f"model.anomaly_scores {MODEL_ROWS}x{F}"] = compare(lambda: model.anomaly_scores(series, scale_scores=True, use_mov_av=True))[0][0]
            print(json.dumps(plain))
            return
        age = (torch.rand((MODEL_ROWS, F), device=dev) < 0.15).to(torch.int32)
        (med, lo, hi), (smed, slo, shi) = compare(lambda: model.anomaly_scores(series, scale_scores=True, use_mov_av=True, age=age),
                                                  lambda: model.anomaly_scores(series, scale_scores=True, use_mov_av=True))
    lines.append(f"MTAD_GAT.anomaly_scores(scale_scores=True, use_mov_av=True), {MODEL_ROWS} x {F}, window 100")
    lines.append(f"  {'with age= (15 % missing)':<34s} {med:9.4f} [{lo:.4f}, {hi:.4f}]")
    lines.append(f"  {'  plain':<34s} {smed:9.4f} [{slo:.4f}, {shi:.4f}]   masked / plain = {med / smed:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
