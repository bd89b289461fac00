"""Cost of the Predictor's score options on top of the forward, timed with HIP events after warm-up:
  anomaly_scores(values), anomaly_scores(values, scale_scores=True), anomaly_scores(values, scale_scores=True, use_mov_av=True)
on a seeded 65 636-row series at the SMD shape (F = out_dim = 38, W = 100) and the MSL shape (out_dim = 1); and, wall clock
(these calls return host tables), the per-feature thresholds of the SMD per-dimension scores: evaluation.find_epsilon per
column against evaluation.find_epsilon_columns.
The "scaling surcharge" is scaled - plain.  --pkg points at another build of the package (an older checkout) to time it with
the same script in the same visit; calls that build does not have are left out.  --trace CALL runs one call three times and
nothing else, for a `rocprofv3 --kernel-trace --stats -- python profiles/score_pipeline_bench.py --trace smoothed` run.
Usage: python profiles/score_pipeline_bench.py [--pkg DIR] [--reps N] [--out FILE] [--trace plain|scaled|smoothed]"""
import argparse
import inspect
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMD = dict(n_features=38, window_size=100, out_dim=38, kernel_size=7, gru_hid_dim=150, forecast_n_layers=1, forecast_hid_dim=150,
           recon_hid_dim=150, dropout=0.2, alpha=0.2)
MSL = dict(n_features=55, window_size=100, out_dim=1, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3, forecast_hid_dim=150,
           recon_hid_dim=150, dropout=0.3, alpha=0.2)
ROWS = 65636
CALLS = {"plain": dict(), "scaled": dict(scale_scores=True), "smoothed": dict(scale_scores=True, use_mov_av=True)}


def timed(fn, reps):
    for _ in range(3):                                        # warm-up at the timed shape
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "mtad-gat-pytorch_amd"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, choices=list(CALLS))
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.pkg), ROOT]
    from mtad_gat import MTAD_GAT
    dev = torch.device("cuda:0")
    known = inspect.signature(MTAD_GAT.anomaly_scores).parameters
    res = {"pkg": os.path.abspath(args.pkg), "rows": ROWS, "reps": args.reps}
    for name, kw in (("smd", SMD), ("msl", MSL)):
        torch.manual_seed(0)
        model = MTAD_GAT(**kw).to(dev).eval()
        g = torch.Generator().manual_seed(1)
        values = torch.rand(ROWS, kw["n_features"], generator=g).to(dev)
        dims = [0] if kw["out_dim"] == 1 else None
        if args.trace:
            if name == "smd":
                with torch.no_grad():
                    for _ in range(3):
                        model.anomaly_scores(values, dims, **CALLS[args.trace])
                torch.cuda.synchronize()
            continue
        row = {}
        with torch.no_grad():
            for call, opts in CALLS.items():
                if all(k in known for k in opts):
                    row[call + "_ms"] = timed(lambda: model.anomaly_scores(values, dims, **opts), args.reps)
        row["scaling_surcharge_ms"] = row["scaled_ms"] - row["plain_ms"]
        if "smoothed_ms" in row:
            row["smoothing_surcharge_ms"] = row["smoothed_ms"] - row["scaled_ms"]
        if name == "smd":
            import evaluation
            with torch.no_grad():
                per_dim = model.anomaly_scores(values, dims)[1]

            def wall(fn, reps=3):
                fn()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / reps * 1e3
            row["find_epsilon_per_column_ms"] = wall(lambda: [evaluation.find_epsilon(per_dim[:, c]) for c in range(per_dim.shape[1])])
            if hasattr(evaluation, "find_epsilon_columns"):
                row["find_epsilon_columns_ms"] = wall(lambda: evaluation.find_epsilon_columns(per_dim))
        res[name] = row
        del model
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
