"""What the peaks-over-threshold thresholds cost, timed with HIP events after warm-up ("SPOT").

  offline   spot_calibrate (level 0.98, q 1e-3, max_peaks 1024) over a 70 000 x 55 training-score matrix, then a dynamic spot_run
            over a 70 000 x 55 test-score matrix (seeded gamma noise with a level shift in the last third), each the median of
            ROUNDS calls with the spread; beside it -- for orientation, not a gate -- the wall time of the numpy specification
            tests/spot_refs.py on the first --ref-columns columns of the same data (0 skips it)
  push      StreamScorer.push of one row for 256 streams at the MSL shape (W = 100, F = 55): with a fixed threshold, and -- when the
            tree has it -- with a SpotState (one calibrated column serving all streams, max_peaks 1024), rows drawn so that about 2 %
            of them refit.  Median of ROUNDS rounds of REPS pushes with the spread.  --tree ROOT measures another checkout of this
            repository (its fixed-threshold push), e.g. the parent commit.

Usage: python profiles/spot_bench.py [--what offline|push|all] [--tree ROOT] [--ref-columns N] [--out FILE]
Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MSL = dict(n_features=55, window_size=100, out_dim=1, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3, forecast_hid_dim=150,
           recon_hid_dim=150, dropout=0.3, alpha=0.2)
ROUNDS, REPS = 5, 200
N, D = 70000, 55


def timed(fn, reps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def fmt(s):
    return f"{s['median']:.3f} ({s['min']:.3f}..{s['max']:.3f})"


def score_matrices():
    rng = np.random.default_rng(70000)
    scale = 0.5 + rng.random(D)
    init = (rng.gamma(4.0, 0.05, (N, D)) * scale).astype(np.float32)
    x = rng.gamma(4.0, 0.05, (N, D)) * scale
    x[N - N // 3:] *= 1.5
    return init, x.astype(np.float32)


def offline(dev, ref_columns, tests_dir):
    import evaluation
    init, x = score_matrices()
    d_init, d_x = torch.from_numpy(init).to(dev), torch.from_numpy(x).to(dev)
    state = evaluation.spot_calibrate(d_init, max_peaks=1024)
    evaluation.spot_run(state.clone(), d_x[:1000])
    cal, run = [], []
    for _ in range(ROUNDS):
        cal.append(timed(lambda: evaluation.spot_calibrate(d_init, max_peaks=1024), 1))
        work = state.clone()
        run.append(timed(lambda: evaluation.spot_run(work, d_x), 1))
    after = work.read()
    res = dict(rows=N, columns=D, calibrate_ms=spread(cal), dynamic_run_ms=spread(run), refits_per_column=float(np.mean(after["Nt"] - state.read()["Nt"])),
               reference_columns=ref_columns, reference_s_per_column=None)
    lines = [f"offline {N} x {D}: spot_calibrate {fmt(res['calibrate_ms'])} ms, dynamic spot_run {fmt(res['dynamic_run_ms'])} ms, "
             f"{res['refits_per_column']:.0f} refits per column"]
    if ref_columns > 0:
        sys.path.insert(0, tests_dir)
        import spot_refs
        t0 = time.perf_counter()
        for c in range(ref_columns):
            st = spot_refs.calibrate(init[:, c], 1e-3, 0.98, 1024)
            spot_refs.run(st, x[:, c], True)
        res["reference_s_per_column"] = (time.perf_counter() - t0) / ref_columns
        lines.append(f"        tests/spot_refs.py (numpy, float64, one CPU thread): {res['reference_s_per_column']:.1f} s per column "
                     f"over {ref_columns} column(s), i.e. about {res['reference_s_per_column'] * D:.0f} s for the matrix")
    else:
        lines.append("        tests/spot_refs.py: not measured")
    return res, lines


def push(dev):
    from mtad_gat import MTAD_GAT
    from streaming import StreamScorer
    import evaluation
    torch.manual_seed(0)
    model = MTAD_GAT(**MSL).to(dev).eval()
    S, F, W = 256, model.n_features, model.window_size
    rows = torch.rand(S, 1, F, device=dev)
    res, lines = {}, []
    kinds = [("fixed", 0.5)]
    if hasattr(evaluation, "spot_calibrate"):
        # scores of random rows through a random model, as the scorer itself computes them: the calibration sample
        probe = StreamScorer(model, S, 0.5, target_dims=[0], max_block=1)
        sample = []
        for _ in range(W + 40):
            sample.append(probe.push(torch.rand(S, 1, F, device=dev))["scores"])
        sample = torch.cat(sample[W:], dim=1).reshape(-1)
        kinds.append(("spot", evaluation.spot_calibrate(sample, max_peaks=1024)))
    for name, threshold in kinds:
        scorer = StreamScorer(model, S, threshold, target_dims=[0], merge_gap=2, min_length=2, max_block=1)
        fresh = [torch.rand(S, 1, F, device=dev) for _ in range(8)]
        k = [0]

        def one():
            k[0] += 1
            scorer.push(fresh[k[0] % 8] if name == "spot" else rows)

        for _ in range(W + 3):
            one()
        t = [timed(one, REPS) for _ in range(ROUNDS)]
        res[name] = spread(t)
        extra = ""
        if name == "spot":
            st = scorer.spot_state().read()
            res["spot_refits_per_stream"] = float(np.mean(st["Nt"]) - threshold.read()["Nt"][0])
            extra = f", {res['spot_refits_per_stream']:.1f} refits per stream over {int(st['n'][0] - threshold.read()['n'][0])} scored rows"
        lines.append(f"push 256 x 1, {name} threshold: {fmt(res[name])} ms{extra}")
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=("offline", "push", "all"))
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--ref-columns", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.tree)
    sys.path[:0] = [os.path.join(root, "mtad-gat-pytorch_amd"), root]
    dev = torch.device("cuda:0")
    res, lines = {"tree": os.path.basename(root)}, []
    if args.what in ("offline", "all"):
        r, l = offline(dev, args.ref_columns, os.path.join(root, "tests"))
        res["offline"] = r
        lines += l
    if args.what in ("push", "all"):
        r, l = push(dev)
        res["push"] = r
        lines += l
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
