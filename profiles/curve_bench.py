"""Time of the ranking calls (evaluation.score_order, ranking_metrics; DESIGN.md section 4, "Ranking curves") beside the same
quantity computed on the same device with stock ops.  Device times are HIP events around a loop of calls after a warm-up at the timed
shape; every pair (ours, stock) is timed alternately for ROUNDS rounds and the median round is reported, with the spread.
  sizes       n = 73 629 (the MSL test series), 2^20 and 2^24 scores; labels in bursts over about 10 % of the samples
  score_order       against torch.sort(descending=True, stable=True) of the same tensor (values and indices)
  ranking_metrics   adjust=None against torch.sort(stable=True) + the labels gathered in rank order + cumsum: the raw curve's tp / fp
                    at every sample, without tie groups, AUROC, average precision or the best F1 -- the stock ops' share of the work
  ranking_metrics   adjust="point" and ("k", 30): no stock counterpart; the times stand alone
ranking_metrics ends in its one device-to-host copy; the stock side ends in a synchronise as well, so both include one.
Usage: python profiles/curve_bench.py [--out FILE] [--sizes N ...]   (a text table, also printed)"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mtad-gat-pytorch_amd"), os.path.join(ROOT, "tests"), ROOT]

ROUNDS = 7


def series(n, seed):
    """Scores that rise inside the labelled bursts, rounded so that ties exist."""
    rng = np.random.default_rng(seed)
    scores = (rng.random(n) * 0.5).astype(np.float32)
    labels = np.zeros(n, bool)
    for at in rng.integers(0, max(1, n - 200), max(1, int(0.10 * n / 110))):
        length = int(rng.integers(20, 201))
        labels[at:at + length] = True
        scores[at:at + length] += (0.5 * rng.random(length)).astype(np.float32)
    return np.round(scores, 4).astype(np.float32), labels


def loop_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def compare(fns, seconds=0.3):
    """{name: (median ms, min, max, reps)} of the callables, timed alternately."""
    reps = {}
    for name, fn in fns.items():
        fn()                                                  # warm-up at the timed shape
        torch.cuda.synchronize()
        reps[name] = max(3, min(1000, int(seconds * 1e3 / max(loop_ms(fn, 2), 1e-3))))
    rounds = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            rounds[name].append(loop_ms(fn, reps[name]))
    return {name: (statistics.median(v), min(v), max(v), reps[name]) for name, v in rounds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="*", default=[73629, 1 << 20, 1 << 24])
    args = ap.parse_args()
    import curve_refs
    import evaluation as ev
    if not torch.cuda.is_available():
        raise SystemExit("curve_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    lines = [f"device: {props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} compute units, "
             f"{props.total_memory >> 30} GiB; rounds per entry: {ROUNDS} (median [min, max] ms per call, reps per round)"]
    for n in args.sizes:
        scores, labels = series(n, seed=n % 1000)
        s, lab = torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev)
        lab_i = lab.to(torch.int64)
        if n <= 1 << 20:                                      # the timed calls compute the right thing
            assert np.array_equal(ev.score_order(s).cpu().numpy(), curve_refs.score_order(scores))
            ref = curve_refs.ranking_metrics(scores, labels)
            got = ev.ranking_metrics(s, lab)
            assert got["auroc"] == ref["auroc"] and got["best_index"] == ref["best_index"]

        def stock_sort():
            torch.sort(s, descending=True, stable=True)

        def stock_curve():
            order = torch.sort(s, descending=True, stable=True).indices
            tp = torch.cumsum(lab_i[order], 0)
            fp = torch.arange(1, n + 1, device=dev) - tp
            torch.cuda.current_stream().synchronize()
            return tp, fp

        res = compare({"score_order": lambda: ev.score_order(s), "torch.sort(stable)": stock_sort})
        res.update(compare({"ranking_metrics(None)": lambda: ev.ranking_metrics(s, lab), "torch.sort + gather + cumsum": stock_curve}))
        res.update(compare({"ranking_metrics('point')": lambda: ev.ranking_metrics(s, lab, "point"),
                            "ranking_metrics(('k', 30))": lambda: ev.ranking_metrics(s, lab, ("k", 30))}))
        lines.append(f"n = {n}  (positives {int(labels.sum())}, distinct scores {np.unique(scores).size})")
        for name, (med, lo, hi, reps) in res.items():
            lines.append(f"  {name:<32s} {med:10.4f} [{lo:.4f}, {hi:.4f}]  x{reps}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
