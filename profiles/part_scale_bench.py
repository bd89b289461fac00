"""Time of the per-part quantiles and score scaling (evaluation.part_quantiles, scale_scores(parts=)) beside the obvious composition
of what the package had before them: a Python loop over the parts with column_quantiles and torch arithmetic per slice, on the same
device.  The method is profiles/curve_bench.py's: HIP events around a loop of calls after a warm-up at the timed shape, every pair
(ours, loop) timed alternately for ROUNDS rounds, the median round reported with the spread.
  sizes and parts   n = 73 629 scores in 27 parts (the MSL test series and its channels), 2^20 and 2^24 scores in 1 024 parts, part
                    lengths varying by a factor of about four (at 2^24 some parts are longer than mtadgat_eval_partq_long() and take
                    the route with bins in memory); d = 1 and d = 38 columns
  part_quantiles          against: column_quantiles of every part's slice
  scale_scores(parts=)    against: column_quantiles of every part's slice, then (a - median) / (1 + IQR) of the slice into one output
  one part of 2^24 rows   the long route alone, beside column_quantiles of the same array
The loop's results are checked against ours at the first size before anything is timed.
Usage: python profiles/part_scale_bench.py [--out FILE] [--cases N:P ...] [--dims D ...]   (a text table, also printed)"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "mtad-gat-pytorch_amd"), os.path.join(ROOT, "tests"), ROOT, HERE]

from curve_bench import ROUNDS, compare  # noqa: E402

WINDOW = 100
QS = [0.25, 0.5, 0.75]


def part_lengths(n, parts, seed):
    """uneven lengths of `parts` parts that add up to n + WINDOW rows"""
    rng = np.random.default_rng(seed)
    w = rng.random(parts) * 3.0 + 1.0
    cuts = np.round(np.cumsum(w) / w.sum() * (n + WINDOW)).astype(np.int64)
    cuts[-1] = n + WINDOW
    return np.diff(np.concatenate(([0], cuts))).tolist()


def scores_on(dev, n, d, sp, seed):
    """(n, d) per-dimension scores made on the device: noise, every part on a scale of its own"""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((n, d), generator=g, device=dev)
    scale = torch.tensor([10.0 ** (p % 5 - 2) for p in range(sp.n_parts)], device=dev)
    owner = torch.searchsorted(sp.tensors(dev)[1], torch.arange(n, device=dev), right=True)
    return x * scale[owner][:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", nargs="*", default=["73629:27", f"{1 << 20}:1024", f"{1 << 24}:1024", f"{1 << 24}:1"])
    ap.add_argument("--dims", type=int, nargs="*", default=[1, 38])
    args = ap.parse_args()
    import evaluation as ev
    if not torch.cuda.is_available():
        raise SystemExit("part_scale_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    long_rows = ev._lib().mtadgat_eval_partq_long()
    lines = [f"device: {props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} compute units, "
             f"{props.total_memory >> 30} GiB; rounds per entry: {ROUNDS} (median [min, max] ms per call, reps per round); "
             f"parts longer than {long_rows} rows keep their bins in memory"]
    checked = False
    for case in args.cases:
        n, parts = (int(v) for v in case.split(":"))
        sp = ev.score_parts(part_lengths(n, parts, seed=n % 1000), WINDOW, device=dev)
        spans = [(int(a), int(b)) for a, b in zip(sp.start_host, sp.end_host) if b > a]
        n_long = sum(b - a > long_rows for a, b in spans)
        for d in args.dims:
            x = scores_on(dev, n, d, sp, seed=n % 1000 + d)

            def loop_quantiles():
                return [ev.column_quantiles(x[a:b], QS) for a, b in spans]

            def loop_scale():
                out = torch.empty_like(x)
                for a, b in spans:
                    q = ev.column_quantiles(x[a:b], QS)
                    out[a:b] = (x[a:b] - q[1]) / (1.0 + (q[2] - q[0]))
                return out

            if not checked:                                          # the timed calls compute the same thing
                ours, theirs = ev.part_quantiles(x, QS, sp), loop_quantiles()
                rows = [p for p, (a, b) in enumerate(zip(sp.start_host, sp.end_host)) if b > a]
                assert all(torch.equal(ours[:, p], theirs[k]) for k, p in enumerate(rows))
                assert torch.allclose(ev.scale_scores(x, parts=sp), loop_scale(), rtol=1e-6, atol=1e-6)
                checked = True
            lines.append(f"n = {n}, d = {d}, {parts} parts of {min(b - a for a, b in spans)} to {max(b - a for a, b in spans)} scores "
                         f"({n_long} of them long)")
            if parts == 1:
                res = compare({"part_quantiles, one part": lambda: ev.part_quantiles(x, QS, sp),
                               "column_quantiles": lambda: ev.column_quantiles(x, QS)})
            else:
                res = compare({"part_quantiles": lambda: ev.part_quantiles(x, QS, sp), "loop: column_quantiles per slice": loop_quantiles})
                res.update(compare({"scale_scores(parts=)": lambda: ev.scale_scores(x, parts=sp), "loop: quantiles, scale per slice": loop_scale}))
            for name, (med, lo, hi, reps) in res.items():
                lines.append(f"  {name:<34s} {med:10.4f} [{lo:.4f}, {hi:.4f}]  x{reps}")
            del x
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
