"""Time of the part-aware score passes (evaluation.adjust_part_scores, moving_average(parts=), find_epsilon_parts) beside the obvious
composition of what the package had before them: a Python loop over the parts on the same device.  The method is
profiles/curve_bench.py's: HIP events around a loop of calls after a warm-up at the timed shape, every pair (ours, loop) timed
alternately for ROUNDS rounds, the median round reported with the spread.
  sizes and parts   n = 73 629 scores in 27 parts (the MSL test series and its channels), 2^20 and 2^24 scores in 1 024 parts; part
                    lengths vary by a factor of about four, every part on a scale of its own
  adjust_part_scores        against: clone, zero a slice per seam, then per part min / max of the slice and (x - lo) / (hi - lo)
  moving_average(parts=)    against: moving_average of every part's slice, written into one output
  find_epsilon_parts        against: find_epsilon of every part's slice (two synchronisations per part; ours has two per call)
The loop's results are checked against ours at the first size before anything is timed.
Usage: python profiles/parts_bench.py [--out FILE] [--cases N:P ...]   (a text table, also printed)"""
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
SPAN = 1280


def series(n, parts, seed):
    """(scores, lengths): noise with a few bursts per part, the parts' lengths uneven and every part on a scale of its own."""
    rng = np.random.default_rng(seed)
    w = rng.random(parts) * 3.0 + 1.0
    cuts = np.round(np.cumsum(w) / w.sum() * (n + WINDOW)).astype(np.int64)
    cuts[-1] = n + WINDOW
    lengths = np.diff(np.concatenate(([0], cuts)))
    scores = rng.random(n) * 0.1
    for at in rng.integers(0, max(1, n - 12), max(3, n // 4000)):
        scores[at:at + int(rng.integers(1, 12))] += 1.0 + 2.0 * rng.random()
    start = np.maximum(np.concatenate(([0], cuts[:-1])) - WINDOW, 0)
    end = np.maximum(cuts - WINDOW, 0)
    for p in range(parts):
        scores[start[p]:end[p]] *= 10.0 ** (p % 5 - 2)
    return scores.astype(np.float32), lengths.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", nargs="*", default=["73629:27", f"{1 << 20}:1024", f"{1 << 24}:1024"])
    args = ap.parse_args()
    import evaluation as ev
    if not torch.cuda.is_available():
        raise SystemExit("parts_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    lines = [f"device: {props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} compute units, "
             f"{props.total_memory >> 30} GiB; rounds per entry: {ROUNDS} (median [min, max] ms per call, reps per round)"]
    for k, case in enumerate(args.cases):
        n, parts = (int(v) for v in case.split(":"))
        scores, lengths = series(n, parts, seed=n % 1000)
        s = torch.from_numpy(scores).to(dev)
        sp = ev.score_parts(lengths, WINDOW, device=dev)
        spans = [(int(a), int(b)) for a, b in zip(sp.start_host, sp.end_host) if b > a]
        seams = [int(t) for t in sp.seams_host]
        before, after = sp.transition

        def loop_adjust():
            x = s.clone()
            for t in seams:
                x[max(t - before, 0):t + after + 1] = 0.0
            for a, b in spans:
                v = x[a:b]
                lo, hi = v.min(), v.max()
                x[a:b] = (v - lo) / (hi - lo)
            return x

        def loop_ewm():
            out = torch.empty_like(s)
            for a, b in spans:
                out[a:b] = ev.moving_average(s[a:b], SPAN)
            return out

        def loop_epsilon():
            return [ev.find_epsilon(s[a:b]) for a, b in spans]

        if k == 0:                                               # the timed calls compute the same thing
            assert float((ev.adjust_part_scores(s, sp) - loop_adjust()).abs().max()) <= 1e-6
            assert torch.allclose(ev.moving_average(s, SPAN, parts=sp), loop_ewm(), rtol=3e-7, atol=0)
            ours, theirs = ev.find_epsilon_parts(s, sp), np.array(loop_epsilon())
            assert np.all(np.abs(ours - theirs) <= 1e-9 * np.abs(theirs)), (ours, theirs)
        res = compare({"adjust_part_scores": lambda: ev.adjust_part_scores(s, sp), "loop: min / max per slice": loop_adjust})
        res.update(compare({"moving_average(parts=)": lambda: ev.moving_average(s, SPAN, parts=sp), "loop: moving_average per slice": loop_ewm}))
        res.update(compare({"find_epsilon_parts": lambda: ev.find_epsilon_parts(s, sp), "loop: find_epsilon per slice": loop_epsilon}))
        lines.append(f"n = {n}, {parts} parts of {min(b - a for a, b in spans)} to {max(b - a for a, b in spans)} scores, {len(seams)} seams, "
                     f"transition {sp.transition}, span {SPAN}")
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
