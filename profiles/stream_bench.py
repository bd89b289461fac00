"""What a StreamScorer.push costs on top of the model forward it contains, timed with HIP events after warm-up at the MSL shape
(W = 100, F = 55; DESIGN.md section 0, "streaming"):
  * push of T rows for S streams: S in {1, 64, 256, 4096} with T = 1, and S = 256 with T = 16
  * in the same process, alternating with it, eng.forward_series(..., want_recons=False, want_last=True) over the same number of
    windows of a device-resident series -- the call score_series makes, and the least a push can cost
  * the same forward through model._checked, as score_series issues it: with the weight fingerprint every model entry point
    (push included) waits for
  * the differences: push - forward_series is everything a push adds; push - checked forward is the stage and score launches,
    the window gather through start indices, and the host side of the scorer
Every figure is the median of ROUNDS rounds of REPS calls each, with the spread (min .. max) beside it.
Usage: python profiles/stream_bench.py [--out FILE]   (a table and one JSON line, also printed)"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mtad-gat-pytorch_amd"), ROOT]

MSL = dict(n_features=55, window_size=100, out_dim=1, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3, forecast_hid_dim=150,
           recon_hid_dim=150, dropout=0.3, alpha=0.2)
SHAPES = ((1, 1), (64, 1), (256, 1), (4096, 1), (256, 16))
ROUNDS = 5


def timed(fn, reps):
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mtad_gat import MTAD_GAT
    from streaming import StreamScorer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = MTAD_GAT(**MSL).to(dev).eval()
    W, F = model.window_size, model.n_features
    res, lines = {}, [f"{'streams':>8} {'T':>3} {'windows':>8} {'push ms':>22} {'forward_series ms':>22} {'checked forward ms':>22} {'push - fwd':>10} {'push - checked':>14}"]
    for S, T in SHAPES:
        windows = S * T
        reps = 200 if windows <= 256 else 50
        scorer = StreamScorer(model, S, 0.5, target_dims=[0], merge_gap=2, min_length=2, max_block=T)
        rows = torch.rand(S, T, F, device=dev)
        series = torch.rand(windows + W - 1, F, device=dev)
        eng = model._sync_engine(dev)
        model._finish_weight_check()

        def push():
            scorer.push(rows)

        def forward():
            eng.forward_series(series, None, 0, 1, windows, want_recons=False, want_last=True)

        def checked():
            model._checked(dev, False, forward_fn)

        def forward_fn(e):
            return e.forward_series(series, None, 0, 1, windows, want_recons=False, want_last=True)

        for _ in range(W // T + 3):                          # past every stream's warm-up rows, and both shapes warmed
            push()
        forward()
        checked()
        p, f, c = [], [], []
        for _ in range(ROUNDS):
            p.append(timed(push, reps))
            f.append(timed(forward, reps))
            c.append(timed(checked, reps))
        pm, fm, cm = statistics.median(p), statistics.median(f), statistics.median(c)
        res[f"S{S}_T{T}"] = dict(windows=windows, push_ms=pm, push_min=min(p), push_max=max(p), forward_ms=fm, forward_min=min(f),
                                 forward_max=max(f), checked_forward_ms=cm, checked_min=min(c), checked_max=max(c),
                                 difference_ms=pm - fm, difference_checked_ms=pm - cm)
        lines.append(f"{S:>8} {T:>3} {windows:>8} {pm:>8.3f} ({min(p):.3f}..{max(p):.3f}) {fm:>8.3f} ({min(f):.3f}..{max(f):.3f}) "
                     f"{cm:>8.3f} ({min(c):.3f}..{max(c):.3f}) {pm - fm:>10.3f} {pm - cm:>14.3f}")
        del scorer
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
