"""Time of the preparation step (preparation.fit_scaler, SeriesScaler.transform under each fill policy, StreamPreparer.push) beside
the same work written in torch ops on the same device, and the memory rate each call of ours achieves.
  method    HIP events around ONE call, WARMUP calls at the timed shape first, then RUNS timed calls of ours and of the torch
            formulation alternately; the median is reported with the minimum and maximum
  sizes     (73 729 x 55) -- the MSL test series --, (2^20 x 38) and (2^22 x 55) float32, 3 % of the samples missing in runs of 1 to 30
  torch     fit: isfinite + where + amin / amax and the three vector operations; zero / none: isfinite + where, mul, add;
            hold: cummax over the row indices of the valid samples + gather + where, mul, add; push: the same state update on
            (S, d) tensors (S = 256 streams, one row each)
  bytes     what the call has to move: fit one read of the array; zero / none one read and one write; hold two reads (the block tails,
            then the resolve pass) and one write, plus 12 bytes of carry per (column, block of rows_per_block() rows)
The torch results are checked against ours at the first size before anything is timed.
Usage: python profiles/prep_bench.py [--out FILE] [--cases N:D ...]   (a text table, also printed)"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "mtad-gat-pytorch_amd"), ROOT, HERE]

WARMUP, RUNS, STREAMS = 3, 20, 256


def raw(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32) * rng.uniform(0.1, 50.0, d).astype(np.float32) + rng.uniform(-100.0, 100.0, d).astype(np.float32)
    flat = x.reshape(-1, order="F")                              # runs go down a column
    for at in rng.integers(0, n * d, max(1, n * d // 500)):
        flat[at:at + int(rng.integers(1, 31))] = np.nan
    return np.ascontiguousarray(flat.reshape(d, n).T)


def one_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def compare(ours, stock):
    """((median, min, max) ms of ours, the same of the torch formulation), RUNS single calls each, alternately"""
    for _ in range(WARMUP):
        ours()
        stock()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(RUNS):
        a.append(one_ms(ours))
        b.append(one_ms(stock))
    return tuple((statistics.median(v), min(v), max(v)) for v in (a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", nargs="*", default=["73729:55", f"{1 << 20}:38", f"{1 << 22}:55"])
    args = ap.parse_args()
    import preparation
    if not torch.cuda.is_available():
        raise SystemExit("prep_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    rb = preparation.rows_per_block()
    lines = [f"device: {props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} compute units, "
             f"{props.total_memory >> 30} GiB; {RUNS} single calls per entry after {WARMUP} warm-up calls, HIP events: "
             f"median [min, max] ms per call; rows per block {rb}"]
    for k, case in enumerate(args.cases):
        n, d = (int(v) for v in case.split(":"))
        x = torch.from_numpy(raw(n, d, seed=n % 1000)).to(dev)
        scaler = preparation.fit_scaler(x)
        rec = scaler.record
        scale, offset, mean = rec[:, 2].contiguous(), rec[:, 3].contiguous(), rec[:, 4].contiguous()
        rows_idx = torch.arange(n, device=dev)[:, None]
        inf = torch.tensor(float("inf"), device=dev)
        tiny = torch.tensor(10.0 * 1.1920929e-07, device=dev)

        def stock_fit():
            ok = torch.isfinite(x)
            lo, hi = torch.where(ok, x, inf).amin(dim=0), torch.where(ok, x, -inf).amax(dim=0)
            rng = hi - lo
            s = 1.0 / torch.where(rng < tiny, torch.ones_like(rng), rng)
            return lo, hi, s, 0.0 - lo * s, torch.where(ok, x, torch.zeros_like(x)).sum(dim=0, dtype=torch.float64) / ok.sum(dim=0)

        def stock_zero():
            return torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0) * scale + offset

        def stock_none():
            return torch.where(torch.isfinite(x), x, torch.nan) * scale + offset

        def stock_hold():
            ok = torch.isfinite(x)
            last = torch.where(ok, rows_idx, -1).cummax(dim=0).values
            held = torch.gather(x, 0, last.clamp(min=0))
            return torch.where(ok, x, torch.where(last >= 0, held, mean)) * scale + offset

        prep = preparation.StreamPreparer(scaler, STREAMS, fill="hold")
        live = x[:STREAMS].contiguous()
        has = torch.zeros(STREAMS, d, dtype=torch.bool, device=dev)
        val = torch.zeros(STREAMS, d, device=dev)

        def stock_push():
            ok = torch.isfinite(live)
            has.logical_or_(ok)
            val.copy_(torch.where(ok, live, val))
            return torch.where(ok, live, torch.where(has, val, mean)) * scale + offset

        if k == 0:                                               # the timed calls compute the same thing
            lo, hi, s, o, m = stock_fit()
            got = scaler.read()
            assert np.array_equal(got["lo"], lo.cpu().numpy()) and np.array_equal(got["hi"], hi.cpu().numpy())
            assert np.allclose(got["mean"], m.cpu().numpy(), rtol=1e-6)
            for fill, stock in (("zero", stock_zero), (None, stock_none), ("hold", stock_hold)):
                assert torch.allclose(scaler.transform(x, fill=fill), stock(), rtol=1e-6, atol=1e-6, equal_nan=True), fill
        cells = n * d * 4
        carry = 12 * d * ((n + rb - 1) // rb)
        entries = [("fit_scaler", lambda: preparation.fit_scaler(x), stock_fit, cells),
                   ("transform(fill='zero')", lambda: scaler.transform(x, fill="zero"), stock_zero, 2 * cells),
                   ("transform(fill=None)", lambda: scaler.transform(x, fill=None), stock_none, 2 * cells),
                   ("transform(fill='hold')", lambda: scaler.transform(x, fill="hold"), stock_hold, 3 * cells + 2 * carry),
                   (f"StreamPreparer.push S={STREAMS} T=1", lambda: prep.push(live), stock_push, None)]
        lines.append(f"n = {n}, d = {d} ({cells / 2 ** 20:.0f} MiB)")
        for name, ours, stock, nbytes in entries:
            (med, lo_, hi_), (smed, slo, shi) = compare(ours, stock)
            rate = f"  {nbytes / med / 1e9:7.3f} TB/s" if nbytes else ""
            lines.append(f"  {name:<34s} {med:9.4f} [{lo_:.4f}, {hi_:.4f}]{rate}")
            lines.append(f"  {'  torch ops':<34s} {smed:9.4f} [{slo:.4f}, {shi:.4f}]   ours / torch = {med / smed:.2f}")
        x = rows_idx = live = None
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
