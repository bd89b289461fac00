"""Cost of training on gappy, concatenated series: the masked step beside the plain one, the window sampler beside the same selection
in torch ops, and the masked validation pass beside the plain one.  SMD shape (F = 38, W = 100, dropout 0.3), one device.
  step       SeriesTrainer.step(series, starts) and .step(series, starts, age=age) at 256 and 8 192 windows: the step-to-step period on
             the device's timeline (HIP events at the top of every step, as profiles/fit_bench.py), median over all steps and the
             smallest / largest round median.  With --parent DIR (a checkout of the parent commit with its library built) the plain
             step is also timed there, parent and change alternating, each in a process of its own: it is the same call sequence, so
             a difference beyond the run-to-run spread of profiles/fit.txt is a defect.
  sampler    fitting.training_windows (one 8-byte host read included) at 73 729 x 55 in 55 parts and 2^22 x 38 in 28 parts, gaps with
             probability 0.15, beside `torch_windows`: comparisons, cumsum, bucketize, nonzero.  Both are checked to select the same
             starts before anything is timed.
  validation MTAD_GAT.series_losses(values) and (values, age=age) at 8 192 and 65 536 windows: wall time of the call (it ends in a host
             copy of the group sums), median of the repetitions.
Usage: python profiles/fit_windows_bench.py [--out FILE] [--parent DIR] [--rounds R]   (a text table, also printed)"""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

F, W, P_DROP, N_ROWS = 38, 100, 0.3, 28479                    # SMD machine-1-1
WARMUP = 3
STEPS = {256: 60, 8192: 8}
P_GAP = 0.15


def use_tree(root):
    sys.path[:0] = [os.path.join(root, "mtad-gat-pytorch_amd"), root]


def gappy_age(n_rows, n_features, dev, seed=3):
    """int32 age of independent gaps with probability P_GAP: k at the k-th consecutive missing row (a running count in torch)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    missing = torch.rand((n_rows, n_features), device=dev, generator=g) < P_GAP
    idx = torch.arange(n_rows, device=dev)[:, None].expand(n_rows, n_features)
    last_seen = torch.cummax(torch.where(missing, torch.full_like(idx, -1), idx), dim=0).values
    return (idx - last_seen).to(torch.int32)


def timed(step, steps):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for k in range(steps):
        marks[k].record()
        step()
    marks[steps].record()
    marks[steps].synchronize()
    return [marks[k].elapsed_time(marks[k + 1]) for k in range(steps)]


def step_rounds(batch, masked, rounds):
    """[[device period ms per step] per round] of the (masked) step at `batch` windows, in this process's tree."""
    import fitting
    from mtad_gat import MTAD_GAT
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    series = torch.rand(N_ROWS, F, generator=g).to(dev)
    age = gappy_age(N_ROWS, F, dev) if masked else None
    torch.manual_seed(0)
    tr = fitting.SeriesTrainer(MTAD_GAT(n_features=F, window_size=W, out_dim=F, dropout=P_DROP).to(dev).train(), seed=5)
    order = torch.randperm(N_ROWS - W, device=dev)
    at = [0]

    def step():
        if at[0] + batch > order.numel():
            at[0] = 0
        s = order[at[0]:at[0] + batch]
        at[0] += batch
        if masked:
            tr.step(series, s, age=age)
        else:
            tr.step(series, s)
    out = []
    for _ in range(rounds):
        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize()
        out.append(timed(step, STEPS.get(batch, 8)))
    return out


def torch_windows(age, max_age, lengths, dims, min_count, window):
    """The sampler's selection in torch ops."""
    dev = age.device
    n_rows = age.shape[0]
    seen = age <= max_age
    prefix = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(seen.sum(dim=1), dim=0)])
    s = torch.arange(n_rows - window, device=dev)
    keep = (prefix[s + window] - prefix[s] >= min_count) & seen[:, dims].any(dim=1)[window:]
    offs = torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int64, device=dev)
    part = torch.bucketize(s, offs, right=True) - 1
    keep &= s + window < offs[part + 1]
    return keep.nonzero().flatten()


def cell(values_by_round):
    per_round = [statistics.median(r) for r in values_by_round]
    return f"{statistics.median([v for r in values_by_round for v in r]):10.3f} [{min(per_round):.3f}, {max(per_round):.3f}]"


def worker(args):
    use_tree(args.tree)
    print("RESULT " + json.dumps(step_rounds(args.batch, False, 1)[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_windows_bench needs the GPU: nothing is measured without one")
    if args.worker:
        return worker(args)
    use_tree(ROOT)
    import fitting
    from mtad_gat import MTAD_GAT
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    lines = [f"device: {props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} compute units; MTAD_GAT F = {F}, W = {W}, "
             f"dropout {P_DROP}; gaps with probability {P_GAP}; {args.rounds} rounds; ms: median over all repetitions [smallest, largest round median]"]

    lines.append("step: device period per step")
    for batch in (256, 8192):
        plain, masked = step_rounds(batch, False, args.rounds), step_rounds(batch, True, args.rounds)
        lines.append(f"  {batch:5d} windows   plain {cell(plain)}   with age {cell(masked)}   "
                     f"with age / plain {statistics.median(sum(masked, [])) / statistics.median(sum(plain, [])):.3f}")
        if args.parent:
            runs = {"parent": [], "change": []}
            for _ in range(args.rounds):
                for name, tree in (("parent", args.parent), ("change", ROOT)):
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--batch", str(batch)],
                                         check=True, capture_output=True, text=True, timeout=600).stdout
                    runs[name].append(json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            lines.append(f"        plain step, a process per run, parent and change alternating:   parent {cell(runs['parent'])}   "
                         f"change {cell(runs['change'])}   change / parent "
                         f"{statistics.median(sum(runs['change'], [])) / statistics.median(sum(runs['parent'], [])):.3f}")
        else:
            lines.append("        (no --parent checkout given: the plain step was not compared with the parent commit)")

    lines.append("sampler: fitting.training_windows beside the same selection in torch ops (cumsum, comparisons, bucketize, nonzero), wall ms per call")
    for n_rows, nf, parts in ((73729, 55, 55), (1 << 22, 38, 28)):
        age = gappy_age(n_rows, nf, dev)
        lengths = [n_rows // parts] * (parts - 1) + [n_rows - (n_rows // parts) * (parts - 1)]
        dims = list(range(nf))
        mc = (W * nf + 1) // 2
        got = fitting.training_windows(n_rows, W, nf, lengths=lengths, age=age, min_observed=0.5, device=dev)
        ref = torch_windows(age, 0, lengths, dims, mc, W)
        assert torch.equal(got, ref), (got.numel(), ref.numel())
        times = {"training_windows": [], "torch ops": []}
        for _ in range(args.rounds):
            for name, fn in (("training_windows", lambda: fitting.training_windows(n_rows, W, nf, lengths=lengths, age=age, min_observed=0.5, device=dev)),
                             ("torch ops", lambda: torch_windows(age, 0, lengths, dims, mc, W))):
                fn()
                torch.cuda.synchronize()
                one = []
                for _ in range(10):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    one.append((time.perf_counter() - t0) * 1e3)
                times[name].append(one)
        a, b = (statistics.median(sum(times[k], [])) for k in ("training_windows", "torch ops"))
        lines.append(f"  {n_rows:8d} x {nf} in {parts} parts, {got.numel()} of {n_rows - W} starts kept   training_windows {cell(times['training_windows'])}   "
                     f"torch ops {cell(times['torch ops'])}   training_windows / torch ops {a / b:.3f}")
        del age, got, ref
        torch.cuda.empty_cache()

    lines.append("validation: MTAD_GAT.series_losses, wall ms per call")
    torch.manual_seed(0)
    model = MTAD_GAT(n_features=F, window_size=W, out_dim=F, dropout=P_DROP).to(dev).eval()
    for n in (8192, 65536):
        g = torch.Generator().manual_seed(2)
        values = torch.rand(n + W, F, generator=g).to(dev)
        age = gappy_age(n + W, F, dev)
        times = {"plain": [], "with age": []}
        for _ in range(args.rounds):
            for name, kw in (("plain", {}), ("with age", dict(age=age))):
                model.series_losses(values, batch_size=256, **kw)
                one = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model.series_losses(values, batch_size=256, **kw)
                    one.append((time.perf_counter() - t0) * 1e3)
                times[name].append(one)
        a, b = (statistics.median(sum(times[k], [])) for k in ("with age", "plain"))
        lines.append(f"  {n:6d} windows   plain {cell(times['plain'])}   with age {cell(times['with age'])}   with age / plain {a / b:.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
