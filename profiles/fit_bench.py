"""Cost of one optimisation step on windows of a series: fitting.SeriesTrainer.step beside the existing route, on the same tree and
machine, at the SMD shape (F = 38, W = 100, dropout 0.3) with 256 and 8 192 windows per step.
  trainer      SeriesTrainer.step(series, starts): the series and the window starts are on the device
  device-fed   the existing route for a series already on the device: series[starts[:, None] + arange(W)], model(x) in train mode,
               torch's sqrt(mse) + sqrt(mse), .backward(), torch.optim.Adam.step()
  loader-fed   the existing route fed as the reference feeds it: a CPU sliding-window dataset behind a shuffling DataLoader
               (utils.py's SlidingWindowDataset restated), a host-to-device copy per batch, then the same step
  method       ROUNDS rounds; in each the three routes run STEPS consecutive steps one after the other (each on its own copy of the
               model, after WARMUP steps at the timed shape).  "device" is the step-to-step period on the device's timeline: HIP
               events recorded at the top of every step, idle gaps while the host prepares the next batch included.  "host" is the
               wall time the host spends inside one step before it returns (nothing synchronises inside a step).  Reported: the
               median over all steps, and the smallest and largest of the rounds' medians.
The routes are checked to compute the same step before anything is timed: from equal weights and the same dropout stream their
parameter gradients agree to 1e-5 of each tensor's largest entry.
Usage: python profiles/fit_bench.py [--out FILE] [--sizes B ...] [--rounds R]   (a text table, also printed)"""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "mtad-gat-pytorch_amd"), ROOT, HERE]

F, W, P_DROP, N_ROWS = 38, 100, 0.3, 28479                    # SMD machine-1-1: 38 features, 28 479 training rows
WARMUP = 3
STEPS = {256: 60, 8192: 8}


class SlidingWindows(torch.utils.data.Dataset):
    """The reference's SlidingWindowDataset (utils.py): (x = data[i : i + W], y = data[i + W : i + W + 1])."""

    def __init__(self, data, window):
        self.data, self.window = data, window

    def __getitem__(self, i):
        return self.data[i:i + self.window], self.data[i + self.window:i + self.window + 1]

    def __len__(self):
        return len(self.data) - self.window


def torch_step(model, opt, x, y):
    mse = torch.nn.MSELoss()
    opt.zero_grad()
    preds, recons = model(x)
    loss = torch.sqrt(mse(y.squeeze(1), preds)) + torch.sqrt(mse(x, recons))
    loss.backward()
    opt.step()


def timed(step, steps):
    """(device periods ms, host ms per step) of `steps` consecutive calls of step()."""
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    host = []
    for k in range(steps):
        marks[k].record()
        t0 = time.perf_counter()
        step()
        host.append((time.perf_counter() - t0) * 1e3)
    marks[steps].record()
    marks[steps].synchronize()
    return [marks[k].elapsed_time(marks[k + 1]) for k in range(steps)], host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", nargs="*", type=int, default=[256, 8192])
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_bench needs the GPU: nothing is measured without one")
    import fitting
    from mtad_gat import MTAD_GAT
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    g = torch.Generator().manual_seed(1)
    host_series = torch.rand(N_ROWS, F, generator=g)
    series = host_series.to(dev)
    torch.manual_seed(0)
    base = MTAD_GAT(n_features=F, window_size=W, out_dim=F, dropout=P_DROP)
    n_params = sum(p.numel() for p in base.parameters())
    lines = [f"device: {props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} compute units; MTAD_GAT F = {F}, "
             f"W = {W}, dropout {P_DROP}, {n_params} parameters; series {N_ROWS} x {F} float32; {args.rounds} rounds, {WARMUP} warm-up steps per "
             f"route and round; ms per step: median over all steps [smallest, largest round median]"]

    # the three routes compute the same step
    arange = torch.arange(W, device=dev)
    starts = torch.randperm(N_ROWS - W, device=dev)[:64]
    a, b = copy.deepcopy(base).to(dev).train(), copy.deepcopy(base).to(dev).train()
    tr = fitting.SeriesTrainer(a, seed=5)
    b.dropout_stream = (tr.step_seed(0), 0)
    tr.step(series, starts)
    torch_step(b, torch.optim.Adam(b.parameters(), lr=1e-3), series[starts[:, None] + arange], series[starts + W].unsqueeze(1))
    import _hipgrad
    worst = 0.0
    for q, (o, n) in zip(_hipgrad.param_order(b), tr._spans):
        worst = max(worst, (tr.grads[o:o + n].view(q.shape) - q.grad).abs().max().item() / max(q.grad.abs().max().item(), 1e-30))
    assert worst <= 1e-5, worst
    pa = torch.cat([p.detach().reshape(-1) for p in _hipgrad.param_order(a)])
    pb = torch.cat([p.detach().reshape(-1) for p in _hipgrad.param_order(b)])
    diff = (pa - pb).abs().max().item()
    lines.append(f"one step from equal weights, 64 windows, the same dropout stream: gradients agree to {worst:.1e} of each tensor's largest; "
                 f"parameters after it differ by at most {diff:.1e} (lr = 1e-3)")
    del a, b, tr

    for batch in args.sizes:
        steps = STEPS.get(batch, 8)
        models = [copy.deepcopy(base).to(dev).train() for _ in range(3)]
        tr = fitting.SeriesTrainer(models[0], seed=5)
        opts = [None] + [torch.optim.Adam(m.parameters(), lr=1e-3) for m in models[1:]]
        order = torch.randperm(N_ROWS - W, device=dev)
        state = {"at": 0, "it": None}
        loader = torch.utils.data.DataLoader(SlidingWindows(host_series, W), batch_size=batch, shuffle=True, drop_last=True)

        def next_starts():
            if state["at"] + batch > order.numel():
                state["at"] = 0
            s = order[state["at"]:state["at"] + batch]
            state["at"] += batch
            return s

        def trainer_step():
            tr.step(series, next_starts())

        def device_step():
            s = next_starts()
            torch_step(models[1], opts[1], series[s[:, None] + arange], series[s + W].unsqueeze(1))

        def loader_step():
            try:
                x, y = next(state["it"])
            except (StopIteration, TypeError):
                state["it"] = iter(loader)
                x, y = next(state["it"])
            torch_step(models[2], opts[2], x.to(dev), y.to(dev))

        routes = [("trainer", trainer_step), ("device-fed", device_step), ("loader-fed", loader_step)]
        dev_ms = {name: [] for name, _ in routes}
        host_ms = {name: [] for name, _ in routes}
        for _ in range(args.rounds):
            for name, step in routes:
                for _ in range(WARMUP):
                    step()
                torch.cuda.synchronize()
                d, h = timed(step, steps)
                dev_ms[name].append(d)
                host_ms[name].append(h)
        lines.append(f"{batch} windows per step, {steps} steps per route and round")
        lines.append(f"  {'':<12s} {'device period':>34s} {'host time in the step':>34s}")
        med = {}
        for name, _ in routes:
            cells = []
            for rounds in (dev_ms[name], host_ms[name]):
                per_round = [statistics.median(r) for r in rounds]
                allm = statistics.median([v for r in rounds for v in r])
                cells.append(f"{allm:10.3f} [{min(per_round):.3f}, {max(per_round):.3f}]")
                med.setdefault(name, []).append(allm)
            lines.append(f"  {name:<12s} {cells[0]:>34s} {cells[1]:>34s}")
        lines.append(f"  trainer / device-fed: device period {med['trainer'][0] / med['device-fed'][0]:.2f}, host {med['trainer'][1] / med['device-fed'][1]:.2f};  "
                     f"trainer / loader-fed: device period {med['trainer'][0] / med['loader-fed'][0]:.2f}")
        del models, tr, opts, loader
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
