"""Time and peak memory of MTAD_GAT.series_losses beside what the package offered before it, on the MSL shape (the shipped MSL
checkpoint's configuration with every feature an output: F = out_dim = 55, W = 100; seeded random weights) over stride-1 windows of
one device-resident series.  The method is profiles/curve_bench.py's: HIP events around a loop of calls after a warm-up at the timed shape, the entries timed alternately for
ROUNDS rounds, the median round reported with the spread.
  series_losses                          the forward chunk by chunk, each chunk's squared errors reduced where it lies
  forward_series(want_recons=False)      the floor: the same forward in one call, no reconstructions written, no loss
  forward_series + torch ops             the (n, W, out) reconstructions materialised, then the two RMSEs from torch ops
  window_sse alone                       the reduction kernel on materialised outputs: its achieved bytes / s
torch.cuda.max_memory_allocated is reported per entry above what was allocated before the call (series and model), with the
engine's cached forward workspace dropped first, so that every entry pays for the workspace it needs.
The losses of the first and the third entry are compared before anything is timed.
Usage: python profiles/series_losses_bench.py [--out FILE] [--windows N ...]   (a text table, also printed)"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "mtad-gat-pytorch_amd"), os.path.join(ROOT, "tests"), ROOT, HERE]

from curve_bench import ROUNDS, compare  # noqa: E402


def peak_bytes(fn, dev, eng):
    """Peak of the caching allocator during fn() above what was allocated before it; the engine's cached workspace is dropped first."""
    torch.cuda.synchronize(dev)
    eng._ws = None
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, nargs="*", default=[8192, 65536])
    args = ap.parse_args()
    import evaluation as ev
    import helpers
    if not torch.cuda.is_available():
        raise SystemExit("series_losses_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    from mtad_gat import MTAD_GAT
    kw = dict(helpers.Case("msl").kwargs, out_dim=55)
    torch.manual_seed(0)
    model = MTAD_GAT(**kw).eval().to(dev)
    model.check_weight_contents = False
    W, F, out = kw["window_size"], kw["n_features"], kw["out_dim"]
    lines = [f"device: {props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} compute units, "
             f"{props.total_memory >> 30} GiB; rounds per entry: {ROUNDS} (median [min, max] ms per call, reps per round)",
             f"model: MSL configuration, seeded random weights, F = {F}, out_dim = {out}, W = {W}, precision '{model.precision}'"]
    for k, n in enumerate(args.windows):
        g = torch.Generator().manual_seed(n % 1000)
        series = torch.rand(n + W, F, generator=g).to(dev)
        eng = model._sync_engine(dev)

        def losses():
            return model.series_losses(series)

        def floor():
            return eng.forward_series(series, None, 0, 1, n, want_recons=False)

        def torch_ops():
            p, r = model.forward_series(series, count=n)
            y = series[W:W + n]
            x = series.unfold(0, W, 1)[:n].permute(0, 2, 1)
            f = torch.sqrt(((p - y) ** 2).mean())
            rr = torch.sqrt(((r - x) ** 2).mean())
            return float(f), float(rr)

        ours, theirs = losses(), torch_ops()
        assert abs(ours.forecast_loss - theirs[0]) <= 1e-5 and abs(ours.recon_loss - theirs[1]) <= 1e-5, (ours, theirs)
        p, r = model.forward_series(series, count=n)

        def sse_alone():
            return ev.window_sse(p, r, series)

        res = compare({"series_losses": losses, "forward_series(want_recons=False)": floor, "forward_series + torch ops": torch_ops,
                       "window_sse alone (outputs given)": sse_alone})
        del p, r
        mem = {"series_losses": peak_bytes(losses, dev, eng), "forward_series(want_recons=False)": peak_bytes(floor, dev, eng),
               "forward_series + torch ops": peak_bytes(torch_ops, dev, eng)}
        chunk = eng.series_losses_chunk()
        lines.append(f"n = {n} windows, series ({n + W}, {F}); series_losses chunk {chunk} windows ({-(-n // chunk)} chunks), "
                     f"workspace {eng.series_losses_workspace_bytes(n) / 2 ** 20:.1f} MiB; forward chunk {eng.chunk_windows()} windows")
        for name, (med, lo, hi, reps) in res.items():
            peak = f"  peak {mem[name] / 2 ** 20:9.1f} MiB" if name in mem else ""
            lines.append(f"  {name:<36s} {med:10.4f} [{lo:.4f}, {hi:.4f}]  x{reps}{peak}")
        fl, ls, sa = res["forward_series(want_recons=False)"][0], res["series_losses"][0], res["window_sse alone (outputs given)"][0]
        read = 4.0 * n * (W + 1) * out
        lines.append(f"  series_losses over the floor: {ls - fl:+.4f} ms ({100.0 * (ls - fl) / fl:+.1f} % of the floor); window_sse alone reads "
                     f"{read / 2 ** 20:.0f} MiB of outputs at {read / (sa * 1e-3) / 1e12:.2f} TB/s")
        if ls - fl > 0.1 * fl:
            chunks = -(-n // chunk)
            lines.append(f"  MORE THAN A TENTH OF THE FLOOR.  Not the reduction ({sa:.3f} ms if run over the whole call's outputs): the floor "
                         f"leaves out the reconstruction decoder and its stores, which series_losses needs"
                         + (f", and the call runs {chunks} chunk forwards of <= {chunk} windows where the floor runs one forward: the large-batch "
                            f"recurrence costs a chunk as much as a 32 768-window piece" if chunks > 1 else "")
                         + f" (forward_series with reconstructions + torch ops: {res['forward_series + torch ops'][0]:.3f} ms).")
        del series
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
