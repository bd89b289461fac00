"""Throughput of score attribution and of the kernels behind it, timed with HIP events after warm-up:
  * attributed timestamps per second at the MSL shape, method="gradient" and Integrated Gradients with 32 steps, 256 / 4 096 indices
  * the data-only backward (mtadgat_backward_data) against the full backward (mtadgat_backward + mtadgat_backward_input)
    at 256 and 8 192 windows of the MSL shape
  * the input gradient of BASELINE config 4 (F = 512, W = 256: the wide-window convolution on the fp32 MFMA)
Usage: python profiles/attribution_bench.py [--out FILE]   (one JSON object, also printed)"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mtad-gat-pytorch_amd"), ROOT]

MSL = dict(n_features=55, window_size=100, out_dim=1, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3, forecast_hid_dim=150,
           recon_hid_dim=150, dropout=0.3, alpha=0.2)
CONFIG4 = dict(n_features=512, window_size=256, out_dim=512, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3, forecast_hid_dim=150,
               recon_hid_dim=150, dropout=0.3, alpha=0.2)


def timed(fn, reps):
    fn()                                                      # warm-up at the timed shape
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
    dev = torch.device("cuda:0")
    res = {}
    torch.manual_seed(0)
    model = MTAD_GAT(**MSL).to(dev).eval()
    W = model.window_size
    values = torch.rand(4096 + W + 1, model.n_features, device=dev)
    for count in (256, 4096):
        idx = list(range(count))
        for method, steps in (("gradient", 0), ("integrated", 32)):
            reps = 3 if count * max(steps, 1) <= 8192 else 1
            ms = timed(lambda: model.score_attribution(values, idx, [0], method=method, steps=max(steps, 1)), reps)
            res[f"attr_{method}{steps or ''}_{count}"] = dict(ms=ms, timestamps_per_s=count / ms * 1e3,
                                                              windows_per_s=2 * count * max(steps, 1) / ms * 1e3)
    eng = model._sync_engine(dev)
    for b in (256, 8192):
        x = torch.rand(b, W, model.n_features, device=dev)
        dp = torch.randn(b, model.out_dim, device=dev)
        dr = torch.randn(b, W, model.out_dim, device=dev)
        _, _, tape = eng.forward_train(x, 0.0, 0)
        _, total = eng.grad_layout()
        grads = torch.zeros(total, device=dev)

        def full():
            eng.backward(x, 0.0, 0, dp, dr, tape, grads)
            eng.backward_input(x)
        full_ms = timed(full, 5)
        data_ms = timed(lambda: eng.backward_data(x, 0.0, 0, dp, dr, tape), 5)
        res[f"backward_{b}"] = dict(full_ms=full_ms, data_only_ms=data_ms, speedup=full_ms / data_ms)
        del tape, x
    del eng, model
    torch.cuda.empty_cache()
    m4 = MTAD_GAT(**CONFIG4).to(dev).eval()
    e4 = m4._sync_engine(dev)
    b = 32
    x = torch.rand(b, 256, 512, device=dev)
    _, _, tape = e4.forward_train(x, 0.0, 0)
    _, total = e4.grad_layout()
    grads = torch.zeros(total, device=dev)
    e4.backward(x, 0.0, 0, torch.randn(b, 512, device=dev), torch.randn(b, 256, 512, device=dev), tape, grads)
    ms = timed(lambda: e4.backward_input(x), 10)
    flop = 2.0 * b * 256 * 512 * 512 * 7
    res["input_grad_config4"] = dict(windows=b, ms=ms, ms_per_window=ms / b, tflops=flop / ms / 1e9)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
