"""Time of the event table (evaluation.anomaly_events) against the host route it replaces, and the bandwidth of the segmented
reductions behind it ("From scores to events").  Device times are HIP events after a warm-up at the timed
shape, repeated to fill about half a second; the host route is scores.cpu() + per_dim.cpu() + the numpy reference of
tests/event_refs.py for the same result, on a host clock after a device synchronise, copies included.
  sizes      n = 73 629, d = 1 (the MSL test series) and n = 2^22, d = 38 (a long SMD-shaped series)
  densities  about 1 % and about 30 % of the samples above the threshold, in bursts of 20-200 samples
  run_stats  mtadgat_eval_run_stats alone on preallocated buffers; bytes = (flagged rows x d + n) x 4
Usage: python profiles/events_bench.py [--out FILE]   (one JSON object, also printed)"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mtad-gat-pytorch_amd"), os.path.join(ROOT, "tests"), ROOT]

THRESHOLD = 0.55
OPTIONS = dict(merge_gap=2, min_length=2, top_k=5)


def series(n, d, density, seed):
    """Scores below the threshold except in bursts that cover about `density` of the samples; the per-dimension scores rise with them."""
    rng = np.random.default_rng(seed)
    scores = (rng.random(n) * 0.5).astype(np.float32)
    per_dim = (rng.random((n, d)) * 0.5).astype(np.float32)
    for at in rng.integers(0, n - 200, max(1, int(density * n / 110))):
        length = int(rng.integers(20, 201))
        scores[at:at + length] = 0.6 + 0.4 * rng.random(length)
        per_dim[at:at + length, ::3] += 0.5
    return scores, per_dim


def timed(fn, seconds=0.5):
    fn()                                                      # warm-up at the timed shape
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    reps = max(3, min(2000, int(seconds * 1e3 / max(t0.elapsed_time(t1), 1e-3))))
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import evaluation as ev
    import event_refs
    dev = torch.device("cuda:0")
    lib = ev._lib()
    res = {}
    for name, n, d in (("msl", 73729 - 100, 1), ("smd_long", 1 << 22, 38)):
        for density in (0.01, 0.30):
            scores, per_dim = series(n, d, density, seed=n % 1000 + int(100 * density))
            thr = np.full(d, 0.9)
            s, pd = torch.from_numpy(scores).to(dev), torch.from_numpy(per_dim).to(dev)
            got = ev.anomaly_events(s, THRESHOLD, per_dim=pd, feature_thresholds=thr, **OPTIONS)
            dev_ms, dev_reps = timed(lambda: ev.anomaly_events(s, THRESHOLD, per_dim=pd, feature_thresholds=thr, **OPTIONS))

            def host():
                return event_refs.events(s.cpu().numpy(), THRESHOLD, pd.cpu().numpy(), thr, **OPTIONS)
            ref = host()
            assert ref["count"] == got["count"] and np.array_equal(ref["peak"], got["peak"].cpu().numpy())
            torch.cuda.synchronize()
            host_reps = 3
            t0 = time.perf_counter()
            for _ in range(host_reps):
                host()
            host_ms = (time.perf_counter() - t0) / host_reps * 1e3
            t0 = time.perf_counter()
            for _ in range(host_reps):
                s.cpu(), pd.cpu()
            copy_ms = (time.perf_counter() - t0) / host_reps * 1e3

            count, start, end = got["count"], got["start"], got["end"]
            rows = int((end - start).sum())
            nbytes = lib.mtadgat_eval_run_stats_scratch(n, count, d)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            thr_d = torch.tensor(thr, dtype=torch.float64, device=dev)
            k = got["top_features"].shape[1]
            o = [torch.empty(count, dtype=torch.int64, device=dev), torch.empty(count, device=dev), torch.empty(count, device=dev),
                 torch.empty(count, d, device=dev), torch.empty(count, k, dtype=torch.int32, device=dev), torch.empty(count, k, device=dev),
                 torch.empty(count, d, dtype=torch.int32, device=dev)]
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def stats():
                rc = lib.mtadgat_eval_run_stats(s.data_ptr(), n, start.data_ptr(), end.data_ptr(), count, pd.data_ptr(), d, pd.stride(0),
                                                thr_d.data_ptr(), k, scratch.data_ptr(), nbytes, *[t.data_ptr() for t in o], stream)
                assert rc == 0, lib.mtadgat_last_error().decode()
            stats_ms, stats_reps = timed(stats)
            assert torch.equal(o[0], got["peak"]) and torch.equal(o[3], got["feature_means"])
            moved = (rows * d + n) * 4
            res[f"{name}_{int(100 * density)}pct"] = dict(
                n=n, d=d, flagged_fraction=float((scores > THRESHOLD).mean()), events=count, flagged_rows=rows,
                device_ms=dev_ms, device_reps=dev_reps, host_route_ms=host_ms, host_copies_ms=copy_ms, host_over_device=host_ms / dev_ms,
                run_stats_ms=stats_ms, run_stats_reps=stats_reps, run_stats_bytes=moved, run_stats_gb_per_s=moved / stats_ms / 1e6)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
