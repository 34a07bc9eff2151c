"""Timing probe of the device CLAHE on one GPU.

Config-2 slide (10k x 10k x 30 uint16, ``synth_slide`` on the device):
``D.clahe`` end to end with ``kernel_size=None`` (an eighth of the image per
axis) and ``kernel_size=64``, beside two comparators taken in the same run on
the same tensor: ``nz_stats`` (the read-once yardstick) and ``mw_rescale``
uint16 -> fp32.  HIP events around each call, warm-up, median of ``--reps``
(>= 10) with the minimum and maximum reported.  The algorithmic bytes of
CLAHE per uint16 element: 2 (histogram read) + 2 (map read) + 4 (write) + 8
(in-place rescale); the range pass reads 2 more.

The stages are separate kernels of one C call: run the probe under
``rocprofv3 --kernel-trace --stats`` (a run of its own, ``--reps 3 --no-cpu``)
for the time of each stage.

Also, at ``--cpu-size`` (2048 x 2048 x 8): ``D.clahe`` next to the float64
numpy oracle of the definition (tests/clahe_oracle.py) on the CPUs of the same
box, and whether the two agree bit for bit.

Usage:  python tools/probe/clahe_time.py [--size 10000 --channels 30 --reps 12 --out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from milwrm_amd import device as D  # noqa: E402


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return ms


def record(rows, name, ms, nbytes, note=""):
    med = statistics.median(ms)
    row = dict(name=name, median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
               reps=len(ms), bytes=int(nbytes), tb_per_s=round(nbytes / med / 1e9, 3), note=note)
    rows.append(row)
    print(json.dumps(row), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", default="none,64", help="comma-separated kernel sizes; 'none' is the default kernel")
    ap.add_argument("--cpu-size", type=int, default=2048)
    ap.add_argument("--cpu-channels", type=int, default=8)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    D.require_gpu()
    torch.cuda.set_device(0)
    H = W = a.size
    C = a.channels
    rows = []
    t, _ = D.synth_slide(H, W, C, seed=20251015)
    n = H * W * C
    nz = record(rows, "nz_stats u16", event_ms(lambda: D.nz_stats(t), a.reps, a.warmup), 2 * n,
                "read-once yardstick, same tensor")
    out = torch.empty((H, W, C), dtype=torch.float32, device=t.device)
    params = np.zeros((C, 5))
    params[:] = (0.0, 65535.0, 0.0, 1.0, D.RESCALE_SCALE)
    d_params = D.h2d(params)
    record(rows, "rescale u16 -> f32", event_ms(lambda: D.rescale(t, d_params, out=out), a.reps, a.warmup), 6 * n,
           "2 B read + 4 B written")
    record(rows, "rescale f32 in place", event_ms(lambda: D.rescale(out, d_params, out=out), a.reps, a.warmup),
           8 * n, "4 B read + 4 B written")
    for ks in a.kernels.split(","):
        k = None if ks.strip().lower() == "none" else int(ks)
        kh, kw, _, _ = D.clahe_args(H, W, k)
        med = record(rows, f"clahe u16 kernel_size={k} ({kh} x {kw}), end to end",
                     event_ms(lambda: D.clahe(t, k, out=out), a.reps, a.warmup), 16 * n,
                     "algorithmic bytes: 2 + 2 + 4 + 8 per element (the range pass reads 2 more)")
        rows[-1]["times_nz_stats"] = round(med / nz, 2)
        print(json.dumps({"name": rows[-1]["name"], "times_nz_stats": rows[-1]["times_nz_stats"]}), flush=True)
    del t, out
    torch.cuda.empty_cache()

    if not a.no_cpu:
        import clahe_oracle as O

        h, c = a.cpu_size, a.cpu_channels
        ts, _ = D.synth_slide(h, h, c, seed=20251015)
        o2 = torch.empty((h, h, c), dtype=torch.float32, device=ts.device)
        record(rows, f"clahe u16 kernel_size=None, {h}x{h}x{c}",
               event_ms(lambda: D.clahe(ts, None, out=o2), a.reps, a.warmup), 16 * h * h * c)
        host = ts.cpu().numpy().view(np.uint16)
        t0 = time.perf_counter()
        ref, ref_luts = O.clahe(host, None)
        ms = [(time.perf_counter() - t0) * 1e3]
        got, luts = D.clahe(ts, None, luts=True)
        same = bool(np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)))
        same_luts = bool(np.array_equal(luts.cpu().numpy(), ref_luts))
        record(rows, f"numpy oracle of the definition, {h}x{h}x{c} float64", ms, 8 * h * h * c,
               f"numpy on {len(os.sched_getaffinity(0))} CPU threads available; device pixels equal bit for bit: "
               f"{same}; tables equal: {same_luts}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
