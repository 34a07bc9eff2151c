"""Timing probe of the median filter on one GPU.

Config-2 slide (10k x 10k x 30 uint16, ``synth_slide`` on the device):
``D.median`` at sizes 2, 3, 5 (selection network), 7 and 9 (rank search), each
with and without the lognorm epilogue, and in the same run on the same tensor
the yardsticks: ``nz_stats`` (a read-once pass), ``rescale`` uint16 -> fp32 (a
read-and-write pass of the epilogue case's byte shape) and ``D.median(s)``
followed by ``D.lognorm`` (what the epilogue replaces).  HIP events around each
call, warm-up, median of ``--reps`` with min and max; every row also as a
fraction of the rescale yardstick.  The slow sizes take fewer repeats
(``--slow-reps``).

Also, at ``--cpu-size`` (one 2048 x 2048 float64 plane): scipy's
``median_filter`` (what skimage's ``filters.median`` runs) for 3x3 and 5x5 on
the CPUs of the same box, next to ``D.median`` of the same plane as uint16.

Usage:  python tools/probe/median_time.py [--size 10000 --channels 30 --reps 10 --out FILE]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="2,3,5,7,9")
    ap.add_argument("--cpu-size", type=int, default=2048)
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
    inv = D.h2d((1.0 / np.linspace(300.0, 9000.0, C)).astype(np.float32))
    out16 = torch.empty_like(t)
    out32 = torch.empty((H, W, C), dtype=torch.float32, device=t.device)
    params = np.zeros((C, 5))
    params[:, 1] = 65535.0
    params[:, 3] = 1.0
    params[:, 4] = D.RESCALE_CLIP
    d_params = D.h2d(params)

    record(rows, "nz_stats u16", event_ms(lambda: D.nz_stats(t), a.reps, a.warmup), 2 * n,
           "read-once yardstick, same tensor")
    base = record(rows, "rescale u16 -> f32", event_ms(lambda: D.rescale(t, d_params, out=out32), a.reps, a.warmup),
                  6 * n, "read-and-write yardstick: 2 B read + 4 B written")
    record(rows, "lognorm u16 -> f32", event_ms(lambda: D.lognorm(t, inv, 1.0, out=out32), a.reps, a.warmup),
           6 * n, "the standalone pass the epilogue replaces")
    for s in [int(x) for x in a.sizes.split(",")]:
        network = s in (2, 3, 5)
        reps = a.reps if network else a.slow_reps
        warm = a.warmup if network else 1
        path = "network" if network else "rank search"
        cases = (
            (f"median {s}x{s} u16 -> u16 ({path})", lambda: D.median(t, s, out=out16), 4 * n),
            (f"median {s}x{s} u16 -> f32, lognorm epilogue ({path})",
             lambda: D.median(t, s, inv, 1.0, out=out32), 6 * n),
            (f"median {s}x{s} u16 -> u16 then lognorm -> f32 (two calls)",
             lambda: D.lognorm(D.median(t, s, out=out16), inv, 1.0, out=out32), 10 * n),
        )
        for name, fn, nbytes in cases:
            med = record(rows, name, event_ms(fn, reps, warm), nbytes)
            rows[-1]["of_rescale"] = round(med / base, 3)
            print(json.dumps({"name": name, "of_rescale": rows[-1]["of_rescale"]}), flush=True)
    del t, out16, out32
    torch.cuda.empty_cache()

    if not a.no_cpu:
        from scipy.ndimage import median_filter

        h = a.cpu_size
        plane = np.random.default_rng(3).integers(0, 65536, size=(h, h)).astype(np.uint16)
        dev = D.to_device_image(plane[:, :, None])
        host = plane.astype(np.float64)  # the reference's img.img plane
        for s in (3, 5):
            ms = []
            for _ in range(2):
                t0 = time.perf_counter()
                ref = median_filter(host, footprint=np.ones((s, s)), mode="nearest")
                ms.append((time.perf_counter() - t0) * 1e3)
            got = D.median(dev, s).cpu().numpy().view(np.uint16)[:, :, 0]
            same = bool(np.array_equal(got.astype(np.float64), ref))
            record(rows, f"scipy median_filter {s}x{s}, {h}x{h} float64 plane", ms, 16 * h * h,
                   f"scipy on {len(os.sched_getaffinity(0))} CPU threads available; device result equal: {same}")
            record(rows, f"median {s}x{s} u16, {h}x{h}x1", event_ms(lambda: D.median(dev, s), a.reps, a.warmup),
                   4 * h * h)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
