"""Timing probe of the bilateral filter on one GPU.

Config-2 slide (10k x 10k x 30 uint16, ``synth_slide`` on the device):
``mw_bilateral`` at sigma 1 (7 x 7 taps) and sigma 2 (13 x 13), raw uint16 with
the log-normalise fused into the load and the fp32 log-normalised slide, plus
``image_moments`` (what sigma_color="std" and the constant-image rule cost) and
``lognorm`` as the read-and-write yardstick.  HIP events around each call, one
warm-up, median of ``--reps`` with min and max.

Also, at ``--cpu-size`` (a 512 x 512 x channels crop of the log-normalised
slide): the float64 numpy brute force of tests/golden/make_golden_bilateral.py
on the CPUs of the same box, its time scaled by area to the whole slide, and the
device result's largest difference from it.

Usage:  python tools/probe/bilateral_time.py [--size 10000 --channels 30 --reps 3 --out FILE]
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

from milwrm_amd import _native as N  # noqa: E402
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


def record(rows, name, ms, note=""):
    row = dict(name=name, median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3),
               max_ms=round(max(ms), 3), reps=len(ms), note=note)
    rows.append(row)
    print(json.dumps(row), flush=True)
    return row["median_ms"]


def kernel(t, sigma, sc, inv, out):
    """mw_bilateral alone (D.bilateral adds the moments pass and a host read)."""
    H, W, C = t.shape
    r = D.bilateral_args(sigma, sc)[2]
    N.call("mw_bilateral", D.P(t), D.dtype_code(t), H, W, C, r, float(sigma), float(sc), 0, 0.0, D.P(inv), 1.0,
           D.P(out), D.stream())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sigmas", default="1,2")
    ap.add_argument("--cpu-size", type=int, default=512)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    D.require_gpu()
    torch.cuda.set_device(0)
    H = W = a.size
    C = a.channels
    rows = []
    t, _ = D.synth_slide(H, W, C, seed=20251015)
    inv = D.h2d((1.0 / np.linspace(300.0, 9000.0, C)).astype(np.float32))
    ln = torch.empty((H, W, C), dtype=torch.float32, device=t.device)
    out = torch.empty_like(ln)
    record(rows, "lognorm u16 -> f32", event_ms(lambda: D.lognorm(t, inv, 1.0, out=ln), a.reps, a.warmup),
           "read-and-write yardstick")
    record(rows, "image_moments u16, lognorm load", event_ms(lambda: D.image_moments(t, inv, 1.0), a.reps, a.warmup),
           "two passes + the host read")
    sc = D.image_std(ln)
    print(json.dumps({"sigma_color": sc}), flush=True)
    for sigma in [float(x) for x in a.sigmas.split(",")]:
        n = 2 * D.bilateral_args(sigma, sc)[2] + 1
        record(rows, f"bilateral sigma {sigma:g} ({n}x{n}) u16, fused lognorm -> f32",
               event_ms(lambda: kernel(t, sigma, sc, inv, out), a.reps, a.warmup))
        record(rows, f"bilateral sigma {sigma:g} ({n}x{n}) f32 -> f32",
               event_ms(lambda: kernel(ln, sigma, sc, None, out), a.reps, a.warmup))

    if not a.no_cpu:
        import importlib.util

        spec = importlib.util.spec_from_file_location(
            "make_golden_bilateral", os.path.join(ROOT, "tests", "golden", "make_golden_bilateral.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        brute_bilateral = gen.brute_bilateral  # one tap at a time: no window array in memory

        h = min(a.cpu_size, H)
        crop = ln[:h, :h].contiguous()
        host = crop.cpu().numpy()
        for sigma in [float(x) for x in a.sigmas.split(",")]:
            t0 = time.perf_counter()
            ref = brute_bilateral(host, sigma, sc)
            ms = (time.perf_counter() - t0) * 1e3
            got = D.bilateral(crop, sigma, sc).cpu().numpy()
            err = float(np.abs(got - ref).max() / np.abs(host).max())
            record(rows, f"numpy float64 brute force sigma {sigma:g}, {h}x{h}x{C} crop", [ms],
                   f"scaled by area to {H}x{W}: {ms * (H / h) * (W / h) / 1e3:.0f} s; device max error / max|a| "
                   f"{err:.2e}; {len(os.sched_getaffinity(0))} CPU threads available")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
