"""Timing probe of the intensity utilities on one GPU.

Config-2 slide (10k x 10k x 30 uint16, ``synth_slide`` on the device):
``nz_stats`` (the like-for-like read-once pass over the same tensor), the
exact selection (per channel, pooled, and on a half-zeros copy of the slide:
heavy ties), the rescale pass and ``img.clip(channels=all)`` end to end with
its single host read.  HIP events around each call, warm-up, median of
``--reps`` (>= 10); the end-to-end figures are host clock around a call that
ends in a device synchronise.  The selection's kernels are separate launches
of one C call: run the probe under ``rocprofv3 --kernel-trace --stats`` (a run
of its own, ``--reps 3``) for the time of each pass.

Also, at ``--cpu-size`` (2048 x 2048 x 8): ``img.clip()`` next to numpy's
``np.nanpercentile`` + the rescale arithmetic on the float64 host image, which
is what the reference's ``clip_values`` runs (numpy on the CPUs of the same
box).

Usage:  python tools/probe/intensity_time.py [--size 10000 --channels 30 --reps 12 --out FILE]
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

from milwrm_amd import MxIF  # noqa: E402
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


def host_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def record(rows, name, ms, nbytes, note=""):
    med = statistics.median(ms)
    row = dict(name=name, median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
               reps=len(ms), bytes=int(nbytes), tb_per_s=round(nbytes / med / 1e9, 3), note=note)
    rows.append(row)
    print(json.dumps(row), flush=True)


def numpy_clip_values(image):
    """The arithmetic of the reference's pooled clip_values on its float64
    image: np.nanpercentile, then rescale_intensity(..., out_range=float32)."""
    vmin, vmax = np.nanpercentile(image[image != -99999], q=(0.5, 99.5))
    omin = 0.0 if vmin >= 0 else -1.0
    x = (np.clip(image, vmin, vmax) - vmin) / (vmax - vmin)
    return np.asarray(x * (1.0 - omin) + omin, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
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
    q = (0.5, 99.5)
    record(rows, "nz_stats u16", event_ms(lambda: D.nz_stats(t), a.reps, a.warmup), 2 * n,
           "read-once yardstick, same tensor")
    record(rows, "quantiles u16 per-channel (2 passes + 2 choices)",
           event_ms(lambda: D.quantiles(t, q), a.reps, a.warmup), 2 * 2 * n)
    record(rows, "quantiles u16 pooled (2 passes + 2 choices)",
           event_ms(lambda: D.quantiles(t, q, pooled=True, skip_sentinel=True), a.reps, a.warmup), 2 * 2 * n)
    half = t.clone()
    half.mul_((torch.rand((H, W, 1), device=t.device) >= 0.5).to(torch.int16))  # probe input only
    torch.cuda.synchronize()
    record(rows, "quantiles u16 per-channel, half-zeros slide",
           event_ms(lambda: D.quantiles(half, q), a.reps, a.warmup), 2 * 2 * n, "heavy ties")
    record(rows, "quantiles u16 pooled, half-zeros slide",
           event_ms(lambda: D.quantiles(half, q, pooled=True, skip_sentinel=True), a.reps, a.warmup),
           2 * 2 * n, "heavy ties")
    del half
    st = D.d2h(D.quantiles(t, q))
    params = np.array([MxIF._clip_params(MxIF._lerp_quantile(s[0, 0], s[0, 1], s[0, 2], q[0]),
                                         MxIF._lerp_quantile(s[1, 0], s[1, 1], s[1, 2], q[1])) for s in st])
    d_params = D.h2d(params)
    out = torch.empty((H, W, C), dtype=torch.float32, device=t.device)
    record(rows, "rescale u16 -> f32 (every channel clip-rescaled)",
           event_ms(lambda: D.rescale(t, d_params, out=out), a.reps, a.warmup), 6 * n, "2 B read + 4 B written")
    record(rows, "rescale f32 in place",
           event_ms(lambda: D.rescale(out, d_params, out=out), a.reps, a.warmup), 8 * n, "4 B read + 4 B written")
    record(rows, "quantiles f32 per-channel (4 passes + 4 choices)",
           event_ms(lambda: D.quantiles(out, q), a.reps, a.warmup), 4 * 4 * n)
    del out

    def clip_all():
        im = MxIF.img.from_device(t)
        im.clip(channels=tuple(range(C)))

    record(rows, "img.clip(channels=all) end to end, u16 slide",
           host_ms(clip_all, a.reps, a.warmup), 2 * 2 * n + 6 * n, "host clock, one host read of the statistics")
    del t
    torch.cuda.empty_cache()

    if not a.no_cpu:
        h, c = a.cpu_size, a.cpu_channels
        ts, _ = D.synth_slide(h, h, c, seed=20251015)

        def clip_pooled():
            im = MxIF.img.from_device(ts)
            im.clip()

        record(rows, f"img.clip() end to end, {h}x{h}x{c} u16", host_ms(clip_pooled, a.reps, a.warmup),
               (2 * 2 + 6) * h * h * c, "host clock")
        host = ts.cpu().numpy().view(np.uint16).astype(np.float64)  # the reference's img.img
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = numpy_clip_values(host)
            ms.append((time.perf_counter() - t0) * 1e3)
        im = MxIF.img.from_device(ts)
        im.clip()
        same = bool(np.array_equal(im._dev.cpu().numpy(), ref))
        record(rows, f"numpy nanpercentile + rescale (clip_values' arithmetic), {h}x{h}x{c} float64", ms,
               8 * h * h * c, f"numpy on {len(os.sched_getaffinity(0))} CPU threads available; "
               f"device result equal: {same}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
