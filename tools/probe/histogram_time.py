"""Timing probe of the device image histogram on one GPU.

Config-2 slide (10k x 10k x 30 uint16, ``synth_slide`` on the device),
resident: ``img.histogram(None, 100)`` (the range pass, one host read of the
extremes, the count pass), ``img.histogram(None, 100, range=(0, 65535))`` (the
count pass alone) and ``nz_stats``, the like-for-like read-once pass over the
same tensor; the two kernels apart (HIP events around ``range_rows`` /
``count_rows``); the count pass over a copy of the slide in which 90 % of the
elements hold one value (the contention path) and over a uniform one.  Then one
streamed run from page-locked host memory (``--stream-rows`` rows of the
slide) next to a bare band-read loop over the same source.  HIP events around
device-only calls, host clock around calls that end in a host read; warm-up,
median of ``--reps``.

Usage:  python tools/probe/histogram_time.py [--size 10000 --channels 30 --reps 12 --out FILE]
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
from milwrm_amd import stream  # noqa: E402


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


def kernels(rows, t, label, reps, warmup, bins=100, rng=None):
    """The range and the count kernel of ``t`` apart."""
    C = int(t.shape[2])
    n = t.numel() * t.element_size()
    st = D.HistogramRows(t.dtype, C, list(range(C)), bins)
    if rng is None:
        record(rows, f"range pass, {label}", event_ms(lambda: st.range_rows(t), reps, warmup), n)
    st.set_range(rng)
    record(rows, f"count pass, {label}, {bins} bins", event_ms(lambda: st.count_rows(t), reps, warmup), n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream-rows", type=int, default=2500, help="rows of the slide in the streamed run")
    ap.add_argument("--band-rows", type=int, default=625)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    D.require_gpu()
    torch.cuda.set_device(0)
    H = W = a.size
    C = a.channels
    rows = []
    t, _ = D.synth_slide(H, W, C, seed=20251015)
    n = H * W * C
    im = MxIF.img.from_device(t)
    record(rows, "nz_stats u16", event_ms(lambda: D.nz_stats(t), a.reps, a.warmup), 2 * n,
           "read-once yardstick, same tensor")
    record(rows, "img.histogram(None, 100) end to end", host_ms(lambda: im.histogram(None, 100), a.reps, a.warmup),
           2 * 2 * n, "host clock: range pass, host read of the extremes, count pass, host read of the counts")
    record(rows, "img.histogram(None, 100, range=(0, 65535)) end to end",
           host_ms(lambda: im.histogram(None, 100, range=(0, 65535)), a.reps, a.warmup), 2 * n,
           "host clock: count pass, host read of the counts")
    kernels(rows, t, "synthetic slide", a.reps, a.warmup)
    kernels(rows, t, "synthetic slide", a.reps, a.warmup, bins=100, rng=(0, 65535))
    kernels(rows, t, "synthetic slide", a.reps, a.warmup, bins=1000, rng=(0, 65535))
    one = t[:, :, :1].contiguous()
    record(rows, "img.histogram(0, 100) of the slide, one channel of 30 selected",
           host_ms(lambda: im.histogram(0, 100), a.reps, a.warmup), 2 * 2 * n, "host clock")
    kernels(rows, one, "one-channel image", a.reps, a.warmup)
    del one
    # probe inputs only: a uniform slide, and one in which 90 % of the elements hold one value
    uni = torch.randint(0, 65536, (H, W, C), device=t.device, dtype=torch.int32).to(torch.int16)
    kernels(rows, uni, "uniform random slide", a.reps, a.warmup, rng=(0, 65535))
    dom = torch.where(torch.rand((H, W, C), device=t.device) < 0.9, torch.full_like(uni, 300), uni)
    del uni
    kernels(rows, dom, "90 % one value (scattered)", a.reps, a.warmup, rng=(0, 65535))
    dom[: (9 * H) // 10] = 300
    kernels(rows, dom, "90 % one value (contiguous background rows)", a.reps, a.warmup, rng=(0, 65535))
    del dom
    torch.cuda.empty_cache()

    # streamed: the first rows of the slide in page-locked host memory, read in bands
    hs = min(H, a.stream_rows)
    host = torch.empty((hs, W, C), dtype=torch.int16, pin_memory=True)
    host.copy_(t[:hs])
    torch.cuda.synchronize()
    del t, im
    torch.cuda.empty_cache()
    src = stream.HostSource(host)
    nb = hs * W * C * 2

    def read_only():
        for _ in stream.bands(src, a.band_rows, 0):
            pass

    reps = max(3, a.reps // 3)
    record(rows, f"bare band-read loop, {hs} rows from page-locked memory", host_ms(read_only, reps, 1), nb,
           f"bands of {a.band_rows} rows")
    record(rows, "stream.histogram(range=(0, 65535)), same source",
           host_ms(lambda: stream.histogram(src, None, 100, (0, 65535), band_rows=a.band_rows), reps, 1), nb,
           "one read of the source")
    record(rows, "stream.histogram(range=None), same source",
           host_ms(lambda: stream.histogram(src, None, 100, None, band_rows=a.band_rows), reps, 1), 2 * nb,
           "two reads of the source")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
