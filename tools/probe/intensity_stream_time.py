"""Timing probe of ``img.clip`` on slides that are not resident
on one GPU.

Config-2 slide (10k x 10k x 30 uint16, ``synth_slide`` on the device), three
runs of the same calls:

* (a) resident: the slide and its fp32 result in HBM (``img.from_device``);
* (b) resident raw, result deferred: a host-backed image under a budget that
  holds the raw slide and not its fp32 result;
* (c) streamed: the slide in page-locked host memory as a ``HostSource`` under
  ``MW_HBM_BUDGET=1``.

For each: the selection of ``clip()`` (pooled 0.5 / 99.5 percentiles); the
rescale of the whole slide, band by band in (b) and (c); and, after
``log_normalize(mean=...)`` and a Gaussian, the subsample and the label pass
with and without the ``clip()`` in front.  (c) also times a bare band-read loop
of the same source, the yardstick of everything that streams: a u16 selection
reads the source twice.

Host clock around each call with a device synchronisation on both sides,
warm-up, median of ``--reps``; minimum and maximum reported.

Usage:  python tools/probe/intensity_stream_time.py [--size 10000 --channels 30 --reps 3 --out FILE]
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
from milwrm_amd.MILWRM import _assign_img  # noqa: E402

CLIP_Q = (0.5, 99.5)


class _Identity:
    """A scaler that leaves the features as they are."""

    def __init__(self, F):
        self.F = F

    def affine(self):
        return np.zeros(self.F), np.ones(self.F)


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


def record(rows, run, name, ms, nbytes, note="", **extra):
    med = statistics.median(ms)
    row = dict(run=run, name=name, median_ms=round(med, 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
               reps=len(ms), bytes=int(nbytes), gb_per_s=round(nbytes / med / 1e6, 1), note=note, **extra)
    rows.append(row)
    print(json.dumps(row), flush=True)
    return med


def read_loop(src, rows):
    for _ in stream.bands(src, rows, 0):
        pass


def measure(rows, run, make, raw_src, a, n, elem, read_ms=None):
    """The calls of one run.  ``make()``: a fresh image of the slide;
    ``raw_src``: its raw pixels as a source (None: resident, whole-slide calls)."""
    F = make().n_ch
    feats = list(range(F))
    extra = {} if read_ms is None else {"read_loop_ms": round(read_ms, 3)}

    def vs(ms):
        return {} if read_ms is None else {"over_read_loop": round(statistics.median(ms) / read_ms, 3)}

    if raw_src is None:
        t = make()._device()
        ms = host_ms(lambda: D.quantiles(t, CLIP_Q, pooled=True, skip_sentinel=True), a.reps, a.warmup)
    else:
        ms = host_ms(lambda: stream.quantiles(raw_src, CLIP_Q, pooled=True, skip_sentinel=True), a.reps, a.warmup)
    record(rows, run, "selection (pooled 0.5 / 99.5), u16: two reads", ms, 2 * n * elem, **vs(ms), **extra)
    im = make()
    im.clip()
    if raw_src is None:
        tab = np.tile(np.array([[0.0, 1000.0, 0.0, 1.0, D.RESCALE_CLIP]]), (F, 1))
        out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        ms = host_ms(lambda: D.rescale(t, tab, out=out), a.reps, a.warmup)
        del out, t
    else:
        src = im._source()
        band = stream.band_rows_for(src)
        ms = host_ms(lambda: read_loop(src, band), a.reps, a.warmup)
        extra = dict(extra, band_rows=band)
    record(rows, run, "rescale of every band (read + fp32 band written)", ms, n * (elem + 4), **vs(ms), **extra)
    for clip in (True, False):
        im = make()
        if clip:
            im.clip()
        im.log_normalize(mean=np.full(F, 0.2 if clip else 100.0))
        im.blurring("gaussian", sigma=2)
        state = "deferred" if im._pending_blur is not None else "materialised"
        X = [None]

        def subsample():
            X[0] = im._subsample_device(feats, 0.2)[0]

        ms = host_ms(subsample, a.reps, a.warmup)
        tag = "after clip()" if clip else "no clip"
        record(rows, run, f"subsample 0.2, gaussian {state}, {tag}", ms, n * elem, **vs(ms))
        centers = X[0][:8].double().cpu().numpy()
        del X
        ms = host_ms(lambda: _assign_img(im, feats, centers, _Identity(F)), a.reps, a.warmup)
        record(rows, run, f"label pass k=8, gaussian {state}, {tag}", ms, n * elem, **vs(ms))
        del im
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    D.require_gpu()
    torch.cuda.set_device(0)
    H = W = a.size
    C = a.channels
    rows = []
    t, mask = D.synth_slide(H, W, C, seed=20251015)
    n = H * W * C
    elem = t.element_size()
    host = stream.pinned_empty((H, W, C), dtype=t.dtype)
    host.copy_(t)
    torch.cuda.synchronize()
    runs = a.runs.split(",")
    os.environ.pop("MW_HBM_BUDGET", None)
    if "a" in runs:
        measure(rows, "a resident", lambda: MxIF.img.from_device(t, mask=mask), None, a, n, elem)
    del t
    torch.cuda.empty_cache()
    if "b" in runs:
        # the raw slide fits the budget, its fp32 result does not
        os.environ["MW_HBM_BUDGET"] = str(int(n * elem * 1.5))
        arr = host.numpy().view(np.uint16)
        hmask = mask.cpu().numpy()
        raw = D.to_device_image(arr)  # (the selection's source; every image of the run uploads its own copy)
        measure(rows, "b resident raw, result deferred", lambda: MxIF.img(arr, mask=hmask),
                stream.DeviceSource(raw), a, n, elem)
        del raw
        torch.cuda.empty_cache()
    if "c" in runs:
        os.environ["MW_HBM_BUDGET"] = "1"
        src = stream.HostSource(host)
        band = stream.band_rows_for(src)
        ms = host_ms(lambda: read_loop(src, band), a.reps, a.warmup)
        read_ms = record(rows, "c streamed", "bare band-read loop (page-locked host memory)", ms, n * elem,
                         band_rows=band)
        before = dict(D.INTENSITY_USED)
        measure(rows, "c streamed", lambda: MxIF.img.from_source(stream.HostSource(host), mask=mask), src, a, n,
                elem, read_ms=read_ms)
        print(json.dumps({k: D.INTENSITY_USED[k] - before[k] for k in before}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
