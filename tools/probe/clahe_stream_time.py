"""Timing probe of ``img.equalize_hist(kernel_size=k, banded=True)`` on slides
that are not resident on one GPU.

Config-2 slide (10k x 10k x 30 uint16, ``synth_slide`` on the device), two runs:

* (c) streamed: the slide in page-locked host memory as a ``HostSource`` under
  ``MW_HBM_BUDGET=1``: the call (three reads of the source plus the table
  stage) against one bare band-read loop of the same source; a read loop of
  the equalised source; and, after ``log_normalize(mean=...)`` and a Gaussian,
  the subsample and the label pass with and without the ``equalize_hist`` in
  front;
* (b) resident raw, result deferred: a host-backed image under a budget that
  holds the raw slide and not its fp32 result: the same calls, against
  ``D.clahe`` of the resident slide end to end.

Host clock around each call with a device synchronisation on both sides,
warm-up, median of ``--reps``; minimum and maximum reported.  ``--trace`` runs
each stage once and nothing else: the run to put under a kernel trace.

Usage:  python tools/probe/clahe_stream_time.py [--size 10000 --channels 30 --kernel 0 --reps 3 --out FILE]
        (--kernel 0: the default kernel, an eighth of the image per axis)
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


def measure(rows, run, make, raw_src, a, n, elem, ks, base_ms, base_name):
    """The calls of one run.  ``make()``: a fresh image of the slide;
    ``raw_src``: its raw pixels as a source; ``base_ms``: the run's yardstick."""
    F = make().n_ch
    feats = list(range(F))

    def vs(ms):
        return {f"over_{base_name}": round(statistics.median(ms) / base_ms, 3)}

    ms = host_ms(lambda: stream.clahe(raw_src, ks), a.reps, a.warmup)
    record(rows, run, "equalize_hist statistics (stream.clahe): three reads and the tables", ms, 3 * n * elem, **vs(ms))
    im = make()
    im.equalize_hist(kernel_size=ks, banded=True)
    assert im._pending_clahe is not None
    src = im._source()
    band = stream.band_rows_for(src)
    ms = host_ms(lambda: read_loop(src, band), a.reps, a.warmup)
    record(rows, run, "read loop of the equalised source (read + fp32 band written)", ms, n * (elem + 4),
           band_rows=band, **vs(ms))
    for eq in (True, False):
        im = make()
        if eq:
            im.equalize_hist(kernel_size=ks, banded=True)
        im.log_normalize(mean=np.full(F, 0.2 if eq else 100.0))
        im.blurring("gaussian", sigma=2)
        state = "deferred" if im._pending_blur is not None else "materialised"
        X = [None]

        def subsample():
            X[0] = im._subsample_device(feats, 0.2)[0]

        ms = host_ms(subsample, a.reps, a.warmup)
        tag = "after equalize_hist(banded=True)" if eq else "no equalize_hist"
        record(rows, run, f"subsample 0.2, gaussian {state}, {tag}", ms, n * elem, **vs(ms))
        centers = X[0][:8].double().cpu().numpy()
        del X
        ms = host_ms(lambda: _assign_img(im, feats, centers, _Identity(F)), a.reps, a.warmup)
        record(rows, run, f"label pass k=8, gaussian {state}, {tag}", ms, n * elem, **vs(ms))
        del im
        torch.cuda.empty_cache()


def trace(t, host, ks):
    """Every kernel once: the resident equalisation, then the banded stages
    over the resident slide in bands of a tenth of it."""
    D.clahe(t, ks)
    src = stream.DeviceSource(t)
    band = max(1, src.H // 10)
    state = stream.clahe(src, ks, band_rows=band)
    eq = stream.ClaheSource(src, state)
    out = torch.empty((band, src.W, src.C), dtype=torch.float32, device=t.device)
    for y0 in range(0, src.H, band):
        eq.read(y0, min(src.H, y0 + band), out)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", default="b,c")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    D.require_gpu()
    torch.cuda.set_device(0)
    H = W = a.size
    C = a.channels
    ks = a.kernel or None
    rows = []
    t, mask = D.synth_slide(H, W, C, seed=20251015)
    n = H * W * C
    elem = t.element_size()
    if a.trace:
        trace(t, None, ks)
        return
    host = stream.pinned_empty((H, W, C), dtype=t.dtype)
    host.copy_(t)
    torch.cuda.synchronize()
    runs = a.runs.split(",")
    os.environ.pop("MW_HBM_BUDGET", None)
    ms = host_ms(lambda: D.clahe(t, ks), a.reps, a.warmup)
    whole_ms = record(rows, "resident", "D.clahe end to end", ms, n * (3 * elem + 12), kernel=a.kernel)
    del t
    torch.cuda.empty_cache()
    if "b" in runs:
        # the raw slide fits the budget, its fp32 result does not
        os.environ["MW_HBM_BUDGET"] = str(int(n * elem * 1.5))
        arr = host.numpy().view(np.uint16)
        hmask = mask.cpu().numpy()
        raw = D.to_device_image(arr)  # (the statistics' source; every image of the run uploads its own copy)
        measure(rows, "b resident raw, result deferred", lambda: MxIF.img(arr, mask=hmask),
                stream.DeviceSource(raw), a, n, elem, ks, whole_ms, "resident_clahe")
        del raw
        torch.cuda.empty_cache()
    if "c" in runs:
        os.environ["MW_HBM_BUDGET"] = "1"
        src = stream.HostSource(host)
        band = stream.band_rows_for(src)
        ms = host_ms(lambda: read_loop(src, band), a.reps, a.warmup)
        read_ms = record(rows, "c streamed", "bare band-read loop (page-locked host memory)", ms, n * elem,
                         band_rows=band)
        before = dict(D.CLAHE_USED)
        measure(rows, "c streamed", lambda: MxIF.img.from_source(stream.HostSource(host), mask=mask), src, a, n,
                elem, ks, read_ms, "read_loop")
        print(json.dumps({k: D.CLAHE_USED[k] - before[k] for k in before}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
