"""Timing probe of the streamed median filter on one GPU.

A config-2 slide (10k x 10k x 30 uint16) that is never resident: a
``stream.SynthSource`` read band by band under ``MW_HBM_BUDGET=1``.  For the
sizes 3 and 5 (``--sizes``):

* ``stream.median_gather`` (sample map, per band mw_median_rows with the
  lognorm epilogue + mw_slot_gather, overflow copies) of 17 M draws;
* the banded label pass ``assign.banded_assign_image`` over a
  ``stream.MedianBand`` (k = 8).

Beside them, in the same run: the bands read and nothing else (what the source
itself costs), the resident form of the same tree (``D.median`` with the
epilogue into an fp32 slide + ``D.gather_rows``; ``assign_image`` of that
slide), and the streamed Gaussian's two passes (``stream.blur_gather`` with its
fused sample epilogue, the banded label pass over a ``stream.GaussianBand``).
Host clock around each pass, ended by a device synchronise; one warm-up, then
``--reps`` repeats: median, min, max.

Usage:  python tools/probe/median_stream_time.py [--size 10000 --channels 30 --reps 3 --out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

os.environ["MW_HBM_BUDGET"] = "1"  # nothing host- or source-backed may stay resident

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from milwrm_amd import assign  # noqa: E402
from milwrm_amd import device as D  # noqa: E402
from milwrm_amd import stream  # noqa: E402


def wall_ms(fn, reps, warmup=1):
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


def record(rows, name, ms, note=""):
    row = dict(name=name, median_ms=round(statistics.median(ms), 2), min_ms=round(min(ms), 2),
               max_ms=round(max(ms), 2), reps=len(ms), note=note)
    rows.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--samples", type=int, default=17_000_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="3,5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    D.require_gpu()
    torch.cuda.set_device(0)
    dev = D.device()
    H = W = a.size
    C = F = a.channels
    n = H * W
    S = min(a.samples, n)
    seed = 20251015
    src = stream.SynthSource(H, W, C, seed)
    mask = D.padded_mask(src.mask_device())
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    idx = torch.randint(0, n, (S,), dtype=torch.int32, device=dev, generator=g)
    r2p = torch.arange(n, dtype=torch.int32, device=dev)  # every pixel is tissue: rank = pixel
    feat = torch.arange(F, dtype=torch.int32, device=dev)
    feats = list(range(F))
    inv_mean = D.h2d((1.0 / np.linspace(30.0, 90.0, C)).astype(np.float32))
    X = torch.empty((S, F), dtype=torch.float32, device=dev)
    stats = torch.zeros(1 + 2 * F, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(3)
    centers = rng.normal(0.0, 1.0, size=(a.k, F))
    mu, inv = np.full(F, 0.3), np.full(F, 4.0)
    rows = []
    band_rows = stream.band_rows_for(src, W * C * 4)

    def read_only():
        for _ in stream.bands(src, band_rows, 2):
            pass

    record(rows, "bands read, no work (device generator)", wall_ms(read_only, a.reps),
           f"{-(-H // band_rows)} bands of {band_rows} rows")
    gauss = stream.GaussianBand(2.0, inv_mean, 1.0)
    record(rows, "streamed gaussian sigma 2: blur_gather (fused sample epilogue)",
           wall_ms(lambda: stream.blur_gather(src, 2.0, inv_mean, 1.0, feat, idx, r2p, X), a.reps))
    record(rows, "streamed gaussian sigma 2: banded label pass",
           wall_ms(lambda: assign.banded_assign_image(src, gauss, feats, mu, inv, centers, mask), a.reps))
    sizes = [int(x) for x in a.sizes.split(",")]
    for s in sizes:
        filt = stream.MedianBand(s, inv_mean, 1.0)
        record(rows, f"streamed median {s}x{s}: median_gather",
               wall_ms(lambda: stream.median_gather(src, s, inv_mean, 1.0, feat, idx, r2p, X), a.reps))
        record(rows, f"streamed median {s}x{s}: banded label pass",
               wall_ms(lambda: assign.banded_assign_image(src, filt, feats, mu, inv, centers, mask), a.reps))
    # the resident form of the same tree, on the generator's own slide
    D.WS.clear()
    torch.cuda.empty_cache()
    t = src.materialize()
    out32 = torch.empty((H, W, C), dtype=torch.float32, device=dev)
    for s in sizes:
        record(rows, f"resident median {s}x{s}: D.median (lognorm epilogue) + gather_rows",
               wall_ms(lambda: D.gather_rows(D.median(t, s, inv_mean, 1.0, out=out32), feat, idx, r2p, X, stats,
                                             False), a.reps))
        record(rows, f"resident median {s}x{s}: assign_image of the filtered slide",
               wall_ms(lambda: assign.assign_image(out32, feats, mu, inv, centers, mask), a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
