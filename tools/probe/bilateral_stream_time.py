"""Timing probe of the streamed bilateral filter on one GPU.

A config-2 slide (10k x 10k x 30 uint16) that is never resident: a
``stream.SynthSource`` read band by band under ``MW_HBM_BUDGET=1``.  For sigma
1 (7 x 7 taps) and sigma 2 (13 x 13) (``--sigmas``):

* ``stream.bilateral_gather`` (sample map, per band mw_bilateral_rows with the
  lognorm load + mw_slot_gather, overflow copies) of 17 M draws;
* the banded label pass ``assign.banded_assign_image`` over a
  ``stream.BilateralBand`` (k = 8).

Beside them, in the same run: the bands read and nothing else (what the source
itself costs), the streamed moments ``stream.image_moments`` (both reads, and
the first alone: what a numeric sigma_color costs at the call), and the
resident form of the same tree (``D.bilateral`` with the lognorm load into an
fp32 slide + ``D.gather_rows``).  Host clock around each pass, ended by a
device synchronise; one warm-up, then ``--reps`` repeats: median, min, max.

Usage:  python tools/probe/bilateral_stream_time.py [--size 10000 --channels 30 --reps 3 --out FILE]
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
    ap.add_argument("--sigmas", default="1,2")
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
    inv_mean = D.h2d((1.0 / np.linspace(300.0, 9000.0, C)).astype(np.float32))
    X = torch.empty((S, F), dtype=torch.float32, device=dev)
    stats = torch.zeros(1 + 2 * F, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(3)
    centers = rng.normal(0.0, 1.0, size=(a.k, F))
    mu, inv = np.full(F, 0.3), np.full(F, 4.0)
    rows = []
    band_rows = stream.band_rows_for(src, W * C * 4)

    def read_only():
        for _ in stream.bands(src, band_rows, 6):
            pass

    record(rows, "bands read, no work (device generator)", wall_ms(read_only, a.reps),
           f"{-(-H // band_rows)} bands of {band_rows} rows")
    record(rows, "streamed moments: stream.image_moments, both reads (sigma_color='std')",
           wall_ms(lambda: stream.image_moments(src, inv_mean, 1.0), a.reps))
    record(rows, "streamed moments: the first read alone (a numeric sigma_color)",
           wall_ms(lambda: stream.image_moments(src, inv_mean, 1.0, m2=False), a.reps))
    m = stream.image_moments(src, inv_mean, 1.0)
    sc = float(np.sqrt(m[2] / m[0]))
    print(json.dumps({"sigma_color": sc, "min": m[3], "max": m[4]}), flush=True)
    sigmas = [float(x) for x in a.sigmas.split(",")]
    for s in sigmas:
        pend = (s, sc, None, "constant", 0.0)
        filt = stream.BilateralBand(pend, inv_mean, 1.0)
        w = 2 * filt.halo + 1
        record(rows, f"streamed bilateral sigma {s:g} ({w}x{w}): bilateral_gather",
               wall_ms(lambda: stream.bilateral_gather(src, pend, inv_mean, 1.0, feat, idx, r2p, X), a.reps))
        record(rows, f"streamed bilateral sigma {s:g} ({w}x{w}): banded label pass",
               wall_ms(lambda: assign.banded_assign_image(src, filt, feats, mu, inv, centers, mask), a.reps))
    # the resident form of the same tree, on the generator's own slide
    D.WS.clear()
    torch.cuda.empty_cache()
    t = src.materialize()
    out32 = torch.empty((H, W, C), dtype=torch.float32, device=dev)
    for s in sigmas:
        w = 2 * D.bilateral_args(s, sc)[2] + 1
        record(rows, f"resident bilateral sigma {s:g} ({w}x{w}): D.bilateral (lognorm load) + gather_rows",
               wall_ms(lambda: D.gather_rows(D.bilateral(t, s, sc, inv_mean=inv_mean, pseudoval=1.0, out=out32),
                                             feat, idx, r2p, X, stats, False), a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
