"""Timing probe of the label pass's background-tile skip on one GPU.

``mw_assign_conf`` alone at config-2 size (10k x 10k x 30 fp32, k = 8) under
masks with a top band of background rows: 0 (the control: nothing can be
skipped, so a difference between two builds is the cost of the mask look-ahead),
0.15 (the benchmark slide's share) and 1.  HIP events around each call, warm-up,
median of ``--reps`` with min and max, and a fingerprint of the outputs so two
builds can be compared.

Usage:  python tools/probe/assign_bgskip_time.py [--size 10000 --channels 30 --k 8 --reps 20
                                                  --fracs 0,0.15,1 --out FILE]
(MW_LIB selects the library build to time.)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fracs", default="0,0.15,1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    D.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    H = W = a.size
    C, k, n = a.channels, a.k, a.size * a.size
    g = torch.Generator(device=dev).manual_seed(20261020)
    img = torch.rand((H, W, C), generator=g, dtype=torch.float32, device=dev)
    rng = np.random.default_rng(7)
    inv = rng.uniform(1.5, 3.0, C)
    mu = rng.uniform(0.3, 0.7, C)
    feat, a32, b32, cen = D.h2d_many([np.arange(C, dtype=np.int32), inv.astype(np.float32),
                                      (-mu * inv).astype(np.float32),
                                      rng.normal(0.0, 0.6, (k, C)).astype(np.float32)], dev)
    lab = torch.empty((H, W), dtype=torch.int8, device=dev)
    conf = torch.empty((H, W), dtype=torch.float32, device=dev)
    dom = torch.empty(3 * k, dtype=torch.float64, device=dev)
    ws = D.WS.get("assign", N.query("mw_assign_ws_bytes", n, k))
    st = D.stream()
    rows = []
    for frac in [float(x) for x in a.fracs.split(",")]:
        mask = torch.ones((H, W), dtype=torch.uint8, device=dev)
        mask[:int(round(frac * H))] = 0

        def run():
            N.call("mw_assign_conf", D.P(img), C, D.P(feat), C, D.P(a32), D.P(b32), D.P(cen), k, D.P(mask), n,
                   D.P(lab), D.P(conf), D.P(ws), st)

        ms = event_ms(run, a.reps, a.warmup)
        N.call("mw_assign_reduce", D.P(ws), n, k, D.P(dom), st)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (lab, conf, dom):
            h.update(t.cpu().numpy().tobytes())
        row = dict(name=f"mw_assign_conf {H}x{W}x{C} k={k}, top {frac:g} of the rows background",
                   median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                   reps=len(ms), fingerprint=h.hexdigest()[:16])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
