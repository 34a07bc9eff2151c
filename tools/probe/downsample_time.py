"""Timing probe of ``img.downsample`` on one GPU.

Config-2 slide (10k x 10k x 30 uint16, ``synth_slide`` on the device):

* ``nz_stats`` of the same tensor: the project's read-once yardstick;
* ``device.block_reduce`` per func at fact 2, 4 and 8 (mean, sum, max, min:
  bytes = the slide read once + the fp32 result written; median re-reads its
  block per key bit and has no target: fewer reps);
* mean against the first-round kernel (``device.block_mean``, which the
  library still carries) at the same facts, the two alternating call by call
  in one process, and whether their results are the same bits;
* streamed: the same slide in page-locked host memory as a ``HostSource``
  under ``MW_HBM_BUDGET=1`` through ``img.downsample(2)``, against the
  resident slide through the same call (host clock; the difference is the
  host read).

HIP events around each call, warm-up, median of ``--reps`` (>= 10), minimum
and maximum reported.

Usage:  python tools/probe/downsample_time.py [--size 10000 --channels 30 --reps 12 --out FILE]
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

FUNCS = {"mean": np.mean, "sum": np.sum, "max": np.max, "min": np.min, "median": np.median}


def one_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [one_ms(fn) for _ in range(reps)]


def event_ms_ab(fa, fb, reps, warmup):
    """``fa`` and ``fb`` alternating call by call."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(one_ms(fa))
        b.append(one_ms(fb))
    return a, b


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


def record(rows, name, ms, nbytes, note="", **extra):
    med = statistics.median(ms)
    row = dict(name=name, median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
               reps=len(ms), bytes=int(nbytes), tb_per_s=round(nbytes / med / 1e9, 3), note=note, **extra)
    rows.append(row)
    print(json.dumps(row), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--channels", type=int, default=30)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--facts", default="2,4,8")
    ap.add_argument("--no-median", action="store_true")
    ap.add_argument("--no-streamed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    D.require_gpu()
    torch.cuda.set_device(0)
    H = W = a.size
    C = a.channels
    facts = [int(f) for f in a.facts.split(",")]
    rows = []
    t, mask = D.synth_slide(H, W, C, seed=20251015)
    n = H * W * C
    elem = t.element_size()
    nz = record(rows, "nz_stats u16", event_ms(lambda: D.nz_stats(t), a.reps, a.warmup), elem * n,
                "read-once yardstick, same tensor")
    for f in facts:
        Ho, Wo = -(-H // f), -(-W // f)
        nbytes = elem * n + 4 * Ho * Wo * C
        out = torch.empty((Ho, Wo, C), dtype=torch.float32, device=t.device)
        for name, fn in FUNCS.items():
            if name == "median":
                if a.no_median:
                    continue
                ms = event_ms(lambda: D.block_reduce_rows(t, 0, H, f, fn, out), 3, 1)
                record(rows, f"block_reduce median fact={f}", ms, nbytes, "exact selection, no target",
                       vs_nz_stats=round(statistics.median(ms) / nz, 3))
                continue
            ms = event_ms(lambda: D.block_reduce_rows(t, 0, H, f, fn, out), a.reps, a.warmup)
            record(rows, f"block_reduce {name} fact={f}", ms, nbytes, vs_nz_stats=round(statistics.median(ms) / nz, 3))
        # mean: the new kernel and the first-round kernel alternating
        new, old = event_ms_ab(lambda: D.block_reduce_rows(t, 0, H, f, np.mean, out), lambda: D.block_mean(t, f),
                               a.reps, a.warmup)
        same = bool(torch.equal(D.block_reduce(t, f, np.mean), D.block_mean(t, f)))
        m_new = record(rows, f"A/B mean fact={f}: block_reduce", new, nbytes, "alternating with block_mean")
        m_old = record(rows, f"A/B mean fact={f}: block_mean (first-round kernel)", old, nbytes,
                       f"same bits: {same}", new_over_old=round(m_new / statistics.median(old), 3))
        del out
        torch.cuda.empty_cache()

    if not a.no_streamed:
        f = 2
        nbytes = elem * n + 4 * (-(-H // f)) * (-(-W // f)) * C
        host = stream.pinned_empty((H, W, C), dtype=t.dtype)
        host.copy_(t)
        torch.cuda.synchronize()

        def resident():
            im = MxIF.img.from_device(t, mask=mask)
            im.downsample(f)

        ms_res = host_ms(resident, 5, 1)
        record(rows, f"img.downsample({f}) resident, slide + device mask", ms_res, nbytes, "host clock")
        del t
        torch.cuda.empty_cache()
        os.environ["MW_HBM_BUDGET"] = "1"
        before = D.FUSED_USED["downsample_streamed"]

        def streamed():
            im = MxIF.img.from_source(stream.HostSource(host), mask=mask)
            im.downsample(f)

        ms_str = host_ms(streamed, 5, 1)
        record(rows, f"img.downsample({f}) streamed from page-locked host memory", ms_str, nbytes,
               f"host clock; MW_HBM_BUDGET=1, bands of {stream.band_rows_for(stream.HostSource(host))} rows; "
               f"streamed passes: {D.FUSED_USED['downsample_streamed'] - before}",
               host_read_ms=round(statistics.median(ms_str) - statistics.median(ms_res), 3))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
