"""CPU-only tests of CLAHE's host side: the numpy oracle's tile
geometry, device.clahe_args, mw_clahe's refusals before any device call (the
pointers are never dereferenced), and the message of a call without
kernel_size=."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clahe_oracle as O  # noqa: E402

from milwrm_amd import MxIF  # noqa: E402
from milwrm_amd import _native as N  # noqa: E402
from milwrm_amd import device as D  # noqa: E402

IMG, OUT, WS = 0x10000, 0x20000, 0x30000  # never dereferenced: every call below is refused before the launch


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("n,k", [(37, 8), (53, 12), (64, 16), (20, 13), (31, 7), (9, 8), (40, 5), (33, 33), (47, 47),
                                 (2, 1), (2, 2), (5, 4)])
def test_reflection_rule_is_numpy_reflect_padding(n, k):
    before, after = k // 2, (k - n % k) % k + math.ceil(k / 2)
    padded = np.pad(np.arange(n), (before, after), mode="reflect")
    rule = np.array([O.reflect(i, n) for i in range(-before, n + after)])
    assert np.array_equal(padded, rule)
    # the tiled axis is the padded one from the first pixel on
    t = O.tile_indices(n, k)
    assert t.size == -(-n // k) * k and np.array_equal(t, padded[before:before + t.size])


@pytest.mark.parametrize("H,W,kh,kw", [(37, 53, 8, 12), (20, 31, 13, 7), (9, 9, 8, 8), (33, 47, 33, 47), (40, 40, 5, 5)])
def test_tiles_start_at_the_first_pixel_and_count_their_area(H, W, kh, kw):
    rng = np.random.default_rng(7)
    b = rng.integers(0, 256, size=(H, W))
    hist = O.tile_hists(b, kh, kw, 256)
    assert hist.shape == (-(-H // kh), -(-W // kw), 256)
    assert np.all(hist.sum(axis=2) == kh * kw)
    assert np.array_equal(hist[0, 0], np.bincount(b[:kh, :kw].ravel(), minlength=256))


def test_oracle_clip_hist_loop_and_degenerate_planes():
    stats = {}
    h = np.array([50, 0, 0, 3, 2, 0, 1, 0], dtype=np.int64)
    out = O.clip_hist(h.copy(), 4, stats)
    assert stats["loop_passes"] >= 1 and out.max() <= 4 and out.min() >= 0
    px, luts = O.clahe_plane(np.full((6, 7), 3.5), 3, 3)
    assert not px.any() and not luts.any() and px.dtype == np.float32 and luts.shape == (2, 3, 256)


# ------------------------------------------------------------------ clahe_args
def test_clahe_args_normalises_kernel_size():
    assert D.clahe_args(37, 53, 8) == (8, 8, 0.01, 256)
    assert D.clahe_args(37, 53, (8, 12), 0.05, 100) == (8, 12, 0.05, 100)
    assert D.clahe_args(37, 53, [np.int64(37), 53]) == (37, 53, 0.01, 256)
    assert D.clahe_args(37, 53, None) == (4, 6, 0.01, 256)
    assert D.clahe_args(5, 7, None) == (1, 1, 0.01, 256)
    assert D.clahe_args(2, 2, 1, clip_limit=1, nbins=2) == (1, 1, 1.0, 2)


@pytest.mark.parametrize("H,W,ks,clip,nbins", [
    (37, 53, (8, 12, 3), 0.01, 256),   # a triple
    (37, 53, (8,), 0.01, 256),
    (37, 53, 0, 0.01, 256),            # below 1
    (37, 53, (8, -1), 0.01, 256),
    (37, 53, 38, 0.01, 256),           # above the extent
    (37, 53, (8, 54), 0.01, 256),
    (37, 53, 2.5, 0.01, 256),          # not an int
    (1, 53, 1, 0.01, 256),             # H below 2
    (37, 1, 1, 0.01, 256),
    (37, 53, 8, 0.0, 256),             # clip_limit not positive / not finite
    (37, 53, 8, -0.01, 256),
    (37, 53, 8, float("nan"), 256),
    (37, 53, 8, float("inf"), 256),
    (37, 53, 8, 0.01, 1),              # nbins below 2
])
def test_clahe_args_value_errors(H, W, ks, clip, nbins):
    with pytest.raises(ValueError):
        D.clahe_args(H, W, ks, clip, nbins)


def test_clahe_args_nbins_limit():
    with pytest.raises(NotImplementedError, match="256"):
        D.clahe_args(37, 53, 8, 0.01, 257)


# ------------------------------------------------------------------ the C entry
def _clahe(H=37, W=53, C=3, kh=8, kw=12, clip=0.01, nbins=256, dtype=N.MW_U16, img=IMG, out=OUT, ws=WS):
    st = N.load().mw_clahe(img, dtype, H, W, C, None, kh, kw, clip, nbins, out, ws, None, None)
    return st, N.last_error()


@pytest.mark.parametrize("ptrs", [dict(), dict(img=None, out=None, ws=None)])
def test_mw_clahe_refuses_before_any_device_call(ptrs):
    for kw in (dict(kh=0), dict(kw=0), dict(kh=38), dict(kw=54), dict(H=1, kh=1), dict(W=1, kw=1), dict(C=0),
               dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan")), dict(clip=float("inf")), dict(nbins=1),
               dict(dtype=7)):
        st, msg = _clahe(**kw, **ptrs)
        assert st == N._EINVAL and "mw_clahe" in msg, (kw, st, msg)
    st, msg = _clahe(nbins=257, **ptrs)
    assert st == N._EUNSUP and "256" in msg
    assert _clahe(C=257, **ptrs)[0] == N._EUNSUP
    assert _clahe(H=2, W=1 << 24, C=200, kh=1, kw=1, **ptrs)[0] == N._EUNSUP  # a row of 2^31 elements or more


def test_mw_clahe_pointer_checks():
    assert _clahe(img=None)[0] == N._EINVAL
    assert _clahe(out=None)[0] == N._EINVAL
    assert _clahe(ws=None)[0] == N._EINVAL
    assert _clahe(img=IMG + 4)[0] == N._EINVAL   # misaligned
    assert _clahe(out=IMG)[0] == N._EINVAL       # aliased
    lib = N.load()
    assert lib.mw_clahe_ws_bytes(37, 53, 3, 8, 12, 256) >= 3 * 5 * 5 * 256 * 4
    assert lib.mw_clahe_ws_bytes(37, 53, 3, 0, 12, 256) == 0


# ------------------------------------------------------------------ selection by kernel_size=
def test_without_kernel_size_names_it():
    im = MxIF.img(np.zeros((4, 4, 2), dtype=np.uint16))
    calls = (lambda: MxIF.CLAHE(), lambda: MxIF.CLAHE(np.zeros((4, 4))), lambda: MxIF.img.equalize_hist(),
             lambda: im.equalize_hist(), lambda: im.equalize_hist(channels=(0,), nbins=64))
    for f in calls:
        with pytest.raises(NotImplementedError, match="kernel_size"):
            f()


def test_arguments_are_checked_before_any_device_call():
    im = MxIF.img(np.zeros((4, 6, 2), dtype=np.uint16))
    with pytest.raises(ValueError):
        im.equalize_hist(kernel_size=5)
    with pytest.raises(ValueError):
        im.equalize_hist(kernel_size=(2, 2, 2))
    with pytest.raises(NotImplementedError, match="256"):
        im.equalize_hist(kernel_size=2, nbins=512)
    with pytest.raises(ValueError):
        MxIF.CLAHE(np.zeros((1, 6)), kernel_size=1)
