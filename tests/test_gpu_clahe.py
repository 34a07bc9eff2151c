"""GPU tests of CLAHE: D.clahe / img.equalize_hist / MxIF.CLAHE
against the float64 numpy oracle of the definition (tests/clahe_oracle.py).
Every integer stage is exact and the floating-point route is fixed, so every
case asserts the look-up tables equal and the pixels equal bit for bit.  The
inputs are seeded with heavy ties (gamma-distributed, half the pixels zero), so
that the clipping and the sequential redistribution loop both run; each case
asserts in the oracle that the loop ran."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clahe_oracle as O  # noqa: E402

from milwrm_amd import MxIF  # noqa: E402
from milwrm_amd import device as D  # noqa: E402

pytestmark = pytest.mark.gpu


def _slide(H, W, C, dtype, seed):
    """Gamma-distributed intensities, half the pixels zero; fp32 also negative."""
    rng = np.random.default_rng(seed)
    a = rng.gamma(2.0, 600.0, size=(H, W, C))
    a[rng.uniform(size=(H, W, C)) < 0.5] = 0.0
    if dtype == np.uint8:
        return np.minimum(a / 16.0, 255.0).astype(np.uint8)
    if dtype == np.uint16:
        return np.minimum(a, 65535.0).astype(np.uint16)
    return (a - 300.0).astype(np.float32)


def _upload(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a).cuda()


def _same_bits(got, ref):
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4], [(got[tuple(i)], ref[tuple(i)]) for i in bad[:4]])


def _ref(a, kernel_size, clip_limit=0.01, nbins=256, channels=None, loop=True):
    """The oracle's pixels and tables; the input must exercise the sequential
    redistribution loop in at least one tile."""
    stats = {}
    ref = O.clahe(a, kernel_size, clip_limit, nbins, channels=channels, stats=stats)
    assert not loop or stats.get("loop_passes", 0) >= 1
    return ref


def _check(a, kernel_size, clip_limit=0.01, nbins=256, loop=True):
    ref, ref_luts = _ref(a, kernel_size, clip_limit, nbins, loop=loop)
    out, luts = D.clahe(_upload(a), kernel_size, clip_limit, nbins, luts=True)
    got_luts, got = D.d2h(luts, out)
    assert np.array_equal(got_luts, ref_luts), np.argwhere(got_luts != ref_luts)[:8]
    _same_bits(got, ref)
    assert got.min() == 0.0 and got.max() == 1.0
    return got


@pytest.mark.parametrize("H,W,C,dtype,ks,clip,nbins", [
    (37, 53, 3, np.uint16, (8, 12), 0.01, 256),    # ragged last tiles, reflection on both axes
    (64, 64, 30, np.uint16, 16, 0.01, 256),        # exact multiples, the config-2 channel count
    (20, 31, 5, np.float32, (13, 7), 0.01, 256),   # negative values, a kernel above half the image
    (33, 47, 1, np.uint8, (33, 47), 0.01, 256),    # one tile: every clamp active
    (40, 40, 50, np.uint16, 5, 0.05, 100),         # channel-group rounds, a bin size that does not divide
    (300, 300, 2, np.uint16, 150, 0.01, 256),      # a tile split over several workgroups, merged by atomics
    (37, 53, 3, np.uint16, None, 0.01, 256),       # the default kernel
    (37, 53, 3, np.uint16, (8, 12), 1e-6, 256),    # clim = 1
    (9, 9, 2, np.float32, 8, 0.05, 256),
    (41, 45, 7, np.uint8, (6, 9), 0.02, 64),       # rows that start off the 16-byte grid, uint8
    # tiles of 8 nbins pixels or more take the map pass that stages the tables in LDS
    (100, 90, 3, np.uint16, (48, 45), 0.01, 256),  # ragged cells, reflection
    (70, 66, 5, np.float32, (35, 33), 0.02, 100),
    (64, 128, 2, np.uint16, (32, 64), 0.01, 256),  # exactly at the threshold
    (64, 80, 40, np.uint8, (40, 64), 0.01, 256),   # more than 7680 table entries: the 128 KB instance
])
def test_clahe_equals_the_oracle(H, W, C, dtype, ks, clip, nbins):
    _check(_slide(H, W, C, dtype, seed=H * 1000 + W + 2), ks, clip, nbins)


def test_clip_limit_one_clips_nothing():
    a = _slide(37, 53, 3, np.uint16, seed=5)
    stats = {}
    O.clahe(a, (8, 12), 1.0, stats=stats)
    assert "loop_passes" not in stats
    _check(a, (8, 12), 1.0, loop=False)


def test_two_d_image():
    a = _slide(37, 53, 1, np.uint16, seed=6)[:, :, 0]
    ref, _ = _ref(a, (8, 12))
    im = MxIF.img(a)
    im.equalize_hist(channels=(0,), kernel_size=(8, 12))  # channels are ignored for a 2-D image
    got = im._dev.cpu().numpy()
    assert got.shape == (37, 53, 1)
    _same_bits(got[:, :, 0], ref)


def test_listed_channels_and_a_channel_listed_twice():
    a = _slide(37, 53, 3, np.uint16, seed=8)
    im = MxIF.img(a, channels=["a", "b", "c"])
    im.equalize_hist(channels=("b",), kernel_size=(8, 12))
    got = im._dev.cpu().numpy()
    ref, _ = _ref(a, (8, 12), channels=(1,))
    _same_bits(got, ref)
    assert np.array_equal(got[:, :, 0], a[:, :, 0].astype(np.float32))
    assert np.array_equal(got[:, :, 2], a[:, :, 2].astype(np.float32))
    # listed twice: the second round equalises the first round's fp32 plane
    twice = MxIF.img(a)
    twice.equalize_hist(channels=(1, 1), kernel_size=(8, 12))
    im.equalize_hist(channels=(1,), kernel_size=(8, 12))
    _same_bits(twice._dev.cpu().numpy(), im._dev.cpu().numpy())
    ref2, _ = _ref(a, (8, 12), channels=(1, 1))
    _same_bits(twice._dev.cpu().numpy(), ref2)


def test_constant_plane_is_zero():
    a = _slide(20, 31, 3, np.uint16, seed=9)
    a[:, :, 1] = 777
    out, luts = D.clahe(_upload(a), (6, 7), luts=True)
    got_luts, got = D.d2h(luts, out)
    ref, ref_luts = _ref(a, (6, 7))
    assert not got[:, :, 1].any() and not got_luts[1].any()
    assert np.array_equal(got_luts, ref_luts)
    _same_bits(got, ref)


def test_after_log_normalize_and_gaussian():
    a = _slide(37, 53, 3, np.uint16, seed=10)
    im = MxIF.img(a, mask=np.ones((37, 53), dtype=np.uint8))
    im.log_normalize()
    im.blurring("gaussian", sigma=2)
    before = im._materialize().cpu().numpy()  # the materialised device image the call starts from
    assert before.dtype == np.float32
    im.equalize_hist(kernel_size=(8, 12))
    ref, _ = _ref(before, (8, 12))
    _same_bits(im._dev.cpu().numpy(), ref)
    assert im._pending is None and not im._filter_deferred()


def test_module_function_on_a_host_array():
    a = _slide(37, 53, 3, np.uint16, seed=11)
    got = MxIF.CLAHE(a.astype(np.float64), channels=(0, 2), kernel_size=(8, 12), clip_limit=0.02)
    assert got.dtype == np.float64 and got.shape == a.shape
    im = MxIF.img(a)
    im.equalize_hist(channels=(0, 2), kernel_size=(8, 12), clip_limit=0.02)
    assert np.array_equal(got, im._dev.cpu().numpy().astype(np.float64))
    ref, _ = _ref(a, (8, 12), 0.02, channels=(0, 2))
    assert np.array_equal(got, ref.astype(np.float64))
    g2 = MxIF.CLAHE(a[:, :, 0].astype(np.float64), kernel_size=(8, 12))
    assert g2.shape == (37, 53) and np.array_equal(g2, O.clahe(a[:, :, 0], (8, 12))[0].astype(np.float64))


def test_row_band_is_refused():
    im = MxIF.img(_slide(20, 31, 2, np.uint16, seed=12))
    im._band = (0, 10)
    with pytest.raises(NotImplementedError, match="band"):
        im.equalize_hist(kernel_size=4)
