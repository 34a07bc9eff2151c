"""CPU-only tests of the bilateral filter's host side: the numpy brute force the
GPU tests use as their oracle (a second implementation of the definition,
DESIGN.md §17, independent of the fixture generator's) reproduces the fixture
(tests/golden/make_golden_bilateral.py) and degenerates to scipy's Gaussian
correlation for a huge sigma_color; the fixture's inputs are moved by the
filter; the arguments are validated before any device call; every kernel
instance compiles for gfx950 without scratch."""
import os

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

WANT_ROWS = 12

# name -> (shape, sigma, win_size, ((mode, cval), ...)): tests/golden/make_golden_bilateral.py
CASES = {
    "basic": ((23, 37, 3), 1.0, None, (("constant", 0.0), ("constant", 0.4), ("edge", 0.0))),
    "c30": ((20, 24, 30), 2.0, None, (("constant", 0.0), ("edge", 0.0))),
    "c50": ((18, 40, 50), 1.0, None, (("constant", 0.4), ("edge", 0.0))),
    "c1": ((19, 45, 1), 1.0, None, (("constant", 0.0), ("edge", 0.0))),
    "c5": ((21, 34, 5), 1.0, None, (("edge", 0.0), ("constant", 0.4))),
    "tiles": ((70, 133, 3), 2.0, None, (("constant", 0.0), ("edge", 0.0))),
    "tiny": ((2, 3, 1), 1.0, None, (("constant", 0.4), ("edge", 0.0))),
    "small": ((5, 4, 2), 1.0, None, (("constant", 0.0), ("edge", 0.0))),
    "win25": ((27, 35, 3), 4.0, 25, (("constant", 0.4), ("edge", 0.0))),
}
VARIANTS = [(name, mode, cval) for name, (_, _, _, vs) in CASES.items() for mode, cval in vs]


def variant_key(mode, cval):
    return f"{mode}_{cval:g}"


def default_win_size(sigma):
    return max(5, 2 * int(np.ceil(3 * sigma)) + 1)


def brute_bilateral(a, sigma, sigma_color, win_size=None, mode="constant", cval=0.0):
    """The definition in float64, every pixel's whole window at once: for the
    taps (dy, dx) in [-r, r]^2, r = (win_size - 1) // 2, q the pixel at (y + dy,
    x + dx) (outside: cval / the clamped pixel), w = exp(-((dy^2 + dx^2) /
    sigma^2 + |q - a[y, x]|^2 / sigma_color^2) / 2), out = sum w q / sum w."""
    a = np.asarray(a, dtype=np.float64)
    r = ((default_win_size(sigma) if win_size is None else win_size) - 1) // 2
    n = 2 * r + 1
    kw = dict(mode="constant", constant_values=float(cval)) if mode == "constant" else dict(mode="edge")
    pad = np.pad(a, ((r, r), (r, r), (0, 0)), **kw)
    win = sliding_window_view(pad, (n, n), axis=(0, 1))  # H x W x C x n x n
    d2 = ((win - a[:, :, :, None, None]) ** 2).sum(axis=2)  # H x W x n x n
    off = np.arange(-r, r + 1, dtype=np.float64)
    sp = (off[:, None] ** 2 + off[None, :] ** 2) / float(sigma) ** 2
    w = np.exp(-0.5 * (sp[None, None] + d2 / float(sigma_color) ** 2))
    return (w[:, :, None] * win).sum(axis=(-1, -2)) / w.sum(axis=(-1, -2))[:, :, None]


@pytest.fixture(scope="session")
def bilateral_want(golden):
    """(name, mode, cval) -> the float64 brute-force result, computed once."""
    g = golden("bilateral")
    cache = {}

    def get(name, mode, cval):
        key = (name, mode, cval)
        if key not in cache:
            _, sigma, win, _ = CASES[name]
            res = brute_bilateral(g[f"{name}_in"], sigma, float(g[f"{name}_sigma_color"]), win, mode, cval)
            res.setflags(write=False)
            cache[key] = res
        return cache[key]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_brute_force_reproduces_the_fixture(golden, bilateral_want, name):
    g = golden("bilateral")
    shape, _, _, variants = CASES[name]
    a = g[f"{name}_in"]
    assert a.dtype == np.float32 and a.shape == shape
    assert float(g[f"{name}_sigma_color"]) == float(a.astype(np.float64).std())
    mode, cval = variants[0]
    want = g[f"{name}_want"]
    got = bilateral_want(name, mode, cval)[:WANT_ROWS]
    assert want.dtype == np.float64 and want.shape == got.shape
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    for mode, cval in variants:
        e32 = float(g[f"{name}_{variant_key(mode, cval)}_e32"])
        assert 5e-8 < e32 < 5e-6, (name, mode, cval, e32)  # fp32's own error on the formula


@pytest.mark.parametrize("name,mode,cval", VARIANTS)
def test_fixture_inputs_are_moved_by_the_filter(golden, bilateral_want, name, mode, cval):
    """A kernel that returned its input must not pass the GPU tests."""
    a = golden("bilateral")[f"{name}_in"].astype(np.float64)
    moved = np.abs(bilateral_want(name, mode, cval) - a).max()
    assert moved >= 0.01 * np.abs(a).max(), (name, mode, cval, moved)


@pytest.mark.parametrize("shape,sigma,win", [((17, 21, 3), 1.0, None), ((9, 30, 2), 2.0, None),
                                             ((12, 11, 1), 1.5, 7), ((4, 5, 2), 1.0, None)])
def test_huge_sigma_color_is_the_normalised_spatial_gaussian(shape, sigma, win):
    from scipy.ndimage import correlate

    a = np.random.default_rng(sum(shape)).uniform(0.0, 1.5, size=shape)
    r = ((default_win_size(sigma) if win is None else win) - 1) // 2
    off = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-0.5 * (off[:, None] ** 2 + off[None, :] ** 2) / sigma ** 2)
    k /= k.sum()
    for mode, cval in (("constant", 0.0), ("constant", 0.4), ("edge", 0.0)):
        got = brute_bilateral(a, sigma, 1e9, win, mode, cval)
        for c in range(shape[2]):
            if mode == "constant":
                # cval counts as a tap: the kernel's sum is 1 after the normalisation
                want = correlate(a[:, :, c], k, mode="constant", cval=cval) / k.sum()
            else:
                want = correlate(a[:, :, c], k, mode="nearest")
            np.testing.assert_allclose(got[:, :, c], want, rtol=1e-12, atol=1e-12)


def _img(shape=(6, 7, 2)):
    from milwrm_amd import MxIF

    return MxIF.img(np.arange(np.prod(shape), dtype=np.uint16).reshape(shape))


@pytest.mark.parametrize("kw", [dict(sigma=0, sigma_color=0.3), dict(sigma=-1.0, sigma_color=0.3),
                                dict(sigma=float("inf"), sigma_color=0.3), dict(sigma=float("nan"), sigma_color=0.3),
                                dict(sigma=1, sigma_color=0), dict(sigma=1, sigma_color=-2.0),
                                dict(sigma=1, sigma_color=float("inf")), dict(sigma=1, sigma_color=float("nan")),
                                dict(sigma=1, sigma_color="sd"), dict(sigma=1, sigma_color=None),
                                dict(sigma=1, sigma_color=0.3, win_size=0), dict(sigma=1, sigma_color=0.3, win_size=-3),
                                dict(sigma=1, sigma_color="std", win_size=0),
                                dict(sigma=1, sigma_color=0.3, cval=float("nan"))])
def test_bad_arguments_raise_value_error_before_any_device_call(kw):
    from milwrm_amd import device as D

    with pytest.raises(ValueError):
        _img().blurring("bilateral", **kw)
    with pytest.raises(ValueError):
        _img().bilateral_filter(**kw)
    if kw["sigma_color"] != "std":
        with pytest.raises(ValueError):
            D.bilateral(None, **kw)  # the checks come before the image is touched


@pytest.mark.parametrize("kw", [dict(sigma=1, sigma_color=0.3, win_size=27), dict(sigma=5, sigma_color=0.3),
                                dict(sigma=1, sigma_color=0.3, mode="reflect"),
                                dict(sigma=1, sigma_color="std", mode="wrap")])
def test_unsupported_arguments_raise_not_implemented_before_any_device_call(kw):
    from milwrm_amd import device as D

    with pytest.raises(NotImplementedError):
        _img().blurring("bilateral", **kw)
    with pytest.raises(NotImplementedError):
        _img().bilateral_filter(**kw)
    if kw["sigma_color"] != "std":
        with pytest.raises(NotImplementedError):
            D.bilateral(None, **kw)


def test_bilateral_args():
    from milwrm_amd import device as D

    assert D.bilateral_args(1, 0.3) == (1.0, 0.3, 3, 0, 0.0)  # win_size 7
    assert D.bilateral_args(0.5, 0.3)[2] == 2  # win_size max(5, 5)
    assert D.bilateral_args(0.2, 0.3)[2] == 2  # win_size max(5, 3)
    assert D.bilateral_args(2, 0.3, mode="edge", cval=0.4) == (2.0, 0.3, 6, 1, 0.4)  # win_size 13
    assert D.bilateral_args(4, 1, None)[2] == 12  # win_size 25
    assert D.bilateral_args(1, 1, 25)[2] == 12
    assert D.bilateral_args(1, 1, 4)[2] == 1 and D.bilateral_args(1, 1, 1)[2] == 0


def test_without_sigma_color_the_call_says_how_to_run_the_filter():
    with pytest.raises(NotImplementedError, match="sigma_color="):
        _img().blurring("bilateral", sigma=1)
    with pytest.raises(NotImplementedError, match="sigma_color="):
        _img().blurring("bilateral", sigma=1, win_size=5)


def test_unknown_options_raise():
    with pytest.raises(NotImplementedError, match="size"):
        _img().blurring("bilateral", sigma=1, sigma_color=0.3, size=3)
    with pytest.raises(NotImplementedError, match="channel_axis"):
        _img().blurring("bilateral", sigma=1, sigma_color="std", channel_axis=2)


def test_no_bilateral_kernel_spills(tmp_path):
    """Every instance of the bilateral kernel (3 dtypes x {plain, lognorm load}
    x 7 channel-group counts) compiles for gfx950 without scratch, at no more
    than 128 registers up to 36 channels (4 waves per SIMD) and 256 beyond (2)."""
    import re
    import subprocess

    from milwrm_amd import build as B

    src = os.path.join(B.CSRC, "bilateral.hip")
    cmd = [B.HIPCC] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                  str(tmp_path / "bilateral.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    agprs = [int(x) for x in re.findall(r" AGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(agprs)
    assert not any(scratch), dict(zip(names, scratch))  # the moments kernels too
    bil = [(n, v + a) for n, v, a in zip(names, vgprs, agprs) if "bilateral_kernel" in n]
    assert len(bil) == 42, names
    for n, regs in bil:
        nq = int(re.search(r"ELi(\d+)EEEv", n).group(1))  # the NQ template argument
        assert nq in (1, 3, 5, 7, 9, 13, 17), n
        assert regs <= (128 if nq <= 9 else 256), (n, regs)
