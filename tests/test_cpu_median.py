"""CPU-only tests of the median filter's host side: the numpy brute force the
GPU tests use as their oracle equals scipy's results in the golden fixture
(tests/golden/make_golden_median.py), and ``img.blurring('median', ...)``
validates ``size`` before any device call while the reference's failure
without ``size`` and the bilateral stub stay as they were."""
import os

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

SIZES = (2, 3, 4, 5, 7, (2, 5), (6, 3), 15)
DTYPES = ("u8", "u16", "f32")


def size_pair(s):
    return (s, s) if isinstance(s, int) else tuple(s)


def size_key(s):
    sy, sx = size_pair(s)
    return f"{sy}x{sx}"


def brute_median(a, size):
    """The element of rank (sy sx) // 2 of every pixel's window, rows y - sy//2
    .. y + sy - 1 - sy//2 and columns likewise, edges replicated; HWC or HW."""
    sy, sx = size_pair(size)
    a = np.asarray(a)
    if a.ndim == 2:
        return brute_median(a[:, :, None], size)[:, :, 0]
    pad = np.pad(a, ((sy // 2, sy - 1 - sy // 2), (sx // 2, sx - 1 - sx // 2), (0, 0)), mode="edge")
    win = sliding_window_view(pad, (sy, sx), axis=(0, 1))  # H x W x C x sy x sx
    flat = np.sort(win.reshape(win.shape[:3] + (sy * sx,)), axis=-1)
    return np.ascontiguousarray(flat[..., (sy * sx) // 2])


@pytest.mark.parametrize("dtype", DTYPES)
def test_brute_force_equals_scipy_fixture(golden, dtype):
    g = golden("median")
    a = g[f"{dtype}_in"]
    assert a.shape == (23, 37, 3)
    for s in SIZES:
        want = g[f"{dtype}_{size_key(s)}"]
        got = brute_median(a, s)
        assert got.dtype == want.dtype == a.dtype
        assert np.array_equal(got, want), (dtype, s)


def test_fixture_holds_the_trap_values(golden):
    g = golden("median")
    u16, f32 = g["u16_in"], g["f32_in"]
    assert u16.dtype == np.uint16 and (u16 > 32767).any() and (u16 < 32768).any()
    assert f32.dtype == np.float32 and (f32 < 0).any()
    tiny = np.finfo(np.float32).tiny
    assert ((f32 != 0) & (np.abs(f32) < tiny)).sum() >= 3  # subnormals
    # some subnormals are selected: a flushing min / max would show
    out = g["f32_3x3"]
    assert ((out != 0) & (np.abs(out) < tiny)).any()
    assert np.unique(f32).size < f32.size  # repeated values


def test_no_median_kernel_spills(tmp_path):
    """Every instance of the median kernel (3 dtypes x {2x2, 3x3, 5x5, generic}
    x {plain, lognorm epilogue}) compiles for gfx950 without scratch."""
    import re
    import subprocess

    from milwrm_amd import build as B

    src = os.path.join(B.CSRC, "median.hip")
    cmd = [B.HIPCC] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                  str(tmp_path / "median.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == 24 and all("median_kernel" in n for n in names), names
    assert len(scratch) == 24 and not any(scratch), dict(zip(names, scratch))
    assert len(vgprs) == 24 and max(vgprs) <= 64, dict(zip(names, vgprs))  # 8 waves per SIMD


def _img(shape=(6, 7, 2)):
    from milwrm_amd import MxIF

    return MxIF.img(np.arange(np.prod(shape), dtype=np.uint16).reshape(shape))


@pytest.mark.parametrize("size", [0, (3,), 2.5, (2, 0), (1, 2, 3), "3", (2, 2.0), -1, True])
def test_median_size_is_validated_before_any_device_call(size):
    with pytest.raises(ValueError):
        _img().blurring("median", size=size)


def test_median_without_size_keeps_the_reference_failure():
    with pytest.raises(TypeError):
        _img().blurring("median", sigma=2)
    with pytest.raises(TypeError):
        _img().blurring("median")


def test_bilateral_stays_a_stub():
    with pytest.raises(NotImplementedError):
        _img().blurring("bilateral")
    with pytest.raises(NotImplementedError):
        _img().blurring("bilateral", size=3)
