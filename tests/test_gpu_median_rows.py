"""The row-window form of the median kernel (mw_median_rows, D.median_rows):
bands of any height tiled over a slide give ``D.median`` of the whole slide
bit for bit (every dtype, both kernel paths, plain and with the lognorm
epilogue), also for scipy's fixture; an array that lacks a needed halo row is
refused before anything is launched."""
import numpy as np
import pytest
import torch

from tests.test_cpu_median import DTYPES, SIZES, size_key
from tests.test_gpu_median import _down, _rand, _up

pytestmark = pytest.mark.gpu

# 3, 5: selection networks; (4, 7): even rows (2 halo rows above, 1 below), asymmetric; 9: rank search
ROW_SIZES = (3, 5, (4, 7), 9)
# below the halo, inside one 16-row tile, the tile, one past it, a last partial band / one band
BAND_HEIGHTS = (1, 5, 16, 17, 37)
# odd C (packed keys with a pad key); two channel chunks of words
SHAPES = {"c7": (45, 70, 7), "c50": (37, 33, 50)}


def _image(dtype, shape, seed, nonneg=False):
    a = _rand(dtype, shape, seed)
    if dtype == "u16":
        assert (a > 32767).any()
    if dtype == "f32":
        a.reshape(-1)[::5] = np.float32(-0.0)
        a.reshape(-1)[1::6] = np.float32(0.0)
        if nonneg:  # the lognorm epilogue's domain
            a = np.abs(a)
            a[a > 1e30] = np.float32(12.5)
    return a


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _banded(t, size, h, inv=None, p=1.0, **kw):
    from milwrm_amd import device as D
    from milwrm_amd import stream

    H = int(t.shape[0])
    sy = D.median_size(size)[0]
    parts = []
    for y0, y1, a, raw in stream.bands(stream.DeviceSource(t), h, sy // 2):
        out = D.median_rows(raw, size, a, H, y0 - a, y1 - a, inv, p, **kw)
        assert tuple(out.shape) == (y1 - y0,) + tuple(t.shape[1:])
        parts.append(out)
    return torch.cat(parts)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_bands_equal_whole_slide(gpu, dtype, shape):
    from milwrm_amd import device as D

    H, W, C = SHAPES[shape]
    rng = np.random.default_rng(C)
    inv = torch.from_numpy((1.0 / rng.uniform(2.0, 30000.0, size=C)).astype(np.float32)).to(gpu)
    for epi in (False, True):
        t = _up(_image(dtype, (H, W, C), 40 + C, nonneg=epi))
        args = (inv, 0.25) if epi else (None, 1.0)
        for s in ROW_SIZES:
            whole = D.median(t, s, *args)
            assert whole.dtype == (torch.float32 if epi else t.dtype)
            for h in BAND_HEIGHTS:
                got = _banded(t, s, h, *args)
                assert got.dtype == whole.dtype
                assert torch.equal(_bits(got), _bits(whole)), (dtype, shape, epi, s, h)
            if s in (3, 5):  # the rank search on a network size: the same bits
                before = dict(D.MEDIAN_USED)
                gen = _banded(t, s, 17, *args, force_generic=True)
                assert D.MEDIAN_USED["generic"] > before["generic"]
                assert D.MEDIAN_USED["network"] == before["network"]
                assert torch.equal(_bits(gen), _bits(whole)), (dtype, shape, epi, s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scipy_fixture_through_bands(gpu, golden, dtype):
    g = golden("median")
    t = _up(g[f"{dtype}_in"])
    for s in SIZES:
        got = _down(_banded(t, s, 7), dtype)
        want = g[f"{dtype}_{size_key(s)}"]
        assert got.dtype == want.dtype
        assert np.array_equal(got, want), (dtype, s)


def test_missing_halo_rows_and_bad_arguments_raise(gpu):
    from milwrm_amd import device as D

    t = _up(_rand("u16", (45, 24, 3), 5))
    H = 45
    for size, hy, below in ((3, 1, 1), ((4, 7), 2, 1), (9, 4, 4)):
        raw = t[10:30]  # slide rows [10, 30)
        out = torch.full((20 - hy - below, 24, 3), 1234, dtype=torch.int16, device=gpu)
        before = dict(D.MEDIAN_USED)
        with pytest.raises(ValueError, match="above"):  # one halo row short at the top
            D.median_rows(raw, size, 10, H, hy - 1, 20 - below - 1, out=out)
        with pytest.raises(ValueError, match="below"):  # one short at the bottom
            D.median_rows(raw, size, 10, H, hy + 1, 20 - below + 1, out=out)
        assert D.MEDIAN_USED == before  # nothing launched
        assert bool((out == 1234).all())
        # exactly the halo: accepted, and the slide's rows
        got = D.median_rows(raw, size, 10, H, hy, 20 - below, out=out)
        assert torch.equal(got, D.median(t, size)[10 + hy:30 - below])
        # the slide's own edges need no halo
        assert torch.equal(D.median_rows(t[:20], size, 0, H, 0, 20 - below), D.median(t, size)[:20 - below])
        assert torch.equal(D.median_rows(t[30:], size, 30, H, hy, 15), D.median(t, size)[30 + hy:])
    with pytest.raises(ValueError):  # rows that are not rows of the slide
        D.median_rows(t[10:30], 3, 30, H, 1, 19)
    for r0, r1 in ((5, 5), (7, 5), (-1, 5), (0, 46)):
        with pytest.raises(ValueError):
            D.median_rows(t, 3, 0, H, r0, r1)
    with pytest.raises(ValueError):
        D.median_rows(t, 0, 0, H, 0, H)
    with pytest.raises(NotImplementedError):
        D.median_rows(t, 16, 0, H, 0, H)
    with pytest.raises(NotImplementedError):
        D.median_rows(t, (3, 16), 0, H, 0, H)
    with pytest.raises(ValueError):  # the output must not alias the rows
        D.median_rows(t, 3, 0, H, 0, H, out=t)
    with pytest.raises(ValueError):  # a compact output of another height
        D.median_rows(t, 3, 0, H, 0, 10, out=torch.empty_like(t))


def test_window_higher_than_the_slide(gpu):
    from milwrm_amd import device as D

    for dtype in DTYPES:
        t = _up(_rand(dtype, (3, 21, 2), 17))
        whole = D.median(t, 9)
        assert torch.equal(_bits(D.median_rows(t, 9, 0, 3, 0, 3)), _bits(whole))
        assert torch.equal(_bits(_banded(t, 9, 1)), _bits(whole))
        assert torch.equal(_bits(D.median_rows(t, 9, 0, 3, 1, 2)), _bits(whole[1:2]))
