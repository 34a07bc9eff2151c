"""The row-window bilateral (mw_bilateral_rows / D.bilateral_rows): bands that
tile a slide give the rows of one D.bilateral call over the whole slide BITWISE
(a pixel's taps are summed in one order whichever tile or band computes it), the
golden fixture driven through bands meets the whole-slide bound, and the
band-wise moments (stream.image_moments) have bits that do not depend on the
band height and equal numpy's float64 values."""
import numpy as np
import pytest

from tests.test_cpu_bilateral import CASES, VARIANTS, bilateral_want, variant_key  # noqa: F401

pytestmark = pytest.mark.gpu

H, W = 45, 40                 # five 8-row tiles and a 5-row rest; one 32-pixel tile and an 8-pixel rest
BANDS = (1, 3, 8, 9, 37)      # below the sigma-1 halo, the tile height, one past it, a last partial band


def _up(a):
    from milwrm_amd import device as D

    return D.to_device_image(a)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _raw(shape, dtype, seed=8):
    """Piecewise-constant 7 x 7 domains times noise (tests/test_gpu_bilateral.py's
    ``_raw``, for the three element types)."""
    rng = np.random.default_rng(seed)
    h, w, C = shape
    top = {"u8": 200, "u16": 50000, "f32": 50000}[dtype]
    lev = rng.integers(20 if dtype == "u8" else 300, top, size=(-(-h // 7), -(-w // 7), C))
    a = np.repeat(np.repeat(lev, 7, axis=0), 7, axis=1)[:h, :w] * rng.uniform(0.9, 1.1, size=shape)
    if dtype == "f32":
        return (a / 20000.0).astype(np.float32)
    return a.astype(np.uint8 if dtype == "u8" else np.uint16)


def _inv(C, dtype, dev):
    import torch

    mean = np.linspace(40.0, 150.0, C) if dtype == "u8" else np.linspace(800.0, 21000.0, C)
    return torch.from_numpy((1.0 / mean).astype(np.float32)).to(dev)


def _banded(t, h, sigma, sc, win, mode, cval, inv, p):
    """The slide filtered in bands of ``h`` output rows, each from its own
    rows plus the halo (stream._plan), into one array."""
    import torch

    from milwrm_amd import device as D
    from milwrm_amd import stream

    Hs = int(t.shape[0])
    r = D.bilateral_args(sigma, sc, win, mode, cval)[2]
    out = torch.full(tuple(t.shape), float("nan"), dtype=torch.float32, device=t.device)
    for y0, y1, a, b in stream._plan(Hs, h, r, 0, Hs):
        got = D.bilateral_rows(t[a:b], sigma, sc, a, Hs, y0 - a, y1 - a, win_size=win, mode=mode, cval=cval,
                               inv_mean=inv, pseudoval=p)
        assert tuple(got.shape) == (y1 - y0, t.shape[1], t.shape[2])
        out[y0:y1] = got
    return out.cpu().numpy()


def _whole_vs_bands(shape, dtype, logn, mode, cval, win, bands):
    from milwrm_amd import device as D

    a = _raw(shape, dtype, seed=sum(shape) + win)
    t = _up(a)
    inv, p = (_inv(shape[2], dtype, t.device), 0.5) if logn else (None, 1.0)
    x = (D.lognorm(t, inv, p) if logn else D.as_float32(t)).cpu().numpy()  # what the filter sees
    sc = float(x.astype(np.float64).std())
    whole = D.bilateral(t, 1.0, sc, win_size=win, mode=mode, cval=cval, inv_mean=inv, pseudoval=p).cpu().numpy()
    assert np.isfinite(whole).all()
    assert np.abs(whole - x).max() > 0.01 * np.abs(x).max()  # the filter moved pixels
    for h in bands:
        got = _banded(t, h, 1.0, sc, win, mode, cval, inv, p)
        assert np.array_equal(_bits(got), _bits(whole)), (h, int((_bits(got) != _bits(whole)).sum()))


@pytest.mark.parametrize("C,dtype,logn,mode,cval,win", [
    (1, "f32", False, "constant", 0.4, 7), (1, "u16", True, "edge", 0.0, 13),
    (4, "u16", True, "constant", 0.4, 13), (4, "u8", False, "edge", 0.0, 7),
    (5, "u8", True, "constant", 0.4, 7), (5, "f32", False, "edge", 0.0, 13),
    (30, "u16", False, "constant", 0.4, 7), (30, "u16", True, "edge", 0.0, 13),
])
def test_bands_equal_the_whole_slide_bitwise(gpu, C, dtype, logn, mode, cval, win):
    _whole_vs_bands((H, W, C), dtype, logn, mode, cval, win, BANDS)


def test_window_higher_than_the_slide(gpu):
    """win_size 25 on an 11-row slide: every band's halo exceeds the slide."""
    for mode, cval in (("constant", 0.4), ("edge", 0.0)):
        _whole_vs_bands((11, W, 4), "u16", True, mode, cval, 25, (1, 3, 8))


def test_fifty_channels(gpu):
    _whole_vs_bands((H, W, 50), "u16", True, "constant", 0.4, 7, (3, 9, 37))


@pytest.mark.parametrize("name,mode,cval", VARIANTS)
def test_golden_fixture_through_seven_row_bands(gpu, golden, bilateral_want, name, mode, cval):
    """tests/test_gpu_bilateral.py::test_equals_brute_force's bound, min(1e-4,
    8 e32) max(max|a|, |cval|), for the slide filtered in 7-row bands."""
    g = golden("bilateral")
    _, sigma, win, _ = CASES[name]
    a = g[f"{name}_in"]
    sc = float(g[f"{name}_sigma_color"])
    got = _banded(_up(a), 7, sigma, sc, win, mode, cval, None, 1.0)
    e32 = float(g[f"{name}_{variant_key(mode, cval)}_e32"])
    tol = min(1e-4, 8 * e32)
    scale = max(float(np.abs(a).max()), abs(cval))
    err = float(np.abs(got.astype(np.float64) - bilateral_want(name, mode, cval)).max()) / scale
    print(f"{name} {mode} {cval}: err {err:.3e}  e32 {e32:.3e}  tol {tol:.3e}")
    assert err <= tol, (name, mode, cval, err, tol)


def test_missing_halo_raises_value_error(gpu):
    import torch

    from milwrm_amd import device as D

    t = _up(_raw((20, 16, 3), "u16"))
    with pytest.raises(ValueError, match="above"):
        D.bilateral_rows(t, 1.0, 3000.0, 10, 45, 2, 17)     # sigma 1: radius 3
    with pytest.raises(ValueError, match="below"):
        D.bilateral_rows(t, 1.0, 3000.0, 10, 45, 3, 18)
    with pytest.raises(ValueError, match="rows of a"):
        D.bilateral_rows(t, 1.0, 3000.0, 30, 45, 3, 17)
    with pytest.raises(ValueError, match="output rows"):
        D.bilateral_rows(t, 1.0, 3000.0, 10, 45, 5, 5)
    with pytest.raises(ValueError, match="out must be"):
        D.bilateral_rows(t, 1.0, 3000.0, 10, 45, 3, 17, out=torch.empty((20, 16, 3), device=t.device))
    got = D.bilateral_rows(t, 1.0, 3000.0, 10, 45, 3, 17)
    assert tuple(got.shape) == (14, 16, 3)


# ------------------------------------------------------------------ moments

def _moment_cases(dev):
    rng = np.random.default_rng(43)
    f = (rng.normal(0.7, 0.4, size=(37, 53, 3)) ** 2).astype(np.float32)
    u = rng.integers(0, 65536, size=(41, 29, 5)).astype(np.uint16)
    return [("f32", f, None), ("u16", u, None), ("u16_lognorm", u, _inv(5, "u16", dev))]


def test_moments_do_not_depend_on_the_bands_and_equal_numpy(gpu):
    from milwrm_amd import device as D
    from milwrm_amd import stream

    for what, a, inv in _moment_cases(D.device()):
        t = _up(a)
        x = (D.lognorm(t, inv, 1.0) if inv is not None else D.as_float32(t)).cpu().numpy().astype(np.float64)
        whole = stream.image_moments(t, inv, 1.0)
        assert whole.dtype == np.float64 and whole.shape == (5,)
        for h in (1, 5, 16):
            m = stream.image_moments(t, inv, 1.0, band_rows=h)
            assert np.array_equal(_bits(m), _bits(whole)), (what, h, m, whole)
        # read from host memory band by band: the same bits again
        m = stream.image_moments(stream.HostSource(a), inv, 1.0, band_rows=5)
        assert np.array_equal(_bits(m), _bits(whole)), (what, "host", m, whole)
        assert whole[0] == x.size and whole[3] == x.min() and whole[4] == x.max()
        assert abs(whole[1] - x.mean()) <= 1e-12 * abs(x.mean())
        got, want = float(np.sqrt(whole[2] / whole[0])), float(x.std())
        print(f"{what}: std {got!r} numpy {want!r} rel {abs(got - want) / want:.2e}")
        assert abs(got - want) <= 1e-12 * want, (what, got, want)
        first = stream.image_moments(t, inv, 1.0, m2=False, band_rows=5)  # the first read only
        assert np.isnan(first[2])
        assert np.array_equal(_bits(first[[0, 1, 3, 4]]), _bits(whole[[0, 1, 3, 4]]))
