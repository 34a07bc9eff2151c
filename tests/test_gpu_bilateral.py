"""Device bilateral filter (csrc/bilateral.hip, D.bilateral / D.image_std,
img.bilateral_filter / img.blurring('bilateral', sigma_color=...), the
labeler's filter_kwargs) against the float64 numpy brute force that
tests/test_cpu_bilateral.py pins to tests/golden/bilateral.npz.

Tolerance: |got - want| <= tol max(max|a|, |cval|), tol = min(1e-4, 8 e32).
e32 (in the fixture, per case) is the error of the same formula evaluated in
numpy float32, i.e. fp32's own error on it; the factor 8 covers the device's
few-ulp exp / divide and another summation order over up to 625 taps; 1e-4 is
the project's fp32 contract and only a ceiling."""
import numpy as np
import pandas as pd
import pytest

from tests.test_cpu_bilateral import CASES, VARIANTS, bilateral_want, brute_bilateral, variant_key  # noqa: F401

pytestmark = pytest.mark.gpu


def _up(a):
    from milwrm_amd import device as D

    return D.to_device_image(a)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check(got, want, a, cval, e32, what):
    tol = min(1e-4, 8 * e32)
    scale = max(float(np.abs(a).max()), abs(cval))
    err = float(np.abs(got.astype(np.float64) - want).max()) / scale
    print(f"{what}: err {err:.3e}  e32 {e32:.3e}  tol {tol:.3e}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("name,mode,cval", VARIANTS)
def test_equals_brute_force(gpu, golden, bilateral_want, name, mode, cval):
    import torch

    from milwrm_amd import device as D

    g = golden("bilateral")
    _, sigma, win, _ = CASES[name]
    a = g[f"{name}_in"]
    sc = float(g[f"{name}_sigma_color"])
    got = D.bilateral(_up(a), sigma, sc, win_size=win, mode=mode, cval=cval)
    assert got.dtype == torch.float32 and tuple(got.shape) == a.shape
    _check(got.cpu().numpy(), bilateral_want(name, mode, cval), a, cval,
           float(g[f"{name}_{variant_key(mode, cval)}_e32"]), (name, mode, cval))


def test_constant_image_comes_back_bit_identical(gpu):
    from milwrm_amd import device as D

    a = np.full((19, 33, 4), np.float32(0.3137), dtype=np.float32)
    for mode, cval in (("constant", 0.0), ("constant", 0.4), ("edge", 0.0)):
        got = D.bilateral(_up(a), 1.0, 0.2, mode=mode, cval=cval).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(a)), (mode, cval)
    u = np.full((9, 12, 2), 777, dtype=np.uint16)
    got = D.bilateral(_up(u), 1.0, 0.2).cpu().numpy()
    assert np.array_equal(got, u.astype(np.float32))


@pytest.mark.parametrize("dtype", ["u8", "u16"])
def test_fused_lognorm_load_equals_lognorm_first(gpu, dtype):
    import torch

    from milwrm_amd import device as D

    rng = np.random.default_rng(31)
    H, W, C = 27, 45, 5
    lev = rng.integers(20, 200 if dtype == "u8" else 50000, size=(4, 7, C))
    a = np.repeat(np.repeat(lev, 7, axis=0), 7, axis=1)[:H, :W] * rng.uniform(0.9, 1.1, size=(H, W, C))
    a = a.astype(np.uint8 if dtype == "u8" else np.uint16)
    if dtype == "u16":
        assert (a > 32767).any()
    t = _up(a)
    inv = torch.from_numpy((1.0 / np.array([30.0, 90.0, 150.0, 40.0, 700.0])).astype(np.float32)).to(t.device)
    for mode, cval, p in (("constant", 0.0, 1.0), ("edge", 0.0, 0.25), ("constant", 0.4, 1.0)):
        ln = D.lognorm(t, inv, p)
        sc = D.image_std(ln)
        fused = D.bilateral(t, 1.0, sc, mode=mode, cval=cval, inv_mean=inv, pseudoval=p).cpu().numpy()
        two = D.bilateral(ln, 1.0, sc, mode=mode, cval=cval).cpu().numpy()
        assert np.array_equal(_bits(fused), _bits(two)), (dtype, mode, cval, p)
        assert np.abs(two - ln.cpu().numpy()).max() > 0.01 * np.abs(two).max()  # the filter did something
        assert D.image_std(t, inv, p) == sc  # the moments take the same load transform


def test_image_std_equals_numpy(gpu):
    import torch

    from milwrm_amd import device as D

    rng = np.random.default_rng(41)
    for shape in ((2, 3, 1), (37, 53, 3), (64, 96, 30), (300, 517, 7)):
        a = (rng.normal(0.7, 0.4, size=shape) ** 2).astype(np.float32)
        a64 = a.astype(np.float64)
        m = D.image_moments(_up(a))
        assert m[0] == a.size and m[3] == a64.min() and m[4] == a64.max()
        assert abs(m[1] - a64.mean()) <= 1e-12 * abs(a64.mean())
        got, want = D.image_std(_up(a)), float(a64.std())
        assert abs(got - want) <= 1e-12 * want, (shape, got, want)
    u = rng.integers(0, 65536, size=(41, 29, 3)).astype(np.uint16)
    got, want = D.image_std(_up(u)), float(u.astype(np.float64).std())
    assert abs(got - want) <= 1e-12 * want
    inv = torch.from_numpy((1.0 / np.array([300.0, 9000.0, 40.0])).astype(np.float32)).to("cuda")
    ln = D.lognorm(_up(u), inv, 1.0).cpu().numpy().astype(np.float64)
    got, want = D.image_std(_up(u), inv, 1.0), float(ln.std())
    assert abs(got - want) <= 1e-12 * want


def test_bad_calls_raise(gpu):
    import torch

    from milwrm_amd import device as D

    a = np.random.default_rng(5).uniform(0, 1, size=(12, 14, 2)).astype(np.float32)
    t = _up(a)
    with pytest.raises(ValueError, match="alias"):
        D.bilateral(t, 1.0, 0.3, out=t)
    with pytest.raises(NotImplementedError):
        D.bilateral(t, 1.0, 0.3, win_size=27)
    with pytest.raises(NotImplementedError):  # the C entry's own limits: 64 channels
        D.bilateral(torch.zeros((4, 4, 65), device=t.device).add_(torch.rand((4, 4, 65), device=t.device)), 1.0, 0.3)
    with pytest.raises(ValueError):  # fp32 weights: exp2(k d^2) with k not finite
        D.bilateral(t, 1.0, 1e-30)


def _raw(shape=(31, 45, 3), seed=8):
    rng = np.random.default_rng(seed)
    H, W, C = shape
    lev = rng.integers(300, 50000, size=(-(-H // 7), -(-W // 7), C))
    a = np.repeat(np.repeat(lev, 7, axis=0), 7, axis=1)[:H, :W] * rng.uniform(0.9, 1.1, size=shape)
    return a.astype(np.uint16)


MEAN = np.array([812.5, 20000.0, 4000.25])


def test_img_log_normalize_then_bilateral(gpu):
    import torch

    import milwrm_amd as M
    from milwrm_amd import device as D

    a = _raw()
    im = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im.log_normalize(mean=MEAN)
    inv, p = im._pending
    im.blurring("bilateral", sigma=1, sigma_color=0.3)
    assert im._pending is None and im._dev.dtype == torch.float32
    want = D.bilateral(_up(a), 1, 0.3, inv_mean=inv, pseudoval=p).cpu().numpy()
    assert im.img.dtype == np.float64
    assert np.array_equal(im.img, want.astype(np.float64))
    # against the definition on the float64 log-normalised image, at the log_normalize golden test's tolerance
    ref = brute_bilateral(np.log10(a.astype(np.float64) / MEAN + 1), 1, 0.3)
    np.testing.assert_allclose(im.img, ref, rtol=1e-5, atol=2e-6)
    assert np.all(im._xbound >= np.abs(im.img).max(axis=(0, 1)))
    # options, bins ignored, a two-dimensional image
    im2 = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im2.log_normalize(mean=MEAN)
    im2.bilateral_filter(1, 0.3, win_size=7, bins=10, mode="edge")
    want2 = D.bilateral(_up(a), 1, 0.3, win_size=7, mode="edge", inv_mean=inv, pseudoval=p).cpu().numpy()
    assert np.array_equal(im2.img, want2.astype(np.float64))
    b = a[:, :, 0].copy()
    im3 = M.img(b)
    im3.blurring("bilateral", sigma=1, sigma_color=2000.0, cval=0.4)
    assert im3.img.shape == b.shape
    want3 = D.bilateral(_up(b[:, :, None]), 1, 2000.0, cval=0.4).cpu().numpy()[:, :, 0]
    assert np.array_equal(im3.img, want3.astype(np.float64))
    assert np.all(im3._xbound >= 65535.0)


def test_img_sigma_color_std(gpu):
    import milwrm_amd as M
    from milwrm_amd import device as D

    a = _raw(seed=9)
    im = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im.log_normalize(mean=MEAN)
    a64 = im.copy().img  # the fp32 log-normalised pixels as float64
    im.blurring("bilateral", sigma=1, sigma_color="std")
    im2 = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im2.log_normalize(mean=MEAN)
    sc = float(np.std(a64))
    im2.blurring("bilateral", sigma=1, sigma_color=sc)
    assert abs(D.image_std(_up(a64.astype(np.float32))) - sc) <= 1e-12 * sc
    np.testing.assert_allclose(im.img, im2.img, rtol=0, atol=1e-6)  # sigma_color equal to 1e-12: the same weights
    assert np.abs(im.img - a64).max() > 0.01 * np.abs(a64).max()


def test_img_pending_median_applies_first(gpu):
    import milwrm_amd as M
    from milwrm_amd import device as D

    a = _raw(seed=10)
    im = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im.log_normalize(mean=MEAN)
    inv, p = im._pending
    im._pending_median = (3, 3)  # as median_filter leaves it on a slide it keeps deferred
    im.blurring("bilateral", sigma=1, sigma_color=0.3)
    assert im._pending_median is None and im._pending is None
    med = D.median(_up(a), 3, inv_mean=inv, pseudoval=p)
    want = D.bilateral(med, 1, 0.3).cpu().numpy()
    assert np.array_equal(im.img, want.astype(np.float64))
    # a materialised median, then the bilateral
    im2 = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im2.log_normalize(mean=MEAN)
    im2.blurring("median", size=3)
    im2.blurring("bilateral", sigma=1, sigma_color=0.3)
    assert np.array_equal(im2.img, im.img)
    # a gaussian first
    im3 = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im3.log_normalize(mean=MEAN)
    im3.blurring("gaussian", sigma=1)
    g = im3.copy().img.astype(np.float32)
    im3.blurring("bilateral", sigma=1, sigma_color=0.3, mode="edge")
    want3 = D.bilateral(_up(g), 1, 0.3, mode="edge").cpu().numpy()
    assert np.array_equal(im3.img, want3.astype(np.float64))


def test_img_refusals(gpu):
    import milwrm_amd as M
    from milwrm_amd import bands, stream

    a = _raw((40, 16, 2), seed=13)
    band = bands.band_image(a, np.ones(a.shape[:2], dtype=np.uint8), 0, 2)
    with pytest.raises(NotImplementedError, match="neighbour rows"):
        band.blurring("bilateral", sigma=1, sigma_color=0.3)
    with pytest.raises(NotImplementedError, match="neighbour rows"):
        band.bilateral_filter(1, 0.3)
    src = M.img.from_source(stream.SynthSource(64, 48, 4, 77))
    with pytest.raises(MemoryError, match="banded form"):
        src.blurring("bilateral", sigma=1, sigma_color=0.3)
    im = M.img(a.copy())
    with pytest.raises(NotImplementedError, match="sigma_color="):
        im.blurring("bilateral", sigma=1)
    with pytest.raises(NotImplementedError):
        im.blurring("bilateral", sigma=1, sigma_color=0.3, size=3)
    with pytest.raises(NotImplementedError):
        im.blurring("bilateral", sigma=1, sigma_color=0.3, win_size=27)


def _slides():
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[:64, :64]
    slides, masks = [], []
    for i in range(2):
        base = np.repeat(np.repeat(rng.integers(0, 3, size=(10, 10)), 7, axis=0), 7, axis=1)[:64, :64]
        prof = rng.integers(200, 60000, size=(3, 4))
        a = (prof[base] * rng.uniform(0.8, 1.2, size=(64, 64, 4))).clip(0, 65535).astype(np.uint16)
        slides.append(a)
        masks.append(((yy - 30 - 3 * i) ** 2 + (xx - 33) ** 2 < (27 - i) ** 2).astype(np.uint8))
    return slides, masks


def test_labeler_with_bilateral_filter(gpu):
    import milwrm_amd as M

    slides, masks = _slides()
    feats = [0, 1, 2, 3]
    imgs = [M.img(a.copy(), mask=m.copy()) for a, m in zip(slides, masks)]
    ests, pix = zip(*[im.calculate_non_zero_mean() for im in imgs])
    df = pd.DataFrame({"Img": imgs, "batch_names": ["b0", "b1"], "mean estimators": list(ests),
                       "pixels": list(pix)})
    lab = M.mxif_labeler(df)
    means = lab._batch_means()
    lab.prep_cluster_data(feats, filter_name="bilateral", sigma=1, fract=0.2, filter_kwargs={"sigma_color": 0.3})
    rows = []
    for a, m, b in zip(slides, masks, ["b0", "b1"]):
        c = M.img(a.copy(), mask=m.copy())
        c.log_normalize(mean=means[b])
        plain = c.copy().img
        c.blurring("bilateral", sigma=1, sigma_color=0.3)
        assert np.abs(c.img - plain).max() > 0.01 * np.abs(plain).max()
        rows.append(c.subsample_pixels(feats, 0.2))
    hand = np.concatenate(rows, axis=0)
    assert hand.shape[0] > 300
    assert np.array_equal(lab._device_rows().X.cpu().numpy(), hand.astype(np.float32))
    mu, inv = lab.scaler.affine()
    assert np.array_equal(_bits(lab.cluster_data), _bits((hand - mu) * inv))
    lab.label_tissue_regions(k=3, plot_out=False, random_state=18)
    lab.confidence_score_images()
    for tid, conf, a, m in zip(lab.tissue_IDs, lab.confidence_IDs, slides, masks):
        tid, conf = np.asarray(tid), np.asarray(conf)
        assert tid.shape == conf.shape == a.shape[:2]
        assert np.array_equal(np.isnan(tid), m == 0)
        assert set(np.unique(tid[m != 0])) <= {0.0, 1.0, 2.0}
        assert np.all(np.isfinite(conf[m != 0]))
