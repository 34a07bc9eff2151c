"""Device median filter (csrc/median.hip, D.median, img.median_filter /
img.blurring('median', size=k), the labeler's filter_kwargs): equality with
scipy's results (tests/golden/median.npz) and with the numpy brute force that
tests/test_cpu_median.py pins to them, on both kernel paths."""
import numpy as np
import pandas as pd
import pytest

from tests.test_cpu_median import DTYPES, SIZES, brute_median, size_key

pytestmark = pytest.mark.gpu

NP_DTYPE = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def _rand(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    if dtype == "u8":
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    if dtype == "u16":
        a = rng.integers(0, 65536, size=shape).astype(np.uint16)
        a.reshape(-1)[::7] = 32768 + (a.reshape(-1)[::7] >> 1)  # plenty above 32767
        return a
    a = rng.normal(0.0, 2.0, size=shape).astype(np.float32)  # negatives
    f = a.reshape(-1)
    f[::11] = np.float32(3e38)
    f[5::13] = np.float32(-3e38)
    f[3::9] = np.array([1e-41, -2e-42, 7e-45], dtype=np.float32)[np.arange(f[3::9].size) % 3]  # subnormals
    return a


def _ties(dtype, shape, seed):
    a = _rand(dtype, shape, seed)
    a[np.random.default_rng(seed + 1).uniform(size=shape) < 0.5] = 0  # half the pixels zero
    a[:, :, -1] = NP_DTYPE[dtype](7)  # one constant plane
    return a


def _up(a):
    from milwrm_amd import device as D

    return D.to_device_image(a)


def _down(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == "u16" else a


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("dtype", DTYPES)
def test_equals_scipy_fixture(gpu, golden, dtype):
    from milwrm_amd import device as D

    g = golden("median")
    a = g[f"{dtype}_in"]
    t = _up(a)
    for s in SIZES:
        got = _down(D.median(t, s), dtype)
        want = g[f"{dtype}_{size_key(s)}"]
        assert got.dtype == want.dtype
        assert np.array_equal(got, want), (dtype, s)


# name -> (maker, shape): heavy ties; images smaller than the window; channel
# counts that break the 16-byte alignment of a pixel row (1, 5, 30, 50; 30 and
# 50 channels are split into chunks of words); more than two 16-row x 64-pixel
# tiles plus a remainder both ways (70 x 133 x 3; at 30 channels the tile is
# 17 pixels wide, at 50 channels 19)
IMAGES = {
    "ties": (_ties, (37, 53, 3)),
    "one": (_rand, (1, 1, 1)),
    "tiny": (_rand, (2, 3, 1)),
    "small": (_rand, (5, 4, 2)),
    "c1": (_rand, (19, 45, 1)),
    "c5": (_rand, (21, 34, 5)),
    "c30": (_rand, (18, 70, 30)),
    "c50": (_rand, (20, 40, 50)),
    "tiles": (_rand, (70, 133, 3)),
}


@pytest.mark.parametrize("name", list(IMAGES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_equals_brute_force(gpu, dtype, name):
    from milwrm_amd import device as D

    make, shape = IMAGES[name]
    a = make(dtype, shape, 100 + len(name) + shape[1])
    if dtype == "u16" and a.size > 8:
        assert (a > 32767).any()
    t = _up(a)
    for s in SIZES:
        got = _down(D.median(t, s), dtype)
        assert np.array_equal(got, brute_median(a, s)), (dtype, name, s)


def test_size_one_is_a_copy(gpu):
    from milwrm_amd import device as D

    for dtype in DTYPES:
        a = _rand(dtype, (9, 11, 3), 3)
        assert np.array_equal(_bits(_down(D.median(_up(a), 1), dtype)), _bits(a))
        assert np.array_equal(_down(D.median(_up(a), (1, 3)), dtype), brute_median(a, (1, 3)))


def test_paths_taken_and_forced_generic_bits(gpu):
    from milwrm_amd import device as D

    for dtype in DTYPES:
        a = _ties(dtype, (37, 53, 3), 11)
        if dtype == "f32":
            a.reshape(-1)[::5] = np.float32(-0.0)  # zeros of both signs in one window
        t = _up(a)
        for s in (2, 3, 5):
            before = dict(D.MEDIAN_USED)
            net = D.median(t, s)
            assert D.MEDIAN_USED["network"] == before["network"] + 1
            assert D.MEDIAN_USED["generic"] == before["generic"]
            gen = D.median(t, s, force_generic=True)
            assert D.MEDIAN_USED["generic"] == before["generic"] + 1
            assert D.MEDIAN_USED["network"] == before["network"] + 1
            assert np.array_equal(_bits(net.cpu().numpy()), _bits(gen.cpu().numpy())), (dtype, s)
        for s in (4, 7, (2, 5)):
            before = dict(D.MEDIAN_USED)
            D.median(t, s)
            assert D.MEDIAN_USED["generic"] == before["generic"] + 1
            assert D.MEDIAN_USED["network"] == before["network"]


def _same_bits_or_nan(a, b):
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lognorm_epilogue_is_lognorm_of_median(gpu, dtype):
    import torch

    from milwrm_amd import device as D

    a = _rand(dtype, (37, 53, 4), 21)
    if dtype == "f32":
        a = np.abs(a)
        a[a > 1e30] = np.float32(12.5)
    t = _up(a)
    with np.errstate(divide="ignore"):  # one channel with inv = inf
        inv_h = (np.float32(1.0) / np.array([3.0, 150.0, 0.0, 4000.0], dtype=np.float32))
    assert np.isinf(inv_h[2])
    inv = torch.from_numpy(inv_h).to(t.device)
    for s in (3, 4):
        for p in (1.0, 0.25):
            fused = D.median(t, s, inv, p)
            assert fused.dtype == torch.float32
            two = D.lognorm(D.median(t, s), inv, p)
            fa, ta = fused.cpu().numpy(), two.cpu().numpy()
            assert np.array_equal(fa, ta, equal_nan=True), (dtype, s, p)
            assert _same_bits_or_nan(fa, ta), (dtype, s, p)
            gen = D.median(t, s, inv, p, force_generic=True).cpu().numpy()
            assert _same_bits_or_nan(fa, gen), (dtype, s, p)


def test_lognorm_epilogue_equals_median_of_lognorm(gpu):
    """Selection commutes with a non-decreasing map: on distinct integers over
    which the device lognorm is non-decreasing (asserted on its downloaded
    values), median-then-lognorm equals the brute-force median of lognorm."""
    import torch

    from milwrm_amd import device as D

    H, W, C = 24, 32, 2
    rng = np.random.default_rng(5)
    vals = np.sort(rng.choice(65536, size=H * W, replace=False)).astype(np.uint16)  # distinct, sorted
    a = np.stack([rng.permutation(vals), rng.permutation(vals)], axis=1).reshape(H, W, C)
    t = _up(a)
    inv = torch.from_numpy((1.0 / np.array([900.0, 31000.0])).astype(np.float32)).to(t.device)
    L = D.lognorm(t, inv, 1.0).cpu().numpy()
    for c in range(C):
        order = np.argsort(a[:, :, c].reshape(-1), kind="stable")
        assert np.all(np.diff(L[:, :, c].reshape(-1)[order]) >= 0), "device lognorm not monotone here"
    for s in (3, 4, (2, 5)):
        got = D.median(t, s, inv, 1.0).cpu().numpy()
        assert np.array_equal(got, brute_median(L, s)), s


def test_blurring_median_keeps_uint16_storage(gpu):
    import torch

    import milwrm_amd as M

    a = _rand("u16", (31, 45, 3), 8)
    im = M.img(a.copy())
    im.blurring("median", size=3)
    assert im._dev.dtype == torch.int16 and tuple(im._dev.shape) == a.shape
    assert im.img.dtype == np.float64
    assert np.array_equal(im.img, brute_median(a.astype(np.float64), 3))


def test_two_dimensional_image_and_median_filter_pair(gpu):
    import milwrm_amd as M

    a = _rand("u16", (29, 41), 9)
    im = M.img(a.copy())
    im.blurring("median", size=3)
    assert im.img.shape == a.shape
    assert np.array_equal(im.img, brute_median(a.astype(np.float64), 3))
    b = _rand("u8", (17, 23, 2), 10)
    im = M.img(b.copy())
    im.median_filter((2, 5))
    assert np.array_equal(im.img, brute_median(b.astype(np.float64), (2, 5)))
    im2 = M.img(a.copy())
    im2.median_filter((2, 5))
    assert np.array_equal(im2.img, brute_median(a.astype(np.float64), (2, 5)))


def test_median_after_log_normalize(gpu):
    """img.log_normalize then blurring('median'): the fused epilogue, against
    the float64 evaluation, with the tolerance of the standalone log_normalize
    golden test (test_gpu_parity.test_lognorm_standalone_and_mean_none)."""
    import torch

    import milwrm_amd as M
    from milwrm_amd import device as D

    a = _rand("u16", (33, 47, 3), 12)
    mean = np.array([812.5, 20000.0, 40.25])
    ref = brute_median(np.log10(a.astype(np.float64) / mean + 1), 3)
    im = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im.log_normalize(mean=mean)
    before = dict(D.MEDIAN_USED)
    im.blurring("median", size=3)
    assert D.MEDIAN_USED["network"] == before["network"] + 1
    assert im._dev.dtype == torch.float32 and im._pending is None
    np.testing.assert_allclose(im.img, ref, rtol=2e-6, atol=1e-6)
    # the same through the materialised path (a gaussian first, then the median)
    im = M.img(a.copy(), mask=np.ones(a.shape[:2]))
    im.log_normalize(mean=mean)
    x = im.img.copy()  # materialises the log_normalize
    im.median_filter(4)
    assert np.array_equal(im.img, brute_median(x.astype(np.float32), 4).astype(np.float64))


def test_row_band_and_bad_sizes_raise(gpu):
    from milwrm_amd import bands
    from milwrm_amd import device as D

    a = _rand("u16", (40, 16, 2), 13)
    band = bands.band_image(a, np.ones(a.shape[:2], dtype=np.uint8), 0, 2)
    with pytest.raises(NotImplementedError, match="neighbour rows"):
        band.blurring("median", size=3)
    with pytest.raises(NotImplementedError, match="neighbour rows"):
        band.median_filter(3)
    t = _up(a)
    with pytest.raises(ValueError):
        D.median(t, 0)
    with pytest.raises(NotImplementedError):
        D.median(t, 16)
    with pytest.raises(NotImplementedError):
        D.median(t, (3, 16))
    with pytest.raises(ValueError):  # the output must not alias the image
        D.median(t, 3, out=t)


def _slides():
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[:64, :64]
    slides, masks = [], []
    for i in range(2):
        base = rng.integers(0, 3, size=(64, 64))  # three rough domains
        base = brute_median(base.astype(np.uint16), 7)
        prof = rng.integers(200, 60000, size=(3, 4))
        a = (prof[base] * rng.uniform(0.6, 1.4, size=(64, 64, 4))).clip(0, 65535).astype(np.uint16)
        a[rng.uniform(size=a.shape) < 0.02] = 65535  # hot pixels
        slides.append(a)
        masks.append(((yy - 30 - 3 * i) ** 2 + (xx - 33) ** 2 < (27 - i) ** 2).astype(np.uint8))
    return slides, masks


def _labeler(slides, masks):
    import milwrm_amd as M

    imgs = [M.img(a.copy(), mask=m.copy()) for a, m in zip(slides, masks)]
    ests, pix = zip(*[im.calculate_non_zero_mean() for im in imgs])
    df = pd.DataFrame({"Img": imgs, "batch_names": ["b0", "b1"], "mean estimators": list(ests),
                       "pixels": list(pix)})
    return M.mxif_labeler(df)


def test_labeler_with_median_filter(gpu):
    import milwrm_amd as M

    slides, masks = _slides()
    feats = [0, 1, 2, 3]
    lab = _labeler(slides, masks)
    means = lab._batch_means()
    lab.prep_cluster_data(feats, filter_name="median", filter_kwargs={"size": 3}, fract=0.2)
    rows = []
    for a, m, b in zip(slides, masks, ["b0", "b1"]):
        c = M.img(a.copy(), mask=m.copy())
        c.log_normalize(mean=means[b])
        c.blurring("median", size=3)
        rows.append(c.subsample_pixels(feats, 0.2))
    hand = np.concatenate(rows, axis=0)
    assert hand.shape[0] > 300
    assert np.array_equal(lab._device_rows().X.cpu().numpy(), hand.astype(np.float32))
    assert np.array_equal(hand.astype(np.float32).astype(np.float64), hand)
    mu, inv = lab.scaler.affine()
    assert np.array_equal(_bits(lab.cluster_data), _bits((hand - mu) * inv))
    lab.label_tissue_regions(k=3, plot_out=False, random_state=18)
    for tid, a, m in zip(lab.tissue_IDs, slides, masks):
        tid = np.asarray(tid)
        assert tid.shape == a.shape[:2]
        assert np.array_equal(np.isnan(tid), m == 0)
        assert set(np.unique(tid[m != 0])) <= {0.0, 1.0, 2.0}


def test_labeler_filter_kwargs_none_changes_nothing(gpu):
    slides, masks = _slides()
    feats = [0, 1, 2, 3]
    lab0 = _labeler(slides, masks)
    lab0.prep_cluster_data(feats, filter_name="gaussian", sigma=2, fract=0.2)
    lab1 = _labeler(slides, masks)
    lab1.prep_cluster_data(feats, filter_name="gaussian", sigma=2, fract=0.2, filter_kwargs=None)
    assert np.array_equal(_bits(lab0.cluster_data), _bits(lab1.cluster_data))
