"""The bilateral filter on slides that are streamed in row bands: with
``banded=True`` a deferred bilateral (``img._pending_bilateral``) is applied
band by band inside the subsample, the label pass and the QC sums
(stream.BilateralBand over mw_bilateral_rows).  A pixel's taps are summed in
one order whichever band computes it, and the whole-slide numbers come from
stream.image_moments, whose bits do not depend on the bands, so every result
of the streamed pipeline is BITWISE the resident one (the keys of
tests/test_gpu_stream.py::_assert_same, the QC estimators included).
Composition with log_normalize and a second filter, a constant slide, eviction
back to the deferred state, a slide that cannot be held whole, and the refusal
without ``banded=True``."""
import numpy as np
import pandas as pd
import pytest

from tests.test_gpu_stream import _assert_same, _slides

pytestmark = pytest.mark.gpu

SC = 0.3  # sigma_color on log-normalised pixels (their spread is a few tenths)


def _host_imgs(slides):
    import milwrm_amd as M

    return [M.img(r.copy(), mask=m.copy()) for r, m in slides]


def _pipeline(imgs, sigma, fkw, k=5):
    """tests/test_gpu_stream.py::_pipeline with the bilateral filter and QC on."""
    import milwrm_amd as M
    from milwrm_amd.MILWRM import estimate_mse_mxif, estimate_percentage_variance_mxif

    C = imgs[0].n_ch
    feats = list(range(C))
    ests, pix = zip(*[im.calculate_non_zero_mean() for im in imgs])
    df = pd.DataFrame({"Img": imgs, "batch_names": ["b1", "b1", "b2"][:len(imgs)],
                       "mean estimators": list(ests), "pixels": list(pix)})
    lab = M.mxif_labeler(df)
    lab.prep_cluster_data(features=feats, filter_name="bilateral", sigma=sigma, filter_kwargs=dict(fkw), fract=0.2)
    lab.label_tissue_regions(k=k, plot_out=False, random_state=18)
    lab.confidence_score_images()
    out = dict(est=np.asarray(ests), pix=np.asarray(pix), mean=lab.scaler.mean_,
               scale=lab.scaler.scale_, idx=lab.kmeans.init_indices_, n_iter=lab.kmeans.n_iter_,
               centers=lab.kmeans.cluster_centers_, inertia=lab.kmeans.inertia_,
               rows=lab.kmeans.labels_, conf_df=lab.confidence_score_df.values,
               tid=[np.nan_to_num(t, nan=-1) for t in lab.tissue_IDs],
               cid=[np.nan_to_num(c, nan=-1) for c in lab.confidence_IDs],
               dom=[d.cpu().numpy() for d in lab._dom_dev],
               np_state=np.random.get_state()[1].copy())
    out["pv"] = [estimate_percentage_variance_mxif(im, False, lab.scaler, lab.kmeans.cluster_centers_,
                                                   feats, t) for im, t in zip(imgs, lab.tissue_IDs)]
    mse = estimate_mse_mxif(imgs, False, list(lab.tissue_IDs), lab.scaler, lab.kmeans.cluster_centers_,
                            feats, k)
    out["mse"] = np.array([mse[i] for i in range(k)])
    assert np.all(np.isfinite(out["pv"]))
    out["resident"] = [im._dev is not None for im in imgs]
    out["deferred"] = [im._pending_bilateral is not None for im in imgs]
    return out


_REF = {}


def _resident_ref(monkeypatch, C, dtype, sigma, n=3):
    """The resident run (no budget cap) on the default path, computed once per case."""
    key = (C, np.dtype(dtype).name, sigma, n)
    if key not in _REF:
        monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
        monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
        _REF[key] = _pipeline(_host_imgs(_slides(C, n=n, dtype=dtype)), sigma, {"sigma_color": SC})
        assert all(_REF[key]["resident"]) and not any(_REF[key]["deferred"])
    return _REF[key]


COUNTERS = (("BILATERAL_USED", "rows_streamed"), ("FUSED_USED", "sample_streamed"),
            ("FUSED_USED", "assign_streamed"))


def _counters():
    from milwrm_amd import device as D

    return {(d, k): getattr(D, d)[k] for d, k in COUNTERS}


# band heights: 2 is below the sigma-1 halo (3 rows) -- the moments and the subsample then run in
# 2-row bands; the label pass and the QC sums take no band under 16 rows (assign.banded_assign_image
# gives up below that), so that case sets their height to 16; sigma 2 is the 13 x 13 window
@pytest.mark.parametrize("C,dtype,band,sigma", [(8, np.uint16, "37", 1), (7, np.uint16, "2", 1),
                                                (5, np.uint8, "29", 2)])
def test_streamed_equals_resident(gpu, monkeypatch, C, dtype, band, sigma):
    ref = _resident_ref(monkeypatch, C, dtype, sigma)
    monkeypatch.setenv("MW_HBM_BUDGET", "1")  # nothing may stay resident: every pass streams
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", band)
    if int(band) < 16:
        monkeypatch.setenv("MW_ASSIGN_BAND_ROWS", "16")
    before = _counters()
    got = _pipeline(_host_imgs(_slides(C, dtype=dtype)), sigma, {"sigma_color": SC, "banded": True})
    assert not any(got["resident"]) and all(got["deferred"])
    for key, n in _counters().items():
        assert n > before[key], key
    _assert_same(got, ref)


def test_std_streamed_equals_resident_given_the_number(gpu, monkeypatch):
    """sigma_color="std" on a streamed slide resolves through
    stream.image_moments; a resident default run given that number agrees."""
    from milwrm_amd import stream

    monkeypatch.setenv("MW_HBM_BUDGET", "1")
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "37")
    before = _counters()
    imgs = _host_imgs(_slides(8, n=1))
    got = _pipeline(imgs, 1, {"sigma_color": "std", "banded": True})
    assert not any(got["resident"]) and all(got["deferred"])
    assert _counters()["BILATERAL_USED", "rows_streamed"] > before["BILATERAL_USED", "rows_streamed"]
    im = imgs[0]
    inv, p = im._pending
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "11")  # another band height: the same bits
    m = stream.image_moments(im._source(), inv, p)
    v = float(np.sqrt(m[2] / m[0]))
    assert v > 0 and im._pending_bilateral[1] == v
    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
    ref = _pipeline(_host_imgs(_slides(8, n=1)), 1, {"sigma_color": v})
    assert all(ref["resident"]) and not any(ref["deferred"])
    _assert_same(got, ref)


def test_device_generator_streamed_equals_resident(gpu, monkeypatch):
    """Slides read band by band from the device generator (img.from_source)
    against host copies of the same generated slides, resident."""
    import milwrm_amd as M
    from milwrm_amd import device as D
    from milwrm_amd import stream

    shapes = [(150 + 17 * i, 176 + 32 * i) for i in range(2)]
    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
    host = []
    for i, (H, W) in enumerate(shapes):
        raw, mask = D.synth_slide(H, W, 8, seed=930 + i)
        host.append((raw.cpu().numpy().view(np.uint16), mask.cpu().numpy()))
    ref = _pipeline(_host_imgs(host), 1, {"sigma_color": SC})
    assert all(ref["resident"])
    monkeypatch.setenv("MW_HBM_BUDGET", "1")
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "45")
    before = _counters()
    imgs = [M.img.from_source(stream.SynthSource(H, W, 8, 930 + i)) for i, (H, W) in enumerate(shapes)]
    got = _pipeline(imgs, 1, {"sigma_color": SC, "banded": True})
    assert not any(got["resident"]) and all(got["deferred"])
    for key, n in _counters().items():
        assert n > before[key], key
    _assert_same(got, ref)


def test_lru_budget_holds_the_raw_copy_but_not_the_result(gpu, monkeypatch):
    """A budget of 1.5 raw copies of the largest slide: its raw pixels are
    resident, its fp32 result (two raw copies) may not be held, so the filter
    stays deferred over the resident slide; the results do not change."""
    from milwrm_amd.stream import RESIDENCY

    slides = _slides(8)
    ref = _resident_ref(monkeypatch, 8, np.uint16, 1)
    raw = max(r.shape[0] * r.shape[1] * r.shape[2] * 2 for r, _ in slides)
    monkeypatch.setenv("MW_HBM_BUDGET", str(int(raw * 1.5)))
    monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
    imgs = _host_imgs(slides)
    got = _pipeline(imgs, 1, {"sigma_color": SC, "banded": True})
    assert got["deferred"][-1]  # the largest slide's result never fits
    assert RESIDENCY.used() <= raw * 1.5
    _assert_same(got, ref)


def _one(monkeypatch, streamed, C=8):
    """A fresh img over the same slide, resident or (budget cap) streamed."""
    import milwrm_amd as M

    raw, mask = _slides(C, n=1, seed=950)[0]
    if streamed:
        monkeypatch.setenv("MW_HBM_BUDGET", "1")
        monkeypatch.setenv("MW_STREAM_BAND_ROWS", "37")
    else:
        monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
        monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
    return M.img(raw.copy(), mask=mask.copy())


MEAN = np.array([61.5, 40.0, 77.25, 55.0, 52.5, 90.0, 33.0, 48.0])
PEND = (1.0, SC, None, "constant", 0.0)


def _bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, want):
    for a, b in zip(got, want):
        assert np.isfinite(b).all()
        assert np.array_equal(_bits64(a), _bits64(b))


def test_log_normalize_then_bilateral_stays_deferred(gpu, monkeypatch):
    from milwrm_amd import device as D

    feats = list(range(8))
    res = {}
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.log_normalize(mean=MEAN)
        im.blurring("bilateral", sigma=1, sigma_color=SC, banded=True)
        if streamed:  # the log_normalize stays pending: the kernel's fused load
            assert im._pending_bilateral == PEND and im._pending is not None and im._dev is None
            assert im._filter_deferred()
        else:  # banded=True only permits deferral: a slide that fits is filtered at once
            assert im._pending_bilateral is None and im._pending is None and im._dev is not None
        before = D.BILATERAL_USED["rows_streamed"]
        X = im.subsample_pixels(feats, 0.2)
        assert (D.BILATERAL_USED["rows_streamed"] > before) == streamed
        if streamed:
            assert im._dev is None and im._pending_bilateral == PEND  # the subsample held nothing
        res[streamed] = (X, im.img.copy())  # .img materialises
        assert im._pending_bilateral is None and im._dev is not None
    assert res[False][0].shape[0] > 1000
    _same(res[True], res[False])


def test_bilateral_then_log_normalize_materialises(gpu, monkeypatch):
    """The bilateral does not commute with the log: a log_normalize after a
    deferred bilateral applies the filter first, with a given mean and with
    the mean of the filtered pixels."""
    out = {}
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.bilateral_filter(1, 4000.0, banded=True)  # raw pixels
        assert (im._pending_bilateral is not None) == streamed
        im.log_normalize(mean=MEAN)
        assert im._pending_bilateral is None and im._pending is not None and im._dev is not None
        im2 = _one(monkeypatch, streamed)
        im2.bilateral_filter(1, 4000.0, banded=True)
        im2.log_normalize()  # mean=None
        assert im2._pending_bilateral is None and im2._pending is not None
        im3 = _one(monkeypatch, streamed)
        im3.log_normalize(mean=MEAN)
        im3.bilateral_filter(1, SC, banded=True)
        im3.log_normalize(mean=MEAN)  # a second log_normalize
        assert im3._pending_bilateral is None and im3._pending is not None
        out[streamed] = (im.img.copy(), im2.img.copy(), im3.img.copy())
    _same(out[True], out[False])


def test_second_filter_in_either_order_materialises(gpu, monkeypatch):
    out = {}
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.log_normalize(mean=MEAN)
        im.blurring("gaussian", sigma=2)
        assert (im._pending_blur is not None) == streamed
        im.bilateral_filter(1, SC, banded=True)  # a second filter: the deferred gaussian is applied first
        assert im._pending_blur is None and im._pending_bilateral is None and im._dev is not None
        a = im.img.copy()
        im = _one(monkeypatch, streamed)
        im.median_filter(3)
        assert (im._pending_median is not None) == streamed
        im.bilateral_filter(1, 4000.0, banded=True)
        assert im._pending_median is None and im._pending_bilateral is None
        b = im.img.copy()
        im = _one(monkeypatch, streamed)
        im.log_normalize(mean=MEAN)
        im.bilateral_filter(1, SC, banded=True)
        assert (im._pending_bilateral is not None) == streamed
        im.blurring("gaussian", sigma=2)  # the other order: the deferred bilateral is applied first
        assert im._pending_bilateral is None and im._pending_blur is None and im._dev is not None
        c = im.img.copy()
        im = _one(monkeypatch, streamed)
        im.log_normalize(mean=MEAN)
        im.bilateral_filter(1, SC, banded=True)
        im.median_filter(3)
        assert im._pending_bilateral is None and im._pending_median is None
        d = im.img.copy()
        im = _one(monkeypatch, streamed)
        im.log_normalize(mean=MEAN)
        im.bilateral_filter(1, SC, banded=True)
        im.scale()  # the intensity utilities take the filtered pixels
        assert im._pending_bilateral is None
        out[streamed] = (a, b, c, d, im.img.copy())
    _same(out[True], out[False])


def test_constant_slide_comes_back_unchanged_with_nothing_pending(gpu, monkeypatch):
    import milwrm_amd as M

    monkeypatch.setenv("MW_HBM_BUDGET", "1")
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "7")
    u = np.full((40, 33, 3), 777, dtype=np.uint16)
    for sc in (0.2, "std"):
        im = M.img(u.copy(), mask=np.ones(u.shape[:2]))
        im.bilateral_filter(1, sc, cval=0.4, banded=True)
        assert im._pending_bilateral is None and im._pending is None and not im._filter_deferred()
        assert np.array_equal(im.img, u.astype(np.float64))
        im = M.img(u.copy(), mask=np.ones(u.shape[:2]))
        im.log_normalize(mean=np.full(3, 300.0))  # one mean for every channel: the normalised slide is constant too
        im.bilateral_filter(1, sc, cval=0.4, banded=True)
        assert im._pending_bilateral is None and im._pending is not None  # the log_normalize stays pending
        want = M.img(u.copy(), mask=np.ones(u.shape[:2]))
        want.log_normalize(mean=np.full(3, 300.0))
        assert np.array_equal(_bits64(im.img), _bits64(want.img))


def test_evicted_copy_returns_to_the_deferred_state(gpu, monkeypatch):
    im = _one(monkeypatch, True)
    im.log_normalize(mean=MEAN)
    im.bilateral_filter(1, SC, banded=True)
    a = im.img.copy()
    assert im._dev is not None and im._pending_bilateral is None and im._pending is None
    im._evict()
    assert im._dev is None and im._pending_bilateral == PEND and im._pending is not None
    assert im._source() is not None
    assert np.array_equal(_bits64(im.img), _bits64(a))


def test_slide_that_cannot_be_held(gpu, monkeypatch):
    import milwrm_amd as M

    ref = _resident_ref(monkeypatch, 8, np.uint16, 1)

    def refuse(self, nbytes):
        raise MemoryError(f"this operation needs the whole raw slide in HBM ({nbytes} bytes): refused")

    monkeypatch.setattr(M.img, "_fits_whole", refuse)
    im = _one(monkeypatch, True)
    im.log_normalize(mean=MEAN)
    im.bilateral_filter(1, SC, banded=True)
    with pytest.raises(MemoryError, match="whole raw slide"):
        im.img
    assert im._pending_bilateral == PEND and im._dev is None  # still deferred
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "37")
    got = _pipeline(_host_imgs(_slides(8)), 1, {"sigma_color": SC, "banded": True})
    assert not any(got["resident"])
    _assert_same(got, ref)


def test_without_banded_a_streamed_slide_is_still_refused(gpu, monkeypatch):
    import milwrm_amd as M
    from milwrm_amd import stream

    monkeypatch.setenv("MW_HBM_BUDGET", "1")
    im = _one(monkeypatch, True)
    with pytest.raises(MemoryError, match="banded form"):
        im.blurring("bilateral", sigma=1, sigma_color=SC)
    with pytest.raises(MemoryError, match="banded=True"):
        im.bilateral_filter(1, SC, banded=False)
    assert im._pending_bilateral is None
    src = M.img.from_source(stream.SynthSource(64, 48, 4, 77))
    with pytest.raises(MemoryError, match="banded form"):
        src.blurring("bilateral", sigma=1, sigma_color=0.3)
    src.blurring("bilateral", sigma=1, sigma_color=0.3, banded=True)
    assert src._pending_bilateral == (1.0, 0.3, None, "constant", 0.0)
