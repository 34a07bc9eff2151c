"""The median filter on slides that are streamed in row bands: a deferred
median (``img._pending_median``) is applied band by band inside the subsample,
the label pass and the QC sums (stream.MedianBand over mw_median_rows), and the
median is an exact selection, so every result of the streamed pipeline is
BITWISE the resident one (the keys of tests/test_gpu_stream.py::_assert_same,
the QC estimators included).  Composition with log_normalize and a second
filter, eviction back to the deferred state, and a slide that cannot be held
whole."""
import numpy as np
import pandas as pd
import pytest

from tests.test_gpu_stream import _assert_same, _slides

pytestmark = pytest.mark.gpu


def _host_imgs(slides):
    import milwrm_amd as M

    return [M.img(r.copy(), mask=m.copy()) for r, m in slides]


def _pipeline(imgs, size, k=5):
    """tests/test_gpu_stream.py::_pipeline with the median filter and QC on."""
    import milwrm_amd as M
    from milwrm_amd.MILWRM import estimate_mse_mxif, estimate_percentage_variance_mxif

    C = imgs[0].n_ch
    feats = list(range(C))
    ests, pix = zip(*[im.calculate_non_zero_mean() for im in imgs])
    df = pd.DataFrame({"Img": imgs, "batch_names": ["b1", "b1", "b2"][:len(imgs)],
                       "mean estimators": list(ests), "pixels": list(pix)})
    lab = M.mxif_labeler(df)
    lab.prep_cluster_data(features=feats, filter_name="median", filter_kwargs={"size": size}, fract=0.2)
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
    return out


_REF = {}


def _resident_ref(monkeypatch, C, dtype, size):
    """The resident run (no budget cap), computed once per case."""
    key = (C, np.dtype(dtype).name, size)
    if key not in _REF:
        monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
        monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
        _REF[key] = _pipeline(_host_imgs(_slides(C, dtype=dtype)), size)
        assert all(_REF[key]["resident"])
    return _REF[key]


COUNTERS = (("MEDIAN_USED", "rows_streamed"), ("FUSED_USED", "sample_streamed"), ("FUSED_USED", "assign_streamed"))


def _counters():
    from milwrm_amd import device as D

    return {(d, k): getattr(D, d)[k] for d, k in COUNTERS}


@pytest.mark.parametrize("C,dtype,band,size", [(8, np.uint16, "37", 3), (7, np.uint16, "29", (4, 7)),
                                               (50, np.uint16, "61", 5), (8, np.uint8, "200", 9)])
def test_streamed_equals_resident(gpu, monkeypatch, C, dtype, band, size):
    ref = _resident_ref(monkeypatch, C, dtype, size)
    monkeypatch.setenv("MW_HBM_BUDGET", "1")  # nothing may stay resident: every pass streams
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", band)
    before = _counters()
    got = _pipeline(_host_imgs(_slides(C, dtype=dtype)), size)
    assert not any(got["resident"])
    for key, n in _counters().items():
        assert n > before[key], key
    _assert_same(got, ref)


def test_device_generator_streamed_equals_resident(gpu, monkeypatch):
    """Slides read band by band from the device generator (img.from_source)
    against host copies of the same generated slides, resident (the device
    generator's slides: the oracle's synth_slide draws its noise from numpy's
    generator and is another slide, so it cannot be the bitwise reference)."""
    import milwrm_amd as M
    from milwrm_amd import device as D
    from milwrm_amd import stream

    shapes = [(150 + 17 * i, 176 + 32 * i) for i in range(3)]
    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
    host = []
    for i, (H, W) in enumerate(shapes):
        raw, mask = D.synth_slide(H, W, 8, seed=930 + i)
        host.append((raw.cpu().numpy().view(np.uint16), mask.cpu().numpy()))
    ref = _pipeline(_host_imgs(host), 3)
    assert all(ref["resident"])
    monkeypatch.setenv("MW_HBM_BUDGET", "1")
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "45")
    before = _counters()
    imgs = [M.img.from_source(stream.SynthSource(H, W, 8, 930 + i)) for i, (H, W) in enumerate(shapes)]
    got = _pipeline(imgs, 3)
    assert not any(got["resident"])
    for key, n in _counters().items():
        assert n > before[key], key
    _assert_same(got, ref)


def test_lru_budget(gpu, monkeypatch):
    """A budget of about 1.2 filtered slides: copies are evicted or the median
    stays deferred; the results do not change."""
    from milwrm_amd.stream import RESIDENCY

    slides = _slides(8)
    ref = _resident_ref(monkeypatch, 8, np.uint16, 3)
    one = max(r.shape[0] * r.shape[1] * r.shape[2] * 4 for r, _ in slides)  # an fp32 filtered copy
    monkeypatch.setenv("MW_HBM_BUDGET", str(int(one * 1.2)))
    ev = RESIDENCY.evictions
    got = _pipeline(_host_imgs(slides), 3)
    assert RESIDENCY.evictions > ev
    assert RESIDENCY.used() <= one * 1.2
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


def _bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_median_and_log_normalize_in_both_orders(gpu, monkeypatch):
    from milwrm_amd import device as D

    feats = list(range(8))
    res = {}
    for streamed in (False, True):
        for order in ("median_first", "lognorm_first"):
            im = _one(monkeypatch, streamed)
            if order == "median_first":
                im.median_filter(5)
                im.log_normalize(mean=MEAN)
            else:
                im.log_normalize(mean=MEAN)
                im.blurring("median", size=5)
            if streamed:  # both orders end in the same deferred state
                assert im._pending_median == (5, 5) and im._pending is not None and im._dev is None
            else:
                assert im._pending_median is None and im._dev is not None
            before = D.MEDIAN_USED["rows_streamed"]
            X = im.subsample_pixels(feats, 0.2)
            assert (D.MEDIAN_USED["rows_streamed"] > before) == streamed
            if streamed:
                assert im._dev is None and im._pending_median == (5, 5)  # the subsample held nothing
            res[streamed, order] = (X, im.img.copy())
    X0, A0 = res[False, "median_first"]
    assert X0.shape[0] > 1000 and np.isfinite(A0).all()
    for key, (X, A) in res.items():
        assert np.array_equal(_bits64(X), _bits64(X0)), key
        assert np.array_equal(_bits64(A), _bits64(A0)), key


def test_second_filter_and_mean_none_materialise(gpu, monkeypatch):
    out = {}
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.log_normalize(mean=MEAN)
        im.median_filter(5)
        assert (im._pending_median is not None) == streamed
        im.blurring("gaussian", sigma=2)  # a second filter: the deferred median is applied first
        assert im._pending_median is None and im._pending_blur is None and im._dev is not None
        g = im.img.copy()
        im = _one(monkeypatch, streamed)
        im.blurring("gaussian", sigma=2)
        assert (im._pending_blur is not None) == streamed
        im.median_filter(3)  # the other order: the deferred gaussian is applied first
        assert im._pending_median is None and im._pending_blur is None
        m = im.img.copy()
        im = _one(monkeypatch, streamed)
        im.median_filter(5)
        assert (im._pending_median is not None) == streamed
        im.log_normalize()  # mean=None: the mean of the filtered pixels
        assert im._pending_median is None and im._pending is not None
        im2 = _one(monkeypatch, streamed)
        im2.log_normalize(mean=MEAN)
        im2.median_filter(5)
        im2.log_normalize(mean=MEAN)  # a second log_normalize
        assert im2._pending_median is None
        out[streamed] = (g, m, im.img.copy(), im2.img.copy())
    for a, b in zip(out[True], out[False]):
        assert np.isfinite(b).all()
        assert np.array_equal(_bits64(a), _bits64(b))


def test_evicted_copy_returns_to_the_deferred_state(gpu, monkeypatch):
    im = _one(monkeypatch, True)
    im.log_normalize(mean=MEAN)
    im.median_filter(5)
    a = im.img.copy()
    assert im._dev is not None and im._pending_median is None and im._pending is None
    im._evict()
    assert im._dev is None and im._pending_median == (5, 5) and im._pending is not None
    assert im._source() is not None
    assert np.array_equal(_bits64(im.img), _bits64(a))


def test_slide_that_cannot_be_held(gpu, monkeypatch):
    import milwrm_amd as M

    ref = _resident_ref(monkeypatch, 8, np.uint16, 3)

    def refuse(self, nbytes):
        raise MemoryError(f"this operation needs the whole raw slide in HBM ({nbytes} bytes): refused")

    monkeypatch.setattr(M.img, "_fits_whole", refuse)
    im = _one(monkeypatch, True)
    im.log_normalize(mean=MEAN)
    im.median_filter(3)
    with pytest.raises(MemoryError, match="whole raw slide"):
        im.img
    assert im._pending_median == (3, 3) and im._dev is None  # still deferred
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "37")
    got = _pipeline(_host_imgs(_slides(8)), 3)
    assert not any(got["resident"])
    _assert_same(got, ref)
