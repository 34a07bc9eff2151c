"""img.equalize_hist(kernel_size=k, banded=True) on slides streamed in row
bands: the statistics are gathered band by band (stream.clahe
over mw_clahe_rows_*), the rounds stay deferred (``img._pending_clahe``) and
every band is equalised as a pass reads it (stream.ClaheSource), after deferred
clip / scale rounds and before a later log_normalize and filter.  Every
reduction is an integer one and the map is elementwise, so everything
downstream is BITWISE the resident run's.  "Streamed": MW_HBM_BUDGET=1 with
MW_STREAM_BAND_ROWS 29, 37 or 61."""
import numpy as np
import pandas as pd
import pytest

from tests.test_gpu_intensity_stream import (CHANNELS, MEAN, _bits64, _env, _filters, _host_imgs, _one, _raw,
                                             _refuse)
from tests.test_gpu_stream import _assert_same, _slides

pytestmark = pytest.mark.gpu

COUNTERS = ("stats_streamed", "map_streamed")
FEATS = list(range(8))


def _counters():
    from milwrm_amd import device as D

    return {k: D.CLAHE_USED[k] for k in COUNTERS}


def _rose(before, keys=COUNTERS):
    now = _counters()
    return all(now[k] > before[k] for k in keys)


@pytest.mark.parametrize("kind,band", [("u8", "29"), ("u16", "37"), ("f32", "61")])
@pytest.mark.parametrize("mode", list(CHANNELS))
@pytest.mark.parametrize("ks", [None, (20, 24), 16], ids=["default", "20x24", "16"])
def test_streamed_equals_resident(gpu, monkeypatch, ks, mode, kind, band):
    """Fails on the parent commit: banded= is an unknown option."""
    ref = _one(monkeypatch, False, kind)
    ref.equalize_hist(channels=CHANNELS[mode], kernel_size=ks, banded=True)  # resident: equalised at once
    assert ref._dev is not None and ref._pending_clahe is None
    im = _one(monkeypatch, True, kind, band)
    before = _counters()
    im.equalize_hist(channels=CHANNELS[mode], kernel_size=ks, banded=True)
    assert im._dev is None and im._pending_clahe is not None
    assert len(im._pending_clahe) == (2 if mode == "twice" else 1)
    assert im._elem_size() == 4 and im._raw_int_max() is None and im._range is None
    assert _rose(before, ("stats_streamed",))
    im.calculate_non_zero_mean()  # a band pass: every band is equalised as it is read
    assert _rose(before) and im._dev is None
    assert np.array_equal(_bits64(im.img), _bits64(ref.img))
    a = ref.img
    for c in range(8) if CHANNELS[mode] is None else set(ref._features(list(CHANNELS[mode]))):
        assert a[:, :, c].min() == 0.0 and a[:, :, c].max() == 1.0


def test_after_a_deferred_clip_both_stay_deferred(gpu, monkeypatch):
    res = []
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.clip(channels=(0, 1, 2, 3))
        im.equalize_hist(channels=(1, 2, 5), kernel_size=(48, 45), banded=True)  # tiles large enough to be staged
        assert (im._pending_rescale is not None and im._pending_clahe is not None and im._dev is None) == streamed
        res.append(im.img.copy())
    assert np.array_equal(_bits64(res[1]), _bits64(res[0]))


@pytest.mark.parametrize("then", ["lognorm", "gaussian", "median", "bilateral"])
def test_equalize_then(gpu, monkeypatch, then):
    """equalize_hist, then log_normalize(mean=MEAN), then each filter: all of
    it stays deferred on the streamed slide; the subsample's bits are the
    resident run's."""
    res = []
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.equalize_hist(kernel_size=(20, 24), banded=True)
        im.log_normalize(mean=MEAN)
        _filters(im, then)
        assert (im._pending_clahe is not None) == streamed
        X = im.subsample_pixels(FEATS, 0.2)
        if streamed and then != "lognorm":  # (with no filter the subsample materialises)
            assert im._dev is None and im._pending_clahe is not None  # the subsample held nothing
        res.append((X, im.img.copy()))
    (X0, A0), (X1, A1) = res
    assert X0.shape[0] > 1000 and np.isfinite(A0).all()
    assert np.array_equal(_bits64(X1), _bits64(X0))
    assert np.array_equal(_bits64(A1), _bits64(A0))


def _pipeline(imgs, est=None, k=5):
    """clip(), equalize_hist(banded=True), then the pipeline and QC of
    tests/test_gpu_stream.py::_pipeline.  ``est``: (mean estimators, pixels)
    to put into the frame instead of the images' own (sums over fp32 pixels
    depend on the bands)."""
    import milwrm_amd as M
    from milwrm_amd.MILWRM import estimate_mse_mxif, estimate_percentage_variance_mxif

    for im in imgs:
        im.clip()
        im.equalize_hist(kernel_size=(20, 24), banded=True)
    ests, pix = zip(*[im.calculate_non_zero_mean() for im in imgs])
    if est is not None:
        np.testing.assert_array_equal(pix, est[1])  # the counts are exact
        ests, pix = est
    df = pd.DataFrame({"Img": imgs, "batch_names": ["b1", "b1", "b2"][:len(imgs)],
                       "mean estimators": list(ests), "pixels": list(pix)})
    lab = M.mxif_labeler(df)
    lab.prep_cluster_data(features=FEATS, sigma=2, fract=0.2)
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
    out["pv"] = [estimate_percentage_variance_mxif(im, False, lab.scaler, lab.kmeans.cluster_centers_, FEATS, t)
                 for im, t in zip(imgs, lab.tissue_IDs)]
    mse = estimate_mse_mxif(imgs, False, list(lab.tissue_IDs), lab.scaler, lab.kmeans.cluster_centers_, FEATS, k)
    out["mse"] = np.array([mse[i] for i in range(k)])
    assert np.all(np.isfinite(out["pv"]))
    out["resident"] = [im._dev is not None for im in imgs]
    out["frame"] = (ests, pix)
    return out


def test_pipeline_streamed_equals_resident(gpu, monkeypatch):
    from milwrm_amd import device as D

    _env(monkeypatch, False)
    ref = _pipeline(_host_imgs(_slides(8)))
    assert all(ref["resident"])
    _env(monkeypatch, True, "37")
    before = _counters()
    streamed = {k: D.FUSED_USED[k] for k in ("sample_streamed", "assign_streamed")}
    got = _pipeline(_host_imgs(_slides(8)), est=ref["frame"])
    assert not any(got["resident"])
    assert _rose(before)
    for key, n in streamed.items():
        assert D.FUSED_USED[key] > n, key
    _assert_same(got, ref)


def test_downsample_and_tissue_mask(gpu, monkeypatch):
    from milwrm_amd import device as D

    res = []
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.equalize_hist(kernel_size=(20, 24), banded=True)
        before = D.FUSED_USED["downsample_streamed"]
        cp = im.copy()
        cp.downsample(2)
        assert (D.FUSED_USED["downsample_streamed"] > before) == streamed
        assert cp._pending_clahe is None and cp._dev is not None
        im.create_tissue_mask()
        assert (im._pending_clahe is not None) == streamed
        res.append((cp.img.copy(), np.asarray(cp.mask).copy(), np.asarray(im.mask).copy()))
    for a, b in zip(*res):
        assert np.array_equal(_bits64(np.asarray(a, dtype=np.float64)), _bits64(np.asarray(b, dtype=np.float64)))
    assert 0 < res[0][2].mean() < 1


def test_module_function_under_the_budget(gpu, monkeypatch):
    from milwrm_amd import MxIF

    raw, _ = _raw("u16")
    _env(monkeypatch, False)
    ref = (MxIF.CLAHE(raw, kernel_size=(20, 24)), MxIF.CLAHE(raw, channels=(0, 2), kernel_size=16, clip_limit=0.02),
           MxIF.CLAHE(raw[:, :, 1], kernel_size=(20, 24), nbins=100))
    _env(monkeypatch, True)
    before = _counters()
    got = (MxIF.CLAHE(raw, kernel_size=(20, 24), banded=True),
           MxIF.CLAHE(raw, channels=(0, 2), kernel_size=16, clip_limit=0.02, banded=True),
           MxIF.CLAHE(raw[:, :, 1], kernel_size=(20, 24), nbins=100, banded=True))
    assert _rose(before, ("stats_streamed",))
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_resident_raw_with_the_result_deferred(gpu, monkeypatch):
    """A budget that holds the raw slide but not its fp32 result: the raw copy
    stays resident and the equalisation deferred over it, its bands zero-copy
    views.  150 x 173 x 7 uint16: 2422 bytes per row, not a multiple of 16, so
    with 37-row bands the views start off the 16-byte grid."""
    import milwrm_amd as M

    raw, mask = _raw("u16")
    raw = np.ascontiguousarray(raw[:, :173, :7])
    mask = np.ascontiguousarray(mask[:, :173])
    assert (raw.shape[1] * raw.shape[2] * 2) % 16 and (37 * raw.shape[1] * raw.shape[2] * 2) % 16
    _env(monkeypatch, False)
    ref = M.img(raw.copy(), mask=mask.copy())
    ref.equalize_hist(channels=(0, 2), kernel_size=(20, 24))
    monkeypatch.setenv("MW_HBM_BUDGET", str(int(raw.nbytes * 1.5)))
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "37")
    im = M.img(raw.copy(), mask=mask.copy())
    before = _counters()
    im.equalize_hist(channels=(0, 2), kernel_size=(20, 24), banded=True)
    assert im._pending_clahe is not None and im._dev is not None and im._dev.dtype != ref._dev.dtype
    assert _counters() == before  # nothing was streamed: the raw slide is resident
    for x in (im, ref):
        x.log_normalize(mean=MEAN[:7])
        x.blurring("median", size=3)
    assert im._pending_median is not None and im._pending_clahe is not None
    feats = list(range(7))
    assert np.array_equal(_bits64(im.subsample_pixels(feats, 0.2)), _bits64(ref.subsample_pixels(feats, 0.2)))
    assert np.array_equal(_bits64(im.img), _bits64(ref.img))


def test_evicted_copy_returns_to_the_deferred_state(gpu, monkeypatch):
    im = _one(monkeypatch, True)
    im.clip()
    im.equalize_hist(kernel_size=(20, 24), banded=True)
    im.log_normalize(mean=MEAN)
    a = im.img.copy()
    assert im._dev is not None and im._pending_clahe is None and im._pending_rescale is None and im._pending is None
    im._evict()
    assert (im._dev is None and im._pending_clahe is not None and im._pending_rescale is not None
            and im._pending is not None)
    assert im._source() is not None
    assert np.array_equal(_bits64(im.img), _bits64(a))


def test_unchanged_behaviour_and_refusals(gpu, monkeypatch, golden):
    import milwrm_amd as M
    from milwrm_amd import bands

    # without banded=True a streamed slide still materialises
    ref = _one(monkeypatch, False)
    ref.equalize_hist(kernel_size=16)
    im = _one(monkeypatch, True)
    im.equalize_hist(kernel_size=16)
    assert im._pending_clahe is None and im._dev is not None
    assert np.array_equal(_bits64(im.img), _bits64(ref.img))
    # clip after a deferred equalisation materialises it
    ref.clip()
    im = _one(monkeypatch, True)
    im.equalize_hist(kernel_size=16, banded=True)
    assert im._pending_clahe is not None and im._dev is None
    im.clip()
    assert im._pending_clahe is None and im._pending_rescale is None and im._dev is not None
    assert np.array_equal(_bits64(im.img), _bits64(ref.img))
    # a row band of a split slide
    g = golden("intensity")
    band = bands.band_image(g["raw"], g["mask"], 0, 2)
    with pytest.raises(NotImplementedError, match="band"):
        band.equalize_hist(kernel_size=4, banded=True)
    with pytest.raises(NotImplementedError, match="options"):
        im.equalize_hist(kernel_size=16, banded=True, tile=3)
    # a log_normalize already pending: materialised first, and that does not fit
    monkeypatch.setattr(M.img, "_fits_whole", _refuse)
    im = _one(monkeypatch, True)
    im.log_normalize(mean=np.full(8, 50.0))
    with pytest.raises(MemoryError, match="whole raw slide"):
        im.equalize_hist(kernel_size=16, banded=True)
    assert im._pending is not None and im._pending_clahe is None
    # a deferred equalisation that cannot be materialised stays deferred
    im = _one(monkeypatch, True)
    im.equalize_hist(kernel_size=16, banded=True)
    with pytest.raises(MemoryError, match="whole raw slide"):
        im.clip()
    assert im._pending_clahe is not None and im._dev is None


def test_tables_that_do_not_fit_name_the_kernel_size(gpu, monkeypatch):
    from milwrm_amd import stream

    im = _one(monkeypatch, True)
    monkeypatch.setattr(stream, "alloc_bytes", lambda dev=None: 1 << 20)
    with pytest.raises(MemoryError, match="larger kernel_size"):
        im.equalize_hist(kernel_size=4, banded=True)
    assert im._pending_clahe is None
