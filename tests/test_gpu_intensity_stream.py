"""img.clip / img.scale on slides streamed in row bands: the selection reads
the slide band by band (stream.quantiles over mw_quantiles_rows_*), the rescale
stays deferred (``img._pending_rescale``) and is applied to every band as a
pass reads it (stream.RescaleSource), before a later log_normalize and filter.
The selection is exact and the rescale elementwise, so everything downstream is
BITWISE the resident run's (the keys of tests/test_gpu_stream.py::_assert_same,
the QC estimators included).  "Streamed": MW_HBM_BUDGET=1 with
MW_STREAM_BAND_ROWS 29, 37 or 61."""
import numpy as np
import pandas as pd
import pytest

from tests.test_gpu_stream import _assert_same, _slides

pytestmark = pytest.mark.gpu

MEAN = np.array([0.21, 0.4, 0.17, 0.55, 0.25, 0.9, 0.33, 0.48])
COUNTERS = ("select_streamed", "rescale_streamed")


def _bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _env(monkeypatch, streamed, band="37"):
    if streamed:
        monkeypatch.setenv("MW_HBM_BUDGET", "1")  # nothing may stay resident: every pass streams
        monkeypatch.setenv("MW_STREAM_BAND_ROWS", band)
    else:
        monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
        monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)


def _raw(kind, C=8, seed=950):
    """One slide as uint8 / uint16 / float32 ("f32": negatives and the -99999
    sentinel; "f32nan": NaN pixels as well)."""
    raw, mask = _slides(C, n=1, seed=seed, dtype=np.uint8 if kind == "u8" else np.uint16)[0]
    if kind.startswith("f32"):
        rng = np.random.default_rng(5)
        raw = (raw.astype(np.float32) - 40.0) * np.float32(0.37)
        raw[3, 5, 0] = raw[11, 7, 2] = -99999.0
        if kind == "f32nan":
            raw[rng.uniform(size=raw.shape) < 0.02] = np.nan
    return raw, mask


def _one(monkeypatch, streamed, kind="u16", band="37"):
    import milwrm_amd as M

    _env(monkeypatch, streamed, band)
    raw, mask = _raw(kind)
    return M.img(raw.copy(), mask=mask.copy())


def _counters():
    from milwrm_amd import device as D

    return {k: D.INTENSITY_USED[k] for k in COUNTERS}


def _rose(before, keys=COUNTERS):
    now = _counters()
    return all(now[k] > before[k] for k in keys)


CHANNELS = {"all": None, "tuple": (0, 2), "names": ("ch_1", "ch_3"), "twice": (1, 1)}
_REF = {}


@pytest.mark.parametrize("kind,band", [("u8", "29"), ("u16", "37"), ("f32", "61"), ("f32nan", "37")])
@pytest.mark.parametrize("mode", list(CHANNELS))
@pytest.mark.parametrize("op", ["clip", "scale"])
def test_streamed_equals_resident(gpu, monkeypatch, op, mode, kind, band):
    """Fails on the parent commit: the slide was simply uploaded whole."""
    ref = _one(monkeypatch, False, kind)
    getattr(ref, op)(channels=CHANNELS[mode])
    assert ref._dev is not None and ref._pending_rescale is None
    im = _one(monkeypatch, True, kind, band)
    before = _counters()
    getattr(im, op)(channels=CHANNELS[mode])
    assert im._dev is None and im._pending_rescale is not None
    assert im._elem_size() == 4 and im._raw_int_max() is None
    assert _rose(before, ("select_streamed",))
    im.calculate_non_zero_mean()  # a band pass: every band is rescaled as it is read
    assert _rose(before) and im._dev is None
    assert np.array_equal(_bits64(im.img), _bits64(ref.img))
    if op == "clip" and kind != "f32nan":
        assert np.isfinite(ref.img).all()


def test_resident_raw_with_the_result_deferred(gpu, monkeypatch):
    """A budget that holds the raw slide but not its fp32 result: the raw copy
    stays resident and the clip deferred over it."""
    import milwrm_amd as M

    raw, mask = _raw("u16")
    _env(monkeypatch, False)
    ref = M.img(raw.copy(), mask=mask.copy())
    ref.clip(channels=(0, 2))
    monkeypatch.setenv("MW_HBM_BUDGET", str(int(raw.nbytes * 1.5)))
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "37")
    im = M.img(raw.copy(), mask=mask.copy())
    im.clip(channels=(0, 2))
    assert im._pending_rescale is not None and im._dev is not None and im._dev.dtype != ref._dev.dtype
    X = im.subsample_pixels(list(range(8)), 0.2)
    assert np.array_equal(_bits64(X), _bits64(ref.subsample_pixels(list(range(8)), 0.2)))
    assert np.array_equal(_bits64(im.img), _bits64(ref.img))


def _filters(im, name):
    if name == "gaussian":
        im.blurring("gaussian", sigma=2)
    elif name == "median":
        im.blurring("median", size=3)
    elif name == "bilateral":
        im.blurring("bilateral", sigma=1.0, sigma_color=0.2, banded=True)


@pytest.mark.parametrize("then", ["scale", "lognorm", "gaussian", "median", "bilateral"])
def test_clip_then(gpu, monkeypatch, then):
    """clip then scale; clip then log_normalize(mean=MEAN) then each filter."""
    feats = list(range(8))
    res = []
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.clip(channels=(0, 1, 2, 3))
        if then == "scale":
            im.scale()
            assert (im._pending_rescale is not None and len(im._pending_rescale[0]) == 2) == streamed
        else:
            im.log_normalize(mean=MEAN)
            assert (im._pending_rescale is not None) == streamed  # log_normalize(mean=...) holds nothing
            _filters(im, then)
            assert (im._pending_rescale is not None) == streamed
        X = im.subsample_pixels(feats, 0.2)
        if streamed and then not in ("scale", "lognorm"):  # (with no filter the subsample materialises)
            assert im._dev is None and im._pending_rescale is not None  # the subsample held nothing
        res.append((X, im.img.copy()))
    (X0, A0), (X1, A1) = res
    assert X0.shape[0] > 1000 and np.isfinite(A0).all()
    assert np.array_equal(_bits64(X1), _bits64(X0))
    assert np.array_equal(_bits64(A1), _bits64(A0))


def test_evicted_copy_returns_to_the_deferred_state(gpu, monkeypatch):
    im = _one(monkeypatch, True)
    im.clip()
    im.log_normalize(mean=MEAN)
    a = im.img.copy()
    assert im._dev is not None and im._pending_rescale is None and im._pending is None
    im._evict()
    assert im._dev is None and im._pending_rescale is not None and im._pending is not None
    assert im._source() is not None
    assert np.array_equal(_bits64(im.img), _bits64(a))


def _refuse(self, nbytes):
    raise MemoryError(f"this operation needs the whole raw slide in HBM ({nbytes} bytes): refused")


def test_slide_that_cannot_be_held(gpu, monkeypatch):
    """Fails on the parent commit: clip itself raised."""
    import milwrm_amd as M

    ref = _one(monkeypatch, False)
    ref.clip()
    monkeypatch.setattr(M.img, "_fits_whole", _refuse)
    im = _one(monkeypatch, True)
    im.clip()
    assert im._pending_rescale is not None and im._dev is None
    with pytest.raises(MemoryError, match="whole raw slide"):
        im.img
    assert im._pending_rescale is not None and im._dev is None  # still deferred
    for x in (im, ref):
        x.log_normalize(mean=MEAN)
        x.blurring("gaussian", sigma=2)
    assert im._pending_rescale is not None and im._pending_blur is not None and im._dev is None
    X0 = ref.subsample_pixels(list(range(8)), 0.2)
    assert np.array_equal(_bits64(im.subsample_pixels(list(range(8)), 0.2)), _bits64(X0))


# ------------------------------------------------------------ the pipeline
def _pipeline(imgs, filt, est=None, k=5):
    """clip(), then tests/test_gpu_stream.py::_pipeline with ``filt`` and QC.
    ``est``: (mean estimators, pixels) to put into the frame instead of the
    images' own (sums over fp32 pixels depend on the bands)."""
    import milwrm_amd as M
    from milwrm_amd.MILWRM import estimate_mse_mxif, estimate_percentage_variance_mxif

    C = imgs[0].n_ch
    feats = list(range(C))
    for im in imgs:
        im.clip()
    ests, pix = zip(*[im.calculate_non_zero_mean() for im in imgs]) if est is None else est
    df = pd.DataFrame({"Img": imgs, "batch_names": ["b1", "b1", "b2"][:len(imgs)],
                       "mean estimators": list(ests), "pixels": list(pix)})
    lab = M.mxif_labeler(df)
    if filt == "median":
        lab.prep_cluster_data(features=feats, filter_name="median", filter_kwargs={"size": 3}, fract=0.2)
    else:
        lab.prep_cluster_data(features=feats, sigma=2, fract=0.2)
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
    out["frame"] = (ests, pix)
    return out


def _host_imgs(slides):
    import milwrm_amd as M

    return [M.img(r.copy(), mask=m.copy()) for r, m in slides]


def _resident_ref(monkeypatch, filt):
    if filt not in _REF:
        _env(monkeypatch, False)
        _REF[filt] = _pipeline(_host_imgs(_slides(8)), filt)
        assert all(_REF[filt]["resident"])
    return _REF[filt]


@pytest.mark.parametrize("filt,band", [("gaussian", "37"), ("median", "29")])
def test_pipeline_streamed_equals_resident(gpu, monkeypatch, filt, band):
    from milwrm_amd import device as D

    ref = _resident_ref(monkeypatch, filt)
    _env(monkeypatch, True, band)
    before = _counters()
    streamed = {k: D.FUSED_USED[k] for k in ("sample_streamed", "assign_streamed")}
    got = _pipeline(_host_imgs(_slides(8)), filt, est=ref["frame"])
    assert not any(got["resident"])
    assert _rose(before)
    for key, n in streamed.items():
        assert D.FUSED_USED[key] > n, key
    _assert_same(got, ref)


def test_pipeline_device_generator(gpu, monkeypatch):
    """Slides read band by band from the device generator (img.from_source)
    against host copies of the same generated slides, resident."""
    import milwrm_amd as M
    from milwrm_amd import device as D
    from milwrm_amd import stream

    shapes = [(150 + 17 * i, 176 + 32 * i) for i in range(3)]
    _env(monkeypatch, False)
    host = []
    for i, (H, W) in enumerate(shapes):
        raw, mask = D.synth_slide(H, W, 8, seed=930 + i)
        host.append((raw.cpu().numpy().view(np.uint16), mask.cpu().numpy()))
    ref = _pipeline(_host_imgs(host), "gaussian")
    assert all(ref["resident"])
    _env(monkeypatch, True, "61")
    before = _counters()
    imgs = [M.img.from_source(stream.SynthSource(H, W, 8, 930 + i)) for i, (H, W) in enumerate(shapes)]
    got = _pipeline(imgs, "gaussian", est=ref["frame"])
    assert not any(got["resident"])
    assert _rose(before)
    _assert_same(got, ref)


def test_non_zero_mean_after_clip(gpu, monkeypatch):
    """Counts exact; the fp64 sums of the fp32 pixels (all in [0, 1]) depend on
    the bands: two sums of N non-negative terms are within 2 (N - 1) 2^-53
    relative of each other."""
    from milwrm_amd import device as D

    out = []
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.clip()
        s, c = D.d2h(*im._nz_stats())
        est, pix = im.calculate_non_zero_mean()
        out.append((s, c, np.asarray(est), pix))
        assert (im._dev is None) == streamed
    (s0, c0, e0, p0), (s1, c1, e1, p1) = out
    N = im.shape[0] * im.shape[1]
    assert np.array_equal(c0, c1) and p0 == p1 and p0 > 0
    bound = 2 * (N - 1) * 2.0 ** -53
    rel = np.abs(s1 - s0) / s0
    print("non-zero sums, streamed against resident: max relative difference", rel.max(), "bound", bound)
    assert (rel <= bound).all()
    # the estimators: the sums' bound and, in each run, a division and a multiplication (2^-53 each)
    assert (np.abs(e1 - e0) / e0 <= bound + 4 * 2.0 ** -53).all()


def test_downsample_and_tissue_mask_after_clip(gpu, monkeypatch):
    from milwrm_amd import device as D

    res = []
    for streamed in (False, True):
        im = _one(monkeypatch, streamed)
        im.clip()
        before = D.FUSED_USED["downsample_streamed"]
        cp = im.copy()
        cp.downsample(2)
        assert (D.FUSED_USED["downsample_streamed"] > before) == streamed
        assert cp._pending_rescale is None and cp._dev is not None
        im.create_tissue_mask()
        assert (im._pending_rescale is not None) == streamed
        res.append((cp.img.copy(), np.asarray(cp.mask).copy(), np.asarray(im.mask).copy()))
    for a, b in zip(*res):
        assert np.array_equal(_bits64(np.asarray(a, dtype=np.float64)), _bits64(np.asarray(b, dtype=np.float64)))
    assert 0 < res[0][2].mean() < 1


def test_refused_states(gpu, monkeypatch, golden):
    import milwrm_amd as M
    from milwrm_amd import bands

    # equalize_hist of a deferred clip materialises it
    ref = _one(monkeypatch, False)
    ref.clip()
    ref.equalize_hist(kernel_size=16)
    im = _one(monkeypatch, True)
    im.clip()
    im.equalize_hist(kernel_size=16)
    assert im._pending_rescale is None and im._dev is not None
    assert np.array_equal(_bits64(im.img), _bits64(ref.img))
    g = golden("intensity")
    band = bands.band_image(g["raw"], g["mask"], 0, 2)
    for op in ("clip", "scale"):
        with pytest.raises(NotImplementedError):
            getattr(band, op)()
    monkeypatch.setattr(M.img, "_fits_whole", _refuse)
    im = _one(monkeypatch, True)
    im.median_filter(3)
    assert im._pending_median is not None
    with pytest.raises(MemoryError, match="whole raw slide"):
        im.clip()  # a pending filter: clip materialises, and that does not fit
    assert im._pending_median is not None and im._pending_rescale is None
    im = _one(monkeypatch, True)
    im.log_normalize(mean=np.full(8, 50.0))
    with pytest.raises(MemoryError, match="whole raw slide"):
        im.scale()
    im = _one(monkeypatch, True)
    im.clip()
    with pytest.raises(MemoryError, match="whole raw slide"):
        im.equalize_hist(kernel_size=16)
    assert im._pending_rescale is not None and im._dev is None


def test_module_functions_under_the_budget(gpu, monkeypatch):
    from milwrm_amd import MxIF

    raw, _ = _raw("u16")
    _env(monkeypatch, False)
    ref = (MxIF.clip_values(raw), MxIF.clip_values(raw, channels=(0, 2)), MxIF.scale_rgb(raw, channels=(1,)),
           MxIF.clip_values(raw[:, :, 1], channels=(0,)), MxIF.scale_rgb(raw))
    _env(monkeypatch, True)
    before = _counters()
    got = (MxIF.clip_values(raw), MxIF.clip_values(raw, channels=(0, 2)), MxIF.scale_rgb(raw, channels=(1,)),
           MxIF.clip_values(raw[:, :, 1], channels=(0,)), MxIF.scale_rgb(raw))
    assert _rose(before, ("select_streamed",))
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
