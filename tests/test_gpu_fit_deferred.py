"""The deferred k-means fit (``mw_kmeans_fit_deferred`` +
``mw_kmeans_fit_finish``, csrc/fit.cpp; ``KMeans._fit_c(defer=True)`` /
``KMeans._finish``) against the eager fit (``mw_kmeans_fit_async_moments``,
``_fit_c(defer=False)``): bit for bit the same centers, iterations and
k-means++ indices straight after ``fit`` with no final pass run, and the same
labels and inertia once they are asked for, with the final pass run once.

Every comparison is an equality: the final pass is one E-step against fixed
centers and an exact fixed-point sum, so running it later over the same rows
gives the same bits.

Rows as in tests/test_gpu_kpp_moments.py (``_data``: overlapping clusters);
the strictly converging cases take the same recipe with one well-separated
blob per cluster.  The tolerance-stop input whose label buffer must differ
from the final labels before the finish (``STALE``) was chosen on the CPU with
oracle.milwrm_oracle's restated fit (kmeans_plusplus + lloyd_iter on the scaled
rows, seed 18): S = 70 001, F = 7, k = 2 stops on the tolerance after 40
iterations with 88 rows that the extra E-step still moves; the other
S = 70 001 tolerance stops leave 63 (F = 7, k = 8), 2 (F = 30, k = 2) and 56
(F = 30, k = 8) such rows, and every smaller S converges strictly before the
tolerance is met.  The separated rows converge strictly in 2 iterations."""
import numpy as np
import pytest

from tests.test_gpu_kpp_moments import _data, _labeler

pytestmark = pytest.mark.gpu

SEED = 18
SIZES = [63, 65, 257, 70_001]
FEATS = [7, 30]
KS = [2, 8]
# ending -> (rows, KMeans arguments)
ENDINGS = {"tol": ("overlap", {}), "strict": ("separated", {"tol": 0}),
           "max_iter1": ("overlap", {"max_iter": 1}), "max_iter2": ("overlap", {"max_iter": 2})}
STALE = (70_001, 7, 2)

_HOST, _EAGER = {}, {}


def _rows_host(kind, S, F, k):
    """(X fp32, mu, inv, per-feature variance of the scaled rows)."""
    key = (kind, S, F, k if kind == "separated" else 0)
    if key not in _HOST:
        if kind == "overlap":
            X, mu, inv, _, _ = _data(S, F)
        else:  # _data's recipe with k blobs twelve spreads apart
            rng = np.random.default_rng(2000 * F + 10 * (S % 997) + k)
            cen = 12.0 * rng.normal(size=(k, F))
            X = cen[rng.integers(0, k, size=S)] + rng.normal(size=(S, F))
            X = (X * rng.uniform(0.5, 20.0, size=F) + rng.uniform(-5.0, 50.0, size=F)).astype(np.float32)
            X[:, 2] = np.float32(3.5)
            X64 = X.astype(np.float64)
            mu, sd = X64.mean(axis=0), X64.std(axis=0)
            sd[sd == 0] = 1.0
            inv = 1.0 / sd
        var = X.astype(np.float64).var(axis=0) * inv * inv
        _HOST[key] = (X, mu, inv, var)
    return _HOST[key]


def _device_rows(kind, S, F, k, gpu):
    import torch

    from milwrm_amd.kmeans import DeviceRows

    X, mu, inv, var = _rows_host(kind, S, F, k)
    return DeviceRows(torch.from_numpy(X).to(gpu), mu, inv, feature_var=var)


def _fit(rows, k, kw, defer):
    from milwrm_amd import kmeans as KM

    km = KM.KMeans(n_clusters=k, random_state=SEED, **kw)
    km._check(rows.S, rows.F)
    return km._set_fitted(rows, *km._fit_c(rows, k, None, defer=defer))


def _eager(ending, S, F, k, gpu):
    """The eager arm's outputs, computed once per case and left unchanged."""
    key = (ending, S, F, k)
    if key not in _EAGER:
        kind, kw = ENDINGS[ending]
        km = _fit(_device_rows(kind, S, F, k, gpu), k, kw, defer=False)
        assert km._pending is None
        _EAGER[key] = dict(centers=km.cluster_centers_.copy(), n_iter=km.n_iter_, idx=km.init_indices_.copy(),
                           labels=km._labels_dev.clone(), inertia=km.inertia_)
    return _EAGER[key]


def _same_fit(km, ref):
    assert km.cluster_centers_.tobytes() == ref["centers"].tobytes()
    assert km.n_iter_ == ref["n_iter"]
    np.testing.assert_array_equal(km.init_indices_, ref["idx"])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("F", FEATS)
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("ending", list(ENDINGS))
def test_deferred_equals_eager(gpu, ending, S, F, k):
    import torch

    from milwrm_amd import kmeans as KM

    ref = _eager(ending, S, F, k, gpu)
    kind, kw = ENDINGS[ending]
    used = KM.FIT_FINISH_USED["finish"]
    km = _fit(_device_rows(kind, S, F, k, gpu), k, kw, defer=True)
    # straight after the fit: the same fit, and no final pass has run
    _same_fit(km, ref)
    assert KM.FIT_FINISH_USED["finish"] == used and km._pending is not None
    strict = km._pending.strict
    before = km._labels_buf.clone()  # the last iteration's labels (the test's own look at the buffer)
    assert KM.FIT_FINISH_USED["finish"] == used
    if ending == "strict":
        assert strict and km.n_iter_ < 300
    if S == 70_001 and ending == "tol":
        assert not strict and km.n_iter_ < 300
    if ending.startswith("max_iter"):
        assert km.n_iter_ == kw["max_iter"]
        if S == 70_001:
            assert not strict
    # asked for: the final pass runs, once
    assert torch.equal(km._labels_dev, ref["labels"])
    assert km.inertia_ == ref["inertia"]
    assert KM.FIT_FINISH_USED["finish"] == used + 1 and km._pending is None
    km.finalize()
    _ = km.labels_, km.inertia_, km._labels_dev
    assert KM.FIT_FINISH_USED["finish"] == used + 1
    stale = int((before != ref["labels"]).sum())
    print(f"{ending} S={S} F={F} k={k}: n_iter {km.n_iter_} strict {strict} stale rows {stale}")
    if strict:
        assert stale == 0  # mode 2 leaves the labels as they are
    if ending == "tol" and (S, F, k) == STALE:
        # without the extra E-step these rows would keep the last iteration's labels
        assert stale >= 1


def test_rows_with_their_maxima_and_moments(gpu):
    """Rows as prep_cluster_data leaves them: column maxima known (no pass for
    them in either arm) and moment records for k-means++."""
    import torch

    from milwrm_amd import device as D
    from milwrm_amd import kmeans as KM

    S, F, k = 70_001, 30, 8
    X, mu, inv, var = _rows_host("overlap", S, F, k)

    def rows():
        Xd = torch.from_numpy(X).to(gpu)
        r = KM.DeviceRows(Xd, mu, inv, feature_var=var, xmax_local=np.abs(X).max(axis=0))
        st = torch.zeros(1 + 2 * F, dtype=torch.float64, device=gpu)
        r.moments = [(0, S) + D.col_stats_rows(Xd, st, accumulate=False, keep_records=True)]
        return r

    ref = _eager("tol", S, F, k, gpu)
    init = dict(KM.KPP_INIT_USED)
    km = KM.KMeans(n_clusters=k, random_state=SEED).fit(rows())
    assert KM.KPP_INIT_USED["moments"] == init["moments"] + 1
    _same_fit(km, ref)
    assert km._pending is not None
    assert km.inertia_ == ref["inertia"] and torch.equal(km._labels_dev, ref["labels"])


@pytest.mark.parametrize("drop_rows", [False, True])
def test_finish_after_the_workspace_was_reused(gpu, drop_rows):
    """Fit A deferred, then fit B over other, more rows (the fit workspace is
    one shared buffer that B grows and overwrites), then A's outputs."""
    import torch

    from milwrm_amd import kmeans as KM

    a = ("tol", 257, 7, 8)
    ref = _eager(*a, gpu)
    used = KM.FIT_FINISH_USED["finish"]
    rows_a = _device_rows("overlap", 257, 7, 8, gpu)
    km_a = KM.KMeans(n_clusters=8, random_state=SEED).fit(rows_a)
    if drop_rows:
        del rows_a  # the model keeps the rows alive
    km_b = KM.KMeans(n_clusters=8, random_state=SEED).fit(_device_rows("overlap", 70_001, 30, 8, gpu))
    torch.cuda.synchronize()
    assert KM.FIT_FINISH_USED["finish"] == used
    assert km_a.inertia_ == ref["inertia"]
    assert torch.equal(km_a._labels_dev, ref["labels"])
    _same_fit(km_a, ref)
    assert KM.FIT_FINISH_USED["finish"] == used + 1
    refb = _eager("tol", 70_001, 30, 8, gpu)
    assert km_b.inertia_ == refb["inertia"] and torch.equal(km_b._labels_dev, refb["labels"])
    assert KM.FIT_FINISH_USED["finish"] == used + 2


def test_a_model_that_is_dropped_never_finishes(gpu):
    from milwrm_amd import kmeans as KM

    used = KM.FIT_FINISH_USED["finish"]
    km = KM.KMeans(n_clusters=2, random_state=SEED).fit(_device_rows("overlap", 257, 7, 2, gpu))
    assert km._pending is not None and km._pending.X.shape == (257, 7)
    del km
    assert KM.FIT_FINISH_USED["finish"] == used


def test_fit_predict_and_labels_straight_after_the_fit(gpu):
    """``fit_predict`` and the ST labeler's read (``kmeans.labels_`` right
    after ``fit``) through a host array, as MILWRM passes ``cluster_data``."""
    from milwrm_amd import kmeans as KM

    X, mu, inv, _ = _rows_host("overlap", 257, 30, 8)
    Xs = (X.astype(np.float64) - mu) * inv
    for read in ("fit_predict", "labels_"):
        ke = KM.KMeans(n_clusters=8, random_state=SEED)
        rows = KM.DeviceRows.from_host(Xs)
        ke._check(rows.S, rows.F)
        ke._set_fitted(rows, *ke._fit_c(rows, 8, None, defer=False))
        used = KM.FIT_FINISH_USED["finish"]
        kd = KM.KMeans(n_clusters=8, random_state=SEED)
        got = kd.fit_predict(Xs) if read == "fit_predict" else kd.fit(Xs).labels_
        assert KM.FIT_FINISH_USED["finish"] == used + 1
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, ke.labels_)
        assert kd.inertia_ == ke.inertia_ and kd.cluster_centers_.tobytes() == ke.cluster_centers_.tobytes()


def test_labeler_never_finishes(gpu):
    """The MxIF label path reads the centers only: no final pass runs, and
    its outputs are those of a labeler whose fit was eager."""
    import torch

    from oracle.milwrm_oracle import synth_slide

    from milwrm_amd import kmeans as KM

    slides = [synth_slide(96, 96, 8, seed=77, mode="hard")]

    def run(defer):
        lab = _labeler(slides)
        if not defer:
            fit_c = KM.KMeans._fit_c
            KM.KMeans._fit_c = lambda self, rows, k, init: fit_c(self, rows, k, init, defer=False)
        try:
            used = KM.FIT_FINISH_USED["finish"]
            lab.label_tissue_regions(k=4, plot_out=False, random_state=18)
            lab.confidence_score_images()
            df = lab.confidence_score_df.values.copy()
            return lab, df, KM.FIT_FINISH_USED["finish"] - used
        finally:
            if not defer:
                KM.KMeans._fit_c = fit_c

    le, dfe, ne = run(False)
    ld, dfd, nd = run(True)
    assert nd == 0 and ne == 0 and le.kmeans._pending is None and ld.kmeans._pending is not None
    assert torch.equal(ld._labels_dev[0], le._labels_dev[0])
    # the fp32 confidences by their bits (NaN outside the mask)
    assert torch.equal(ld._conf_dev[0].view(torch.int32), le._conf_dev[0].view(torch.int32))
    assert np.asarray(dfd, dtype=np.float64).tobytes() == np.asarray(dfe, dtype=np.float64).tobytes()
    used = KM.FIT_FINISH_USED["finish"]
    assert ld.kmeans.inertia_ == le.kmeans.inertia_
    assert KM.FIT_FINISH_USED["finish"] == used + 1
    assert torch.equal(ld.kmeans._labels_dev, le.kmeans._labels_dev)
