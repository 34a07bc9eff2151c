"""The k-means fit up to its documented limits, n_clusters <= 64 and F <= 64,
against the fp64 oracle: k-means++ at T = 2 + int(ln k) = 5 and 6 trials
(k = 21..54, 55..64), the first Lloyd pass's M-step instances above k = 20
(kFirst with 2 and 4 label blocks, kFirstAtomic at FM = 32, 52 and 64), whole
fits through the C driver and the Python loop, and the pass kinds of a batched
sweep whose k list crosses the dense pass's limits (20 and 32 centres).

Rows are Gaussian-mixture data stored as fp32 (``DeviceRows.from_host``); the
oracle sees the same fp32 values widened to fp64.

Two conditions on the data stand where a tolerance would otherwise: they are
asserted, and a shape that misses one takes another data seed.

* k-means++ picks the oracle's indices when the oracle's own decisions are not
  within rounding of a boundary: both margins of ``_kpp_margins`` (target to
  cumulative-sum boundary, best to second-best trial potential) >= 1e-9
  relative; the device's fp64 distances differ from the oracle's by ~1e-13.
* a whole fit takes the oracle's iterations when no row comes within TAU
  (relative top-2 gap) of a tie at any iteration of the oracle's trajectory:
  a row that legitimately goes the other way changes n_iter.  The seeds of
  ``FITS`` were searched on the CPU among 0..49 (``trajectory``); their
  margins are listed there."""
import contextlib
import sys

import numpy as np
import pytest

from oracle import milwrm_oracle as O
from tests.test_oracle_golden import _kpp_margins

pytestmark = pytest.mark.gpu
TAU = 1e-5
RTOL = 1e-4
NEAR_TIE_SHARE = 1e-3
KPP_MARGIN = 1e-9
S_BIG = 20011

# (k, F) -> data seed
# (cumulative-sum margins 1.1e-8 .. 1.3e-7, trial gaps 1.3e-5 .. 3.2e-4; (64, 64) at seed 0: 4.2e-9)
KPP = {(21, 30): 0, (54, 8): 0, (55, 30): 0, (33, 45): 0, (64, 50): 0, (64, 64): 2}
STEP = [(21, 16), (33, 8), (64, 16), (32, 30), (33, 30), (64, 30), (21, 50), (64, 64)]
# (k, F, S) -> (data seed, the oracle trajectory's smallest top-2 gap, its iterations)
# (smallest clusters met: 4, 11, 6 and 41 rows; no empty cluster, so no relocation)
FITS = {(33, 30, 3001): (0, 2.405e-5, 26), (64, 64, 3001): (16, 6.207e-5, 18), (64, 16, 3001): (1, 2.282e-5, 25),
        (21, 50, 3001): (0, 3.905e-5, 15)}
SWEEP_KS = [19, 21, 32, 33, 48, 64]


def mixture(S, F, seed, n_comp=12):
    """S x F fp32 rows: ``n_comp`` unit Gaussians around N(0, 2^2) centres."""
    rng = np.random.default_rng(seed)
    cen = rng.normal(0.0, 2.0, size=(n_comp, F))
    return (cen[rng.integers(0, n_comp, S)] + rng.normal(0.0, 1.0, size=(S, F))).astype(np.float32)


def top2_gap(X, centers, chunk=8192):
    """(argmin, relative top-2 gap) of fp64 direct-difference distances."""
    lab = np.empty(X.shape[0], dtype=np.int64)
    gap = np.empty(X.shape[0])
    for s in range(0, X.shape[0], chunk):
        d = ((X[s:s + chunk, None, :] - centers[None]) ** 2).sum(-1)
        lab[s:s + chunk] = d.argmin(1)
        d.sort(axis=1)
        gap[s:s + chunk] = (d[:, 1] - d[:, 0]) / np.maximum(d[:, 1], 1e-300)
    return lab, gap


def trajectory(X, k, seed=18, max_iter=300, tol=1e-4):
    """``O.kmeans_fit`` step by step: its result, the smallest relative top-2
    gap of any row at any E-step (the final one included), the smallest
    relative distance of the centre-shift test from its threshold, and the
    smallest cluster size met."""
    X = np.array(X, dtype=np.float64)
    _tol = float(np.mean(np.var(X, axis=0)) * tol)
    mean = X.mean(axis=0)
    Xc = X - mean
    centers, idx = O.kmeans_plusplus(Xc, k, np.random.RandomState(seed))
    labels_old = np.full(X.shape[0], -1, dtype=np.int32)
    gmin, tmin, wmin, strict = np.inf, np.inf, np.inf, False
    for it in range(max_iter):
        gmin = min(gmin, float(top2_gap(Xc, centers)[1].min()))
        labels, centers, w, shift = O.lloyd_iter(Xc, centers)
        wmin = min(wmin, float(w.min()))
        if np.array_equal(labels, labels_old):
            strict = True
            break
        s2 = float((shift ** 2).sum())
        tmin = min(tmin, abs(s2 - _tol) / _tol)
        if s2 <= _tol:
            break
        labels_old = labels.copy()
    if not strict:
        gmin = min(gmin, float(top2_gap(Xc, centers)[1].min()))
        labels = O.lloyd_iter(Xc, centers, update_centers=False)[0]
    fit = dict(cluster_centers_=centers + mean, labels_=labels, inertia_=O.inertia_dense(Xc, centers, labels),
               n_iter_=it + 1, init_indices=idx)
    return fit, gmin, tmin, wmin


def _rows(X32):
    from milwrm_amd.kmeans import DeviceRows

    return DeviceRows.from_host(X32)


# ------------------------------------------------------------ a. k-means++

@pytest.mark.parametrize("k,F", list(KPP), ids=[f"k{k}F{F}" for k, F in KPP])
def test_kpp_indices_five_and_six_trials(gpu, k, F):
    from milwrm_amd.kmeans import _kmeans_plusplus_device

    assert 2 + int(np.log(k)) == (5 if k <= 54 else 6)
    X32 = mixture(S_BIG, F, KPP[(k, F)])
    X = X32.astype(np.float64)
    Xc = X - X.mean(axis=0)
    cm, sg = (min(v) for v in zip(*_kpp_margins(Xc, k)))
    print(f"k-means++ k={k} F={F}: cumulative-sum margin {cm:.3g}, trial gap {sg:.3g}")
    assert cm >= KPP_MARGIN and sg >= KPP_MARGIN, "data condition: pick another seed"
    _, want = O.kmeans_plusplus(Xc, k, np.random.RandomState(18))
    cen, idx = _kmeans_plusplus_device(_rows(X32), k, np.random.RandomState(18))
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(cen, X[want])


# ------------------------------------------------------------ b. one Lloyd step

@pytest.mark.parametrize("k,F", STEP, ids=[f"k{k}F{F}" for k, F in STEP])
def test_first_lloyd_step_above_k20(gpu, k, F):
    """kFirst at MBF = 2 (21, 16), 3 and 4 (33, 8), (64, 16), MBF NBF = 4
    (32, 30); kFirstAtomic at FM = 32 (33, 30), (64, 30), 52 (21, 50), 64
    (64, 64).  Labels = the fp64 argmin outside near-ties; sizes = the counts
    of the device's own labels; sums / size = the fp64 means over the device's
    own labels (so a near-tie row cannot hide a wrong sum)."""
    from milwrm_amd.kmeans import lloyd_step_device

    X32 = mixture(S_BIG, F, 100 + k + F)
    X = X32.astype(np.float64)
    _, idx = O.kmeans_plusplus(X - X.mean(axis=0), k, np.random.RandomState(18))
    cin = X[idx]  # rows of the data: exact in fp32, the centres the device uses
    lab, sums, w = lloyd_step_device(_rows(X32), cin)
    lab = lab.cpu().numpy().astype(np.int64)
    ref, gap = top2_gap(X, cin)
    near = gap < TAU
    print(f"lloyd step k={k} F={F}: near-tie share {near.mean():.3g}, moved {int((lab != ref).sum())}")
    assert near.mean() <= NEAR_TIE_SHARE
    assert lab.min() >= 0 and lab.max() < k
    assert not np.any((lab != ref) & ~near)
    np.testing.assert_array_equal(w, np.bincount(lab, minlength=k))
    assert np.all(w > 0)
    means = np.zeros((k, F))
    np.add.at(means, lab, X)
    means /= w[:, None]
    np.testing.assert_allclose(sums / w[:, None], means, rtol=RTOL, atol=1e-6)


# ------------------------------------------------------------ c. whole fits

@pytest.fixture(scope="module")
def oracle_fits():
    made = {}
    yield made
    made.clear()


@pytest.mark.parametrize("k,F,S", list(FITS), ids=[f"k{k}F{F}S{S}" for k, F, S in FITS])
def test_whole_fit_against_oracle(gpu, monkeypatch, oracle_fits, k, F, S):
    """KMeans(k, random_state=18).fit through the C driver and through the
    Python loop: bitwise each other's; the oracle's k-means++ indices, n_iter
    and labels (outside near-ties of the final centres), centres and inertia
    within RTOL, inertia within 1e-6 of an fp64 recompute from the fit's own
    labels and centres."""
    from milwrm_amd import kmeans as KM

    seed, gap_seen, iters_seen = FITS[(k, F, S)]
    X32 = mixture(S, F, seed)
    X = X32.astype(np.float64)
    want, gmin, tmin, wmin = trajectory(X, k)
    print(f"fit k={k} F={F} S={S} seed={seed}: trajectory gap {gmin:.3g}, shift-test margin {tmin:.3g}, "
          f"smallest cluster {wmin:.0f}, n_iter {want['n_iter_']}")
    assert gmin >= TAU and tmin >= 1e-6 and wmin >= 1, "data condition: pick another seed"
    assert abs(gmin - gap_seen) <= 1e-3 * gap_seen and want["n_iter_"] == iters_seen  # as recorded above
    chk = O.kmeans_fit(X, k, random_state=18)  # the stepwise restatement is the oracle's fit
    assert chk["n_iter_"] == want["n_iter_"] and np.array_equal(chk["labels_"], want["labels_"])
    rows = _rows(X32)
    got = {}
    # the whole fit in C; k-means++ from Python with the iterations in C; every pass from Python
    for name, use_c, use_c_fits in (("c", True, True), ("py", False, True), ("py_passes", False, False)):
        monkeypatch.setattr(KM, "USE_C_FIT", use_c)
        monkeypatch.setattr(KM, "USE_C_FITS", use_c_fits)
        with contextlib.redirect_stdout(sys.stderr):
            km = KM.KMeans(n_clusters=k, random_state=18).fit(rows)
        got[name] = (km.labels_.copy(), km.cluster_centers_.copy(), float(km.inertia_), int(km.n_iter_),
                     np.asarray(km.init_indices_).copy())
    a = got["c"]
    for name in ("py", "py_passes"):
        b = got[name]
        np.testing.assert_array_equal(a[0], b[0], err_msg=name)
        np.testing.assert_array_equal(a[1], b[1], err_msg=name)
        assert a[2] == b[2] and a[3] == b[3], name
        np.testing.assert_array_equal(a[4], b[4], err_msg=name)
    lab, cen, inertia, n_iter, idx = a
    np.testing.assert_array_equal(idx, want["init_indices"])
    assert n_iter == want["n_iter_"]
    _, gap = top2_gap(X, want["cluster_centers_"])
    assert not np.any((lab != want["labels_"]) & ~(gap < TAU))
    assert np.max(np.abs(cen - want["cluster_centers_"])) <= RTOL * np.max(np.abs(want["cluster_centers_"]))
    assert abs(inertia - want["inertia_"]) <= RTOL * want["inertia_"]
    own = float(((X - cen[lab]) ** 2).sum())
    print(f"fit k={k} F={F}: inertia against its own fp64 recompute {abs(inertia - own) / own:.3g}")
    assert abs(inertia - own) <= 1e-6 * own


# ------------------------------------------------------------ d. pass kinds

@pytest.mark.parametrize("F", [30, 50])
def test_pass_kinds_equal_full_estep_above_k20(gpu, monkeypatch, F):
    """fit_many over k = 19..64 in one batched sweep: every bounded pass
    forced to kTile, or to kList, or the project defaults (the dense pass
    enabled: a k list that crosses its limits of 20 and 32 centres must fall
    back to the bounded passes) against the plain E-step every pass
    (MW_LLOYD_NOBOUND=1): labels, centres and n_iter bit for bit."""
    from milwrm_amd import kmeans as KM

    rows = _rows(mixture(S_BIG, F, 7))
    defaults = (KM.QUEUE_BELOW, KM.QUEUE_KIND, KM.USE_DENSE)
    out = {}
    for name, qb, qk, dense, nobound in [("full", -1.0, KM.KIND_QUEUE, False, True),
                                         ("tile", -1.0, KM.KIND_QUEUE, False, False),
                                         ("list", 2.0, KM.KIND_LIST, False, False),
                                         ("default",) + defaults + (False,)]:
        monkeypatch.setattr(KM, "QUEUE_BELOW", qb)
        monkeypatch.setattr(KM, "QUEUE_KIND", qk)
        monkeypatch.setattr(KM, "USE_DENSE", dense)
        if nobound:
            monkeypatch.setenv("MW_LLOYD_NOBOUND", "1")
        else:
            monkeypatch.delenv("MW_LLOYD_NOBOUND", raising=False)
        with contextlib.redirect_stdout(sys.stderr):
            fits = KM.fit_many(rows, SWEEP_KS, random_state=18)
        out[name] = [(np.asarray(m.labels_).copy(), m.cluster_centers_.copy(), m.n_iter_) for m in fits]
    assert defaults[2], "the default run has the dense pass enabled"
    for name in ("tile", "list", "default"):
        for i, k in enumerate(SWEEP_KS):
            a, b = out["full"][i], out[name][i]
            assert a[2] == b[2], f"F={F} k={k} {name}: n_iter {b[2]} vs {a[2]}"
            np.testing.assert_array_equal(b[0], a[0], err_msg=f"F={F} k={k} {name} labels")
            np.testing.assert_array_equal(b[1], a[1], err_msg=f"F={F} k={k} {name} centers")


# ------------------------------------------------------------ e. limits

def test_limits_raise_not_implemented(gpu):
    from milwrm_amd import _native as N
    from milwrm_amd.kmeans import KMeans, fit_many

    rng = np.random.default_rng(0)
    rows = _rows(rng.normal(size=(200, 8)).astype(np.float32))
    with pytest.raises(NotImplementedError, match="64"):
        KMeans(n_clusters=65, random_state=18).fit(rows)
    wide = _rows(rng.normal(size=(200, 65)).astype(np.float32))
    with pytest.raises(NotImplementedError, match="64"):
        KMeans(n_clusters=8, random_state=18).fit(wide)
    with pytest.raises(NotImplementedError, match="64"):
        fit_many(wide, [4, 8], random_state=18)
    assert N.query("mw_kmeans_fit_ws_bytes", 200, 8, 65) == 0
    assert N.query("mw_kmeans_fit_ws_bytes", 200, 65, 8) == 0
    assert N.query("mw_kmeans_fit_ws_bytes", 200, 64, 64) > 0
