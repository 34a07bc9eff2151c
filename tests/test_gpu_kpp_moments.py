"""k-means++ whose first step takes its block potentials from the gather's
per-block moment records (``mw_kpp_init_moments``, csrc/kpp.hip) against the
init-pass form (``mw_kpp_init`` + ``mw_kpp_step(c = 1)``), through the
low-level calls with chosen draws, and end to end through the labeler.

``mw_kpp_init_moments`` is the init and step 1 in one call (it needs step 1's
draws), so the moments form is that call followed by ``mw_kpp_step`` for
c = 2..k-1; the init-pass form is ``mw_kpp_init`` and ``mw_kpp_step`` for
c = 1..k-1.  Both end with ``mw_kpp_indices``.  The state compared after step
1 is ``cur`` and the halves of the block-sum and tile-sum sections that step
1's pass writes (the sections ping-pong by step parity); the other halves
hold what came before step 1, which is the init pass's sums in one form and
the located blocks' tile sums in the other.

Where a tolerance appears (the moment block sums, 1e-12 relative): the sums
are a handful of fp64 operations per feature on records that are themselves
two-pass / Chan-merged fp64 moments of sums of non-negative terms, a few
1e-16 relative each; a numpy fp64 check of the identity gave 6e-16."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

# k = 2..20 in the three groups that share n_local_trials T = 2 + int(ln k):
# within a group the centers of a smaller k are a prefix of the largest k's
GROUPS = [(2, 2), (3, 7), (4, 20)]  # (T, largest k)
SIZES = [63, 64, 65, 255, 257, 70_001, 300_007]  # the last: more than 256 rows per moment block
FEATS = [7, 30, 50]

_DATA = {}


def _data(S, F):
    """Overlapping clusters in fp32 with offsets and scales per feature, one
    zero-variance column, two rows that duplicate the first center (distance
    clipped to 0), and the fp64 reference distances to the first center."""
    if (S, F) not in _DATA:
        rng = np.random.default_rng(1000 * F + S % 997)
        cen = rng.normal(size=(5, F))
        X = cen[rng.integers(0, 5, size=S)] + rng.normal(size=(S, F))  # spread = separation: overlap
        X = (X * rng.uniform(0.5, 20.0, size=F) + rng.uniform(-5.0, 50.0, size=F)).astype(np.float32)
        X[:, 2] = np.float32(3.5)
        first = S // 3
        X[10] = X[first]
        X[S // 2] = X[first]
        X64 = X.astype(np.float64)
        mu = X64.mean(axis=0)
        sd = X64.std(axis=0)
        sd[sd == 0] = 1.0
        inv = 1.0 / sd
        d = (((X64 - X64[first]) * inv) ** 2).sum(axis=1)
        _DATA[(S, F)] = (X, mu, inv, first, d)
    return _DATA[(S, F)]


def _u_at(d, row):
    """The draw whose target falls in the middle of ``row``'s share of the
    cumulative distances (far from any rounding of either form's sums)."""
    cum = np.cumsum(d)
    assert d[row] > 0
    return float((cum[row] - 0.5 * d[row]) / cum[-1])


def _draws(S, d, T, kmax, bounds):
    """Draws of steps 1..kmax-1; step 1's are chosen: 0, just below 1, and
    targets in the first block, the last block and the last (partial) tile."""
    from milwrm_amd import _native as N

    rng = np.random.default_rng(7 * S + T)
    us = rng.random((kmax - 1, 8))
    off, n = bounds[-1]
    rpb = N.query("mw_rows_per_block", n)
    last_block = off + ((n - 1) // rpb) * rpb  # first row of the last moment block
    pos = lambda r: r if d[r] > 0 else r + 1  # noqa: E731  (skip a duplicate of the first center)
    first_blk, last_blk, last_tile = _u_at(d, pos(1)), _u_at(d, pos(last_block)), _u_at(d, pos(S - 2))
    below1 = float(np.nextafter(1.0, 0.0))
    chosen = {2: [last_tile, 0.0], 3: [first_blk, below1, last_blk], 4: [0.0, below1, first_blk, last_tile]}[T]
    us[0, :T] = chosen
    return us


def _segments(Xd, mu, inv, bounds):
    """DeviceRows over Xd with the moment records mw_col_stats_rows writes for
    the row ranges ``bounds`` (the records a gather of those rows leaves)."""
    import torch

    from milwrm_amd import device as D
    from milwrm_amd.kmeans import DeviceRows

    F = Xd.shape[1]
    rows = DeviceRows(Xd, mu, inv)
    rows.moments = []
    for off, n in bounds:
        st = torch.zeros(1 + 2 * F, dtype=torch.float64, device=Xd.device)
        rows.moments.append((off, n) + D.col_stats_rows(Xd[off:off + n], st, accumulate=False, keep_records=True))
    return rows


def _sections(S, T):
    from milwrm_amd import _native as N

    out = np.zeros(7, dtype=np.int64)
    N.load().mw_kpp_ws_sections(S, T, out.ctypes.data)
    return dict(zip(("cur", "bsum", "tsum", "mom", "G", "NTL", "cap"), (int(v) for v in out)))


def _kpp(rows, first, us, T, kmax, moments):
    """One seeding of kmax centers through the low-level calls: the chosen
    indices after every step (k = 2..kmax), the state after step 1 (cur and
    step 1's halves of the block-sum and tile-sum sections) and the workspace."""
    import torch

    from milwrm_amd import _native as N
    from milwrm_amd import device as D

    S, F = rows.S, rows.F
    X, mu, inv, st = D.P(rows.X), D.P(rows.mu64), D.P(rows.inv64), D.stream()
    ws = torch.zeros(N.query("mw_kpp_ws_bytes", S, T), dtype=torch.uint8, device=rows.X.device)
    c0 = X + int(first) * F * 4
    u = lambda c: np.ascontiguousarray(us[c - 1], dtype=np.float64)  # noqa: E731
    if moments:
        n_seg, segs = rows.moment_segments()
        u1 = u(1)
        N.call("mw_kpp_init_moments", X, S, F, mu, inv, c0, u1.ctypes.data, T, n_seg, C.addressof(segs),
               D.P(ws), st)
    else:
        N.call("mw_kpp_init", X, S, F, mu, inv, c0, T, D.P(ws), st)
        u1 = u(1)
        N.call("mw_kpp_step", X, S, F, mu, inv, 1, u1.ctypes.data, T, D.P(ws), st)
    sec = _sections(S, T)
    G, NTL = sec["G"], sec["NTL"]
    w64 = ws.view(torch.float64)
    state = dict(cur=w64[sec["cur"] // 8:sec["cur"] // 8 + S].clone(),
                 bsum=w64[sec["bsum"] // 8 + T * G:sec["bsum"] // 8 + 2 * T * G].clone(),  # step parity 1
                 tsum=w64[sec["tsum"] // 8 + T * NTL:sec["tsum"] // 8 + 2 * T * NTL].clone())
    idx = {}
    out = torch.empty(kmax, dtype=torch.int64, device=rows.X.device)
    for c in range(1, kmax):
        if c >= 2:
            uc = u(c)
            N.call("mw_kpp_step", X, S, F, mu, inv, c, uc.ctypes.data, T, D.P(ws), st)
        N.call("mw_kpp_indices", D.P(ws), S, T, c + 1, D.P(out), st)
        idx[c + 1] = out[:c + 1].cpu().numpy().copy()
    return idx, state, ws


def _compare(X, mu, inv, first, d, bounds, dev):
    """Both forms over the same rows: indices for k = 2..20, the state after
    step 1, and the moment block sums against numpy fp64."""
    import torch

    S, F = X.shape
    rows = _segments(torch.from_numpy(X).to(dev), mu, inv, bounds)
    for T, kmax in GROUPS:
        kmax = min(kmax, S)
        us = _draws(S, d, T, kmax, bounds)
        ia, sa, _ = _kpp(rows, first, us, T, kmax, moments=False)
        ib, sb, ws = _kpp(rows, first, us, T, kmax, moments=True)
        for k in ia:
            np.testing.assert_array_equal(ia[k], ib[k], err_msg=f"S={S} F={F} T={T} k={k}")
        for key in ("cur", "bsum", "tsum"):
            assert torch.equal(sa[key], sb[key]), f"S={S} F={F} T={T}: {key} after step 1"
    # moment block sums (T = 4 workspace of the last group) against the rows
    sec = _sections(S, 4)
    got = ws.view(torch.float64)[sec["mom"] // 8:sec["mom"] // 8 + sec["cap"]].cpu().numpy()
    X64 = X.astype(np.float64)
    b = 0
    for off, n, rpb, _ in rows.moments:
        for lo in range(off, off + n, rpb):
            hi = min(off + n, lo + rpb)
            want = (((X64[lo:hi] - X64[first]) * inv) ** 2).sum()
            rel = abs(got[b] - want) / want
            assert rel < 1e-12, f"S={S} F={F} moment block {b} rows [{lo}, {hi}): {got[b]} vs {want} ({rel:.2e})"
            b += 1


@pytest.mark.parametrize("F", FEATS)
@pytest.mark.parametrize("S", SIZES)
def test_moments_form_equals_init_pass_form(gpu, S, F):
    X, mu, inv, first, d = _data(S, F)
    _compare(X, mu, inv, first, d, [(0, S)], gpu)


@pytest.mark.parametrize("S1,S2,F", [(1000, 333, 30), (70_001, 5_003, 30), (321, 4_097, 7)])
def test_two_images_in_one_X(gpu, S1, S2, F):
    """Two segments; the second starts at a row that is no multiple of 64."""
    X, mu, inv, first, d = _data(S1 + S2, F)
    _compare(X, mu, inv, first, d, [(0, S1), (S1, S2)], gpu)


# ------------------------------------------------------------- end to end

def _labeler(slides, comm=None, k=8):
    import pandas as pd

    import milwrm_amd as M

    imgs = [M.img(r.copy(), mask=m.copy()) for r, m in slides]
    ests, pix = zip(*[im.calculate_non_zero_mean() for im in imgs])
    df = pd.DataFrame({"Img": imgs, "batch_names": ["b"] * len(imgs), "mean estimators": list(ests),
                       "pixels": list(pix)})
    lab = M.mxif_labeler(df)
    lab.prep_cluster_data(features=list(range(slides[0][0].shape[2])), sigma=2, fract=0.2, comm=comm)
    return lab


def _fit_out(lab, comm=None, k=8):
    from milwrm_amd import kmeans as KM

    used = dict(KM.KPP_INIT_USED)
    lab.label_tissue_regions(k=k, plot_out=False, random_state=18, comm=comm)
    km = lab.kmeans
    return dict(idx=km.init_indices_, n_iter=km.n_iter_, centers=km.cluster_centers_, inertia=km.inertia_,
                labels=km.labels_, tid=[np.nan_to_num(t, nan=-1) for t in lab.tissue_IDs],
                used={key: KM.KPP_INIT_USED[key] - used[key] for key in used})


def test_labeler_bitwise_with_and_without_moments(gpu):
    from oracle.milwrm_oracle import synth_slide

    from milwrm_amd import kmeans as KM

    slides = [synth_slide(256, 256, 30, seed=77, mode="hard")]
    lab = _labeler(slides)
    assert lab._rows.moments and len(lab._rows.moments) == 1
    a = _fit_out(lab)
    assert a["used"] == {"moments": 1, "pass": 0}, a["used"]
    # a sorted fit_many (the sweep's form) keeps the init pass
    used = dict(KM.KPP_INIT_USED)
    assert lab._rows.draws
    KM.fit_many(lab._rows, [3, 4], random_state=18)
    assert KM.KPP_INIT_USED["moments"] == used["moments"] and KM.KPP_INIT_USED["pass"] > used["pass"]
    lab2 = _labeler(slides)
    lab2._rows.moments = None  # withheld
    b = _fit_out(lab2)
    assert b["used"] == {"moments": 0, "pass": 1}, b["used"]
    for key in ("idx", "centers", "labels"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["n_iter"] == b["n_iter"] and a["inertia"] == b["inertia"]
    np.testing.assert_array_equal(a["tid"][0], b["tid"][0])
    # the Python k-means++ loop takes the moments too, to the same indices
    used = dict(KM.KPP_INIT_USED)
    KM.USE_C_FIT = False
    try:
        km = KM.KMeans(n_clusters=8, random_state=18).fit(lab._rows)
    finally:
        KM.USE_C_FIT = True
    assert KM.KPP_INIT_USED["moments"] == used["moments"] + 1
    np.testing.assert_array_equal(km.init_indices_, a["idx"])
    np.testing.assert_array_equal(km.labels_, a["labels"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_slides():
    from oracle.milwrm_oracle import synth_slide

    return [synth_slide(128, 128 + 32 * i, 8, seed=500 + i, mode="hard") for i in range(2)]


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from milwrm_amd.dist import DistComm

        comm = DistComm(device=torch.device("cpu"))
        res = _fit_out(_labeler([_shard_slides()[rank]], comm=comm, k=6), comm=comm, k=6)
        torch.cuda.synchronize()
        q.put((rank, res))
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_fit_keeps_the_init_pass(gpu):
    """Two ranks sharing the GPU, one slide each: the row-sharded k-means++
    starts with the init pass, and gives the single process's (moments) fit."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict(q.get(timeout=240) for _ in ps)
    for p in ps:
        p.join(60)
    for r in (0, 1):
        assert not isinstance(got[r], str), got[r]
        assert ps[r].exitcode == 0
    ref = _fit_out(_labeler(_shard_slides(), k=6), k=6)
    assert ref["used"] == {"moments": 1, "pass": 0}, ref["used"]
    for r in (0, 1):
        assert got[r]["used"] == {"moments": 0, "pass": 1}, got[r]["used"]
        np.testing.assert_array_equal(got[r]["idx"], ref["idx"])
        np.testing.assert_array_equal(got[r]["centers"], ref["centers"])
        assert got[r]["n_iter"] == ref["n_iter"] and got[r]["inertia"] == ref["inertia"]
    np.testing.assert_array_equal(np.concatenate([got[0]["labels"], got[1]["labels"]]), ref["labels"])
