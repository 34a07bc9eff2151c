"""CPU-only tests of the deferred fit's host side: mw_kmeans_fit_finish refuses
bad arguments before any device call (the pointers here are never
dereferenced: every case returns before the first launch or copy, which on a
machine without a device would come back as a HIP error, not MW_EINVAL), and
its workspace is sized against the fit's."""
import pytest

from milwrm_amd import _native as N

X, LAB, WS = 0x10000, 0x20000, 0x30000  # device pointers, never dereferenced
MU, INV, XMAX, CEN, REC, IEXP = 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000  # host, likewise

SHAPES = [(63, 7, 2), (65, 30, 8), (257, 1, 1), (70_001, 30, 8), (70_001, 64, 64), (3_000_000_000, 50, 20)]


def _finish(S=257, F=7, k=4, ws_bytes=None, strict=0, **ptr):
    p = dict(x=X, mu=MU, inv=INV, xmax=XMAX, cen=CEN, lab=LAB, ws=WS, rec=REC, iexp=IEXP)
    p.update(ptr)
    if ws_bytes is None:
        ws_bytes = N.query("mw_kmeans_fit_finish_ws_bytes", S, F, k)
    st = N.load().mw_kmeans_fit_finish(p["x"], S, F, p["mu"], p["inv"], p["xmax"], k, p["cen"], strict, p["lab"],
                                       p["ws"], ws_bytes, p["rec"], p["iexp"], None)
    return st, N.last_error()


@pytest.mark.parametrize("name", ["x", "mu", "inv", "xmax", "cen", "lab", "ws", "rec", "iexp"])
def test_finish_refuses_a_null_pointer(name):
    st, msg = _finish(**{name: None})
    assert st == N._EINVAL and "mw_kmeans_fit_finish" in msg and "null" in msg


@pytest.mark.parametrize("kw,word", [(dict(k=0), "n_clusters"), (dict(k=65), "n_clusters"), (dict(F=65), "F=65"),
                                     (dict(F=0), "F=0"), (dict(S=3, k=4), "n_samples")])
def test_finish_refuses_a_shape_out_of_range(kw, word):
    # the size query answers 0 for these shapes: any workspace size must still be refused for the shape
    st, msg = _finish(ws_bytes=1 << 30, **kw)
    assert st == N._EINVAL and "mw_kmeans_fit_finish" in msg and word in msg


@pytest.mark.parametrize("S,F,k", SHAPES)
def test_finish_refuses_a_workspace_one_byte_short(S, F, k):
    need = N.query("mw_kmeans_fit_finish_ws_bytes", S, F, k)
    st, msg = _finish(S=S, F=F, k=k, ws_bytes=need - 1)
    assert st == N._EINVAL and "workspace" in msg and str(need) in msg


@pytest.mark.parametrize("S,F,k", SHAPES)
def test_finish_workspace_against_the_fit_workspace(S, F, k):
    """The finish holds the scaler, the center table, the pass's per-block
    records and its record, all of which the fit's workspace holds too, and
    neither of the fit's two fp32 bounds per row."""
    fin = N.query("mw_kmeans_fit_finish_ws_bytes", S, F, k)
    fit = N.query("mw_kmeans_fit_ws_bytes", S, F, k)
    rec = N.query("mw_lloyd_rec_len", k, F) * 8
    records = N.query("mw_lloyd_ws_bytes_kinds", S, k, F, 0)
    assert fin % 256 == 0
    assert fin >= 3 * 64 * 4 + (k * F + 2 * k) * 4 + records + rec
    assert fin + 8 * S <= fit


def test_finish_workspace_is_zero_out_of_range():
    for S, F, k in [(0, 8, 4), (-1, 8, 4), (200, 0, 4), (200, 65, 8), (200, 8, 0), (200, 8, 65)]:
        assert N.query("mw_kmeans_fit_finish_ws_bytes", S, F, k) == 0
        assert N.query("mw_kmeans_fit_ws_bytes", S, F, k) == 0
    assert N.query("mw_kmeans_fit_finish_ws_bytes", 200, 64, 64) > 0


def test_deferred_fit_refuses_a_null_strict_flag():
    st = N.load().mw_kmeans_fit_deferred(X, 257, 7, MU, INV, None, XMAX, 4, None, 18, 300, 1e-4, LAB, CEN, IEXP,
                                         None, WS, 1 << 30, 0, None, None, None)
    assert st == N._EINVAL and "h_strict" in N.last_error()
