"""CPU-only tests of the banded CLAHE: the rule by which
mw_clahe_rows_hist counts a band's rows into the tiles' histograms, restated in
numpy and accumulated band by band, gives the oracle's histograms of the whole
image; and the band entries refuse bad arguments before any device call (the
pointers here are never dereferenced: every case returns before a launch)."""
import numpy as np
import pytest

from milwrm_amd import _native as N
from tests import clahe_oracle as O
from tests.test_gpu_clahe import _slide

ROWS, STATE, OUT = 0x10000, 0x20000, 0x30000  # never dereferenced


def _band_hists(b, y0, rows, kh, kw, nbins, hist):
    """The rule of mw_clahe_rows_hist for the rows [y0, y0 + rows) of the
    quantised plane ``b``: row y into tile row y // kh and, when r = 2 H - 2 - y
    lies in [H, nby kh), once more into tile row r // kh.  Columns as the
    oracle's (the reflection stays inside a row)."""
    H, W = b.shape
    nby = hist.shape[0]
    xs = O.tile_indices(W, kw)
    for y in range(y0, y0 + rows):
        row = b[y, xs].reshape(-1, kw)  # [nbx, kw]
        targets = [y // kh]
        r = 2 * H - 2 - y
        if H <= r < nby * kh:
            assert r // kh == nby - 1  # the rows past the image all lie in the last tile row
            targets.append(r // kh)
        for ti in targets:
            for tj in range(row.shape[0]):
                hist[ti, tj] += np.bincount(row[tj], minlength=nbins)


@pytest.mark.parametrize("H,W,ks,band", [(33, 53, (8, 12), 5), (97, 90, (48, 45), 29), (37, 53, (8, 12), 1),
                                         (41, 45, (6, 9), 7), (45, 38, (13, 7), 11)])
def test_row_rule_accumulated_over_bands_is_the_tile_histogram(H, W, ks, band):
    a = _slide(H, W, 3, np.uint16, seed=H * 1000 + W + 2)
    kh, kw = ks
    nby, nbx = -(-H // kh), -(-W // kw)
    assert nby * kh - H < kh <= H  # a row is reflected at most once, row H - 1 never
    stats = {}
    O.clahe(a, ks, stats=stats)
    assert stats.get("loop_passes", 0) >= 16  # the input drives the oracle's redistribution loop
    reflected_elsewhere = False
    for c in range(a.shape[2]):
        b = O.quantise(a[:, :, c].astype(np.float64), 256)
        ref = O.tile_hists(b, kh, kw, 256)
        hist = np.zeros((nby, nbx, 256), dtype=np.int64)
        for y0 in range(0, H, band):
            _band_hists(b, y0, min(band, H - y0), kh, kw, 256, hist)
        assert np.array_equal(hist, ref)
        assert hist.sum() == nby * kh * nbx * kw
    for y in range(H):
        r = 2 * H - 2 - y
        if H <= r < nby * kh and (y // kh != nby - 1 or y // band != (H - 1) // band):
            reflected_elsewhere = True
    if (H, ks) == (33, (8, 12)):  # reflected rows of tile row nby - 2, in a band before the last
        assert reflected_elsewhere


def _hist(y0=0, rows=5, H=33, W=53, C=3, kh=8, kw=12, nbins=256, dtype=N.MW_U16, ptr=ROWS, state=STATE):
    lib = N.load()
    out = []
    for name, extra in (("mw_clahe_rows_hist", ()), ("mw_clahe_rows_extremes", ()), ("mw_clahe_rows_map", (OUT,))):
        st = getattr(lib, name)(ptr, dtype, y0, rows, H, W, C, None, kh, kw, nbins, state, *extra, None)
        out.append((st, N.last_error()))
    assert len({st for st, _ in out}) == 1, out
    return out[0]


def test_band_entries_refuse_before_any_launch():
    assert _hist(y0=-1)[0] == N._EINVAL
    st, msg = _hist(y0=30, rows=4)  # y0 + rows > H
    assert st == N._EINVAL and "rows" in msg and "mw_clahe_rows" in msg
    assert _hist(rows=0)[0] == N._EINVAL
    assert _hist(rows=-3)[0] == N._EINVAL
    assert _hist(kh=34)[0] == N._EINVAL            # a kernel above the image
    assert _hist(kw=54)[0] == N._EINVAL
    assert _hist(nbins=257)[0] == N._EUNSUP
    assert _hist(nbins=1)[0] == N._EINVAL
    assert _hist(dtype=7)[0] == N._EINVAL
    assert _hist(state=None)[0] == N._EINVAL
    assert _hist(ptr=None)[0] == N._EINVAL
    assert _hist(ptr=ROWS + 1)[0] == N._EINVAL     # not aligned to the uint16 element
    assert _hist(C=257)[0] == N._EUNSUP


def test_other_entries_refuse_before_any_launch():
    lib = N.load()
    assert lib.mw_clahe_rows_begin(N.MW_U16, 33, 53, 3, 8, 12, 0.01, 256, None, None) == N._EINVAL
    assert lib.mw_clahe_rows_begin(N.MW_U16, 33, 53, 3, 34, 12, 0.01, 256, STATE, None) == N._EINVAL
    assert lib.mw_clahe_rows_begin(N.MW_U16, 33, 53, 3, 8, 12, 0.0, 256, STATE, None) == N._EINVAL
    assert lib.mw_clahe_rows_begin(N.MW_U16, 33, 53, 3, 8, 12, 0.01, 300, STATE, None) == N._EUNSUP
    assert lib.mw_clahe_rows_begin(9, 33, 53, 3, 8, 12, 0.01, 256, STATE, None) == N._EINVAL
    assert lib.mw_clahe_rows_range(ROWS, N.MW_U16, 0, 53, 3, STATE, None) == N._EINVAL
    assert lib.mw_clahe_rows_range(ROWS, 7, 5, 53, 3, STATE, None) == N._EINVAL
    assert lib.mw_clahe_rows_range(ROWS, N.MW_U16, 5, 53, 3, None, None) == N._EINVAL
    assert lib.mw_clahe_rows_range(None, N.MW_U16, 5, 53, 3, STATE, None) == N._EINVAL
    assert lib.mw_clahe_rows_luts(33, 53, 3, 8, 12, 0.01, 256, None, None, None) == N._EINVAL
    assert lib.mw_clahe_rows_luts(33, 53, 3, 8, 12, 0.01, 257, STATE, None, None) == N._EUNSUP
    assert lib.mw_clahe_rows_finish(3, None, None, None) == N._EINVAL
    assert lib.mw_clahe_rows_finish(0, None, STATE, None) == N._EINVAL
    # the map's output: null, or the band itself unless that is fp32
    assert lib.mw_clahe_rows_map(ROWS, N.MW_U16, 0, 5, 33, 53, 3, None, 8, 12, 256, STATE, None, None) == N._EINVAL
    assert lib.mw_clahe_rows_map(ROWS, N.MW_U16, 0, 5, 33, 53, 3, None, 8, 12, 256, STATE, ROWS, None) == N._EINVAL


def test_the_rows_entries_are_exported():
    for name in ("begin", "range", "hist", "luts", "extremes", "finish", "map"):
        assert f"mw_clahe_rows_{name}" in N.EXPORTED
