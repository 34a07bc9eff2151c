"""img.histogram on the device: the counts are np.histogram's of the float64
pixels and the edges np.linspace's, bit for bit -- resident, of the current
(pending) pixels, and band by band of a slide that is not resident
("streamed": MW_HBM_BUDGET=1 with MW_STREAM_BAND_ROWS 29, 37 or 61, as
tests/test_gpu_intensity_stream.py).  The slides and the explicit (range,
bins) pairs: tests/histogram_data.py (guarded by tests/test_cpu_histogram.py)."""
import matplotlib

matplotlib.use("Agg")

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

from tests import histogram_data as HD  # noqa: E402

pytestmark = pytest.mark.gpu

BINS = (1, 2, 51, 100, 1000)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _env(monkeypatch, streamed, band="37"):
    if streamed:
        monkeypatch.setenv("MW_HBM_BUDGET", "1")  # nothing may stay resident: every pass streams
        monkeypatch.setenv("MW_STREAM_BAND_ROWS", band)
    else:
        monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
        monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)


def _img(kind, C=8, two_d=False):
    import milwrm_amd as M

    raw, mask = HD.slide(kind, C)
    return M.img((raw[:, :, 0] if two_d else raw).copy(), mask=mask.copy()), raw, mask


def _check(got, planes, bins, rng=None):
    """``got`` = (counts, edges) against np.histogram of every plane of ``planes``."""
    counts, edges = got
    assert counts.dtype == np.int64 and edges.dtype == np.float64
    assert counts.shape == (len(planes), bins) and edges.shape == (len(planes), bins + 1)
    for i, x in enumerate(planes):
        ref_c, ref_e = HD.numpy_histogram(x, bins, rng)
        assert np.array_equal(edges[i].view(np.uint64), ref_e.view(np.uint64)), (i, bins, rng)
        assert np.array_equal(counts[i], ref_c), (i, bins, rng, np.flatnonzero(counts[i] != ref_c)[:8])


@pytest.mark.parametrize("kind", HD.KINDS)
def test_resident_equals_numpy(gpu, monkeypatch, kind):
    """Every kind, C in {1, 3, 8, 30}, bins in {1, 2, 51, 100, 1000}, the range from the data."""
    _env(monkeypatch, False)
    for C in HD.CHANNELS:
        im, raw, _ = _img(kind, C)
        for bins in BINS:
            _check(im.histogram(None, bins), [raw[:, :, c] for c in range(C)], bins)


@pytest.mark.parametrize("kind,rng,bins", HD.EXPLICIT)
def test_explicit_ranges_need_both_corrections(gpu, monkeypatch, kind, rng, bins):
    """The pairs whose uncorrected index is wrong for values of the slide."""
    _env(monkeypatch, False)
    for C in HD.CHANNELS:
        im, raw, _ = _img(kind, C)
        _check(im.histogram(None, bins, range=rng), [raw[:, :, c] for c in range(C)], bins, rng)


@pytest.mark.parametrize("kind,rng", [("u16", (1000, 40000.5)), ("f32nan", (-20.25, 35.0)), ("u8", (17, 17)),
                                      ("f32", (-1e6, 1e6))])
def test_range_narrower_or_wider_than_the_data(gpu, monkeypatch, kind, rng):
    """Elements outside the range are dropped; an empty range is widened as numpy's."""
    _env(monkeypatch, False)
    im, raw, _ = _img(kind, 3)
    for bins in (1, 37, 100):
        _check(im.histogram(None, bins, range=rng), [raw[:, :, c] for c in range(3)], bins, rng)


@pytest.mark.parametrize("kind", ["u16", "f32nan"])
def test_channel_selections(gpu, monkeypatch, kind):
    _env(monkeypatch, False)
    im, raw, _ = _img(kind, 8)
    for channels, idx in [(None, list(range(8))), ((0, 2), [0, 2]), (("ch_1", "ch_3"), [1, 3]), ((1, 1), [1, 1]),
                          ([7, 0, 7], [7, 0, 7]), (5, [5]), ("ch_6", [6]), (-1, [7])]:
        _check(im.histogram(channels, 100), [raw[:, :, c] for c in idx], 100)
        _check(im.histogram(channels, 51, range=(0, 255)), [raw[:, :, c] for c in idx], 51, (0, 255))


def test_two_d_image_is_one_channel(gpu, monkeypatch):
    _env(monkeypatch, False)
    for kind in ("u8", "f32nan"):
        im, raw, mask = _img(kind, 3, two_d=True)
        _check(im.histogram(bins=100), [raw[:, :, 0]], 100)
        _check(im.histogram(0, 51, range=(0, 255)), [raw[:, :, 0]], 51, (0, 255))
        _check(im.histogram(bins=100, mask_out=True), [raw[:, :, 0][mask != 0]], 100)


@pytest.mark.parametrize("kind", ["u8", "u16lo", "f32nan", "dom"])
def test_mask_out(gpu, monkeypatch, kind):
    """Only pixels of the mask count, in the range and in the counts."""
    _env(monkeypatch, False)
    for C in HD.CHANNELS:
        im, raw, mask = _img(kind, C)
        planes = [raw[:, :, c][mask != 0] for c in range(C)]
        _check(im.histogram(None, 100, mask_out=True), planes, 100)
        _check(im.histogram(None, 100, range=(0, 100), mask_out=True), planes, 100, (0, 100))
    im, raw, mask = _img(kind, 8)
    _check(im.histogram((6, 1), 51, mask_out=True), [raw[:, :, c][mask != 0] for c in (6, 1)], 51)


def _ops():
    return {"clip": lambda im: im.clip(),
            "lognorm_gaussian": lambda im: (im.log_normalize(), im.blurring("gaussian", sigma=2)),
            "clahe": lambda im: im.equalize_hist(kernel_size=16),
            "clip_deferred_rescale": lambda im: im.clip(),
            "clahe_banded": lambda im: im.equalize_hist(kernel_size=16, banded=True)}


@pytest.mark.parametrize("op", ["clip", "lognorm_gaussian", "clahe"])
def test_current_pixels(gpu, monkeypatch, op):
    """The histogram is of what ``img`` returns, and reading it changes nothing."""
    _env(monkeypatch, False)
    im, _, _ = _img("u16", 8)
    _ops()[op](im)
    fresh = im.histogram(None, 100)  # whatever is still pending is applied by the call
    before = im.img.copy()
    for rng in (None, (0.0, 0.5)):
        _check(im.histogram(None, 100, range=rng), [before[:, :, c] for c in range(8)], 100, rng)
    _check(im.histogram((3, 0), 51, mask_out=True), [before[:, :, c][np.asarray(im.mask) != 0] for c in (3, 0)], 51)
    assert np.array_equal(_bits(im.img), _bits(before))
    _check(fresh, [before[:, :, c] for c in range(8)], 100)


def _used():
    from milwrm_amd import device as D

    return dict(D.HISTOGRAM_USED)


@pytest.mark.parametrize("kind,band", [("u8", "29"), ("u16", "37"), ("f32nan", "61")])
def test_streamed_equals_resident_raw(gpu, monkeypatch, kind, band):
    _env(monkeypatch, False)
    ref, raw, _ = _img(kind, 8)
    want = [ref.histogram(None, 100), ref.histogram((2, 5, 2), 51, range=(0, 255)),
            ref.histogram(None, 100, mask_out=True)]
    _check(want[0], [raw[:, :, c] for c in range(8)], 100)
    _env(monkeypatch, True, band)
    im, _, _ = _img(kind, 8)
    before = _used()
    got = [im.histogram(None, 100), im.histogram((2, 5, 2), 51, range=(0, 255)),
           im.histogram(None, 100, mask_out=True)]
    assert im._dev is None and _used()["streamed"] == before["streamed"] + 3
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(_bits(g[1]), _bits(w[1]))


@pytest.mark.parametrize("op,band", [("clip_deferred_rescale", "29"), ("clahe_banded", "37"),
                                     ("lognorm_gaussian", "61"), ("lognorm_gaussian", "29")])
def test_streamed_equals_resident_pending(gpu, monkeypatch, op, band):
    """Deferred clip / CLAHE rounds and a deferred filter are applied per band; nothing pending is cleared."""
    _env(monkeypatch, False)
    ref, _, _ = _img("u16", 8)
    _ops()[op](ref)
    want = ref.histogram(None, 100), ref.histogram((1, 6), 51, range=(0.0, 0.75), mask_out=True)
    pix = ref.img
    _check(want[0], [pix[:, :, c] for c in range(8)], 100)
    _env(monkeypatch, True, band)
    im, _, _ = _img("u16", 8)
    _ops()[op](im)
    pending = (im._pending, im._pending_blur, im._pending_rescale, im._pending_clahe)
    assert im._dev is None and any(p is not None for p in pending[1:])
    before = _used()
    got = im.histogram(None, 100), im.histogram((1, 6), 51, range=(0.0, 0.75), mask_out=True)
    assert im._dev is None and _used()["streamed"] == before["streamed"] + 2
    assert all(a is b for a, b in zip(pending, (im._pending, im._pending_blur, im._pending_rescale,
                                                im._pending_clahe)))
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(_bits(g[1]), _bits(w[1]))
    assert np.array_equal(_bits(im.img), _bits(pix))


def _counting_source(raw):
    from milwrm_amd import stream

    class Counting(stream.HostSource):
        """Counts how often every row is delivered."""

        def __init__(self, a):
            super().__init__(a)
            self.rows = np.zeros(self.H, dtype=np.int64)

        def read(self, y0, y1, out):
            self.rows[y0:y1] += 1
            return super().read(y0, y1, out)

    return Counting(raw)


@pytest.mark.parametrize("band", HD.BANDS)
def test_source_rows_are_read_twice_or_once(gpu, monkeypatch, band):
    import milwrm_amd as M
    from milwrm_amd import stream

    _env(monkeypatch, True, band)
    raw, mask = HD.slide("u16", 3)
    src = _counting_source(raw)
    im = M.img.from_source(src, mask=mask.copy())
    _check(im.histogram(None, 100), [raw[:, :, c] for c in range(3)], 100)
    assert (src.rows == 2).all()  # the planes' extremes, then the counts
    src.rows[:] = 0
    _check(im.histogram(None, 100, range=(0, 65535)), [raw[:, :, c] for c in range(3)], 100, (0, 65535))
    assert (src.rows == 1).all()
    # a deferred Gaussian: every band is read with its halo rows, which are counted apart
    im.log_normalize(mean=np.full(3, 900.0))
    im.blurring("gaussian", sigma=2)
    assert im._pending_blur is not None and im._dev is None
    halo = stream.band_filter(im).halo
    cover = np.zeros(HD.H, dtype=np.int64)  # bands that read the row, as core or as halo
    for _, _, a, b in stream._plan(HD.H, int(band), halo, 0, HD.H):
        cover[a:b] += 1
    assert halo == 8 and cover.min() == 1 and cover.max() == 2
    src.rows[:] = 0
    one = im.histogram(None, 100, range=(0.0, 2.0))
    assert np.array_equal(src.rows, cover)  # core rows once, halo rows once more per neighbouring band
    src.rows[:] = 0
    two = im.histogram(None, 100)
    assert np.array_equal(src.rows, 2 * cover)
    pix = im.img
    _check(one, [pix[:, :, c] for c in range(3)], 100, (0.0, 2.0))
    _check(two, [pix[:, :, c] for c in range(3)], 100)


def test_band_heights_and_starts_of_a_resident_tensor(gpu):
    """stream.histogram over views of a resident tensor: bands start at any
    element (no 16-byte alignment) and any heights give the same counts."""
    from milwrm_amd import device as D
    from milwrm_amd import stream

    for kind, C in (("u8", 3), ("u16lo", 30), ("f32nan", 1), ("dom", 8)):
        raw, mask = HD.slide(kind, C)
        t = D.to_device_image(raw)
        m = torch.from_numpy(mask).to(t.device)
        whole = D.histogram(t, None, 100, None, m)
        _check(whole, [raw[:, :, c][mask != 0] for c in range(C)], 100)
        for rows in (1, 5, 29):
            got = stream.histogram(t, None, 100, None, m, band_rows=rows)
            assert np.array_equal(got[0], whole[0]) and np.array_equal(_bits(got[1]), _bits(whole[1]))


def test_errors(gpu, monkeypatch):
    import milwrm_amd as M
    from milwrm_amd import device as D

    _env(monkeypatch, False)
    raw, mask = HD.slide("f32", 3)
    bad = raw.copy()
    bad[:, :, 1] = np.nan
    with pytest.raises(ValueError, match="ch_1"):
        M.img(bad).histogram()
    with pytest.raises(ValueError, match="'ch_1'"):
        M.img(bad).histogram(("ch_2", "ch_1"))
    _check(M.img(bad).histogram((0, 2), 10), [bad[:, :, 0], bad[:, :, 2]], 10)  # the other planes are fine
    _check(M.img(bad).histogram(None, 10, range=(0, 1)), [bad[:, :, c] for c in range(3)], 10, (0, 1))
    bad = raw.copy()
    bad[5, 7, 2] = np.inf
    with pytest.raises(ValueError, match="ch_2"):
        M.img(bad).histogram()
    bad[5, 7, 2] = -np.inf
    with pytest.raises(ValueError, match="ch_2"):
        M.img(bad).histogram(2)
    _check(M.img(bad).histogram(2, 10, range=(-5, 5)), [bad[:, :, 2]], 10, (-5, 5))
    hidden = raw.copy()
    hidden[:9] = np.nan  # all of it under the mask's zero rows
    _check(M.img(hidden, mask=mask.copy()).histogram(None, 10, mask_out=True),
           [raw[:, :, c][mask != 0] for c in range(3)], 10)
    with pytest.raises(ValueError, match="mask"):
        M.img(raw.copy()).histogram(mask_out=True)
    with pytest.raises(NotImplementedError):
        M.img(raw.copy()).histogram(bins=D.HISTOGRAM_MAX_BINS + 1)
    _check(M.img(raw.copy()).histogram(0, D.HISTOGRAM_MAX_BINS), [raw[:, :, 0]], D.HISTOGRAM_MAX_BINS)


def test_plot_draws_the_device_counts(gpu, monkeypatch, tmp_path):
    import matplotlib.pyplot as plt

    _env(monkeypatch, False)
    im, raw, _ = _img("u16", 8)
    out = tmp_path / "hist.png"
    gs = im.plot_image_histogram(channels=[0, "ch_2"], save_to=str(out))
    assert (gs.nrows, gs.ncols) == (1, 2) and out.exists() and out.stat().st_size > 0
    for ax, ch, c in zip(gs.figure.axes, [0, "ch_2"], [0, 2]):
        counts, edges = im.histogram(ch, bins=100)
        assert np.array_equal(np.array([p.get_height() for p in ax.patches]), counts[0])
        assert np.array_equal(counts[0], HD.numpy_histogram(raw[:, :, c], 100)[0])
        assert ax.get_title() == str(ch)
    plt.close(gs.figure)
