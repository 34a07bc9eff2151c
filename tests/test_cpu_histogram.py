"""img.histogram / img.plot_image_histogram without a device: the host checks
of the arguments, the guard that keeps tests/test_gpu_histogram.py biting, and
the drawing half from monkeypatched counts."""
import matplotlib

matplotlib.use("Agg")

import numpy as np  # noqa: E402
import pytest  # noqa: E402

from milwrm_amd import MxIF  # noqa: E402
from milwrm_amd import device as D  # noqa: E402
from tests import histogram_data as HD  # noqa: E402


def test_histogram_args_accepts_valid_input():
    assert D.histogram_args(100) == (100, None)
    assert D.histogram_args(np.int64(1), (0, 255)) == (1, (0.0, 255.0))
    assert D.histogram_args(51, [np.float32(-1.5), 2]) == (51, (-1.5, 2.0))
    assert D.histogram_args(7, (3, 3)) == (7, (3.0, 3.0))  # an empty range is widened later, as numpy's
    assert D.histogram_args(D.HISTOGRAM_MAX_BINS) == (D.HISTOGRAM_MAX_BINS, None)


@pytest.mark.parametrize("bins", [0, -3, 2.5, "auto", True, None])
def test_histogram_args_rejects_bins(bins):
    with pytest.raises(ValueError):
        D.histogram_args(bins)


@pytest.mark.parametrize("rng", [(0, np.inf), (-np.inf, 1), (np.nan, 1), (0, np.nan), (2, 1), (1,), 5, "ab"])
def test_histogram_args_rejects_range(rng):
    with pytest.raises(ValueError):
        D.histogram_args(10, rng)


def test_histogram_args_bins_above_the_cap():
    with pytest.raises(NotImplementedError):
        D.histogram_args(D.HISTOGRAM_MAX_BINS + 1)


def test_histogram_edges_are_numpys():
    for lo, hi, bins in [(0, 255, 51), (-3.25, 17.5, 100), (7, 7, 4), (0, 65535, 1000)]:
        ref = np.histogram(np.array([lo, hi], dtype=np.float64), bins=bins, range=(lo, hi))[1]
        got = D.histogram_edges(float(lo), float(hi), bins)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), ref.view(np.uint64))


@pytest.mark.parametrize("kind,rng,bins", HD.EXPLICIT)
def test_explicit_pairs_need_the_edge_corrections(kind, rng, bins):
    """For every explicit (range, bins) pair of the GPU test the uncorrected
    index differs from numpy's bin for a value the slide holds in every plane:
    a kernel without the two corrections against the edge table fails there."""
    for C in HD.CHANNELS:
        raw, _ = HD.slide(kind, C)
        for c in range(C):
            vals = np.unique(raw[:, :, c])
            vals = vals[(vals >= rng[0]) & (vals <= rng[1])]
            assert (HD.naive_bins(vals, rng, bins) != HD.numpy_bins(vals, rng, bins)).any(), (kind, rng, bins, C, c)


def test_the_issues_values_change_their_bin():
    for rng, bins, vals in [((0, 255), 51, [155]), ((0, 100), 100, [29, 57, 58]), ((0, 49), 49, [1, 2, 4, 8]),
                            ((0, 1000), 100, [290, 570, 580])]:
        assert (HD.naive_bins(vals, rng, bins) != HD.numpy_bins(vals, rng, bins)).all(), (rng, bins)


def test_slides_are_what_the_gpu_test_expects():
    for kind in HD.KINDS:
        raw, mask = HD.slide(kind, 3)
        assert raw.shape == (HD.H, HD.W, 3) and mask.shape == (HD.H, HD.W)
        assert not mask[:9].any() and mask.any() and not mask[9:].all()
        again, _ = HD.slide(kind, 3)
        assert np.array_equal(raw, again, equal_nan=raw.dtype.kind == "f")
    for esize in (1, 2, 4):
        assert (HD.W * esize) % 16 and (HD.W * 3 * esize) % 16
    nan = np.isnan(HD.slide("f32nan", 8)[0]).mean()
    assert 0.01 < nan < 0.03 and (HD.slide("f32", 8)[0] < 0).any()
    dom = HD.slide("dom", 8)[0]
    assert 0.88 < (dom == 300).mean() < 0.92
    assert HD.slide("u16lo", 1)[0].max() == 1000 and np.unique(HD.slide("const", 8)[0]).size == 1


# ----------------------------------------------------------------- drawing

def _fake(monkeypatch, n_ch=6):
    """An img whose ``histogram`` returns seeded counts without a device."""
    im = MxIF.img(np.zeros((4, 5, n_ch), dtype=np.uint16))
    calls = []

    def histogram(self, channels=None, bins=100, range=None, mask_out=False):
        f = self._features(channels)
        assert len(f) == 1 and bins == 100
        calls.append((channels, range, mask_out))
        lo, hi = (0.0, 10.0 + f[0]) if range is None else range
        counts = np.random.default_rng(f[0]).integers(0, 1000, size=(1, bins)).astype(np.int64)
        return counts, np.linspace(lo, hi, bins + 1)[None]

    monkeypatch.setattr(MxIF.img, "histogram", histogram)
    return im, calls


@pytest.mark.parametrize("channels,shape", [([2], (1, 1)), ([0, "ch_3", 1, 5], (1, 4)), ([0, 1, "ch_2", 3, 4], (2, 4))])
def test_plot_draws_the_counts(monkeypatch, tmp_path, channels, shape):
    import matplotlib.pyplot as plt

    im, calls = _fake(monkeypatch)
    out = tmp_path / "hist.png"
    gs = im.plot_image_histogram(channels=channels, save_to=str(out))
    assert (gs.nrows, gs.ncols) == shape
    fig = gs.figure
    assert len(fig.axes) == len(channels) and [c[0] for c in calls] == channels
    for ax, ch in zip(fig.axes, channels):
        f = im._features(ch)[0]
        want = np.random.default_rng(f).integers(0, 1000, size=100)
        assert np.array_equal(np.array([p.get_height() for p in ax.patches]), want)
        assert np.allclose([p.get_x() for p in ax.patches], np.linspace(0.0, 10.0 + f, 101)[:-1])
        assert ax.get_title() == str(ch) and ax.title.get_fontweight() == "bold" and ax.title.get_fontsize() == 16
    assert out.exists() and out.stat().st_size > 0
    plt.close(fig)


def test_plot_passes_its_options_on(monkeypatch):
    import matplotlib.pyplot as plt

    im, calls = _fake(monkeypatch)
    gs = im.plot_image_histogram(channels=("ch_1",), ncols=2, range=(0.0, 50.0), mask_out=True, density=True,
                                 color="k")
    assert calls == [("ch_1", (0.0, 50.0), True)]
    ax = gs.figure.axes[0]
    heights = np.array([p.get_height() for p in ax.patches])
    want = np.random.default_rng(1).integers(0, 1000, size=100).astype(np.float64)
    assert np.allclose(heights, want / want.sum() / 0.5)  # density over bins 0.5 wide
    plt.close(gs.figure)


def test_plot_without_channels_still_raises():
    im = MxIF.img(np.zeros((4, 5, 2), dtype=np.uint16))
    for call in (MxIF.img.plot_image_histogram, im.plot_image_histogram, lambda: im.plot_image_histogram(ncols=2)):
        with pytest.raises(NotImplementedError) as e:
            call()
        msg = str(e.value).lower()
        assert "channels=" in msg and not any(w in msg for w in ("clip", "scale", "intensity"))
    with pytest.raises(NotImplementedError):
        MxIF.img.show()


def test_histogram_checks_before_any_device_call():
    """Host-only refusals of img.histogram (no device is touched)."""
    im = MxIF.img(np.zeros((4, 5, 2), dtype=np.uint16))
    with pytest.raises(ValueError):
        im.histogram(bins=0)
    with pytest.raises(ValueError):
        im.histogram(range=(3, 1))
    with pytest.raises(NotImplementedError):
        im.histogram(bins=D.HISTOGRAM_MAX_BINS + 1)
    with pytest.raises(IndexError):
        im.histogram(channels=[2])
    with pytest.raises(ValueError):
        im.histogram(mask_out=True)  # no mask
