"""``img.downsample(fact, func)`` and ``img.create_tissue_mask`` on the device,
resident and streamed in row bands (mw_block_reduce_rows, stream.downsample).

The reference is the numpy restatement of skimage's ``block_reduce(x, (f, f,
1), func, cval=0)`` in float64, cast to fp32, compared with
``assert_array_equal``: integer slides have exact fp64 sums, and the fp32
slides hold multiples of 1/8 below 2^20 in magnitude, whose fp64 sums are
exact in any order, so every func is exact.  A streamed slide is compared bit
for bit with the resident one."""
import numpy as np
import pytest
import torch

from oracle import milwrm_oracle as O
from tests.test_cpu_downsample import block_reduce_np

pytestmark = pytest.mark.gpu

H0, W0 = 150, 176  # no multiple of most facts
FUNCS = {"mean": np.mean, "sum": np.sum, "max": np.max, "min": np.min, "median": np.median}
FACTS = (1, 2, 3, 5, 16, 200)  # 200: one block
_SLIDES = {}
_REF = {}


def _slide(C, dtype):
    """(raw, mask) from the oracle's generator, as ``dtype``; computed once."""
    key = (C, np.dtype(dtype).name)
    if key not in _SLIDES:
        raw, mask = O.synth_slide(H0, W0, C, seed=40 + C)
        if dtype == np.uint8:
            raw = (raw % 251).astype(np.uint8)
        elif dtype == np.float32:
            # multiples of 1/8, |x| < 2^20, both signs; the last rows and columns all negative:
            # an edge block's max is then the pad's 0
            a = (raw.astype(np.int64) * 37 - 3000) / 8.0
            a[-6:] = -np.abs(a[-6:]) - 0.125
            a[:, -2:] = -np.abs(a[:, -2:]) - 0.125
            assert np.abs(a).max() < 2 ** 20 and (a > 0).any()
            raw = a.astype(np.float32)
            assert np.array_equal(raw.astype(np.float64), a)
        raw.setflags(write=False)
        mask.setflags(write=False)
        _SLIDES[key] = (raw, mask)
    return _SLIDES[key]


def _ref(C, dtype, f, name):
    """The restatement as fp32, computed once per case."""
    key = (C, np.dtype(dtype).name, f, name)
    if key not in _REF:
        _REF[key] = block_reduce_np(_slide(C, dtype)[0], f, FUNCS[name]).astype(np.float32)
    return _REF[key]


def _dev(a):
    from milwrm_amd import device as D

    a = np.array(a)  # (the cached slides are read-only)
    return D.to_device_image(a if a.ndim == 3 else a[:, :, None])


def _funcs_for(f):
    return [n for n in FUNCS if n != "median" or f <= 16]  # median: fact <= 16


# ------------------------------------------------- 1. funcs against numpy
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("C", [1, 7, 8, 50])
def test_funcs_equal_restatement(gpu, C, dtype):
    from milwrm_amd import device as D

    t = _dev(_slide(C, dtype)[0])
    for f in FACTS:
        for name in _funcs_for(f):
            got = D.block_reduce(t, f, FUNCS[name])
            assert got.dtype == torch.float32 and tuple(got.shape) == (-(-H0 // f), -(-W0 // f), C)
            np.testing.assert_array_equal(got.cpu().numpy(), _ref(C, dtype, f, name), err_msg=f"{name} f={f}")


def test_pad_takes_part(gpu):
    """An all-negative edge block: max 0 from the pad; median fact=3 at an
    edge block that is mostly pad zeros ranks them; fact=2 averages."""
    from milwrm_amd import device as D

    raw = _slide(7, np.float32)[0]
    t = _dev(raw)
    mx = D.block_reduce(t, 16, np.max).cpu().numpy()  # 150 = 9 * 16 + 6: the last block row is padded
    assert (raw[-6:] < 0).all() and (mx[-1] == 0).all() and (mx[:-1] > 0).any()
    md = D.block_reduce(t, 3, np.median).cpu().numpy()  # 176 = 58 * 3 + 2: 3 pad zeros of 9, all data < 0
    col = raw[:, -2:].astype(np.float64).reshape(50, 3, 2, -1)
    want = np.sort(np.concatenate([col.reshape(50, 6, -1), np.zeros((50, 3, 7))], axis=1), axis=1)[:, 4]
    np.testing.assert_array_equal(md[:, -1], want.astype(np.float32))
    ev = D.block_reduce(t, 2, np.median).cpu().numpy()
    b = np.sort(raw[:2, :2].astype(np.float64).reshape(4, -1), axis=0)
    np.testing.assert_array_equal(ev[0, 0], ((b[1] + b[2]) / 2).astype(np.float32))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_fact_larger_than_image(gpu, dtype):
    from milwrm_amd import device as D

    rng = np.random.default_rng(3)
    a = rng.integers(0, 200, size=(5, 7, 3)).astype(dtype)
    if dtype == np.float32:
        a = (a - 100) / 8
    t = _dev(a.astype(dtype))
    for f in (2, 4, 8, 16, 200):
        for name in _funcs_for(f):
            want = block_reduce_np(a, f, FUNCS[name]).astype(np.float32)
            np.testing.assert_array_equal(D.block_reduce(t, f, FUNCS[name]).cpu().numpy(), want,
                                          err_msg=f"{name} f={f}")


def test_nan_block(gpu):
    """A NaN makes its block NaN for all five funcs; the neighbours stay finite."""
    from milwrm_amd import device as D

    a = _slide(7, np.float32)[0].copy()
    a[10, 11, 2] = np.nan
    a[149, 175, 5] = np.nan  # in a padded corner block
    t = _dev(a)
    for f in (3, 4):
        for name, fn in FUNCS.items():
            got = D.block_reduce(t, f, fn).cpu().numpy()
            with np.errstate(invalid="ignore"):
                want = block_reduce_np(a, f, fn).astype(np.float32)
            bad = np.isnan(got)
            assert bad.sum() == 2 and bad[10 // f, 11 // f, 2] and bad[149 // f, 175 // f, 5], (name, f)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} f={f}")


def test_median_fact_limit_and_band_arguments(gpu):
    from milwrm_amd import device as D

    t = _dev(_slide(7, np.uint16)[0])
    with pytest.raises(NotImplementedError, match="median"):
        D.block_reduce(t, 17, np.median)
    assert D.block_reduce(t, 17, np.mean).shape == (9, 11, 7)
    out = torch.empty((50, 59, 7), dtype=torch.float32, device=t.device)
    with pytest.raises(ValueError, match="multiple of fact"):
        D.block_reduce_rows(t[4:10], 4, H0, 3, np.mean, out)  # the band does not start on a block row
    with pytest.raises(ValueError, match="multiple of fact"):
        D.block_reduce_rows(t[3:10], 3, H0, 3, np.mean, out)  # 7 rows that do not end the slide
    with pytest.raises(ValueError):
        D.block_reduce_rows(t[147:150], 150, H0, 3, np.mean, out)  # past the slide


# ------------------------------------------------- 2. mean keeps its bits
@pytest.mark.parametrize("f", [2, 3, 7])
def test_mean_keeps_block_mean_bits(gpu, f):
    from milwrm_amd import device as D

    g = torch.Generator().manual_seed(f)
    t = (torch.randn((H0, W0, 7), generator=g) * 1000.0).to(gpu)
    assert torch.equal(D.block_reduce(t, f, np.mean), D.block_mean(t, f))
    for dt in (np.uint16, np.uint8):
        u = _dev(_slide(8, dt)[0])
        assert torch.equal(D.block_reduce(u, f, np.mean), D.block_mean(u, f))


# ------------------------------------------------- 3. band invariance
def _refusing_source(raw):
    from milwrm_amd import stream

    class NoWhole(stream.HostSource):
        whole = 0

        def materialize(self):
            NoWhole.whole += 1
            raise AssertionError("the streamed slide was materialised whole")

    return NoWhole(raw.copy()), NoWhole


def _prepare(im, variant, raw):
    C = raw.shape[2]
    if variant == "gaussian":
        im.log_normalize(mean=raw.reshape(-1, C).mean(axis=0, dtype=np.float64))
        im.blurring("gaussian", sigma=2)
    elif variant == "median":
        im.blurring("median", size=3)
    elif variant == "lognorm":
        im.log_normalize(mean=raw.reshape(-1, C).mean(axis=0, dtype=np.float64))
    elif variant == "bilateral":
        im.log_normalize(mean=raw.reshape(-1, C).mean(axis=0, dtype=np.float64))
        im.blurring("bilateral", sigma=1, sigma_color=0.3, banded=True)


def _resident(monkeypatch, variant, name, f, C=8):
    """(pixels, mask) of the resident slide downsampled, once per case."""
    import milwrm_amd as M

    key = ("resident", variant, name, f, C)
    if key not in _REF:
        monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
        monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
        raw, mask = _slide(C, np.uint16)
        im = M.img(raw.copy(), mask=mask.copy())
        _prepare(im, variant, raw)
        assert im._source() is None
        im.downsample(f, FUNCS[name])
        _REF[key] = (im._dev.clone(), np.asarray(im.mask).copy())
    return _REF[key]


@pytest.mark.parametrize("name", list(FUNCS))
@pytest.mark.parametrize("variant", ["raw", "lognorm", "gaussian", "median", "bilateral"])
def test_streamed_equals_resident(gpu, monkeypatch, variant, name):
    import milwrm_amd as M
    from milwrm_amd import device as D

    raw, mask = _slide(8, np.uint16)
    for f in (2, 5):
        want, want_mask = _resident(monkeypatch, variant, name, f)
        if variant == "raw":  # (the resident raw slide against numpy once more, through img)
            np.testing.assert_array_equal(want.cpu().numpy(), _ref(8, np.uint16, f, name))
        for band in ("37", "5", "1"):
            monkeypatch.setenv("MW_STREAM_BAND_ROWS", band)
            src, cls = _refusing_source(raw)
            im = M.img.from_source(src, mask=mask.copy())
            _prepare(im, variant, raw)
            before = D.FUSED_USED["downsample_streamed"]
            im.downsample(f, FUNCS[name])
            assert D.FUSED_USED["downsample_streamed"] == before + 1
            assert cls.whole == 0
            assert im._dev.dtype == torch.float32 and im.shape == tuple(want.shape)
            assert torch.equal(im._dev, want), (variant, name, f, band)
            assert isinstance(im.mask, np.ndarray) and im.mask.dtype == np.float64
            np.testing.assert_array_equal(im.mask, want_mask)
            assert im._pending is None and not im._filter_deferred() and im._source() is None


# ------------------------------------------------- 4. shrunk bands
@pytest.mark.parametrize("variant", ["raw", "gaussian"])
def test_shrunk_bands_stay_on_block_rows(gpu, monkeypatch, variant):
    """HBM short on the first band buffer (stream.alloc_rows handing back 38
    rows, no multiple of fact = 4): the lowered bands still start on block
    rows and the result is the resident one."""
    import milwrm_amd as M
    from milwrm_amd import stream

    raw, mask = _slide(8, np.uint16)
    want, _ = _resident(monkeypatch, variant, "mean", 4)
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", str(H0))
    real = stream.alloc_rows
    calls = []

    def short(rows, row_shape, dtype, min_rows=1, dev=None):
        calls.append(rows)
        if len(calls) == 1:
            return real(38, row_shape, dtype, min_rows=1, dev=dev)
        return real(rows, row_shape, dtype, min_rows=min_rows, dev=dev)

    monkeypatch.setattr(stream, "alloc_rows", short)
    src, cls = _refusing_source(raw)
    im = M.img.from_source(src, mask=mask.copy())
    _prepare(im, variant, raw)
    im.downsample(4, np.mean)
    assert calls[0] > 38 and len(calls) >= 2 and cls.whole == 0  # (more was asked for than the 38 rows granted)
    assert torch.equal(im._dev, want)


# ------------------------------------------------- 5. the mask
@pytest.mark.parametrize("name", ["mean", "max"])
@pytest.mark.parametrize("kind", ["host", "device"])
def test_mask_through_the_same_func(gpu, monkeypatch, kind, name):
    import milwrm_amd as M
    from milwrm_amd.MxIF import _DeviceMask

    raw, mask = _slide(8, np.uint16)
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "37")
    for f in (2, 5):
        want = block_reduce_np(mask, f, FUNCS[name])[:, :, 0]
        assert 0 < np.count_nonzero(want) < want.size
        src, _ = _refusing_source(raw)
        m = torch.from_numpy(mask.copy()).to(gpu) if kind == "device" else mask.copy()
        im = M.img.from_source(src, mask=m)
        im.downsample(f, FUNCS[name])
        if kind == "device":  # stays in HBM, fp32
            assert isinstance(im.mask, _DeviceMask) and im.mask._t.is_cuda and im.mask._t.dtype == torch.float32
            assert im.mask.shape == want.shape and im.mask.dtype == np.float32
        else:
            assert isinstance(im.mask, np.ndarray) and im.mask.dtype == np.float64
        np.testing.assert_array_equal(np.asarray(im.mask), want.astype(np.float32))
        md = im._mask_device()
        assert md.dtype == torch.uint8 and tuple(md.shape) == want.shape
        np.testing.assert_array_equal(md.cpu().numpy(), (want != 0).astype(np.uint8))


# ------------------------------------------------- 6. streamed tissue mask
def test_streamed_tissue_mask_equals_resident(gpu, monkeypatch):
    import milwrm_amd as M

    raw, mask = _slide(8, np.uint16)
    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_STREAM_BAND_ROWS", raising=False)
    res = M.img(raw.copy(), mask=mask.copy())
    res.create_tissue_mask()
    assert res.mask.shape == (H0, W0) and 0 < res.mask.sum() < H0 * W0
    monkeypatch.setenv("MW_HBM_BUDGET", "1")
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "37")
    src, cls = _refusing_source(raw)
    im = M.img.from_source(src, mask=mask.copy())
    im.create_tissue_mask()
    assert cls.whole == 0
    np.testing.assert_array_equal(im.mask, res.mask)
    with pytest.raises(ValueError, match="features"):
        im.create_tissue_mask(features=[0, 1, 2])
    assert cls.whole == 0


# ------------------------------------------------- 7. a result that does not fit
def test_result_that_does_not_fit(gpu, monkeypatch):
    import milwrm_amd as M
    from milwrm_amd import stream

    raw, mask = _slide(8, np.uint16)
    src, _ = _refusing_source(raw)
    im = M.img.from_source(src, mask=mask.copy())
    monkeypatch.setattr(stream, "alloc_bytes", lambda dev=None: 1 << 20)
    with pytest.raises(MemoryError, match="larger fact"):
        im.downsample(2)
    assert im.shape == (H0, W0, 8) and im.mask.shape == (H0, W0)  # untouched
