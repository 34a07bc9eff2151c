"""The exact selection fed in bands of rows (mw_quantiles_rows_*,
device.RowQuantiles): the record must be BITWISE ``D.quantiles`` of the whole
array -- the histograms are integer sums -- and, where numpy can say, the order
statistics of tests/test_gpu_intensity.py::_ref_record.  The bands are views of
the resident tensor, so with W * C odd (u8, u16) or not a multiple of 4 (fp32)
they start off a 16-byte boundary and in the middle of the kernel's vectors;
one case copies every band into a fresh (aligned) buffer instead."""
import numpy as np
import pytest
import torch

from milwrm_amd import device as D
from tests.test_gpu_intensity import _ref_record, _upload

pytestmark = pytest.mark.gpu

SPLITS = ("rows", "primes", "one", "last1", "first1")


def _heights(H, kind):
    if kind == "rows":
        return [1] * H
    if kind == "one" or H == 1:
        return [H]
    if kind == "last1":
        return [H - 1, 1]
    if kind == "first1":
        return [1, H - 1]
    out, y, i = [], 0, 0
    while y < H:  # prime-sized bands, 7 and 13 in turn
        h = min((7, 13)[i % 2], H - y)
        out.append(h)
        y += h
        i += 1
    return out


def _banded(t, kind, qs, pooled=False, skip=False, copy=False):
    sel = D.RowQuantiles(t.dtype, int(t.shape[2]), qs, pooled, skip)
    for _ in range(sel.passes):
        y = 0
        for h in _heights(int(t.shape[0]), kind):
            band = t[y:y + h]
            sel.count(band.clone() if copy else band)
            y += h
        assert y == t.shape[0]
        last = sel.choose()
    assert last
    return D.d2h(sel.out)


def _check(a, qs=(0.5, 99.5), pooled=False, skip=False, splits=SPLITS, copy=False, numpy_ref=True):
    t = _upload(a)
    whole = D.d2h(D.quantiles(t, qs, pooled=pooled, skip_sentinel=skip))
    if numpy_ref:
        ref = (_ref_record(a, qs, skip)[None] if pooled
               else np.stack([_ref_record(a[:, :, c], qs) for c in range(a.shape[2])]))
        assert np.array_equal(whole, ref, equal_nan=True)
    misaligned = 0
    for kind in splits:
        got = _banded(t, kind, qs, pooled, skip, copy)
        assert got.shape == whole.shape
        assert got.tobytes() == whole.tobytes(), (kind, np.argwhere(got != whole)[:8])
        row = a.shape[1] * a.shape[2] * a.itemsize
        misaligned += sum(1 for y in np.cumsum(_heights(a.shape[0], kind))[:-1] if (y * row) % 16)
    return misaligned


def test_u8_odd_sizes(gpu):
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, size=(31, 23, 5)).astype(np.uint8)  # W * C = 115 bytes a row
    assert _check(a) > 0
    _check(a, pooled=True, skip=True)


def test_u16_heavy_ties_odd_row(gpu):
    rng = np.random.default_rng(12)
    a = rng.integers(0, 65536, size=(31, 23, 5)).astype(np.uint16)  # W * C odd: every odd row is misaligned
    a[rng.uniform(size=a.shape) < 0.85] = 137  # a background value in 85 % of the elements
    assert _check(a) > 0
    _check(a, pooled=True, skip=True)


def test_u16_many_blocks_from_a_misaligned_row(gpu):
    """A band of 256 rows that starts at row 1 of a slide with W * C odd: more
    than one workgroup, and only the first vector of the first holds elements
    from before the band."""
    rng = np.random.default_rng(13)
    a = rng.integers(0, 65536, size=(257, 33, 5)).astype(np.uint16)
    a[:, :, 3] >>= 7
    assert _check(a, splits=("first1", "primes")) > 0


def _f32_hard():
    rng = np.random.default_rng(14)
    a = rng.normal(0, 5, size=(37, 39, 3)).astype(np.float32)  # W * C = 117 floats a row
    a[rng.uniform(size=a.shape) < 0.1] = 0.0
    a[rng.uniform(size=a.shape) < 0.1] = -0.0
    a[rng.uniform(size=a.shape) < 0.03] = np.nan
    a[:, :, 2] = np.nan  # an all-NaN channel
    a[3, 5, 0] = a[7, 7, 1] = a[36, 38, 1] = -99999.0
    return a


def test_f32_negatives_zeros_nans(gpu):
    a = _f32_hard()
    assert _check(a) > 0
    _check(a, pooled=True, skip=True)
    _check(a, pooled=True, skip=False)
    _check(a, qs=(0.0, 100.0))


@pytest.mark.parametrize("C,dtype", [(50, np.uint16), (60, np.uint16), (50, np.float32), (60, np.uint8)])
def test_many_channels(gpu, C, dtype):
    """50 channels, and 60: more than the 56 LDS tables of pass 1."""
    rng = np.random.default_rng(15 + C)
    if dtype == np.float32:
        a = rng.normal(0, 100, size=(29, 11, C)).astype(np.float32)
    else:
        a = rng.integers(0, np.iinfo(dtype).max + 1, size=(29, 11, C)).astype(dtype)
    _check(a, splits=("primes", "rows", "one"))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_three_percentiles_lds_prefixes(gpu, dtype):
    """nq = 3: six ranks a channel, the live prefixes in LDS."""
    rng = np.random.default_rng(16)
    if dtype == np.float32:
        a = rng.normal(0, 3, size=(31, 23, 5)).astype(np.float32)
    else:
        a = rng.integers(0, 65536, size=(31, 23, 5)).astype(np.uint16)
        a[:, :, 1] >>= 9
    assert _check(a, qs=(0.5, 50.0, 99.5)) > 0


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 2, 1)])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_tiny(gpu, shape, dtype):
    rng = np.random.default_rng(17)
    _check(rng.integers(1, 200, size=shape).astype(dtype))


def test_bands_copied_into_fresh_buffers(gpu):
    rng = np.random.default_rng(18)
    a = rng.integers(0, 65536, size=(31, 23, 5)).astype(np.uint16)
    _check(a, copy=True)
    _check(_f32_hard(), copy=True, pooled=True, skip=True)


def test_stream_quantiles_over_sources(gpu, monkeypatch):
    """stream.quantiles: a resident source is one band, a host source is read
    once per pass in bands of MW_STREAM_BAND_ROWS."""
    from milwrm_amd import stream

    rng = np.random.default_rng(19)
    a = rng.integers(0, 65536, size=(67, 23, 5)).astype(np.uint16)
    t = _upload(a)
    whole = D.d2h(D.quantiles(t, (0.5, 99.5)))
    assert D.d2h(stream.quantiles(t, (0.5, 99.5))).tobytes() == whole.tobytes()
    monkeypatch.setenv("MW_STREAM_BAND_ROWS", "13")
    before = D.INTENSITY_USED["select_streamed"]
    got = D.d2h(stream.quantiles(stream.HostSource(a), (0.5, 99.5)))
    assert got.tobytes() == whole.tobytes()
    assert D.INTENSITY_USED["select_streamed"] == before + 1


def test_bad_arguments_are_refused_before_any_launch(gpu):
    t = torch.zeros((4, 4, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        D.RowQuantiles(torch.float32, 3, tuple(range(9)))  # nq > 8
    with pytest.raises(ValueError):
        D.RowQuantiles(torch.float32, 3, (50.0, 101.0))
    with pytest.raises(NotImplementedError):
        D.RowQuantiles(torch.float32, 257, (50.0,))  # per-channel selection takes up to 256 channels
    D.RowQuantiles(torch.float32, 257, (50.0,), pooled=True)
    with pytest.raises(TypeError):
        D.RowQuantiles(torch.float64, 3, (50.0,))
    sel = D.RowQuantiles(torch.float32, 3, (50.0,))
    with pytest.raises(ValueError):
        sel.count(t.to(torch.uint8))  # another element type
    with pytest.raises(ValueError):
        sel.count(t[:, :, :2])  # another channel count
    with pytest.raises(ValueError):
        sel.count(t[:, ::2])  # not contiguous
    for _ in range(sel.passes):
        sel.count(t)
        sel.choose()
    with pytest.raises(ValueError):
        sel.count(t)
    with pytest.raises(ValueError):
        sel.choose()
    assert D.d2h(sel.out)[0, 0, 2] == 16
