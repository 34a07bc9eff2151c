"""GPU tests of the intensity utilities: the exact order-statistic selection
(D.quantiles) against np.sort, the rescale pass against a float64 numpy
evaluation rounded to float32 (the kernel's arithmetic is fp64 without
contraction, so equality is asserted), and img.clip / img.scale against numpy
and the reference's own outputs (tests/golden/intensity.npz)."""
import numpy as np
import pytest
import torch

from milwrm_amd import MxIF
from milwrm_amd import bands
from milwrm_amd import device as D

pytestmark = pytest.mark.gpu

QS = (0.0, 0.5, 50.0, 99.5, 100.0)
ULP1 = 2.0 ** -23  # one fp32 ulp at 1.0, the outputs' range


# ------------------------------------------------------------------ helpers
def _upload(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a).cuda()


def _ref_record(values, qs=QS, skip=False):
    """[nq, 4] reference of one channel: order statistics of rank floor(v) and
    min(floor(v) + 1, n - 1), the kept count and the NaN count."""
    v = np.asarray(values).reshape(-1)
    nan = np.isnan(v) if v.dtype.kind == "f" else np.zeros(v.shape, bool)
    keep = ~nan
    if skip:
        keep &= v != -99999
    s = np.sort(v[keep]).astype(np.float64)
    n = s.size
    out = np.empty((len(qs), 4))
    for i, q in enumerate(qs):
        if n:
            lo = int(np.floor(q / 100 * (n - 1)))
            out[i, :2] = s[lo], s[min(lo + 1, n - 1)]
        else:
            out[i, :2] = np.nan
        out[i, 2:] = n, nan.sum()
    return out


def _check_select(a, pooled=False, skip=False, qs=QS):
    got = D.d2h(D.quantiles(_upload(a), qs, pooled=pooled, skip_sentinel=skip))
    if pooled:
        ref = _ref_record(a, qs, skip)[None]
    else:
        ref = np.stack([_ref_record(a[:, :, c], qs) for c in range(a.shape[2])])
    assert got.shape == ref.shape
    # == on float64: bit equality but for the sign of a zero, which orders equal
    assert np.array_equal(got, ref, equal_nan=True), np.argwhere(~np.isclose(got, ref, rtol=0, atol=0,
                                                                              equal_nan=True))[:8]
    return got


def _u16_ties():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 65536, size=(64, 96, 5)).astype(np.uint16)
    a[:, :, 0] = 0
    a[:, :, 1] = 1234
    a[:, :, 2][rng.uniform(size=(64, 96)) < 0.5] = 0
    return a


def _f32_hard():
    """Negatives, both zeros, ~3 % NaNs; channel 1: ranks lo and lo + 1 of
    q = 0.5 differ in the top key byte (lo + 1 values in [1, 2), the rest in
    [2, 4))."""
    rng = np.random.default_rng(3)
    a = np.empty((40, 40, 2), dtype=np.float32)
    c0 = rng.normal(0, 5, size=1600).astype(np.float32)
    c0[rng.uniform(size=1600) < 0.1] = 0.0
    c0[rng.uniform(size=1600) < 0.1] = -0.0
    c0[rng.uniform(size=1600) < 0.03] = np.nan
    n_nan = 48
    n = 1600 - n_nan
    lo = int(np.floor(0.5 / 100 * (n - 1)))
    c1 = np.concatenate([rng.uniform(1, 2, size=lo + 1), rng.uniform(2, 4, size=n - lo - 1),
                         np.full(n_nan, np.nan)]).astype(np.float32)
    c1 = np.clip(c1, None, np.float32(3.999))
    assert (c1[:lo + 1] < 2).all() and (c1[lo + 1:n] >= 2).all()
    a[:, :, 0] = c0.reshape(40, 40)
    a[:, :, 1] = rng.permutation(c1).reshape(40, 40)
    return a


# ------------------------------------------------- order statistics, counts
def test_select_u8_odd_sizes(gpu):
    rng = np.random.default_rng(1)
    _check_select(rng.integers(0, 256, size=(13, 17, 3)).astype(np.uint8))


def test_select_u16_ties(gpu):
    _check_select(_u16_ties())


@pytest.mark.parametrize("shape", [(2, 2, 1), (1, 1, 1)])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_select_tiny(gpu, shape, dtype):
    rng = np.random.default_rng(4)
    _check_select((rng.integers(1, 200, size=shape)).astype(dtype))


def test_select_f32_fifty_channels(gpu):
    rng = np.random.default_rng(5)
    _check_select(rng.normal(0, 100, size=(33, 40, 50)).astype(np.float32))


def test_select_f32_negatives_zeros_nans_split_prefix(gpu):
    a = _f32_hard()
    got = _check_select(a)
    # the two ranks of q = 0.5 in channel 1 straddle [1, 2) | [2, 4)
    assert got[1, 1, 0] < 2.0 <= got[1, 1, 1]
    assert got[0, 0, 3] > 0 and got[1, 0, 3] == 48


def test_select_u16_many_blocks(gpu):
    rng = np.random.default_rng(6)
    a = rng.integers(0, 65536, size=(1024, 1024, 4)).astype(np.uint16)
    a[:, :, 3] >>= 7  # a channel that lives in two top-byte bins
    _check_select(a)
    _check_select(a, pooled=True, skip=True)


def test_select_pooled(gpu):
    _check_select(_u16_ties(), pooled=True, skip=True)
    a = _f32_hard()
    a[3, 5, 0] = a[7, 7, 1] = a[39, 39, 1] = -99999.0
    with_s = _check_select(a, pooled=True, skip=True)
    without = _check_select(a, pooled=True, skip=False)
    assert with_s[0, 0, 2] == without[0, 0, 2] - 3
    assert without[0, 0, 0] == -99999.0 and with_s[0, 0, 0] > -99999.0


def test_select_two_percentiles(gpu):
    """clip's and scale's lists: at most four live prefixes per channel, which
    later passes hold in registers."""
    for qs in ((0.5, 99.5), (0.0, 100.0), (50.0,)):
        _check_select(_u16_ties(), qs=qs)
        _check_select(_f32_hard(), qs=qs)
        _check_select(_f32_hard(), pooled=True, skip=True, qs=qs)


def test_select_more_channels_than_lds_tables(gpu):
    """More channels than a workgroup has tables: every pass walks its part of
    the image once per group of tables."""
    rng = np.random.default_rng(11)
    _check_select(rng.integers(0, 256, size=(9, 7, 70)).astype(np.uint8))
    _check_select(rng.integers(0, 65536, size=(6, 5, 200)).astype(np.uint16), qs=(0.5, 99.5))
    _check_select(rng.normal(size=(6, 5, 130)).astype(np.float32))


def test_select_all_nan_channel(gpu):
    a = np.ones((5, 7, 2), dtype=np.float32)
    a[:, :, 1] = np.nan
    got = _check_select(a)
    assert got[1, 0, 2] == 0 and got[1, 0, 3] == 35 and np.isnan(got[1, :, :2]).all()


def test_quantiles_bad_arguments(gpu):
    t = torch.zeros((4, 4, 2), dtype=torch.float32, device=gpu)
    for q in ([], list(range(9)), [101.0], [-1.0], [float("nan")]):
        with pytest.raises(ValueError):
            D.quantiles(t, q)


# ------------------------------------------------------------------ rescale
def _rescale_ref(a, params):
    x = a.astype(np.float64)
    out = np.empty(a.shape, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c, (lo, hi, omin, omax, mode) in enumerate(params):
            p = x[:, :, c]
            if mode == D.RESCALE_PASS:
                y = p
            elif mode == D.RESCALE_CLIP:
                y = (np.clip(p, lo, hi) - lo) / (hi - lo) * (omax - omin) + omin
            elif mode == D.RESCALE_FLAT:
                y = np.clip(p, omin, omax)
            else:
                y = (p - lo) / (hi - lo)
            out[:, :, c] = y.astype(np.float32)
    return out


_MODES = [(-3.7, 11.3, -1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0), (2.5, 2.5, 0.0, 1.0, 2.0),
          (-8.1, 13.9, 0.0, 1.0, 3.0), (1.3, 7.7, 0.0, 1.0, 1.0)]


def test_rescale_every_mode_f32(gpu):
    rng = np.random.default_rng(7)
    a = rng.normal(2, 6, size=(37, 29, 5)).astype(np.float32)
    a[rng.uniform(size=a.shape) < 0.02] = np.nan
    params = np.array(_MODES)
    ref = _rescale_ref(a, params)
    t = _upload(a)
    got = D.rescale(t, params).cpu().numpy()
    assert np.array_equal(got, ref, equal_nan=True)
    assert np.array_equal(np.isnan(got[:, :, [0, 1, 2, 4]]), np.isnan(a[:, :, [0, 1, 2, 4]]))
    assert got[:, :, 1].tobytes() == a[:, :, 1].tobytes()  # pass-through: the input's bits
    inplace = D.rescale(t, params, out=t)
    assert inplace is t and np.array_equal(t.cpu().numpy(), ref, equal_nan=True)


@pytest.mark.parametrize("dtype,shape", [(np.uint8, (13, 17, 3)), (np.uint16, (31, 23, 5))])
def test_rescale_integer_inputs(gpu, dtype, shape):
    rng = np.random.default_rng(8)
    a = rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    hi = float(np.iinfo(dtype).max) * 0.9
    params = np.array([(3.5, hi, 0.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0), (1.0, hi, 0.0, 1.0, 3.0),
                       (7.0, 7.0, 0.0, 1.0, 2.0), (0.25, 99.75, 0.0, 1.0, 1.0)][:shape[2]])
    got = D.rescale(_upload(a), params).cpu().numpy()
    assert np.array_equal(got, _rescale_ref(a, params))
    assert np.array_equal(got[:, :, 1], a[:, :, 1].astype(np.float32))  # exact conversion


def test_rescale_const_plane_scale_is_nan(gpu):
    a = np.full((6, 5, 1), 3.0, dtype=np.float32)
    got = D.rescale(_upload(a), np.array([(3.0, 3.0, 0.0, 1.0, 3.0)])).cpu().numpy()
    assert np.isnan(got).all()


# -------------------------------------------------- public API, the golden
def _pct(plane, pooled=False):
    p = np.asarray(plane, dtype=np.float64)
    if pooled:
        p = p[p != -99999]
    return np.nanpercentile(p, q=(0.5, 99.5))


def _clip_ref(x64, channels):
    """clip_values on a float64 image, its rescale evaluated in float64 and
    rounded to float32; also the (vmin, vmax) pairs used."""
    out = x64.astype(np.float32)
    pairs = {}
    planes = [None] if channels is None else list(channels)
    for c in planes:
        p = x64 if c is None else x64[:, :, c]
        vmin, vmax = _pct(p, pooled=c is None)
        pairs[c] = (vmin, vmax)
        omin = 0.0 if vmin >= 0 else -1.0
        y = ((np.clip(p, vmin, vmax) - vmin) / (vmax - vmin) * (1.0 - omin) + omin).astype(np.float32)
        if c is None:
            out = y
        else:
            out[:, :, c] = y
    return out, pairs


def _scale_ref(x64, channels):
    out = x64.astype(np.float32)
    if channels is None:
        return ((x64 - x64.min()) / (x64.max() - x64.min())).astype(np.float32)
    for c in channels:
        p = x64[:, :, c]
        out[:, :, c] = ((p - p.min()) / (p.max() - p.min())).astype(np.float32)
    return out


CASES = [("clip", "clip", None), ("clip02", "clip", (0, 2)), ("scale", "scale", None),
         ("scale1", "scale", (1,))]


def _run(im, op, channels):
    getattr(im, op)(**({} if channels is None else dict(channels=channels)))
    assert im._dev.dtype == torch.float32 and im._xbound is None and im._lognorm_host is None
    return im._dev.cpu().numpy()


@pytest.mark.parametrize("tag,op,channels", CASES)
def test_public_api_raw_u16(gpu, golden, tag, op, channels):
    g = golden("intensity")
    raw = g["raw"]
    got = _run(MxIF.img(raw.copy(), mask=g["mask"].copy()), op, channels)
    x64 = raw.astype(np.float64)
    ref = (_clip_ref(x64, channels)[0] if op == "clip" else _scale_ref(x64, channels))
    assert np.array_equal(got, ref)  # fp64 route: the float64 evaluation's float32 rounding
    gold = g["raw_" + tag]
    done = list(range(4)) if channels is None else list(channels)
    assert np.abs(got[:, :, done].astype(np.float64) - gold[:, :, done].astype(np.float64)).max() <= ULP1
    if channels is not None:  # unlisted channels: the exact conversion of the raw values
        rest = [c for c in range(4) if c not in channels]
        assert np.array_equal(got[:, :, rest], raw[:, :, rest].astype(np.float32))
        assert np.array_equal(got[:, :, rest], gold[:, :, rest])
    if op == "clip":  # vmin / vmax from the device's order statistics: numpy's bits
        t = _upload(raw)
        pooled = channels is None
        st = D.d2h(D.quantiles(t, (0.5, 99.5), pooled=pooled, skip_sentinel=pooled))
        for c in ([0] if pooled else channels):
            want = _pct(x64 if pooled else x64[:, :, c], pooled)
            have = [MxIF._lerp_quantile(st[c, i, 0], st[c, i, 1], st[c, i, 2], q) for i, q in enumerate((0.5, 99.5))]
            assert np.array(have).tobytes() == np.asarray(want, dtype=np.float64).tobytes()


@pytest.mark.parametrize("tag,op,channels", CASES)
def test_public_api_float(gpu, golden, tag, op, channels):
    g = golden("intensity")
    f32 = g["flt"].astype(np.float32)  # what the device holds
    got = _run(MxIF.img(f32.copy(), mask=g["mask"].copy()), op, channels)
    x64 = f32.astype(np.float64)
    ref = (_clip_ref(x64, channels)[0] if op == "clip" else _scale_ref(x64, channels))
    assert np.array_equal(got, ref)
    gold = g["flt_" + tag].astype(np.float64)
    keep = np.abs(gold) > 1e-3
    assert (~keep).mean() <= 0.01
    rel = np.abs(got.astype(np.float64) - gold)[keep] / np.abs(gold)[keep]
    assert rel.max() <= 1e-4, rel.max()


def test_module_functions_dtypes(gpu, golden):
    g = golden("intensity")
    raw = g["raw"]
    a = MxIF.clip_values(raw)
    assert a.dtype == np.float32 and np.array_equal(a, _clip_ref(raw.astype(np.float64), None)[0])
    b = MxIF.clip_values(raw, channels=(0, 2))
    assert b.dtype == np.float64 and np.array_equal(b, _clip_ref(raw.astype(np.float64), (0, 2))[0])
    c = MxIF.scale_rgb(raw, channels=(1,))
    assert c.dtype == np.float64 and np.array_equal(c, _scale_ref(raw.astype(np.float64), (1,)))
    d = MxIF.clip_values(raw[:, :, 1], channels=(0,))  # a 2-D image: the pooled branch
    assert d.dtype == np.float32 and d.shape == raw.shape[:2]
    assert np.array_equal(d, _clip_ref(raw[:, :, 1:2].astype(np.float64), None)[0][:, :, 0])


def test_deferred_lognorm_then_clip_equals_materialised(gpu, golden):
    g = golden("intensity")
    ims = [MxIF.img(g["raw"].copy(), mask=g["mask"].copy()) for _ in range(2)]
    for im in ims:
        im.log_normalize()
    assert ims[0]._pending is not None
    _ = ims[1].img  # materialises the log-normalise
    assert ims[1]._pending is None
    for im in ims:
        im.clip()
    assert ims[0]._pending is None and torch.equal(ims[0]._dev, ims[1]._dev)


def test_scale_plane_with_a_nan(gpu):
    rng = np.random.default_rng(9)
    a = rng.uniform(1, 5, size=(9, 11, 3)).astype(np.float32)
    a[4, 4, 1] = np.nan
    im = MxIF.img(a.copy())
    im.scale(channels=(1, 2))
    got = im._dev.cpu().numpy()
    assert np.isnan(got[:, :, 1]).all()
    assert np.array_equal(got[:, :, [0, 2]], _scale_ref(a.astype(np.float64), (2,))[:, :, [0, 2]])
    im = MxIF.img(a.copy())
    im.scale()
    assert np.isnan(im._dev.cpu().numpy()).all()


def test_clip_keeps_nans_and_leaves_out_sentinel(gpu):
    rng = np.random.default_rng(10)
    a = rng.uniform(-2, 9, size=(21, 19, 2)).astype(np.float32)
    a[rng.uniform(size=a.shape) < 0.05] = np.nan
    a[0, 0, 0] = a[5, 6, 1] = -99999.0
    im = MxIF.img(a.copy())
    im.clip()
    got = im._dev.cpu().numpy()
    assert np.array_equal(got, _clip_ref(a.astype(np.float64), None)[0], equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(a)) and got[0, 0, 0] == -1.0


def test_channel_listed_twice_is_processed_twice(gpu, golden):
    """The reference's loop clips a plane once per listing."""
    raw = golden("intensity")["raw"]
    twice = MxIF.img(raw.copy())
    twice.clip(channels=(1, 1))
    seq = MxIF.img(raw.copy())
    seq.clip(channels=(1,))
    seq.clip(channels=(1,))
    assert torch.equal(twice._dev, seq._dev)
    once = MxIF.img(raw.copy())
    once.clip(channels=(1,))
    assert not torch.equal(twice._dev, once._dev)


def test_clip_on_a_band_raises(gpu, golden):
    g = golden("intensity")
    im = bands.band_image(g["raw"], g["mask"], 0, 2)
    with pytest.raises(NotImplementedError):
        im.clip()
    with pytest.raises(NotImplementedError):
        im.scale(channels=(0,))
