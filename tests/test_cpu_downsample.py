"""``img.downsample``'s host side (no GPU): the func table, the ``fact``
check, the row-quantum band plans that keep every streamed band on block
boundaries, and the numpy restatement of skimage's ``block_reduce`` that the
GPU tests compare against (checked here against the oracle's block mean)."""
import numpy as np
import pytest

from oracle import milwrm_oracle as O


def block_reduce_np(a, f, func):
    """skimage.measure.block_reduce(a, (f, f, 1), func, cval=0) in float64:
    zero pad at the bottom and right to multiples of ``f``, ``func`` over each
    f x f block (pad zeros included)."""
    a = np.asarray(a, dtype=np.float64)
    a = a if a.ndim == 3 else a[:, :, None]
    H, W, C = a.shape
    p = np.pad(a, [(0, (-H) % f), (0, (-W) % f), (0, 0)], mode="constant", constant_values=0)
    Ho, Wo = p.shape[0] // f, p.shape[1] // f
    with np.errstate(invalid="ignore"):
        return func(p.reshape(Ho, f, Wo, f, C), axis=(1, 3))


def test_func_table():
    from milwrm_amd import device as D

    assert D.reduce_func(np.mean) == "mean"
    assert D.reduce_func(np.sum) == "sum"
    assert D.reduce_func(np.max) == D.reduce_func(np.amax) == "max"
    assert D.reduce_func(np.min) == D.reduce_func(np.amin) == "min"
    assert D.reduce_func(np.median) == "median"
    assert D.reduce_func("median") == "median"
    assert set(D.REDUCE_CODES) == {"mean", "sum", "max", "min", "median"}
    assert sorted(D.REDUCE_CODES.values()) == [0, 1, 2, 3, 4]
    for bad in (np.std, lambda x, axis=None: x.mean(axis), None, "std", np.nanmean):
        with pytest.raises(NotImplementedError, match="np.median"):
            D.reduce_func(bad)


def test_fact_validation():
    from milwrm_amd import device as D

    assert D.reduce_fact(1) == 1 and D.reduce_fact(np.int64(7)) == 7
    for bad in (0, -2, 2.0, 2.5, "2", None, True):
        with pytest.raises(ValueError, match="fact"):
            D.reduce_fact(bad)


def test_downsample_rejects_before_any_device_call():
    """A bad func or fact is refused on the host: no device is needed."""
    import milwrm_amd as M

    im = M.img(np.zeros((6, 6, 2), dtype=np.uint16))
    with pytest.raises(NotImplementedError, match="np.mean"):
        im.downsample(2, np.std)
    with pytest.raises(NotImplementedError):
        im.downsample(2, lambda x, axis: x.mean(axis))
    for bad in (0, 1.5, -1):
        with pytest.raises(ValueError, match="fact"):
            im.downsample(bad)


def _old_plan(H, band_rows, halo, r0, r1):
    """stream._plan before it took a quantum."""
    plan = []
    for y0 in range(r0, r1, max(1, band_rows)):
        y1 = min(r1, y0 + band_rows)
        plan.append((y0, y1, max(0, y0 - halo), min(H, y1 + halo)))
    return plan


def test_plan_quantum_one_is_unchanged():
    from milwrm_amd import stream

    for H, band_rows, halo in [(301, 37, 8), (150, 150, 0), (150, 1, 3), (40, 64, 8), (1000, 333, 12), (7, 2, 0)]:
        for r0, r1 in [(0, H), (H // 3, H - 1)]:
            assert stream._plan(H, band_rows, halo, r0, r1) == _old_plan(H, band_rows, halo, r0, r1)
            assert stream._plan(H, band_rows, halo, r0, r1, 1) == _old_plan(H, band_rows, halo, r0, r1)


@pytest.mark.parametrize("f", [2, 3, 4, 5, 16, 200])
def test_plan_quantum_keeps_block_boundaries(f):
    from milwrm_amd import stream

    for H in (150, 149, 5, 301):
        for band_rows in (1, 5, 37, 40, 150, 1000):
            for halo in (0, 8):
                plan = stream._plan(H, band_rows, halo, 0, H, quantum=f)
                assert plan[0][0] == 0 and plan[-1][1] == H
                for i, (y0, y1, a, b) in enumerate(plan):
                    assert y0 % f == 0
                    assert y1 == H or (y1 - y0) % f == 0
                    assert (a, b) == (max(0, y0 - halo), min(H, y1 + halo))
                    if i:
                        assert y0 == plan[i - 1][1]  # the bands tile [0, H)
                assert all(y1 - y0 <= max(f, band_rows) for y0, y1, _, _ in plan)


def test_restatement_mean_is_the_oracle():
    raw, mask = O.synth_slide(37, 45, 3, seed=5)
    for f in (1, 2, 3, 5, 16, 50):
        np.testing.assert_array_equal(block_reduce_np(raw, f, np.mean), O.block_reduce_mean(raw, f))
        np.testing.assert_array_equal(block_reduce_np(mask, f, np.mean)[:, :, 0], O.block_reduce_mean(mask, f))


def test_restatement_pad_takes_part():
    a = -np.ones((3, 3, 1))
    assert block_reduce_np(a, 2, np.max).tolist() == [[[-1.0], [0.0]], [[0.0], [0.0]]]
    assert block_reduce_np(a, 2, np.min)[1, 1, 0] == -1.0
    assert block_reduce_np(a, 2, np.sum)[:, :, 0].tolist() == [[-4.0, -2.0], [-2.0, -1.0]]
    assert block_reduce_np(a, 2, np.median)[:, :, 0].tolist() == [[-1.0, -0.5], [-0.5, 0.0]]
    assert block_reduce_np(a, 2, np.mean)[1, 1, 0] == -0.25
