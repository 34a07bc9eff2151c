"""GPU tests of the banded CLAHE: stream.clahe gathers the
statistics band by band through mw_clahe_rows_* and stream.ClaheSource maps
each band.  Every reduction is an integer one and the map is mw_clahe's code,
so for every band height the tables equal D.clahe's and the oracle's exactly,
and the pixels equal them bit for bit (tests/clahe_oracle.py).  The slide is a
resident tensor cut into bands of 1, 5, 29 rows and whole: its bands are views
that start off the 16-byte grid."""
import numpy as np
import pytest
import torch

from tests import clahe_oracle as O
from tests.test_gpu_clahe import _same_bits, _slide, _upload

pytestmark = pytest.mark.gpu

BANDS = (1, 5, 29, None)


def _banded(t, band, ks, clip, nbins, enable=None):
    """(pixels, tables) of the slide tensor ``t`` equalised in bands of
    ``band`` rows: statistics and map, both cut the same way."""
    from milwrm_amd import device as D
    from milwrm_amd import stream

    src = stream.DeviceSource(t)
    H, W, C = src.shape
    state, luts = stream.clahe(src, ks, clip, nbins, enable=enable, band_rows=band, luts=True)
    eq = stream.ClaheSource(src, state)
    assert eq.dtype == torch.float32 and eq.shape == src.shape and not eq.zero_copy
    out = torch.empty((H, W, C), dtype=torch.float32, device=t.device)
    step = H if band is None else band
    for y0 in range(0, H, step):
        y1 = min(H, y0 + step)
        got = eq.read(y0, y1, out[y0:y1])
        assert got.data_ptr() == out[y0:y1].data_ptr()
    return D.d2h(out, luts)


@pytest.mark.parametrize("H,W,C,dtype,ks,clip,nbins", [
    (33, 53, 3, np.uint16, (8, 12), 0.01, 256),    # reflected rows of another tile row and of other bands; 318-byte rows
    (97, 90, 3, np.uint16, (48, 45), 0.01, 256),   # the staged map form, its cells cut by the bands
    (41, 45, 7, np.uint8, (6, 9), 0.02, 64),
    (45, 38, 5, np.float32, (13, 7), 0.02, 100),   # negative values
    (40, 40, 50, np.uint16, 5, 0.05, 100),         # channel-group rounds of the histogram pass
    (64, 80, 40, np.uint8, (40, 64), 0.01, 256),   # more than 7680 table entries: the 128 KB instance
    (33, 47, 1, np.uint8, (33, 47), 0.01, 256),    # one tile: every clamp active
])
def test_any_bands_equal_the_whole_image_and_the_oracle(H, W, C, dtype, ks, clip, nbins):
    """Fails on the parent commit: there is no stream.clahe."""
    from milwrm_amd import device as D

    a = _slide(H, W, C, dtype, seed=H * 1000 + W + 2)
    stats = {}
    ref, ref_luts = O.clahe(a, ks, clip, nbins, stats=stats)
    assert stats.get("loop_passes", 0) >= 1
    t = _upload(a)
    whole, whole_luts = D.clahe(t, ks, clip, nbins, luts=True)
    whole, whole_luts = D.d2h(whole, whole_luts)
    assert np.array_equal(whole_luts, ref_luts)
    _same_bits(whole, ref)
    for band in BANDS:
        got, luts = _banded(t, band, ks, clip, nbins)
        assert np.array_equal(luts, whole_luts), (band, np.argwhere(luts != whole_luts)[:8])
        _same_bits(got, whole)
        _same_bits(got, ref)
        assert got.min() == 0.0 and got.max() == 1.0


def test_fp32_band_mapped_in_place():
    """An fp32 band that is not a view of a resident slide is read into the
    output buffer and mapped there."""
    from milwrm_amd import device as D
    from milwrm_amd import stream

    a = _slide(45, 38, 5, np.float32, seed=45 * 1000 + 38 + 2)
    ref, _ = O.clahe(a, (13, 7), 0.02, 100)
    src = stream.HostSource(a)
    state = stream.clahe(src, (13, 7), 0.02, 100, band_rows=11)
    eq = stream.ClaheSource(src, state)
    out = torch.empty((45, 38, 5), dtype=torch.float32, device="cuda")
    before = D.CLAHE_USED["map_streamed"]
    for y0 in range(0, 45, 7):
        eq.read(y0, min(45, y0 + 7), out[y0:])
    assert D.CLAHE_USED["map_streamed"] == before + 7
    _same_bits(out.cpu().numpy(), ref)


def test_enabled_subset_with_a_constant_plane():
    a = _slide(33, 53, 4, np.uint16, seed=9)
    a[:, :, 1] = 777
    ref, ref_luts = O.clahe(a, (8, 12), channels=(1, 3))
    for band in BANDS:
        got, luts = _banded(_upload(a), band, (8, 12), 0.01, 256, enable=(1, 3))
        assert np.array_equal(luts, ref_luts) and not luts[0].any() and not luts[1].any() and not luts[2].any()
        _same_bits(got, ref)
        assert not got[:, :, 1].any()                                             # the constant plane: zeros
        assert np.array_equal(got[:, :, 0], a[:, :, 0].astype(np.float32))        # untouched: fp32 copies
        assert np.array_equal(got[:, :, 2], a[:, :, 2].astype(np.float32))
        assert got[:, :, 3].min() == 0.0 and got[:, :, 3].max() == 1.0


def test_two_rounds_stack():
    """A second round takes its statistics through the first round's source:
    the plane is equalised twice, as the resident rounds do."""
    from milwrm_amd import stream

    a = _slide(33, 53, 3, np.uint16, seed=8)
    ref, _ = O.clahe(a, (8, 12), channels=(1, 1))
    src = stream.DeviceSource(_upload(a))
    for _ in range(2):
        src = stream.ClaheSource(src, stream.clahe(src, (8, 12), enable=(1,), band_rows=5))
    out = torch.empty((33, 53, 3), dtype=torch.float32, device="cuda")
    for y0 in range(0, 33, 5):
        src.read(y0, min(33, y0 + 5), out[y0:])
    _same_bits(out.cpu().numpy(), ref)


def test_arguments_are_checked_before_any_launch():
    from milwrm_amd import device as D
    from milwrm_amd import stream

    t = _upload(_slide(33, 53, 3, np.uint16, seed=3))
    with pytest.raises(ValueError):
        stream.clahe(t, (34, 12))
    with pytest.raises(NotImplementedError):
        stream.clahe(t, (8, 12), nbins=257)
    st = D.ClaheRows(t.dtype, 33, 53, 3, (8, 12))
    with pytest.raises(ValueError, match="rows"):
        st.hist(t[30:33], 31)
    with pytest.raises(ValueError, match="band must be"):
        st.range(t[:, :, :2].contiguous())
    with pytest.raises(ValueError, match="finish"):
        st.map(t[:5], 0, torch.empty((5, 53, 3), dtype=torch.float32, device="cuda"))
