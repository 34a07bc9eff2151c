"""CPU-only tests of the row-window median's host side: mw_median_rows refuses
a window the array cannot serve before any device call (the pointers here are
never dereferenced: every case returns before the launch), and the deferred
median's band filter asks for the halo the kernel needs."""
import pytest

from milwrm_amd import _native as N

IMG, OUT = 0x10000, 0x20000  # never dereferenced: every call below is refused before the launch


def _rows(H, row_off, slide_H, r0, r1, size, W=8, C=3, dtype=N.MW_U16, img=IMG, out=OUT):
    sy, sx = size
    st = N.load().mw_median_rows(img, dtype, H, W, C, row_off, slide_H, r0, r1, sy, sx, 0, None, 1.0, out, None)
    return st, N.last_error()


@pytest.mark.parametrize("size,hy,below", [((3, 3), 1, 1), ((4, 7), 2, 1), ((9, 9), 4, 4), ((2, 2), 1, 0),
                                           ((15, 1), 7, 7)])
def test_missing_halo_row_is_einval(size, hy, below):
    # rows [10, 30) of a 45-row slide: hy rows above r0 and `below` rows under r1 must be in the array
    st, msg = _rows(20, 10, 45, hy - 1, 20 - below, size)
    assert st == N._EINVAL and "above" in msg and "mw_median_rows" in msg
    if below:
        st, msg = _rows(20, 10, 45, hy, 20 - below + 1, size)
        assert st == N._EINVAL and "below" in msg
    # the array ends the slide: nothing is needed below, the top still is
    st, msg = _rows(20, 25, 45, hy - 1, 20, size)
    assert st == N._EINVAL and "above" in msg
    # the array starts the slide: nothing is needed above, the bottom still is
    if below:
        st, msg = _rows(20, 0, 45, 0, 20, size)
        assert st == N._EINVAL and "below" in msg


def test_other_arguments_as_mw_median():
    assert _rows(20, 10, 45, 5, 5, (3, 3))[0] == N._EINVAL       # r0 >= r1
    assert _rows(20, 10, 45, 1, 21, (3, 3))[0] == N._EINVAL      # r1 past the array
    assert _rows(20, -1, 45, 1, 19, (3, 3))[0] == N._EINVAL      # rows that are not rows of the slide
    assert _rows(20, 30, 45, 1, 19, (3, 3))[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, (0, 3))[0] == N._EINVAL      # size < 1
    assert _rows(20, 10, 45, 1, 19, (3, 3), dtype=7)[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, (3, 3), out=IMG)[0] == N._EINVAL  # aliased output
    assert _rows(20, 10, 45, 1, 19, (3, 3), img=None)[0] == N._EINVAL
    assert _rows(20, 10, 45, 8, 12, (16, 3))[0] == N._EUNSUP     # a size above 15: nothing launched
    assert _rows(20, 10, 45, 1, 19, (3, 16))[0] == N._EUNSUP


def test_median_band_halo_serves_the_kernel():
    """stream.bands hands a band its halo rows above and below (clipped to the
    slide); with MedianBand's halo every band passes the entry's check."""
    from milwrm_amd import stream

    for sy in range(1, 16):
        filt = stream.MedianBand((sy, 3))
        assert filt.halo == sy // 2
        for H, h in ((45, 1), (45, 7), (45, 45), (3, 1), (16, 16), (17, 16)):
            for y0, y1, a, b in stream._plan(H, h, filt.halo, 0, H):
                r0, r1 = y0 - a, y1 - a
                assert a == 0 or r0 >= sy // 2
                assert b == H or (b - a) - r1 >= sy - 1 - sy // 2
