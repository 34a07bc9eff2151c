"""CPU-only tests of the row-window bilateral's host side: mw_bilateral_rows
refuses an array that lacks an in-slide tap row of a requested output row
before any device call (the pointers here are never dereferenced: every case
returns before the launch), and the deferred bilateral's band filter asks for
the halo the kernel needs."""
import pytest

from milwrm_amd import _native as N

IMG, OUT = 0x10000, 0x20000  # never dereferenced: every call below is refused before the launch


def _rows(H, row_off, slide_H, r0, r1, radius, W=8, C=3, dtype=N.MW_U16, img=IMG, out=OUT, sigma=1.0,
          sigma_color=0.3, mode=0, cval=0.0):
    st = N.load().mw_bilateral_rows(img, dtype, H, W, C, row_off, slide_H, r0, r1, radius, sigma, sigma_color,
                                    mode, cval, None, 1.0, out, None)
    return st, N.last_error()


@pytest.mark.parametrize("r", [1, 3, 6, 12])
def test_missing_halo_row_is_einval(r):
    # rows [30, 70) of a 100-row slide: r rows above r0 and r rows under r1 must be in the array
    st, msg = _rows(40, 30, 100, r - 1, 40 - r, r)
    assert st == N._EINVAL and "above" in msg and "mw_bilateral_rows" in msg
    st, msg = _rows(40, 30, 100, r, 40 - r + 1, r)
    assert st == N._EINVAL and "below" in msg and "mw_bilateral_rows" in msg
    # the array ends the slide: nothing is needed below, the top still is
    st, msg = _rows(40, 60, 100, r - 1, 40, r)
    assert st == N._EINVAL and "above" in msg
    # the array starts the slide: nothing is needed above, the bottom still is
    st, msg = _rows(40, 0, 100, 0, 40, r)
    assert st == N._EINVAL and "below" in msg


def test_other_arguments_as_mw_bilateral():
    assert _rows(20, 10, 45, 5, 5, 1)[0] == N._EINVAL       # r0 >= r1
    assert _rows(20, 10, 45, 6, 5, 1)[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 21, 1)[0] == N._EINVAL      # r1 past the array
    assert _rows(20, 10, 45, -1, 19, 1)[0] == N._EINVAL
    assert _rows(20, -1, 45, 1, 19, 1)[0] == N._EINVAL      # rows that are not rows of the slide
    assert _rows(20, 30, 45, 1, 19, 1)[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, 1, out=IMG)[0] == N._EINVAL  # aliased output
    assert _rows(20, 10, 45, 1, 19, 1, img=None)[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, 1, dtype=7)[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, 1, mode=2)[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, 1, sigma=0.0)[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, 1, sigma_color=float("nan"))[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, 1, cval=float("inf"))[0] == N._EINVAL
    assert _rows(20, 10, 45, 1, 19, -1)[0] == N._EINVAL
    st, msg = _rows(40, 10, 100, 13, 27, 13)                # radius 13: nothing launched
    assert st == N._EUNSUP and "mw_bilateral_rows" in msg
    assert _rows(20, 10, 45, 1, 19, 1, C=65)[0] == N._EUNSUP


def test_whole_slide_entry_keeps_its_name_in_messages():
    st = N.load().mw_bilateral(IMG, N.MW_U16, 20, 8, 3, 13, 1.0, 0.3, 0, 0.0, None, 1.0, OUT, None)
    assert st == N._EUNSUP and N.last_error().startswith("mw_bilateral:")
    st = N.load().mw_bilateral(IMG, 7, 20, 8, 3, 1, 1.0, 0.3, 0, 0.0, None, 1.0, OUT, None)
    assert st == N._EINVAL and N.last_error().startswith("mw_bilateral:")


def test_moments_rows_refuses_bad_arguments():
    lib = N.load()
    assert lib.mw_image_moments_rows_ws_bytes(100) >= 100 * 24
    assert lib.mw_image_moments_rows(IMG, N.MW_U16, 20, 8, 3, 30, 45, 0, None, 1.0, OUT, None) == N._EINVAL
    assert lib.mw_image_moments_rows(IMG, N.MW_U16, 20, 8, 3, -1, 45, 0, None, 1.0, OUT, None) == N._EINVAL
    assert lib.mw_image_moments_rows(IMG, N.MW_U16, 20, 8, 3, 10, 45, 2, None, 1.0, OUT, None) == N._EINVAL
    assert lib.mw_image_moments_rows(IMG, 7, 20, 8, 3, 10, 45, 0, None, 1.0, OUT, None) == N._EINVAL
    assert lib.mw_image_moments_rows(None, N.MW_U16, 20, 8, 3, 10, 45, 0, None, 1.0, OUT, None) == N._EINVAL
    assert lib.mw_image_moments_rows_final(0, 8, 3, 0, IMG, OUT, None) == N._EINVAL
    assert lib.mw_image_moments_rows_final(45, 8, 3, 0, None, OUT, None) == N._EINVAL


def test_bilateral_band_halo_serves_the_kernel():
    """stream.bands hands a band its halo rows above and below (clipped to the
    slide); with BilateralBand's halo every band passes the entry's check."""
    from milwrm_amd import stream

    for r in range(0, 13):
        filt = stream.BilateralBand((1.0, 0.3, 2 * r + 1, "constant", 0.0))
        assert filt.halo == r
        for H, h in ((45, 1), (45, 7), (45, 45), (3, 1), (8, 8), (9, 8)):
            plan = stream._plan(H, h, filt.halo, 0, H)
            assert [p[0] for p in plan] == list(range(0, H, h)) and plan[-1][1] == H
            for y0, y1, a, b in plan:
                r0, r1 = y0 - a, y1 - a
                assert 0 <= a and b <= H and 0 <= r0 < r1 <= b - a
                assert a == 0 or r0 >= r
                assert b == H or (b - a) - r1 >= r


def test_banded_is_a_keyword_of_the_filter_and_of_blurring():
    import inspect

    from milwrm_amd import MxIF

    assert inspect.signature(MxIF.img.bilateral_filter).parameters["banded"].default is False
