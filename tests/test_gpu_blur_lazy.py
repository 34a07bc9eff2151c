"""The gaussian blur of a resident slide with a mask writes the rows the
labelling path can read and leaves the rest pending until something else reads
the image (mw_blur_rows_table / mw_blur_part, img._blur_rest).

A pixel is needed when its 64-aligned flat tile (p >> 6, p = y W + x) holds a
mask pixel; a blur workgroup (64 columns x 512 rows) blurs the hull [a, b) of
its rows that hold a needed pixel.  The oracle for the table is that
definition in numpy; the oracle for every blurred bit is the whole blur of the
parent path (mw_blur, the eager arm).

Shapes: H = 600 (row bands of 512 + 88 rows), W = 130 (column bands of 64, 64
and 2; 130 % 64 != 0, so flat tiles wrap over image rows), C = 6 and 30 (one
and two channel tiles), uint16 and float32 input with and without the
log-normalise, sigma = 2 (r = 8) and one case at sigma = 0.5 (r = 2)."""
import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 600, 130
BW, BH = 64, 512
NBX, NBY = -(-W // BW), -(-H // BH)
MASKS = ["top150", "edge508", "rect", "x0_pixel", "last_pixel", "empty", "full"]
SKIPPING = MASKS[:5]  # masks that leave rows out


def make_mask(name):
    m = np.zeros((H, W), np.uint8)
    if name == "top150":  # the tissue edge lies inside the first row band
        m[150:] = 1
    elif name == "edge508":  # the tissue edge is within r = 8 rows of the band edge at 512
        m[508:] = 1
    elif name == "rect":  # nothing in the third column band, nothing in the second row band
        m[100:400, 10:100] = 1
    elif name == "x0_pixel":  # its flat tile starts on the row above
        assert (300 * W) % 64 != 0
        m[300, 0] = 1
    elif name == "last_pixel":
        m[H - 1, W - 1] = 1
    elif name == "full":
        m[:] = 1
    elif name != "empty":
        raise KeyError(name)
    return m


def np_needed(mask):
    """H x W bool: the pixel's 64-aligned flat tile holds a mask pixel."""
    n = mask.size
    nt = -(-n // 64)
    pad = np.zeros(nt * 64, bool)
    pad[:n] = mask.reshape(-1) != 0
    return np.repeat(pad.reshape(nt, 64).any(axis=1), 64)[:n].reshape(mask.shape)


def np_hulls(mask):
    """([tiles, 2] int32 hulls, H x W bool of the pixels inside them)."""
    need = np_needed(mask)
    tab = np.zeros((NBY * NBX, 2), np.int32)
    inside = np.zeros(mask.shape, bool)
    for by in range(NBY):
        y0, y1 = by * BH, min(H, (by + 1) * BH)
        for bx in range(NBX):
            x0, x1 = bx * BW, min(W, (bx + 1) * BW)
            rows = np.nonzero(need[y0:y1, x0:x1].any(axis=1))[0]
            a, b = (y0, y0) if rows.size == 0 else (y0 + rows[0], y0 + rows[-1] + 1)
            tab[by * NBX + bx] = (a, b)
            inside[a:b, x0:x1] = True
    return tab, inside


def rows_left_out(tab):
    """Rows of all workgroups that the needed-rows launch does not blur."""
    left = 0
    for t, (a, b) in enumerate(np.asarray(tab)):
        by = t // NBX
        left += min(H, (by + 1) * BH) - by * BH - (int(b) - int(a))
    return left


def make_raw(dev, dtype, C):
    g = torch.Generator(device="cpu").manual_seed(7 * C + (dtype == torch.float32))
    if dtype == torch.float32:
        return (torch.rand((H, W, C), generator=g) * 900.0).to(dev)
    return torch.randint(0, 4000, (H, W, C), generator=g, dtype=torch.int16).to(dev)  # uint16 bits


_WHOLE = {}


def whole_blur(dev, dtype, C, logn, sigma):
    """(raw, inv_mean, the whole blur: mw_blur), once per configuration."""
    from milwrm_amd import device as D

    key = (dtype, C, logn, sigma)
    if key not in _WHOLE:
        raw = make_raw(dev, dtype, C)
        inv = (1.0 / torch.linspace(200.0, 600.0, C)).to(dev) if logn else None
        full = D.blur(raw, sigma, inv_mean=inv, pseudoval=1.0)
        assert bool(torch.isfinite(full).all())
        _WHOLE[key] = (raw, inv, full)
    return _WHOLE[key]


@pytest.mark.parametrize("name", MASKS)
def test_table_equals_the_numpy_hulls(gpu, name):
    from milwrm_amd import device as D

    mask = make_mask(name)
    want, _ = np_hulls(mask)
    got = D.blur_rows_table(torch.from_numpy(mask).to(gpu)).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert rows_left_out(got) == rows_left_out(want)
    if name in SKIPPING:
        assert rows_left_out(got) > 0
    else:  # every row of every workgroup, or none
        assert rows_left_out(got) == (H * NBX if name == "empty" else 0)


CONFIGS = [(torch.int16, 6, True, 2.0), (torch.int16, 30, True, 2.0), (torch.int16, 30, False, 2.0),
           (torch.float32, 6, False, 2.0), (torch.float32, 30, False, 2.0), (torch.float32, 30, True, 2.0),
           (torch.int16, 30, True, 0.5)]


@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("dtype,C,logn,sigma", CONFIGS,
                         ids=lambda v: str(v).replace("torch.", "") if not isinstance(v, bool) else ("logn" if v else "raw"))
def test_needed_rows_then_rest(gpu, dtype, C, logn, sigma, name):
    from milwrm_amd import device as D

    raw, inv, full = whole_blur(gpu, dtype, C, logn, sigma)
    mask = make_mask(name)
    need = torch.from_numpy(np_needed(mask)).to(gpu)
    inside = torch.from_numpy(np_hulls(mask)[1]).to(gpu)
    out = torch.full((H, W, C), float("nan"), dtype=torch.float32, device=gpu)
    got, rest = D.blur_needed(raw, sigma, torch.from_numpy(mask).to(gpu), inv_mean=inv, pseudoval=1.0, out=out)
    assert got is out and rest is not None
    assert torch.equal(out[need], full[need])
    assert torch.equal(out[inside], full[inside])
    assert bool(torch.isnan(out[~inside]).all())  # rows outside the hulls were not written
    if name in SKIPPING:
        assert int((~inside).sum()) > 0
    before = D.BLUR_REST_USED["rest"]
    D.blur_rest(out, rest)
    assert torch.equal(out, full)
    assert D.BLUR_REST_USED["rest"] == before + 1


def _image(dev, C, name, dtype=np.uint16, mask=True):
    import milwrm_amd as M

    rng = np.random.default_rng(31 * C + len(name))
    raw = rng.integers(0, 4000, size=(H, W, C)).astype(dtype)
    return M.img(raw, mask=make_mask(name).astype(np.float64) if mask else None), raw


def test_img_completes_once_when_read(gpu, monkeypatch):
    from milwrm_amd import device as D

    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_FUSED_BLUR", raising=False)
    mean = np.linspace(200.0, 600.0, 6)
    lazy, _ = _image(gpu, 6, "top150")
    eager, _ = _image(gpu, 6, "top150")
    for im, kw in ((lazy, {}), (eager, {"_eager": True})):
        im.log_normalize(mean=mean)
        im.blurring("gaussian", sigma=2, **kw)
    assert lazy._blur_rest is not None and eager._blur_rest is None
    assert lazy.shape == (H, W, 6) and lazy._blur_rest is not None  # metadata reads finish nothing
    before = D.BLUR_REST_USED["rest"]
    want = eager._dev
    assert D.BLUR_REST_USED["rest"] == before
    inside = torch.from_numpy(np_hulls(make_mask("top150"))[1]).to(gpu)
    assert torch.equal(lazy._needed_pixels()[inside], want[inside]) and lazy._blur_rest is not None
    assert torch.equal(lazy._dev, want)  # any other reader completes first
    assert lazy._blur_rest is None and D.BLUR_REST_USED["rest"] == before + 1
    assert torch.equal(lazy._dev, want) and D.BLUR_REST_USED["rest"] == before + 1
    np.testing.assert_array_equal(lazy.img, eager.img)


def test_second_transform_completes_first(gpu, monkeypatch):
    from milwrm_amd import device as D

    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_FUSED_BLUR", raising=False)
    ims = []
    for kw in ({}, {"_eager": True}):
        im, _ = _image(gpu, 6, "rect")
        im.log_normalize(mean=np.linspace(200.0, 600.0, 6))
        im.blurring("gaussian", sigma=2, **kw)
        ims.append(im)
    assert ims[0]._blur_rest is not None
    before = D.BLUR_REST_USED["rest"]
    for im in ims:
        im.blurring("gaussian", sigma=0.5, _eager=True)
    assert D.BLUR_REST_USED["rest"] == before + 1
    assert torch.equal(ims[0]._dev, ims[1]._dev)


def test_whole_blur_without_a_mask_or_off_the_matrix_core_kernel(gpu, monkeypatch):
    from milwrm_amd import device as D

    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_FUSED_BLUR", raising=False)
    before = D.BLUR_REST_USED["rest"]
    for C, mask in ((6, False), (7, True)):  # no mask; odd C (VALU / two-pass kernels)
        im, raw = _image(gpu, C, "top150", mask=mask)
        im.log_normalize(mean=np.linspace(200.0, 600.0, C), mask=mask)
        inv = im._pending[0]
        im.blurring("gaussian", sigma=2)
        assert im._blur_rest is None
        want = D.blur(torch.from_numpy(raw.view(np.int16)).to(gpu), 2.0, inv_mean=inv, pseudoval=1.0)
        assert torch.equal(im._dev, want)
    assert D.BLUR_REST_USED["rest"] == before


def _poisoned(fn):
    """D.blur_needed with every pixel outside the hulls overwritten with NaN,
    +Inf and 3e38 (as tests/test_gpu_assign_bgskip.py does for the label pass)."""
    def run(img, sigma, mask_u8, **kw):
        out, rest = fn(img, sigma, mask_u8, **kw)
        assert rest is not None
        inside = torch.from_numpy(np_hulls(mask_u8.cpu().numpy())[1]).to(out.device)
        bad = torch.tensor([float("nan"), float("inf"), 3e38], device=out.device)
        fill = bad[torch.arange(H * W, device=out.device) % 3].reshape(H, W, 1)
        out.copy_(torch.where(inside.unsqueeze(-1), out, fill.expand(H, W, out.shape[2])))
        return out, rest
    return run


def _cohort(dev, fkw):
    import milwrm_amd as M

    imgs = [_image(dev, 6, name)[0] for name in ("top150", "rect")]
    ests, pix = zip(*[im.calculate_non_zero_mean() for im in imgs])
    df = pd.DataFrame({"Img": imgs, "batch_names": ["b1", "b2"], "mean estimators": list(ests),
                       "pixels": list(pix)})
    lab = M.mxif_labeler(df)
    lab.prep_cluster_data(features=list(range(6)), sigma=2, fract=0.2, filter_kwargs=fkw)
    lab.label_tissue_regions(k=4, plot_out=False, random_state=18)
    lab.confidence_score_images()
    out = dict(cluster_data=lab.cluster_data.copy(), mean=lab.scaler.mean_, scale=lab.scaler.scale_,
               centers=lab.kmeans.cluster_centers_, n_iter=lab.kmeans.n_iter_,
               tid=[np.nan_to_num(t, nan=-1) for t in lab.tissue_IDs],
               cid=[np.nan_to_num(c, nan=-1) for c in lab.confidence_IDs],
               conf_df=lab.confidence_score_df.values)
    return imgs, out


def test_cohort_with_poisoned_rest_equals_the_eager_arm(gpu, monkeypatch):
    from milwrm_amd import device as D

    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_FUSED_BLUR", raising=False)
    eager_imgs, want = _cohort(gpu, {"_eager": True})
    assert all(im._blur_rest is None for im in eager_imgs)
    monkeypatch.setattr(D, "blur_needed", _poisoned(D.blur_needed))
    before = D.BLUR_REST_USED["rest"]
    imgs, got = _cohort(gpu, None)
    assert D.BLUR_REST_USED["rest"] == before  # gather and label pass left the rest pending
    assert all(im._blur_rest is not None for im in imgs)
    for key in ("cluster_data", "mean", "scale", "centers", "conf_df"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert got["n_iter"] == want["n_iter"]
    for key in ("tid", "cid"):
        for x, y in zip(got[key], want[key]):
            np.testing.assert_array_equal(x, y, err_msg=key)
    for n, (im, ref) in enumerate(zip(imgs, eager_imgs)):
        np.testing.assert_array_equal(im.img, ref.img)  # the completion overwrites the poison
        assert D.BLUR_REST_USED["rest"] == before + n + 1


def _pair(dev, name="top150"):
    """(partly blurred image, the eager arm's image) of the same slide."""
    out = []
    for kw in ({}, {"_eager": True}):
        im, _ = _image(dev, 6, name)
        im.log_normalize(mean=np.linspace(200.0, 600.0, 6))
        im.blurring("gaussian", sigma=2, **kw)
        out.append(im)
    assert out[0]._blur_rest is not None and out[1]._blur_rest is None
    return out


@pytest.mark.parametrize("op", ["downsample", "clip", "log_normalize", "copy", "mask"])
def test_other_readers_complete_first(gpu, monkeypatch, op):
    """Whatever reads or replaces the pixels of a partly blurred image, or its
    mask, completes it once and gives the eager arm's bits."""
    from milwrm_amd import device as D

    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_FUSED_BLUR", raising=False)
    lazy, eager = _pair(gpu)
    before = D.BLUR_REST_USED["rest"]
    got = []
    for im in (lazy, eager):
        if op == "downsample":
            im.downsample(4)
        elif op == "clip":
            im.clip()
        elif op == "log_normalize":  # a second transform, deferred: it completes when it applies
            im.log_normalize(mean=np.full(6, 0.5), pseudoval=4.0)
            assert (im is eager) or im._blur_rest is not None
            im._materialize()
        elif op == "copy":
            im = im.copy()
        else:
            im.mask = np.ones((H, W))
        assert im._blur_rest is None
        got.append(im._dev)
    assert D.BLUR_REST_USED["rest"] == before + 1
    assert torch.equal(got[0], got[1])
    assert lazy._blur_rest is None


def test_evicted_copy_is_blurred_whole_again(gpu, monkeypatch):
    """Eviction drops a partly blurred copy with its rest (nothing is
    completed); the redo from the raw slide gives the eager arm's bits."""
    from milwrm_amd import device as D
    from milwrm_amd.stream import RESIDENCY

    monkeypatch.delenv("MW_HBM_BUDGET", raising=False)
    monkeypatch.delenv("MW_FUSED_BLUR", raising=False)
    lazy, eager = _pair(gpu, "rect")
    # the budget counts the raw slide the rest keeps (2 bytes per element) next to the fp32 copy
    assert RESIDENCY._lru[id(lazy)][1] == H * W * 6 * (4 + 2)
    assert RESIDENCY._lru[id(eager)][1] == H * W * 6 * 4
    before = D.BLUR_REST_USED["rest"]
    lazy._evict()
    RESIDENCY.forget(lazy)
    assert lazy._dev_t is None and lazy._blur_rest is None and lazy._pending_blur is not None
    assert torch.equal(lazy._materialize(), eager._dev)
    assert D.BLUR_REST_USED["rest"] == before
