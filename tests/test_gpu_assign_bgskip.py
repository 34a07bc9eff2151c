"""The label pass does not read tiles that lie wholly outside the mask
(assign_kernel): labels, confidences and domain records are the
bits of a pass that reads every tile, for every mask, and the features of a
background pixel never reach an output.

Oracle: ``assign_image`` on the same image with an all-ones mask (no tile can
be skipped), masked on the host; the domain records from exact int64 sums of
rint(conf * 2^32).

Size: the launch is at most 1024 blocks of at most 4 waves (``assign_waves``
in csrc/kmeans.hip starts at 4 and only lowers it, the XL instances take 4),
tiles interleaved over all waves of the grid, so N_PIX gives every wave 5 or 6
tiles whatever the instance: the look-ahead ring turns over several times.
The width is odd (tiles straddle image rows), N_PIX % 64 = 21 (a partial last
tile) and N_PIX * C is no multiple of 4 for C = 30, 50 (the scalar tail)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 1283, 1031
N_PIX = H * W
TILE = 64
N_TILE = -(-N_PIX // TILE)
MAX_BLOCKS, MAX_WAVES = 1024, 4
assert N_PIX % TILE == 21 and N_TILE >= 5 * MAX_BLOCKS * MAX_WAVES

# (C, k): XL + SC | LDS centres, non-XL | SC, non-XL | CMAX 52, XL | CMAX 64
SHAPES = [(30, 8), (30, 12), (16, 8), (50, 8), (64, 8)]
MASKS = ["top_band", "runs", "all_bg", "all_tissue", "two_pixels", "tail_bg", "tail_in_behind_skip"]


def _tile_mask(tile_on):
    """Per-pixel uint8 mask from a per-tile 0/1 array."""
    return np.repeat(np.asarray(tile_on, dtype=np.uint8), TILE)[:N_PIX].copy()


def _run_tiles(seed):
    """Alternating runs of 1-4 background and 1-4 in-mask tiles.  A wave's
    tiles are 4096 (or fewer waves: a divisor of it) apart, so consecutive
    tiles of one ring slot are independent draws: every slot meets
    skip -> load and load -> skip."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 5, size=N_TILE)
    on = np.repeat(np.arange(N_TILE) & 1, lens)[:N_TILE]
    return on.astype(np.uint8)


def make_mask(name):
    if name == "top_band":  # 150 rows and 37 pixels of background: the boundary tile is mixed
        nbg = 150 * W + 37
        assert nbg % TILE
        m = np.ones(N_PIX, np.uint8)
        m[:nbg] = 0
    elif name == "runs":
        m = _tile_mask(_run_tiles(11))
    elif name == "all_bg":
        m = np.zeros(N_PIX, np.uint8)
    elif name == "all_tissue":
        m = np.ones(N_PIX, np.uint8)
    elif name == "two_pixels":  # lane 0 of one tile, lane 63 of another
        m = np.zeros(N_PIX, np.uint8)
        m[5000 * TILE] = 1
        m[9001 * TILE + 63] = 1
    elif name == "tail_bg":  # the partial last tile all background, the rest by runs
        on = _run_tiles(12)
        on[-1] = 0
        on[-2] = 1
        m = _tile_mask(on)
    elif name == "tail_in_behind_skip":
        # the partial last tile in the mask; the tile before it in its wave's
        # sequence (and in its ring slot, for one or two tiles in flight) skipped
        on = _run_tiles(13)
        on[-1] = 1
        for nw in (1, 2, 3, 4):
            for slots in (1, 2):
                on[N_TILE - 1 - slots * MAX_BLOCKS * nw] = 0
        m = _tile_mask(on)
    else:
        raise KeyError(name)
    return m.reshape(H, W)


def expected(full, mask, k):
    """(labels, confidences, dom) of the masked pass from the all-ones pass."""
    lab_f, conf_f, _ = full
    inm = mask != 0
    lab = torch.where(inm, lab_f, torch.full_like(lab_f, -1))
    conf = torch.where(inm, conf_f, torch.full_like(conf_f, float("nan")))
    # conf in [0, 1] fp32: conf * 2^32 is exact in fp64, round = rint (half to even)
    q = torch.round(conf_f.double() * 4294967296.0).to(torch.int64)[inm]
    lb = lab_f[inm].to(torch.int64)
    s = torch.zeros(k, dtype=torch.int64, device=lab.device).scatter_add_(0, lb, q)
    cnt = torch.bincount(lb, minlength=k)
    dom = torch.cat([s >> 32, s & 0xFFFFFFFF, cnt]).to(torch.float64)  # all < 2^53
    return lab, conf, dom


def assert_same(got, want):
    for g, w, what in zip(got, want, ("labels", "confidences", "dom")):
        if g.is_floating_point():
            assert torch.equal(torch.isnan(g), torch.isnan(w)), f"{what}: NaN positions"
            g, w = torch.nan_to_num(g, nan=-1.0), torch.nan_to_num(w, nan=-1.0)
        assert torch.equal(g, w), f"{what}: {int((g != w).sum())} entries differ"


class Case:
    """One (C, k): the image, the model and the all-ones pass, computed once."""

    def __init__(self, dev, C, k):
        g = torch.Generator(device=dev).manual_seed(1000 * C + k)
        self.C, self.k = C, k
        self.img = torch.rand((H, W, C), generator=g, dtype=torch.float32, device=dev)
        rng = np.random.default_rng(C * 100 + k)
        self.feats = np.arange(C)
        self.mu = rng.uniform(0.3, 0.7, C)
        self.inv = rng.uniform(1.5, 3.0, C)
        self.centers = rng.normal(0.0, 0.6, (k, C))
        self.full = self.run(torch.ones((H, W), dtype=torch.uint8, device=dev))
        assert not bool(torch.isnan(self.full[1]).any()) and int(self.full[0].min()) >= 0

    def run(self, mask, img=None):
        from milwrm_amd.assign import assign_image

        return assign_image(self.img if img is None else img, self.feats, self.mu, self.inv,
                            self.centers, mask)


@pytest.fixture(scope="module")
def cases():
    made = {}  # about 1 GB of images in all, dropped with the module
    yield made
    made.clear()


@pytest.fixture
def case(gpu, cases, request):
    C, k = request.param
    if (C, k) not in cases:
        cases[(C, k)] = Case(gpu, C, k)
    return cases[(C, k)]


@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("case", SHAPES, indirect=True, ids=lambda p: f"C{p[0]}k{p[1]}")
def test_masked_pass_equals_the_masked_full_pass(case, name):
    mask = torch.from_numpy(make_mask(name)).to(case.img.device)
    assert_same(case.run(mask), expected(case.full, mask, case.k))


@pytest.mark.parametrize("case", SHAPES, indirect=True, ids=lambda p: f"C{p[0]}k{p[1]}")
def test_background_features_do_not_matter(case):
    """Mask "runs" with every background pixel's features NaN, +Inf or 3e38:
    the outputs are those of the clean image."""
    mask = torch.from_numpy(make_mask("runs")).to(case.img.device)
    bad = torch.tensor([float("nan"), float("inf"), 3e38], device=mask.device)
    fill = bad[(torch.arange(N_PIX, device=mask.device) % 3)].reshape(H, W, 1)
    img = torch.where((mask != 0).unsqueeze(-1), case.img, fill.expand(H, W, case.C)).contiguous()
    assert_same(case.run(mask, img), expected(case.full, mask, case.k))


class _Identity:
    """A band filter that hands the fp32 rows through (no halo)."""
    halo = 0
    streamed = False

    def rows(self, raw, a, y0, y1, H, out_f32):
        return raw[y0 - a:y1 - a]


@pytest.mark.parametrize("case", [(30, 8)], indirect=True, ids=["C30k8"])
def test_banded_pass_equals_one_pass(case):
    """Bands of 100 rows over 150 rows + 37 pixels of background: the boundary
    at row 100 lies in the background, the others in tissue."""
    from milwrm_amd.assign import banded_assign_image

    mask = torch.from_numpy(make_mask("top_band")).to(case.img.device)
    got = banded_assign_image(case.img, _Identity(), case.feats, case.mu, case.inv, case.centers, mask,
                              band_rows=100)
    assert got is not None
    one = case.run(mask)
    assert_same(got, one)
    assert_same(one, expected(case.full, mask, case.k))


def test_fewer_tiles_than_waves(gpu):
    """100 x 37 pixels: 58 tiles for 15 blocks x 4 waves, the last one partial."""
    from milwrm_amd.assign import assign_image

    h, w, C, k = 100, 37, 30, 8
    g = torch.Generator(device="cpu").manual_seed(5)
    img = torch.rand((h, w, C), generator=g, dtype=torch.float32).to(gpu)
    rng = np.random.default_rng(5)
    mu, inv, cen = rng.uniform(0.3, 0.7, C), rng.uniform(1.5, 3.0, C), rng.normal(0.0, 0.6, (k, C))
    full = assign_image(img, np.arange(C), mu, inv, cen, torch.ones((h, w), dtype=torch.uint8, device=gpu))
    m = np.ones(h * w, np.uint8)
    on = rng.integers(0, 2, size=-(-h * w // TILE))
    m *= np.repeat(on.astype(np.uint8), TILE)[:h * w]
    m[7 * TILE + 5] = 1
    for last in (0, 1):
        m[(h * w // TILE) * TILE:] = last
        mask = torch.from_numpy(m.reshape(h, w).copy()).to(gpu)
        assert_same(assign_image(img, np.arange(C), mu, inv, cen, mask), expected(full, mask, k))
