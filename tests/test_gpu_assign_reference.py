"""The label pass (``assign.assign_image``, mw_assign_conf) against a plain
fp64 reference over its whole documented range, k <= 127 and F <= C <= 64:
every CMAX (8, 16, 32, 52, 64) and KS (64, 128) instance, scalar-load and LDS
centres, XL, blocks of 4, 3, 2 and 1 waves ((64, 33) 3, (64, 64) 2, (64, 127)
and (8, 127) 1), and feature subsets (``s_ident == 0``).

Reference and checks: tests/assign_ref.py (the kernel's exact fp32 inputs
widened to fp64; labels equal outside near-ties of the reference, their share
<= 1e-3; |conf - cid| <= 1e-5; -1 / NaN exactly outside the mask; dom from the
pass's own maps, exactly).  tests/test_cpu_assign_ref.py shows that the checks
reject a wrong kernel.

Small image: 131 x 97 = 12 707 pixels = 199 tiles, the last of 35 pixels;
n C is no multiple of 4 for odd C (the scalar tail).  The mask is
pixel-granular at about 85 %; every pixel is finite (non-finite background
next to tissue at C < CMAX is the documented limitation of DESIGN.md §18).
Ring-size image: 1283 x 1031 with the "runs" mask of
tests/test_gpu_assign_bgskip.py, where every wave's look-ahead ring turns over.

Measured max |conf - cid| on an MI355X, per CMAX (bound 1e-5): see
DESIGN.md §6."""
import numpy as np
import pytest
import torch

from oracle import milwrm_oracle as O
from tests.assign_ref import check_label_pass, kernel_inputs, label_pass_reference
from tests.test_gpu_assign_bgskip import H as RH, W as RW, make_mask
from tests.test_gpu_parity import RTOL, _labels_match

pytestmark = pytest.mark.gpu

H, W = 131, 97
assert (H * W) % 64 == 35 and -(-H * W // 64) == 199

PAIRS = [(8, 2), (5, 8), (8, 9), (8, 127),
         (9, 8), (16, 12), (16, 65),
         (17, 8), (30, 8), (32, 8), (30, 9), (30, 20), (31, 64), (30, 65),
         (33, 8), (50, 8), (52, 8), (53, 8), (64, 8),
         (50, 20), (64, 33), (64, 64), (64, 127)]
RING = [(30, 65), (64, 33), (64, 127)]
RECORDS = [(64, 33), (64, 64), (64, 127)]
# name -> (C, feature channels, k): all with ident false
SUBSETS = {
    "C30F5k8": (30, [29, 0, 7, 3, 11], 8),
    "C16perm16k5": (16, [int(f) for f in np.random.default_rng(16).permutation(16)], 5),
    "C50F11k12": (50, [41, 3, 17, 49, 0, 22, 8, 30, 5, 44, 13], 12),
    "C64F63k70": (64, list(range(1, 64)), 70),
}
assert SUBSETS["C16perm16k5"][1] != list(range(16))


def _ids(p):
    return f"C{p[0]}k{p[1]}"


class Case:
    """One image, model and reference; the reference is computed once and not
    changed."""

    def __init__(self, dev, C, k, feats=None, ties=(), ring=False):
        seed = 1000 * C + k + (7 if feats is not None else 0)
        rng = np.random.default_rng(seed)
        self.C, self.k, self.ties = C, k, ties
        self.feats = np.arange(C) if feats is None else np.asarray(feats)
        F = len(self.feats)
        if ring:
            g = torch.Generator(device=dev).manual_seed(seed)
            self.img = torch.rand((RH, RW, C), generator=g, dtype=torch.float32, device=dev)
            mask = make_mask("runs")
        else:
            self.img = torch.from_numpy(rng.random((H, W, C), dtype=np.float32)).to(dev)
            mask = (rng.random((H, W)) < 0.85).astype(np.uint8)
        self.mask_np = mask
        self.mask = torch.from_numpy(mask).to(dev)
        self.mu = rng.uniform(0.3, 0.7, F)
        self.inv = rng.uniform(1.5, 3.0, F)
        self.centers = rng.normal(0.0, 0.6, (k, F))
        for lo, hi in ties:
            self.centers[hi] = self.centers[lo]
        self.a, self.b, self.c = kernel_inputs(self.mu, self.inv, self.centers)
        self.ref = tuple(r.cpu() for r in label_pass_reference(self.img, self.feats, self.a, self.b, self.c))

    def run(self):
        from milwrm_amd.assign import assign_image

        return assign_image(self.img, self.feats, self.mu, self.inv, self.centers, self.mask)

    def check(self, out, what):
        got = check_label_pass(*out, self.ref, self.mask_np, self.k, tie_pairs=self.ties)
        print(f"label pass {what}: C={self.C} F={len(self.feats)} k={self.k} "
              f"max|conf-cid|={got['conf_err']:.3g} near-tie share={got['near_share']:.3g} "
              f"excused={got['excused']}")
        return got


@pytest.fixture(scope="module")
def cases():
    made = {}
    yield made
    made.clear()


def _case(cases, dev, C, k):
    if (C, k) not in cases:
        cases[(C, k)] = Case(dev, C, k)
    return cases[(C, k)]


@pytest.mark.parametrize("C,k", PAIRS, ids=[_ids(p) for p in PAIRS])
def test_small_image_against_fp64_reference(gpu, cases, C, k):
    case = _case(cases, gpu, C, k)
    case.check(case.run(), "small")


@pytest.mark.parametrize("name", list(SUBSETS))
def test_feature_subsets_against_fp64_reference(gpu, name):
    C, feats, k = SUBSETS[name]
    case = Case(gpu, C, k, feats=feats)
    case.check(case.run(), "subset")


@pytest.mark.parametrize("C,k", RING, ids=[_ids(p) for p in RING])
def test_ring_size_image_against_fp64_reference(gpu, C, k):
    case = Case(gpu, C, k, ring=True)
    case.check(case.run(), "ring")


@pytest.mark.parametrize("C,k,ties", [(16, 12, ((2, 9), (4, 6))), (30, 8, ((4, 6),))], ids=["C16k12", "C30k8"])
def test_identical_centres_go_to_the_lower_index(gpu, C, k, ties):
    """Centres 2 = 9 and 4 = 6 (LDS centres), 4 = 6 (scalar-load XL): a pixel
    whose reference winner is one of a pair gets the lower index and the
    confidence 0.0 exactly (asserted apart from the near-tie rule, which would
    excuse them: check_label_pass, tie_pairs)."""
    case = Case(gpu, C, k, ties=ties)
    case.check(case.run(), "ties")


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("C,k", RECORDS, ids=[_ids(p) for p in RECORDS])
def test_tile_order_and_records_from_maps(gpu, cases, monkeypatch, C, k):
    """Blocks of 3, 2 and 1 waves: the block-row tile order (MW_ASSIGN_IL=0,
    read on every call) gives the bits of the interleaved default, and
    mw_domain_records + mw_assign_reduce on the pass's own maps give its dom
    bits (include/milwrm_amd.h: the same partition and order)."""
    from milwrm_amd import _native as N
    from milwrm_amd import device as D

    case = _case(cases, gpu, C, k)
    lab, conf, dom = case.run()
    monkeypatch.setenv("MW_ASSIGN_IL", "0")
    lab0, conf0, dom0 = case.run()
    monkeypatch.delenv("MW_ASSIGN_IL")
    assert torch.equal(_bits(lab), _bits(lab0)) and torch.equal(_bits(conf), _bits(conf0))
    assert torch.equal(_bits(dom), _bits(dom0))
    n = H * W
    ws = torch.empty(N.query("mw_assign_ws_bytes", n, k), dtype=torch.uint8, device=gpu)
    dom1 = torch.full_like(dom, -1.0)
    N.call("mw_domain_records", D.P(lab), D.P(conf), n, C, k, D.P(ws), D.stream())
    N.call("mw_assign_reduce", D.P(ws), n, k, D.P(dom1), D.stream())
    assert torch.equal(_bits(dom), _bits(dom1))


@pytest.mark.parametrize("feats", [None, SUBSETS["C30F5k8"][1]], ids=["all", "subset"])
def test_reference_and_pass_against_the_oracle(gpu, cases, feats):
    """(30, 8) once against the oracle the goldens pin (O.tissue_ids,
    O.confidence_mxif with the unrounded mu, scale and centres): the torch
    reference and the pass, by the project's near-tie rule and RTOL."""
    case = _case(cases, gpu, 30, 8) if feats is None else Case(gpu, 30, 8, feats=feats)
    img = case.img.cpu().numpy()
    fl = [int(f) for f in case.feats]
    tid = O.tissue_ids(img, case.mask_np, fl, case.centers, case.mu, 1.0 / case.inv)
    cid, _ = O.confidence_mxif(img, case.mask_np, fl, case.centers, case.mu, 1.0 / case.inv, tid)
    ok = case.mask_np != 0
    lab, conf, _ = case.run()
    rlab = case.ref[0].numpy().reshape(H, W).astype(np.float64)
    rcid = case.ref[1].numpy().reshape(H, W)
    rlab[~ok] = np.nan
    for what, l, c in (("reference", rlab, rcid), ("pass", lab.cpu().numpy().astype(np.float64), conf.cpu().numpy())):
        l = np.where(l < 0, np.nan, l)
        _labels_match(l, tid, cid)
        np.testing.assert_allclose(c[ok], cid[ok], rtol=RTOL, atol=RTOL, err_msg=what)
