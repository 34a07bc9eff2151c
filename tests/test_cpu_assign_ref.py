"""The label pass's checker bites (tests/assign_ref.py), without a GPU: a
numpy fp32 emulation of the kernel's arithmetic passes ``check_label_pass``
against the fp64 reference, and four emulations that are each wrong the way a
kernel instance could be are rejected.  Also the entry point's documented
limits (k <= 127, F <= C <= 64): refused before anything is launched."""
import numpy as np
import pytest
import torch

from tests.assign_ref import (check_label_pass, emulate_label_pass, kernel_inputs,
                              label_pass_reference)

H, W = 131, 97
SHAPES = [(30, 12), (16, 65)]
TIES = ((2, 9), (4, 6))


def _case(C, k, ties=()):
    rng = np.random.default_rng(C * 100 + k)
    img = rng.random((H, W, C), dtype=np.float32)
    mask = (rng.random((H, W)) < 0.85).astype(np.uint8)
    mu, inv = rng.uniform(0.3, 0.7, C), rng.uniform(1.5, 3.0, C)
    cen = rng.normal(0.0, 0.6, (k, C))
    for lo, hi in ties:
        cen[hi] = cen[lo]
    a, b, c = kernel_inputs(mu, inv, cen)
    feats = np.arange(C)
    ref = label_pass_reference(torch.from_numpy(img), feats, a, b, c)
    return img, feats, a, b, c, mask, ref


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: f"C{p[0]}k{p[1]}")
def case(request):
    return request.param, _case(*request.param)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: f"C{p[0]}k{p[1]}")
def tied_case(request):
    return request.param, _case(*request.param, ties=TIES)


def _check(case, ties=(), **broken):
    (C, k), (img, feats, a, b, c, mask, ref) = case
    lab, conf, dom = emulate_label_pass(img, feats, a, b, c, mask, **broken)
    return check_label_pass(lab, conf, dom, ref, mask, k, tie_pairs=ties)


def test_correct_emulation_passes(case):
    got = _check(case)
    assert got["conf_err"] <= 1e-6, got  # fp32 against fp64 on the same inputs: far inside the bound


def test_correct_emulation_passes_with_tied_centres(tied_case):
    _check(tied_case, ties=TIES)


def test_dropped_feature_pair_is_rejected(case):
    with pytest.raises(AssertionError):
        _check(case, drop_last_pair=True)


def test_second_smallest_within_the_winners_group_is_rejected(case):
    with pytest.raises(AssertionError, match="conf|confidence"):
        _check(case, second_in_group=True)


def test_ties_to_the_highest_index_are_rejected(tied_case):
    with pytest.raises(AssertionError, match="tied pixels"):
        _check(tied_case, ties=TIES, ties_to_highest=True)


def test_lost_count_is_rejected(case):
    with pytest.raises(AssertionError, match="dom counts"):
        _check(case, lose_one_count=True)


def test_reference_in_chunks_equals_one_chunk(case):
    _, (img, feats, a, b, c, mask, ref) = case
    again = label_pass_reference(torch.from_numpy(img), feats, a, b, c, chunk=1000)
    for r, g in zip(ref, again):
        assert torch.equal(torch.nan_to_num(r.double(), nan=-2.0), torch.nan_to_num(g.double(), nan=-2.0))


# ---- limits: refused before the launch (the pointers are never dereferenced)

P = [0x10000 * (i + 1) for i in range(9)]


def _assign(C, F, k, n=1000):
    from milwrm_amd import _native as N

    img, feat, a, b, cen, mask, lab, conf, ws = P
    st = N.load().mw_assign_conf(img, C, feat, F, a, b, cen, k, mask, n, lab, conf, ws, None)
    return st, N.last_error()


@pytest.mark.parametrize("C,F,k,limit", [(30, 30, 128, "k <= 127"), (65, 65, 8, "C <= 64"), (30, 31, 8, "F <= C")],
                         ids=["k128", "C65", "F_above_C"])
def test_limits_are_refused_with_the_limit_in_the_message(C, F, k, limit):
    from milwrm_amd import _native as N

    st, msg = _assign(C, F, k)
    assert st == N._EUNSUP and limit in msg and "mw_assign_conf" in msg
    with pytest.raises(NotImplementedError, match=limit):
        N.check(st, "mw_assign_conf")
