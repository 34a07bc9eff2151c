"""An fp64 reference of the label pass (``assign.assign_image``) and the checks
that compare a pass with it.  A helper, not a test module: the GPU tests run
the kernels through it, tests/test_cpu_assign_ref.py runs a numpy fp32
emulation of the kernel (and four broken ones) through it.

The reference starts from the exact fp32 values the kernel receives (the
scaler as ``a = float32(inv)``, ``b = float32(-mu * inv)``, the centres
rounded to fp32, all built as ``assign_image`` builds them) widened to fp64,
so what is left between the two is the kernel's fp32 arithmetic alone:

    x'  = x[feats] * a + b
    d_j = sum_f (x'_f - c_jf)^2            (direct differences)
    label = argmin_j d_j                   (the lowest index on equal values)
    cid   = (d2 - d1) / d2                 (the two smallest distances)

Bounds.  ``TAU``: the project's near-tie rule (a label may differ where the
reference's relative top-2 gap is below it).  ``CONF_ATOL``: an fp32 distance
of F/2 packed pairs carries at most about (F/2 + 3) 2^-24 ~ 2e-6 relative
error at F = 64, and conf = 1 - d1/d2 moves by at most (d1/d2)(e1 + e2) <=
4e-6; 1e-5 absolute leaves a factor of two (the numpy fp32 emulation of
tests/test_cpu_assign_ref.py stays below 1e-6)."""
import numpy as np
import torch

TAU = 1e-5
NEAR_TIE_SHARE = 1e-3
CONF_ATOL = 1e-5
_TWO32 = 4294967296.0


def kernel_inputs(mu, inv, centers):
    """(a32, b32, c32): the scaler and the centres as ``assign_image`` hands
    them to the kernel."""
    mu = np.asarray(mu, dtype=np.float64)
    inv = np.asarray(inv, dtype=np.float64)
    return inv.astype(np.float32), (-mu * inv).astype(np.float32), np.asarray(centers, dtype=np.float32)


def label_pass_reference(img_f32, feats, a32, b32, c32, mask=None, chunk=65536):
    """Labels (int64, n), cid (fp64, n) and the relative top-2 gap (fp64, n:
    cid with 0 where both distances are 0) of every pixel of an HWC fp32
    image, in torch fp64 on the image's device, ``chunk`` pixels at a time.
    Every pixel is computed; ``mask`` (when given) only marks the pixels
    outside it: label -1, cid and gap NaN."""
    assert img_f32.dtype == torch.float32
    dev = img_f32.device
    C = img_f32.shape[-1]
    X = img_f32.reshape(-1, C)
    n = X.shape[0]
    ft = torch.as_tensor(np.asarray(feats, dtype=np.int64), device=dev)
    a = torch.as_tensor(np.asarray(a32, dtype=np.float32), device=dev).double()
    b = torch.as_tensor(np.asarray(b32, dtype=np.float32), device=dev).double()
    c = torch.as_tensor(np.asarray(c32, dtype=np.float32), device=dev).double()
    k = c.shape[0]
    lab = torch.empty(n, dtype=torch.int64, device=dev)
    cid = torch.empty(n, dtype=torch.float64, device=dev)
    gap = torch.empty(n, dtype=torch.float64, device=dev)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    for s in range(0, n, chunk):
        x = X[s:s + chunk].index_select(1, ft).double() * a + b
        m = x.shape[0]
        m1 = inf.expand(m).clone()
        m2 = inf.expand(m).clone()
        lb = torch.zeros(m, dtype=torch.int64, device=dev)
        for j in range(k):  # running top two: strict '<', so the lowest index keeps an equal value
            dd = ((x - c[j]) ** 2).sum(dim=1)
            win = dd < m1
            m2 = torch.where(win, m1, torch.minimum(m2, dd))
            lb = torch.where(win, torch.full_like(lb, j), lb)
            m1 = torch.where(win, dd, m1)
        lab[s:s + m] = lb
        cid[s:s + m] = (m2 - m1) / m2
        gap[s:s + m] = torch.where(m2 > 0, (m2 - m1) / m2, torch.zeros_like(m2))
    if mask is not None:
        out = torch.as_tensor(mask).reshape(-1).to(dev) == 0
        lab[out] = -1
        cid[out] = float("nan")
        gap[out] = float("nan")
    return lab, cid, gap


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def dom_from_maps(lab, conf, k):
    """The domain records [hi k | lo k | count k] of label / confidence maps:
    counts of the labels, and the exact integer sums of rint(conf * 2^32)
    (conf in [0, 1] fp32: the product is exact in fp64) as two 32-bit limbs."""
    lab = _np(lab).reshape(-1).astype(np.int64)
    conf = _np(conf).reshape(-1).astype(np.float64)
    inm = lab >= 0
    q = np.rint(conf[inm] * _TWO32).astype(np.int64)
    s = np.zeros(k, dtype=np.int64)
    np.add.at(s, lab[inm], q)
    cnt = np.bincount(lab[inm], minlength=k).astype(np.int64)
    return np.concatenate([s >> 32, s & 0xFFFFFFFF, cnt]).astype(np.float64)


def check_label_pass(lab, conf, dom, ref, mask, k, tie_pairs=(), conf_atol=CONF_ATOL):
    """Assert a label pass's (labels, confidences, dom) against
    ``label_pass_reference``'s ``ref`` under ``mask``.

    ``tie_pairs``: pairs (lo, hi) of identical centres.  A pixel whose
    reference winner belongs to a pair is an exact tie, which the near-tie
    rule would excuse: it is asserted on its own (the lower index, confidence
    exactly 0.0) and does not count as a near-tie.

    Returns the measured figures: max |conf - cid|, the near-tie share, the
    number of labels the near-tie rule excused."""
    lab = _np(lab).reshape(-1).astype(np.int64)
    conf = _np(conf).reshape(-1)
    assert conf.dtype == np.float32
    dom = _np(dom).astype(np.float64)
    rlab, rcid, rgap = (_np(r).reshape(-1) for r in ref)
    inm = _np(mask).reshape(-1) != 0
    n_in = int(inm.sum())
    assert lab.shape == rlab.shape == inm.shape and dom.shape == (3 * k,)

    # outside the mask, and only there: -1 / NaN
    assert np.array_equal(lab == -1, ~inm), "label -1 does not fall exactly on mask == 0"
    assert np.array_equal(np.isnan(conf), ~inm), "NaN confidence does not fall exactly on mask == 0"
    assert np.all((lab[inm] >= 0) & (lab[inm] < k))
    cin = conf[inm].astype(np.float64)
    assert np.all((cin >= 0.0) & (cin <= 1.0)), "confidence outside [0, 1] inside the mask"

    # exact ties of identical centres: the lower index, confidence exactly 0
    tied = np.zeros(lab.shape, dtype=bool)
    for lo, hi in tie_pairs:
        assert lo < hi
        t = inm & (rlab == lo)  # the reference gives an exact tie its lower index
        assert not np.any(inm & (rlab == hi)), "reference broke a tie upwards"
        assert t.any(), f"no pixel is won by the tied centres {lo}, {hi}"
        assert np.all(rgap[t] == 0.0)
        assert np.all(lab[t] == lo), f"{int((lab[t] != lo).sum())} tied pixels of ({lo}, {hi}) not labelled {lo}"
        assert np.all(conf[t] == 0.0), f"tied pixels of ({lo}, {hi}) with a confidence other than 0.0"
        tied |= t

    # near-ties, measured on the reference alone
    near = inm & ~tied & (rgap < TAU)
    share = float(near.sum()) / max(n_in, 1)
    assert share <= NEAR_TIE_SHARE, f"near-tie share {share:.3g} of the reference above {NEAR_TIE_SHARE}"
    wrong = inm & (lab != rlab)
    assert not np.any(wrong & ~near), f"{int((wrong & ~near).sum())} labels differ outside near-ties"

    err = float(np.max(np.abs(cin - rcid[inm]))) if n_in else 0.0
    assert err <= conf_atol, f"max |conf - cid| = {err:.3g} above {conf_atol}"

    # dom: the counts and the exact fixed-point sums of the pass's own maps
    want = dom_from_maps(lab, conf, k)
    assert np.array_equal(dom[2 * k:], want[2 * k:]), "dom counts are not the bincount of the labels"
    assert np.array_equal(dom[:2 * k], want[:2 * k]), "dom limbs are not the sum of rint(conf * 2^32)"
    return {"conf_err": err, "near_share": share, "excused": int((wrong & near).sum())}


# ---- a numpy fp32 emulation of the kernel's arithmetic (the CPU test's subject)

def _fma32(x, y, z):
    """fp32 fma: the product of two fp32 is exact in fp64; one fp64 rounding
    before the fp32 one (double rounding: rare, and within the checks' bounds)."""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def emulate_label_pass(img, feats, a32, b32, c32, mask, drop_last_pair=False, second_in_group=False,
                       ties_to_highest=False, lose_one_count=False):
    """(labels int8, conf fp32, dom fp64) as the kernel computes them: the
    scaled row by one fp32 fma, each centre's distance as two packed fma
    chains (even features, odd features, then their sum), a running strict
    top two, conf = (m2 - m1) / m2 in fp32, the exact fixed-point dom.  The
    keywords break it, one way each."""
    C = img.shape[-1]
    X = np.asarray(img, dtype=np.float32).reshape(-1, C)
    feats = np.asarray(feats)
    F = len(feats)
    k = c32.shape[0]
    n = X.shape[0]
    x = _fma32(X[:, feats], a32[None, :], b32[None, :])
    NP = (F + 1) // 2 - (1 if drop_last_pair else 0)
    d = np.empty((n, k), dtype=np.float32)
    for j in range(k):
        acc = [np.zeros(n, np.float32), np.zeros(n, np.float32)]
        for p in range(NP):
            for h in (0, 1):
                f = 2 * p + h
                if f < F:
                    df = x[:, f] - c32[j, f]
                    acc[h] = _fma32(df, df, acc[h])
        d[:, j] = acc[0] + acc[1]
    m1 = d.min(axis=1)
    if ties_to_highest:
        lab = k - 1 - np.argmin(d[:, ::-1], axis=1)
    else:
        lab = np.argmin(d, axis=1)
    rest = d.copy()
    rest[np.arange(n), lab] = np.inf
    if second_in_group:
        grp = (np.arange(k)[None, :] // 4) == (lab[:, None] // 4)
        rest[~grp] = np.inf
    m2 = rest.min(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        conf = ((m2 - m1) / m2).astype(np.float32)
    inm = np.asarray(mask).reshape(-1) != 0
    lab = np.where(inm, lab, -1).astype(np.int8)
    conf = np.where(inm, conf, np.float32(np.nan)).astype(np.float32)
    dom = dom_from_maps(lab, np.nan_to_num(conf, posinf=1.0), k)
    if lose_one_count:
        dom[2 * k + int(lab[inm][0])] -= 1
    return lab, conf, dom
