"""Float64 numpy oracle of the project's CLAHE definition: the
published equalize_adapthist / _clahe procedure restated step by step.  It is
the specification evaluated literally, one plane at a time, slowly; nothing
here was checked against scikit-image, which is not installed."""
import math

import numpy as np

G = 16384  # grey levels of the quantised plane


def reflect(i, n):
    """Index ``i`` of an axis of ``n`` >= 2 samples reflected without repeating
    the edge (numpy's pad mode 'reflect')."""
    p = 2 * (n - 1)
    t = abs(int(i)) % p
    return p - t if t >= n else t


def kernel_of(kernel_size, H, W):
    if kernel_size is None:
        return max(H // 8, 1), max(W // 8, 1)
    if isinstance(kernel_size, (tuple, list)):
        kh, kw = kernel_size
        return int(kh), int(kw)
    return int(kernel_size), int(kernel_size)


def clip_hist(h, clim, stats=None):
    """Step 3, integer arithmetic on ``h`` (int64[nbins]) in place.  ``stats``
    (a dict) counts the passes of the sequential redistribution loop."""
    ex = h > clim
    n_ex = int(h[ex].sum() - ex.sum() * clim)
    h[ex] = clim
    incr = n_ex // h.size
    upper = clim - incr
    low = h < upper
    n_ex -= int(low.sum()) * incr
    h[low] += incr
    mid = (h >= upper) & (h < clim)  # after the increment above
    n_ex += int(h[mid].sum() - mid.sum() * clim)
    h[mid] = clim
    while n_ex > 0:
        if stats is not None:
            stats["loop_passes"] = stats.get("loop_passes", 0) + 1
        prev = n_ex
        for index in range(h.size):
            under = h < clim
            step = max(1, int(np.count_nonzero(under)) // n_ex)
            u = under[index::step]
            h[index::step][u] += 1
            n_ex -= int(np.count_nonzero(u))
            if n_ex <= 0:
                break
        if prev == n_ex:
            break
    return h


def tile_indices(n, k):
    """Source indices of the tiled axis: ceil(n / k) * k entries, tile t owns
    [t k, (t + 1) k), coordinates past the axis reflected."""
    nb = -(-n // k)
    return np.array([reflect(i, n) for i in range(nb * k)], dtype=np.int64)


def quantise(a, nbins):
    """Step 1: the bin of every sample of a float64 plane, or None when the
    plane is constant."""
    lo, hi = a.min(), a.max()
    if lo == hi:
        return None
    v = np.rint((a - lo) / (hi - lo) * (G - 1))
    return (v // (1 + G // nbins)).astype(np.int64)


def tile_hists(b, kh, kw, nbins):
    """Step 2: [nby, nbx, nbins] int64 counts."""
    H, W = b.shape
    ys, xs = tile_indices(H, kh), tile_indices(W, kw)
    t = b[np.ix_(ys, xs)]
    nby, nbx = ys.size // kh, xs.size // kw
    hist = np.zeros((nby, nbx, nbins), dtype=np.int64)
    for i in range(nby):
        for j in range(nbx):
            hist[i, j] = np.bincount(t[i * kh:(i + 1) * kh, j * kw:(j + 1) * kw].ravel(), minlength=nbins)
    return hist


def clahe_plane(a, kh, kw, clip_limit=0.01, nbins=256, stats=None):
    """Steps 1-6 of one plane: (float32 [H, W] pixels, int32 [nby, nbx, nbins]
    LUTs).  A constant plane gives zeros for both."""
    a = np.asarray(a, dtype=np.float64)
    H, W = a.shape
    nby, nbx = -(-H // kh), -(-W // kw)
    b = quantise(a, nbins)
    if b is None:
        return np.zeros((H, W), np.float32), np.zeros((nby, nbx, nbins), np.int32)
    hist = tile_hists(b, kh, kw, nbins)
    clim = int(max(clip_limit * kh * kw, 1.0))
    scale = (G - 1) / (kh * kw)
    luts = np.empty((nby, nbx, nbins), dtype=np.int64)
    for i in range(nby):
        for j in range(nbx):
            h = clip_hist(hist[i, j], clim, stats)
            luts[i, j] = np.minimum(np.cumsum(h).astype(np.float64) * scale, G - 1).astype(np.int64)
    py, px = np.arange(H) + kh // 2, np.arange(W) + kw // 2
    I, J = py // kh, px // kw
    ry, rx = (py % kh) / kh, (px % kw) / kw
    res = None
    for Ia, wy in ((I - 1, 1.0 - ry), (I, ry)):
        for Ja, wx in ((J - 1, 1.0 - rx), (J, rx)):
            m = luts[np.clip(Ia, 0, nby - 1)[:, None], np.clip(Ja, 0, nbx - 1)[None, :], b]
            term = (m.astype(np.float64) * (wy[:, None] * wx[None, :])).astype(np.float32)
            res = term if res is None else res + term  # float32 sum, in the defined order
    assert res.dtype == np.float32
    rmin, rmax = float(res.min()), float(res.max())
    if rmin == rmax:
        return np.zeros((H, W), np.float32), luts.astype(np.int32)
    out = ((res.astype(np.float64) - rmin) / (rmax - rmin)).astype(np.float32)
    return out, luts.astype(np.int32)


def clahe(image, kernel_size, clip_limit=0.01, nbins=256, channels=None, stats=None):
    """An H x W x C (or H x W) image: (float32 pixels of the image's shape,
    int32 [C, nby, nbx, nbins] LUTs).  Planes outside ``channels`` become the
    float32 conversion of their values and have zero LUTs."""
    a = np.asarray(image)
    a3 = a[:, :, None] if a.ndim == 2 else a
    H, W, C = a3.shape
    kh, kw = kernel_of(kernel_size, H, W)
    nby, nbx = math.ceil(H / kh), math.ceil(W / kw)
    out = a3.astype(np.float32)
    luts = np.zeros((C, nby, nbx, nbins), dtype=np.int32)
    done = set()
    for c in (range(C) if channels is None else channels):  # a plane listed twice is equalised twice
        src = out[:, :, c] if c in done else a3[:, :, c]
        out[:, :, c], luts[c] = clahe_plane(src, kh, kw, clip_limit, nbins, stats)
        done.add(c)
    return (out[:, :, 0] if a.ndim == 2 else out), luts
