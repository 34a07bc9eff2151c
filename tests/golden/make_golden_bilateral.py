"""Regenerate tests/golden/bilateral.npz: a float64 brute force of the bilateral
filter as this project defines it, self-contained numpy.

For output pixel (y, x) and every tap (dy, dx) in [-r, r]^2, r = (win_size - 1)
// 2, win_size = max(5, 2 ceil(3 sigma) + 1) by default: q = a[y + dy, x + dx, :]
(outside the image: cval in every channel in mode 'constant', the pixel at the
clamped coordinates in mode 'edge'), w = exp(-((dy^2 + dx^2) / sigma^2 + |q -
a[y, x, :]|^2 / sigma_color^2) / 2), out = sum w q / sum w.

Inputs: piecewise-constant domains (blocks of 7 px -- of half the shorter side
where the image is smaller than two blocks --, a level per block and channel
in [0.05, 1.2]) plus Gaussian noise of sd 0.03, clipped at 0, fp32;
sigma_color is the image's float64 standard deviation.  (Uniform noise is not
usable: with 30 channels of it the filter moves no pixel by more than 2e-5, and
a kernel that returned its input would pass.)

Per case the fixture holds the input, sigma_color, for every (mode, cval)
variant ``e32`` = the largest error of the same formula evaluated in numpy
float32 against the float64 result, over max|a| (the GPU test's yardstick),
and the float64 result of the first variant on the first WANT_ROWS rows (it
pins the tests' own brute force; whole float64 results would not fit a 1 MiB
file).

    python tests/golden/make_golden_bilateral.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WANT_ROWS = 12

# name -> (shape, sigma, win_size, ((mode, cval), ...))
CASES = {
    "basic": ((23, 37, 3), 1.0, None, (("constant", 0.0), ("constant", 0.4), ("edge", 0.0))),
    "c30": ((20, 24, 30), 2.0, None, (("constant", 0.0), ("edge", 0.0))),
    "c50": ((18, 40, 50), 1.0, None, (("constant", 0.4), ("edge", 0.0))),
    "c1": ((19, 45, 1), 1.0, None, (("constant", 0.0), ("edge", 0.0))),
    "c5": ((21, 34, 5), 1.0, None, (("edge", 0.0), ("constant", 0.4))),
    "tiles": ((70, 133, 3), 2.0, None, (("constant", 0.0), ("edge", 0.0))),
    "tiny": ((2, 3, 1), 1.0, None, (("constant", 0.4), ("edge", 0.0))),
    "small": ((5, 4, 2), 1.0, None, (("constant", 0.0), ("edge", 0.0))),
    "win25": ((27, 35, 3), 4.0, 25, (("constant", 0.4), ("edge", 0.0))),
}


def variant_key(mode, cval):
    return f"{mode}_{cval:g}"


def default_win_size(sigma):
    return max(5, 2 * int(np.ceil(3 * sigma)) + 1)


def domains(shape, seed, block=7, sd=0.03):
    H, W, C = shape
    block = max(1, min(block, min(H, W) // 2))  # at least two domains each way
    rng = np.random.default_rng(seed)
    levels = rng.uniform(0.05, 1.2, size=(-(-H // block), -(-W // block), C))
    a = np.repeat(np.repeat(levels, block, axis=0), block, axis=1)[:H, :W]
    a = a + rng.normal(0.0, sd, size=shape)
    return np.clip(a, 0.0, None).astype(np.float32)


def brute_bilateral(a, sigma, sigma_color, win_size=None, mode="constant", cval=0.0, dtype=np.float64):
    """The definition, one tap at a time over the whole image, every operation
    in ``dtype``."""
    f = dtype
    a = np.asarray(a).astype(f)
    H, W, C = a.shape
    r = ((default_win_size(sigma) if win_size is None else win_size) - 1) // 2
    if mode == "constant":
        pad = np.pad(a, ((r, r), (r, r), (0, 0)), mode="constant", constant_values=f(cval))
    else:
        pad = np.pad(a, ((r, r), (r, r), (0, 0)), mode="edge")
    num = np.zeros((H, W, C), dtype=f)
    den = np.zeros((H, W), dtype=f)
    s2, c2 = f(sigma) * f(sigma), f(sigma_color) * f(sigma_color)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            q = pad[r + dy:r + dy + H, r + dx:r + dx + W]
            d = q - a
            d2 = (d * d).sum(axis=2, dtype=f)
            w = np.exp(f(-0.5) * (f(dy * dy + dx * dx) / s2 + d2 / c2)).astype(f)
            den += w
            num += w[:, :, None] * q
    out = num / den[:, :, None]
    assert out.dtype == f
    return out


def main():
    out = {}
    for i, (name, (shape, sigma, win, variants)) in enumerate(CASES.items()):
        a = domains(shape, 20261020 + i)
        sc = float(a.astype(np.float64).std())
        out[f"{name}_in"] = a
        out[f"{name}_sigma_color"] = np.float64(sc)
        amax = float(np.abs(a).max())
        for k, (mode, cval) in enumerate(variants):
            r64 = brute_bilateral(a, sigma, sc, win, mode, cval)
            r32 = brute_bilateral(a, sigma, sc, win, mode, cval, dtype=np.float32)
            e32 = float(np.abs(r32.astype(np.float64) - r64).max()) / amax
            out[f"{name}_{variant_key(mode, cval)}_e32"] = np.float64(e32)
            if k == 0:
                out[f"{name}_want"] = r64[:WANT_ROWS].copy()
            moved = float(np.abs(r64 - a).max()) / amax
            print(f"{name:6s} {mode:8s} cval {cval:g}: e32 {e32:.2e}  max|want - in| / max|in| {moved:.3f}")
    path = os.path.join(HERE, "bilateral.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
