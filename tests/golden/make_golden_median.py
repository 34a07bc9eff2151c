"""Regenerate tests/golden/median.npz: scipy's median filter with a ones
footprint and mode='nearest' (= skimage.filters.median(plane, footprint)), per
channel, on small uint8 / uint16 / float32 images.  The reference project
cannot make this fixture: its median branch raises (MxIF.py:403).

    python tests/golden/make_golden_median.py
"""
import os

import numpy as np
from scipy.ndimage import median_filter

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (2, 3, 4, 5, 7, (2, 5), (6, 3), 15)
SHAPE = (23, 37, 3)


def size_key(s):
    sy, sx = (s, s) if isinstance(s, int) else s
    return f"{sy}x{sx}"


def inputs():
    rng = np.random.default_rng(20261020)
    u8 = rng.integers(0, 256, size=SHAPE).astype(np.uint8)
    u8[rng.uniform(size=SHAPE) < 0.3] = 0  # ties
    u16 = rng.integers(0, 65536, size=SHAPE).astype(np.uint16)  # both sides of 32768
    u16[rng.uniform(size=SHAPE) < 0.1] = 32768
    u16[rng.uniform(size=SHAPE) < 0.1] = 32767
    f32 = rng.normal(0.0, 3.0, size=SHAPE).astype(np.float32)  # negatives
    f32[rng.uniform(size=SHAPE) < 0.25] = np.float32(1.5)  # repeated values
    f32[rng.uniform(size=SHAPE) < 0.1] = np.float32(-2.25)
    sub = rng.uniform(size=SHAPE) < 0.05  # a few subnormals of either sign
    f32[sub] = (rng.integers(1, 1 << 22, size=int(sub.sum())).astype(np.uint32)
                | (rng.integers(0, 2, size=int(sub.sum())).astype(np.uint32) << 31)).view(np.float32)
    return {"u8": u8, "u16": u16, "f32": f32}


def main():
    out = {}
    for name, a in inputs().items():
        out[f"{name}_in"] = a
        for s in SIZES:
            sy, sx = (s, s) if isinstance(s, int) else s
            fp = np.ones((sy, sx))
            res = np.stack([median_filter(a[:, :, c], footprint=fp, mode="nearest")
                            for c in range(a.shape[2])], axis=2)
            assert res.dtype == a.dtype
            out[f"{name}_{size_key(s)}"] = res
    path = os.path.join(HERE, "median.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
