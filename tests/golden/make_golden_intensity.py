"""Generate ``intensity.npz``: the REFERENCE's own ``img.clip`` / ``img.scale``
(MxIF.py:29-92, 330-358) on a small synthetic slide (build container only).

As ``make_golden.py`` (whose import stubs are reused), with one more stub:
scikit-image is not installed here, so ``skimage.exposure.rescale_intensity``
restates its published semantics for the one call the reference makes,
``rescale_intensity(x, in_range=(vmin, vmax), out_range=np.float32)``
(documented assumption): the output range of the float32
dtype is [-1, 1], its lower end raised to 0 when vmin >= 0; the image is
clipped to [vmin, vmax], mapped linearly onto the output range in float64 and
cast to float32; a degenerate input range clips to the output range instead.
The percentiles are numpy's own ``np.nanpercentile``.

The fixture holds inputs and outputs only.

Usage:  python tests/golden/make_golden_intensity.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402


def rescale_intensity(image, in_range="image", out_range="dtype"):
    assert out_range is np.float32 and isinstance(in_range, tuple)
    imin, imax = map(float, in_range)
    omin, omax = (0.0 if imin >= 0 else -1.0), 1.0
    image = np.clip(image, imin, imax)
    if imin != imax:
        image = (image - imin) / (imax - imin)
        return np.asarray(image * (omax - omin) + omin, dtype=np.float32)
    return np.clip(image, omin, omax).astype(np.float32)


def main():
    G._install_stubs()
    sys.modules["skimage.exposure"].rescale_intensity = rescale_intensity
    _, MxIF = G._import_reference()  # installs the stubs again: set the function after it too
    sys.modules["skimage.exposure"].rescale_intensity = rescale_intensity
    MxIF.exposure.rescale_intensity = rescale_intensity

    raw, mask = G._synth(48, 64, 4, seed=20251015, mode="hard")
    raw = raw.astype(np.uint16)
    pre = MxIF.img(raw.copy(), mask=mask.copy())
    pre.log_normalize()
    pre.blurring("gaussian", sigma=2)
    flt = pre.img.copy()  # float64

    out = dict(raw=raw, mask=mask, flt=flt)
    for name, src in (("raw", raw), ("flt", flt)):
        for tag, op, kw in (("clip", "clip", {}), ("clip02", "clip", dict(channels=(0, 2))),
                            ("scale", "scale", {}), ("scale1", "scale", dict(channels=(1,)))):
            im = MxIF.img(src.copy(), mask=mask.copy())
            getattr(im, op)(**kw)
            res = np.asarray(im.img)
            out[f"{name}_{tag}"] = res
            print(name, tag, res.dtype, float(np.nanmin(res)), float(np.nanmax(res)))
    np.savez_compressed(os.path.join(HERE, "intensity.npz"), **out)
    print("intensity.npz:", os.path.getsize(os.path.join(HERE, "intensity.npz")), "bytes")


if __name__ == "__main__":
    main()
