"""Seeded slides and the explicit (range, bins) pairs of the histogram tests
(tests/test_cpu_histogram.py guards what tests/test_gpu_histogram.py relies
on).  Every slide is 67 x 53: rows are no multiple of 16 bytes for any element
type, and bands of 29 / 37 / 61 rows cut it unevenly."""
import numpy as np

H, W = 67, 53
CHANNELS = (1, 3, 8, 30)
KINDS = ("u8", "u16", "u16lo", "f32", "f32nan", "const", "dom")
BANDS = ("29", "37", "61")

# explicit pairs whose uncorrected index (int)((x - lo) / (hi - lo) * bins) puts a value
# of the slide into another bin than numpy does: (kind, range, bins)
EXPLICIT = (("u8", (0, 255), 51), ("u16lo", (0, 100), 100), ("u16lo", (0, 49), 49), ("u16lo", (0, 1000), 100))


def slide(kind, C=8, seed=2710):
    """(raw [H, W, C], mask [H, W] uint8 whose top rows are zero).  "u16lo": a
    uint16 slide confined to 0..1000, every value present in every plane;
    "f32": negatives; "f32nan": about 2 % NaN as well; "const": one value;
    "dom": 90 % of the elements hold one value."""
    rng = np.random.default_rng([seed, C, KINDS.index(kind)])
    n = H * W
    if kind == "u8":
        raw = rng.integers(0, 256, size=(H, W, C)).astype(np.uint8)
    elif kind == "u16":
        raw = rng.integers(0, 65536, size=(H, W, C)).astype(np.uint16)
    elif kind == "u16lo":
        raw = np.stack([rng.permutation(np.resize(np.arange(1001), n)) for _ in range(C)], -1)
        raw = raw.reshape(H, W, C).astype(np.uint16)
    elif kind in ("f32", "f32nan"):
        raw = (rng.normal(size=(H, W, C)) * 50.0 + 10.0).astype(np.float32)
        if kind == "f32nan":
            raw[rng.uniform(size=raw.shape) < 0.02] = np.nan
    elif kind == "const":
        raw = np.full((H, W, C), 7, dtype=np.uint16)
    elif kind == "dom":
        raw = rng.integers(0, 1001, size=(H, W, C)).astype(np.uint16)
        raw[rng.uniform(size=raw.shape) < 0.9] = 300
    else:
        raise KeyError(kind)
    mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.uint8)
    mask[:9] = 0
    return raw, mask


def numpy_histogram(x, bins, range=None):
    """What matplotlib's ``hist`` gives for the plane ``x``: np.histogram of
    its float64 values over ``range`` or its own (nanmin, nanmax)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if range is None:
        range = (np.nanmin(x), np.nanmax(x))
    with np.errstate(invalid="ignore"):
        return np.histogram(x, bins=bins, range=range)


def naive_bins(values, range, bins):
    """The uncorrected index of each value in [lo, hi], fp64."""
    lo, hi = float(range[0]), float(range[1])
    v = np.asarray(values, dtype=np.float64)
    i = ((v - lo) / (hi - lo) * bins).astype(np.int64)
    return np.where(i == bins, bins - 1, i)


def numpy_bins(values, range, bins):
    """numpy's bin of each value in [lo, hi]."""
    return np.array([int(np.argmax(np.histogram([v], bins=bins, range=range)[0])) for v in values], dtype=np.int64)
