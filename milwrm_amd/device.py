"""Device engine: thin typed wrappers over the C ABI that take torch tensors
(PyTorch supplies HBM allocations and the current HIP stream — plumbing only;
every computation is a hand-written HIP kernel in ``csrc/``)."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _native as N
from . import profiling

_DTYPE_CODE = {torch.uint8: N.MW_U8, torch.int16: N.MW_U16, torch.float32: N.MW_F32}


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("milwrm_amd runs on an AMD Instinct GPU (HIP); no device is visible "
                           "and there is no CPU fallback")
    N.load()


def device():
    require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    """Raw device pointer of a tensor (or None)."""
    return None if t is None else t.data_ptr()


class Workspace:
    """Grow-only scratch buffers per (device, tag); never freed inside a pass."""

    def __init__(self):
        self._bufs = {}

    def get(self, tag: str, nbytes: int) -> torch.Tensor:
        dev = torch.cuda.current_device()
        key = (dev, tag)
        b = self._bufs.get(key)
        nbytes = max(int(nbytes), 256)
        if b is None or b.numel() < nbytes:
            self._bufs.pop(key, None)
            b = None
            try:
                b = torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", dev))
            except torch.OutOfMemoryError:  # the other passes' cached scratch goes first
                self.drop()
                torch.cuda.empty_cache()
                b = torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", dev))
            self._bufs[key] = b
        return b

    def cached_bytes(self) -> int:
        return sum(b.numel() for b in self._bufs.values())

    def drop(self) -> int:
        """Hand every cached scratch buffer back to the allocator (they are
        made again on their next use; the kernels that used them were
        enqueued on the current stream, so stream-ordered reuse is safe).
        Returns the bytes dropped.  Config 5 at 4 slides per GPU: the fit's
        workspace (~21 B per row, 21 GiB) and the sample map (8 B per pixel,
        12 GiB) would otherwise stay cached through the label pass."""
        n = self.cached_bytes()
        self._bufs.clear()
        return n

    def clear(self):
        self._bufs.clear()


WS = Workspace()


class _PinnedPool:
    """Page-locked staging buffers allocated once per process and reused.

    torch's caching host allocator sometimes (per process, not per box) fails
    to reuse its blocks and then pays a page-locking allocation of several ms
    on every small transfer (measured: +50 ms per bench step).  Here a buffer
    is handed out again only when the event recorded after its last
    asynchronous copy has completed, so a non-blocking host-to-device copy is
    never overwritten before the DMA has read it."""

    def __init__(self):
        self._slots = {}  # bucket bytes -> list of [uint8 pinned tensor, event or None]

    def take(self, nbytes: int):
        bucket = 1 << max(12, (max(int(nbytes), 1) - 1).bit_length())
        lst = self._slots.setdefault(bucket, [])
        for slot in lst:
            ev = slot[1]
            if ev is None or ev.query():
                slot[1] = None
                return slot
        slot = [torch.empty(bucket, dtype=torch.uint8, pin_memory=True), None]
        lst.append(slot)
        return slot


_PINNED = _PinnedPool()


class _Busy:
    """Event stand-in for a slot held by a d2h call until it returns."""

    @staticmethod
    def query():
        return False


def _staged(slot, a: np.ndarray) -> torch.Tensor:
    """Flat typed view of a pinned slot holding a copy of ``a``."""
    v = slot[0][:a.nbytes].view(torch.from_numpy(a.reshape(-1)[:0]).dtype)
    v.numpy()[:] = a.reshape(-1)
    return v


def _mark(slot):
    ev = torch.cuda.Event()
    ev.record()
    slot[1] = ev


def h2d(a, device=None) -> torch.Tensor:
    """Small host array → device without a synchronous pageable copy: staged
    through a pooled pinned buffer, copied non-blocking on the current
    stream."""
    a = np.ascontiguousarray(a)
    dev = device if device is not None else torch.cuda.current_device()
    if a.nbytes == 0:
        return torch.from_numpy(a).to(dev)
    slot = _PINNED.take(a.nbytes)
    out = _staged(slot, a).to(dev, non_blocking=True).view(a.shape)
    _mark(slot)
    return out


def h2d_many(arrays, device=None):
    """Several small host arrays → device in ONE staged copy (16-byte aligned
    sections of one buffer); returns device views with the arrays' dtypes and
    shapes."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    offs, n = [], 0
    for a in arrays:
        offs.append(n)
        n += (a.nbytes + 15) & ~15
    buf = np.zeros(max(n, 16), dtype=np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = h2d(buf, device)
    return [dev[o:o + a.nbytes].view(torch.from_numpy(a.reshape(-1)[:0]).dtype).view(a.shape)
            for a, o in zip(arrays, offs)]


def h2d_into(dst: torch.Tensor, a) -> None:
    """dst (contiguous device tensor) ← host array of the same size, staged
    like h2d."""
    a = np.ascontiguousarray(a, dtype=torch.empty(0, dtype=dst.dtype).numpy().dtype)
    assert a.size == dst.numel() and dst.is_contiguous()
    slot = _PINNED.take(a.nbytes)
    dst.view(-1).copy_(_staged(slot, a), non_blocking=True)
    _mark(slot)


class PendingD2H:
    """Device → host copies queued by ``d2h_async``; ``wait()`` returns the
    arrays (one or a tuple) after the copies, not after work queued later."""

    def __init__(self, staged, ev):
        self._staged, self._ev, self._out = staged, ev, None

    def wait(self):
        if self._out is None:
            self._ev.synchronize()
            arrs = tuple(v.numpy().copy().reshape(shape) for _, v, shape in self._staged)
            for slot, _, _ in self._staged:
                slot[1] = None
            self._staged = ()
            self._out = arrs[0] if len(arrs) == 1 else arrs
        return self._out


def d2h_async(*ts: torch.Tensor) -> PendingD2H:
    """Queue device tensors → host copies: each is copied non-blocking into a
    pooled pinned buffer (DMA straight into page-locked memory, no pageable
    staging by the runtime), followed by an event.  The host may queue more
    device work before it waits (``PendingD2H.wait``)."""
    staged = []
    for t in ts:
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        slot = _PINNED.take(nbytes)
        slot[1] = _Busy
        v = slot[0][:nbytes].view(t.dtype)
        v.copy_(t.reshape(-1), non_blocking=True)
        staged.append((slot, v, tuple(t.shape)))
    ev = torch.cuda.Event()
    ev.record()
    return PendingD2H(staged, ev)


def d2h(*ts: torch.Tensor):
    """Device tensors → host numpy arrays (fresh copies) with ONE
    synchronisation (on the copies).  Returns one array or a tuple."""
    return d2h_async(*ts).wait()


def dtype_code(t: torch.Tensor) -> int:
    try:
        return _DTYPE_CODE[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported device image dtype {t.dtype}") from None


def to_device_image(arr: np.ndarray) -> torch.Tensor:
    """Upload an HWC host image keeping a compact element type: uint8/uint16
    stay integral (uint16 travels as int16 bits), everything else → fp32."""
    require_gpu()
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint8:
        h = torch.from_numpy(a)
    elif a.dtype == np.uint16:
        h = torch.from_numpy(a.view(np.int16))
    elif a.dtype == np.bool_:
        h = torch.from_numpy(a.astype(np.uint8))
    else:
        if np.issubdtype(a.dtype, np.integer) and a.size and (a.min() >= 0 and a.max() <= 65535):
            h = torch.from_numpy(a.astype(np.uint16).view(np.int16))
        else:
            h = torch.from_numpy(a.astype(np.float32))
    return h.to(device(), non_blocking=False)


def as_float32(t: torch.Tensor) -> torch.Tensor:
    """Element-type cast of a raw device image (uint16 travels as int16)."""
    if t.dtype == torch.float32:
        return t
    if t.dtype == torch.int16:
        return (t.to(torch.int32) & 0xFFFF).to(torch.float32)
    return t.to(torch.float32)


def to_host_float64(t: torch.Tensor) -> np.ndarray:
    if t.dtype == torch.int16:
        return t.cpu().numpy().view(np.uint16).astype(np.float64)
    return t.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------ kernels

def nz_stats(img: torch.Tensor):
    """Per-channel (sum, count) of non-zero elements of an HWC image."""
    H, W, C = img.shape
    n_pix = H * W
    s = torch.empty(C, dtype=torch.float64, device=img.device)
    c = torch.empty(C, dtype=torch.int64, device=img.device)
    ws = WS.get("nz", N.query("mw_nz_stats_ws_bytes", n_pix, C))
    with profiling.timed("nz_stats", n_pix * C * img.element_size()):
        N.call("mw_nz_stats", P(img), dtype_code(img), n_pix, C, P(s), P(c), P(ws), stream())
    return s, c


def lognorm(img: torch.Tensor, inv_mean: torch.Tensor, pseudoval: float, out=None):
    H, W, C = img.shape
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.float32, device=img.device)
    N.call("mw_lognorm", P(img), dtype_code(img), H * W, C, P(inv_mean), float(pseudoval),
           P(out), stream())
    return out


def quantiles(img: torch.Tensor, q, pooled: bool = False, skip_sentinel: bool = False) -> torch.Tensor:
    """Exact order statistics of an HWC image for the percentiles ``q`` (numpy's
    'linear' rule): a device fp64 tensor [channels, len(q), 4] of the order
    statistics of rank floor(v) and min(floor(v) + 1, n - 1), v = q/100 (n - 1),
    the kept count n and the NaN count.  ``pooled``: the image as one channel
    (``skip_sentinel``: without the elements equal to -99999).  Nothing is
    synchronised: the caller reads the result when it needs it."""
    H, W, C = img.shape
    if not img.is_contiguous():
        raise ValueError("quantiles: the image must be contiguous")
    qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
    nq = int(qa.size)
    out = torch.empty((1 if pooled else C, nq, 4), dtype=torch.float64, device=img.device)
    ws = WS.get("quantiles", N.query("mw_quantiles_ws_bytes", C, max(1, min(nq, 8))))
    passes = {torch.uint8: 1, torch.int16: 2}.get(img.dtype, 4)
    with profiling.timed("quantiles", passes * H * W * C * img.element_size()):
        N.call("mw_quantiles", P(img), dtype_code(img), H * W, C, int(bool(pooled)), qa.ctypes.data, nq,
               int(bool(skip_sentinel)), P(out), P(ws), stream())
    return out


class RowQuantiles:
    """``quantiles`` of a slide that is handed over in bands of rows
    (mw_quantiles_rows_*; stream.quantiles): per pass ``count`` every band,
    then ``choose``; after the last pass ``out`` is the record ``quantiles``
    gives for the whole slide, bit for bit, whatever the bands.  A band is a
    contiguous [rows, W, C] tensor of the slide's element type that may start
    anywhere (a view into a resident slide: no 16-byte alignment is asked).
    Nothing is synchronised."""

    def __init__(self, dtype, C: int, q, pooled: bool = False, skip_sentinel: bool = False, dev=None):
        try:
            self.code = _DTYPE_CODE[dtype]
        except KeyError:
            raise TypeError(f"unsupported device image dtype {dtype}") from None
        self.dtype, self.C = dtype, int(C)
        self.qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        self.nq = int(self.qa.size)
        if not ((self.qa >= 0) & (self.qa <= 100)).all():  # (NaN too) before the first launch
            raise ValueError(f"quantiles: percentiles {self.qa.tolist()} outside [0, 100]")
        self.pooled, self.skip = int(bool(pooled)), int(bool(skip_sentinel))
        self.passes = N.query("mw_quantiles_passes", self.code)
        self.elem = torch.empty(0, dtype=dtype).element_size()
        self.ps = 0
        dev = device() if dev is None else dev
        self.ws = WS.get("quantiles", N.query("mw_quantiles_ws_bytes", self.C, max(1, min(self.nq, 8))))
        N.call("mw_quantiles_rows_begin", self.C, self.pooled, self.nq, P(self.ws), stream())
        self.out = torch.empty((1 if pooled else self.C, self.nq, 4), dtype=torch.float64, device=dev)

    def count(self, rows: torch.Tensor):
        """Add a band to the current pass (every band once in every pass)."""
        if rows.dtype != self.dtype or rows.dim() != 3 or int(rows.shape[2]) != self.C:
            raise ValueError(f"quantiles: a band must be [rows, W, {self.C}] of {self.dtype}, got "
                             f"{tuple(rows.shape)} of {rows.dtype}")
        if not rows.is_contiguous():
            raise ValueError("quantiles: the band must be contiguous")
        if self.ps >= self.passes:
            raise ValueError("quantiles: every pass of this selection has been chosen")
        n_pix = int(rows.shape[0]) * int(rows.shape[1])
        if n_pix == 0:
            return
        with profiling.timed("quantiles", n_pix * self.C * self.elem):
            N.call("mw_quantiles_rows_count", P(rows), self.code, n_pix, self.C, self.pooled, self.nq, self.skip,
                   self.ps, P(self.ws), stream())

    def choose(self) -> bool:
        """End the current pass after its last band; True once ``out`` is written."""
        if self.ps >= self.passes:
            raise ValueError("quantiles: every pass of this selection has been chosen")
        N.call("mw_quantiles_rows_choose", self.code, self.C, self.pooled, self.qa.ctypes.data, self.nq, self.ps,
               P(self.out), P(self.ws), stream())
        self.ps += 1
        return self.ps == self.passes


RESCALE_PASS, RESCALE_CLIP, RESCALE_FLAT, RESCALE_SCALE = 0.0, 1.0, 2.0, 3.0


def rescale(img: torch.Tensor, params, out=None) -> torch.Tensor:
    """Elementwise intensity rescale to fp32.  ``params``: [C, 5] float64 rows
    (lo, hi, omin, omax, mode), host array or device tensor; mode as the
    RESCALE_* constants.  ``out`` may be ``img`` itself when it is fp32."""
    H, W, C = img.shape
    if not img.is_contiguous():
        raise ValueError("rescale: the image must be contiguous")
    if not isinstance(params, torch.Tensor):
        params = h2d(np.ascontiguousarray(params, dtype=np.float64).reshape(C, 5), img.device)
    if params.dtype != torch.float64 or tuple(params.shape) != (C, 5) or not params.is_contiguous():
        raise ValueError(f"rescale: params must be a contiguous float64 [{C}, 5] array")
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.float32, device=img.device)
    with profiling.timed("rescale", H * W * C * (img.element_size() + 4)):
        N.call("mw_rescale", P(img), dtype_code(img), H * W, C, P(params), P(out), stream())
    return out


CLAHE_MAX_BINS = 256


def clahe_args(H, W, kernel_size, clip_limit=0.01, nbins=256):
    """The arguments of CLAHE checked on the host (no device call): (kh, kw,
    clip_limit, nbins).  ``kernel_size``: an int k for (k, k), a (rows, cols)
    pair, or None for (max(H // 8, 1), max(W // 8, 1)).  ValueError: a pair of
    another length, kh or kw below 1 or above the image's extent, H or W below
    2, clip_limit not finite or not positive, nbins below 2;
    NotImplementedError: nbins above 256."""
    def whole(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"CLAHE {name} must be an int, got {v!r}")
        return int(v)

    H, W = int(H), int(W)
    if H < 2 or W < 2:
        raise ValueError(f"CLAHE needs an image of at least 2 x 2 pixels, got {H} x {W}")
    if kernel_size is None:
        kh, kw = max(H // 8, 1), max(W // 8, 1)
    elif isinstance(kernel_size, (tuple, list, np.ndarray)):
        if len(kernel_size) != 2:
            raise ValueError(f"CLAHE kernel_size must be an int, a (rows, cols) pair or None, got {kernel_size!r}")
        kh, kw = whole(kernel_size[0], "kernel_size"), whole(kernel_size[1], "kernel_size")
    else:
        kh = kw = whole(kernel_size, "kernel_size")
    if kh < 1 or kw < 1:
        raise ValueError(f"CLAHE kernel_size must be at least 1, got {kernel_size!r}")
    if kh > H or kw > W:
        raise ValueError(f"CLAHE kernel_size {(kh, kw)} exceeds the image's extent {(H, W)}")
    if isinstance(clip_limit, (bool, str)) or not isinstance(clip_limit, (int, float, np.integer, np.floating)):
        raise ValueError(f"CLAHE clip_limit must be a positive finite number, got {clip_limit!r}")
    clip_limit = float(clip_limit)
    if not (np.isfinite(clip_limit) and clip_limit > 0):
        raise ValueError(f"CLAHE clip_limit must be a positive finite number, got {clip_limit!r}")
    nbins = whole(nbins, "nbins")
    if nbins < 2:
        raise ValueError(f"CLAHE nbins must be at least 2, got {nbins}")
    if nbins > CLAHE_MAX_BINS:
        raise NotImplementedError(f"CLAHE nbins {nbins} (up to {CLAHE_MAX_BINS})")
    return kh, kw, clip_limit, nbins


def clahe(img: torch.Tensor, kernel_size, clip_limit=0.01, nbins=256, enable=None, out=None, luts: bool = False):
    """Contrast-limited adaptive histogram equalisation of an HWC image per
    plane (mw_clahe; the definition: DESIGN.md §21), fp32 out.  ``enable``: the
    planes to equalise (indices; None: all of them), the others come back as
    the fp32 conversion of their values.  ``luts``: also return the look-up
    tables, int32 [C, nby, nbx, nbins].  Arguments are checked on the host
    first (``clahe_args``); nothing is synchronised."""
    H, W, C = img.shape
    kh, kw, clip_limit, nbins = clahe_args(H, W, kernel_size, clip_limit, nbins)
    if not img.is_contiguous():
        raise ValueError("clahe: the image must be contiguous")
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.float32, device=img.device)
    elif out.dtype != torch.float32 or out.shape != img.shape or not out.is_contiguous():
        raise ValueError(f"clahe: out must be a contiguous float32 tensor of shape {tuple(img.shape)}")
    if out.data_ptr() == img.data_ptr():
        raise ValueError("clahe: the output must not alias the image")
    en = None
    if enable is not None:
        en = np.zeros(C, dtype=np.int32)
        en[np.asarray(list(enable), dtype=np.int64)] = 1
    nby, nbx = -(-H // kh), -(-W // kw)
    lut = torch.empty((C, nby, nbx, nbins), dtype=torch.int32, device=img.device) if luts else None
    ws = WS.get("clahe", N.query("mw_clahe_ws_bytes", H, W, C, kh, kw, nbins))
    # the image read three times (range, histograms, map), the output written once and rescaled in place
    with profiling.timed("clahe", H * W * C * (3 * img.element_size() + 12)):
        N.call("mw_clahe", P(img), dtype_code(img), H, W, C, None if en is None else en.ctypes.data, kh, kw,
               clip_limit, nbins, P(out), P(ws), P(lut), stream())
    return (out, lut) if luts else out


class ClaheRows:
    """``clahe`` of a slide that is handed over in bands of rows
    (mw_clahe_rows_*; stream.clahe, stream.ClaheSource).  Three
    loops over the bands, every band once in each: ``range``; ``hist``, then
    ``luts``; ``extremes``, then ``finish``.  After that ``map`` writes any
    band's final fp32 pixels, bit for bit the rows ``clahe`` gives for the
    whole slide, whatever the bands.  The object owns the state (the tables
    among them) for as long as bands are mapped.  A band is a contiguous
    [rows, W, C] tensor of the slide's element type that may start anywhere (a
    view into a resident slide: no 16-byte alignment is asked).  Arguments are
    checked on the host first (``clahe_args``); nothing is synchronised."""

    def __init__(self, dtype, H: int, W: int, C: int, kernel_size, clip_limit=0.01, nbins=256, enable=None,
                 dev=None):
        try:
            self.code = _DTYPE_CODE[dtype]
        except KeyError:
            raise TypeError(f"unsupported device image dtype {dtype}") from None
        self.dtype, self.H, self.W, self.C = dtype, int(H), int(W), int(C)
        self.kh, self.kw, self.clip_limit, self.nbins = clahe_args(H, W, kernel_size, clip_limit, nbins)
        self.en = None
        if enable is not None:
            self.en = np.zeros(self.C, dtype=np.int32)
            self.en[np.asarray(list(enable), dtype=np.int64)] = 1
        self.elem = torch.empty(0, dtype=dtype).element_size()
        self.finished = False
        dev = device() if dev is None else dev
        self.state = torch.empty(self.state_bytes(H, W, C, self.kh, self.kw, self.nbins), dtype=torch.uint8,
                                 device=dev)
        N.call("mw_clahe_rows_begin", self.code, self.H, self.W, self.C, self.kh, self.kw, self.clip_limit,
               self.nbins, P(self.state), stream())

    @staticmethod
    def state_bytes(H, W, C, kh, kw, nbins) -> int:
        return N.query("mw_clahe_ws_bytes", int(H), int(W), int(C), int(kh), int(kw), int(nbins))

    def _en(self):
        return None if self.en is None else self.en.ctypes.data

    def _band(self, rows: torch.Tensor, y0: int) -> int:
        if rows.dtype != self.dtype or tuple(rows.shape[1:]) != (self.W, self.C):
            raise ValueError(f"clahe: a band must be [rows, {self.W}, {self.C}] of {self.dtype}, got "
                             f"{tuple(rows.shape)} of {rows.dtype}")
        if not rows.is_contiguous():
            raise ValueError("clahe: the band must be contiguous")
        n = int(rows.shape[0])
        if n < 1 or y0 < 0 or y0 + n > self.H:
            raise ValueError(f"clahe: the band's rows [{y0}, {y0 + n}) are not rows of the {self.H}-row slide")
        return n

    def range(self, rows: torch.Tensor):
        n = self._band(rows, 0)
        with profiling.timed("clahe_range", n * self.W * self.C * self.elem):
            N.call("mw_clahe_rows_range", P(rows), self.code, n, self.W, self.C, P(self.state), stream())

    def hist(self, rows: torch.Tensor, y0: int):
        n = self._band(rows, y0)
        with profiling.timed("clahe_hist", n * self.W * self.C * self.elem):
            N.call("mw_clahe_rows_hist", P(rows), self.code, int(y0), n, self.H, self.W, self.C, self._en(), self.kh,
                   self.kw, self.nbins, P(self.state), stream())

    def luts(self, out: bool = False):
        """The counts become the tables; ``out``: return them, int32 [C, nby, nbx, nbins]."""
        lut = None
        if out:
            lut = torch.empty((self.C, -(-self.H // self.kh), -(-self.W // self.kw), self.nbins), dtype=torch.int32,
                              device=self.state.device)
        N.call("mw_clahe_rows_luts", self.H, self.W, self.C, self.kh, self.kw, self.clip_limit, self.nbins,
               P(self.state), P(lut), stream())
        return lut

    def extremes(self, rows: torch.Tensor, y0: int):
        n = self._band(rows, y0)
        with profiling.timed("clahe_extremes", n * self.W * self.C * self.elem):
            N.call("mw_clahe_rows_extremes", P(rows), self.code, int(y0), n, self.H, self.W, self.C, self._en(),
                   self.kh, self.kw, self.nbins, P(self.state), stream())

    def finish(self):
        N.call("mw_clahe_rows_finish", self.C, self._en(), P(self.state), stream())
        self.finished = True

    def map(self, rows: torch.Tensor, y0: int, out: torch.Tensor) -> torch.Tensor:
        """The final pixels of the band into ``out`` (fp32, the band's shape;
        it may be the band itself when that is fp32)."""
        n = self._band(rows, y0)
        if not self.finished:
            raise ValueError("clahe: map before finish")
        if out.dtype != torch.float32 or out.shape != rows.shape or not out.is_contiguous():
            raise ValueError(f"clahe: out must be a contiguous float32 tensor of shape {tuple(rows.shape)}")
        with profiling.timed("clahe_map", n * self.W * self.C * (self.elem + 4)):
            N.call("mw_clahe_rows_map", P(rows), self.code, int(y0), n, self.H, self.W, self.C, self._en(), self.kh,
                   self.kw, self.nbins, P(self.state), P(out), stream())
        return out


_range = range  # (the histogram functions take a ``range`` argument, as numpy's)
HISTOGRAM_MAX_BINS = 4096  # mw_hist_max_bins(): one channel's table and edges in a workgroup's LDS
# histograms taken (tests read it): of a resident tensor, or band by band from a slide that is not resident
HISTOGRAM_USED = {"resident": 0, "streamed": 0}


def histogram_args(bins, range=None):
    """The arguments of a histogram checked on the host (no device call):
    (bins, None or (lo, hi) as floats).  ValueError: ``bins`` not an int or
    below 1, a range that is not a pair of finite numbers or has lo > hi;
    NotImplementedError: ``bins`` above HISTOGRAM_MAX_BINS."""
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)):
        raise ValueError(f"histogram: bins must be an int >= 1 (uniform bins), got {bins!r}")
    bins = int(bins)
    if bins < 1:
        raise ValueError(f"histogram: bins must be an int >= 1, got {bins}")
    if bins > HISTOGRAM_MAX_BINS:
        raise NotImplementedError(f"histogram: bins {bins} (up to {HISTOGRAM_MAX_BINS})")
    if range is None:
        return bins, None
    try:
        lo, hi = (float(v) for v in range)
    except (TypeError, ValueError):
        raise ValueError(f"histogram: range must be a (lo, hi) pair of numbers, got {range!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"histogram: range {(lo, hi)} is not finite")
    if lo > hi:
        raise ValueError(f"histogram: range {(lo, hi)} has lo > hi")
    return bins, (lo, hi)


def histogram_edges(lo: float, hi: float, bins: int) -> np.ndarray:
    """numpy's bin edges of ``bins`` uniform bins over (lo, hi), float64:
    an empty range is widened by a half on either side, as np.histogram does."""
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, bins + 1, dtype=np.float64)


class HistogramRows:
    """np.histogram of the selected planes of a slide that is handed over in
    bands of rows (mw_hist_rows_*; stream.histogram).  With the
    range taken from the data: ``range_rows`` every band, ``set_range()``;
    with a given one: ``set_range((lo, hi))``.  Then ``count_rows`` every band
    and ``finish()``.  A band is a contiguous [rows, W, C] tensor of the
    slide's element type that may start anywhere (a view into a resident
    slide: no 16-byte alignment is asked), ``mask_rows`` the uint8 [rows, W]
    mask of the same rows or None: only pixels whose byte is not zero take
    part.  ``channels``: plane indices, a plane listed twice comes back twice;
    ``names``: what the error messages call the planes.  The counts and the
    extremes are integer reductions, so the result is the whole slide's, bit
    for bit, whatever the bands.  Arguments are checked on the host first
    (``histogram_args``); ``set_range()`` and ``finish`` synchronise on the
    few numbers they read."""

    def __init__(self, dtype, C: int, channels, bins, names=None, dev=None):
        try:
            self.code = _DTYPE_CODE[dtype]
        except KeyError:
            raise TypeError(f"unsupported device image dtype {dtype}") from None
        self.bins, _ = histogram_args(bins)
        self.dtype, self.C = dtype, int(C)
        self.channels = [int(c) for c in channels]
        if not self.channels or not all(0 <= c < self.C for c in self.channels):
            raise ValueError(f"histogram: channels {self.channels} of a {self.C}-channel image")
        self.names = list(names) if names is not None else list(self.channels)
        sel = sorted(set(self.channels))
        self.rows_of = [sel.index(c) for c in self.channels]  # the table row of every requested channel
        self.en = np.zeros(self.C, dtype=np.int32)
        self.en[sel] = 1
        self.n_sel = len(sel)
        self.elem = torch.empty(0, dtype=dtype).element_size()
        self.dev = device() if dev is None else dev
        self.edges = self.d_edges = None
        nbytes = N.query("mw_hist_ws_bytes", self.C, self.bins)
        if nbytes == 0:
            raise NotImplementedError(f"histogram: {self.C} channels, {self.bins} bins (up to 256 channels, "
                                      f"{HISTOGRAM_MAX_BINS} bins)")
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        N.call("mw_hist_rows_begin", self.C, self.bins, P(self.state), stream())

    def _band(self, rows, mask_rows) -> int:
        if rows.dtype != self.dtype or rows.dim() != 3 or int(rows.shape[2]) != self.C:
            raise ValueError(f"histogram: a band must be [rows, W, {self.C}] of {self.dtype}, got "
                             f"{tuple(rows.shape)} of {rows.dtype}")
        if not rows.is_contiguous():
            raise ValueError("histogram: the band must be contiguous")
        if mask_rows is not None and (mask_rows.dtype != torch.uint8 or tuple(mask_rows.shape) != tuple(rows.shape[:2])
                                      or not mask_rows.is_contiguous()):
            raise ValueError(f"histogram: the band's mask must be a contiguous uint8 {tuple(rows.shape[:2])} tensor")
        return int(rows.shape[0]) * int(rows.shape[1])

    def range_rows(self, rows: torch.Tensor, mask_rows=None):
        """Fold a band into the planes' extremes (every band once)."""
        n_pix = self._band(rows, mask_rows)
        if n_pix == 0:
            return
        with profiling.timed("hist_range", n_pix * self.C * self.elem):
            N.call("mw_hist_rows_range", P(rows), self.code, n_pix, self.C, self.en.ctypes.data, self.bins,
                   P(mask_rows), P(self.state), stream())

    def set_range(self, range=None) -> np.ndarray:
        """Make the edges and upload them: np.linspace over ``range`` for
        every plane, or (None, after the last ``range_rows``) over each
        plane's own (nanmin, nanmax).  ValueError naming the plane when it
        holds no element that is not NaN, or an infinite one.  Returns the
        float64 [n requested, bins + 1] edges."""
        if range is not None:
            _, (lo, hi) = histogram_args(self.bins, range)
            table = np.tile(histogram_edges(lo, hi, self.bins), (self.n_sel, 1))
        else:
            rec = torch.empty((self.n_sel, 4), dtype=torch.float64, device=self.dev)
            N.call("mw_hist_rows_finish", self.code, self.C, self.en.ctypes.data, self.bins, None, P(rec),
                   P(self.state), stream())
            rec = d2h(rec)
            table = np.empty((self.n_sel, self.bins + 1), dtype=np.float64)
            for name, r in zip(self.names, self.rows_of):
                lo, hi, n = rec[r, 0], rec[r, 1], rec[r, 2]
                if n == 0:
                    raise ValueError(f"histogram: channel {name!r} holds no element that is not NaN")
                if not (np.isfinite(lo) and np.isfinite(hi)):
                    raise ValueError(f"histogram: channel {name!r} has the infinite range {(float(lo), float(hi))}")
                table[r] = histogram_edges(float(lo), float(hi), self.bins)
        self.edges = table[self.rows_of]
        self.d_edges = h2d(table, self.dev)
        return self.edges

    def count_rows(self, rows: torch.Tensor, mask_rows=None):
        """Add a band to the counts (every band once, after ``set_range``)."""
        if self.d_edges is None:
            raise ValueError("histogram: count_rows before set_range")
        n_pix = self._band(rows, mask_rows)
        if n_pix == 0:
            return
        with profiling.timed("hist_count", n_pix * self.C * self.elem):
            N.call("mw_hist_rows_count", P(rows), self.code, n_pix, self.C, self.en.ctypes.data, self.bins,
                   P(self.d_edges), P(mask_rows), P(self.state), stream())

    def finish(self):
        """(counts int64 [n requested, bins], edges float64 [n requested,
        bins + 1]) as host arrays, in the order of ``channels``."""
        if self.d_edges is None:
            raise ValueError("histogram: finish before set_range")
        counts = torch.empty((self.n_sel, self.bins), dtype=torch.int64, device=self.dev)
        N.call("mw_hist_rows_finish", self.code, self.C, self.en.ctypes.data, self.bins, P(counts), None,
               P(self.state), stream())
        return d2h(counts)[self.rows_of], self.edges.copy()


def histogram(t: torch.Tensor, channels=None, bins=100, range=None, mask=None, names=None):
    """np.histogram of the planes ``channels`` (indices; None: all) of a
    resident HWC tensor, each as float64: (counts int64 [n, bins], edges
    float64 [n, bins + 1]) on the host.  ``range`` None: each plane's own
    (nanmin, nanmax), as matplotlib's ``hist`` passes it.  ``mask``: uint8
    [H, W], only pixels whose byte is not zero take part.  The one-band case of
    ``HistogramRows``: the tensor is read twice, once when a range is given."""
    H, W, C = t.shape
    bins, range = histogram_args(bins, range)  # before any device call
    if not t.is_contiguous():
        raise ValueError("histogram: the image must be contiguous")
    st = HistogramRows(t.dtype, C, list(_range(C)) if channels is None else channels, bins, names, t.device)
    if range is None:
        st.range_rows(t, mask)
    st.set_range(range)
    st.count_rows(t, mask)
    HISTOGRAM_USED["resident"] += 1
    return st.finish()


def gaussian_taps(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """scipy ``_gaussian_kernel1d`` order 0 (radius int(truncate*sigma+0.5)),
    computed in fp64 then rounded to fp32 for the kernel."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    return (phi / phi.sum())[::-1].astype(np.float32).copy()  # correlate1d(weights[::-1])


def blur(img: torch.Tensor, sigma: float, inv_mean=None, pseudoval: float = 1.0, out=None,
         truncate: float = 4.0):
    H, W, C = img.shape
    w = gaussian_taps(sigma, truncate)
    r = (len(w) - 1) // 2
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.float32, device=img.device)
    wsb = N.query("mw_blur_ws_bytes", H, W, C, r)
    ws = WS.get("blur", wsb) if wsb else None
    with profiling.timed("blur", H * W * C * (img.element_size() + 4)):
        N.call("mw_blur", P(img), dtype_code(img), H, W, C, P(inv_mean), float(pseudoval),
               w.ctypes.data, r, P(out), P(ws), stream())
    return out


BLUR_REST_USED = {"rest": 0}  # completions of a partly blurred image (blur_rest), for tests


def blur_rows_table(mask_u8: torch.Tensor) -> torch.Tensor:
    """Per workgroup tile of the matrix-core blur the hull [a, b) of its output
    rows that hold a needed pixel -- one whose 64-aligned flat tile holds a
    pixel of the H x W uint8 ``mask_u8`` (mw_blur_rows_table):
    int32 [tiles, 2] on the device, never read by the host."""
    H, W = mask_u8.shape
    tab = torch.empty((N.query("mw_blur_rows_tiles", H, W), 2), dtype=torch.int32, device=mask_u8.device)
    N.call("mw_blur_rows_table", P(mask_u8), H, W, P(tab), stream())
    return tab


def blur_needed(img: torch.Tensor, sigma: float, mask_u8: torch.Tensor, inv_mean=None, pseudoval: float = 1.0,
                truncate: float = 4.0, out=None):
    """``blur`` of the rows the labelling path can read (the hulls of
    ``blur_rows_table(mask_u8)``); the other rows of the output stay unwritten
    until ``blur_rest``.  Returns (out, rest), ``rest`` the arguments of the
    completion -- or (the whole blur, None) for shapes the matrix-core kernel
    does not take.  The ``blur`` region is credited the whole slide's bytes."""
    H, W, C = img.shape
    w = gaussian_taps(sigma, truncate)
    r = (len(w) - 1) // 2
    # the matrix-core kernel's shape limits (mw_blur_part), checked before the table is built
    takes = (C % 2 == 0 and C <= 64 and 1 <= r <= 8 and (W * C) % 4 == 0
             and os.environ.get("MW_BLUR_IMPL", "")[:1] != "v")
    if not takes or not img.is_contiguous() or not mask_u8.is_contiguous() or tuple(mask_u8.shape) != (H, W):
        return blur(img, sigma, inv_mean=inv_mean, pseudoval=pseudoval, out=out, truncate=truncate), None
    tab = blur_rows_table(mask_u8)
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.float32, device=img.device)
    with profiling.timed("blur", H * W * C * (img.element_size() + 4)):
        ok = N.try_call("mw_blur_part", P(img), dtype_code(img), H, W, C, P(inv_mean), float(pseudoval),
                        w.ctypes.data, r, P(out), P(tab), 1, stream())
    if not ok:
        return blur(img, sigma, inv_mean=inv_mean, pseudoval=pseudoval, out=out, truncate=truncate), None
    return out, (img, w, r, inv_mean, float(pseudoval), tab)


def blur_rest(out: torch.Tensor, rest) -> torch.Tensor:
    """Blur the rows ``blur_needed`` left out into ``out``: the whole blur,
    bit for bit."""
    img, w, r, inv_mean, pseudoval, tab = rest
    H, W, C = img.shape
    BLUR_REST_USED["rest"] += 1
    with profiling.timed("blur_rest", 0):
        N.call("mw_blur_part", P(img), dtype_code(img), H, W, C, P(inv_mean), pseudoval, w.ctypes.data, r,
               P(out), P(tab), 2, stream())
    return out


def median_size(size):
    """``size`` of a median window as (rows, cols): an int or a pair of ints,
    each at least 1 (ValueError otherwise; no device call)."""
    def one(v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"median size must be an int or a (rows, cols) pair of ints, got {size!r}")
        if v < 1:
            raise ValueError(f"median size must be at least 1, got {size!r}")
        return int(v)

    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError(f"median size must be an int or a (rows, cols) pair of ints, got {size!r}")
        return one(size[0]), one(size[1])
    return one(size), one(size)


def median(img: torch.Tensor, size, inv_mean=None, pseudoval: float = 1.0, out=None,
           force_generic: bool = False):
    """Median filter of an HWC image per channel, window ``size`` (an int or
    (rows, cols), up to 15), edges replicated: scipy's ``median_filter`` with a
    ones footprint and ``mode='nearest'``, exact.  Without ``inv_mean`` the
    output has the image's dtype; with it the output is fp32,
    ``lognorm(median(img))`` bit for bit, written once.  ``force_generic``:
    the rank search also where a selection network exists (2, 3, 5)."""
    H, W, C = img.shape
    sy, sx = median_size(size)
    if not img.is_contiguous():
        raise ValueError("median: the image must be contiguous")
    out_dtype = img.dtype if inv_mean is None else torch.float32
    if out is None:
        out = torch.empty((H, W, C), dtype=out_dtype, device=img.device)
    elif out.dtype != out_dtype or out.shape != img.shape or not out.is_contiguous():
        raise ValueError(f"median: out must be a contiguous {out_dtype} tensor of shape {tuple(img.shape)}")
    if inv_mean is not None and (inv_mean.dtype != torch.float32 or inv_mean.numel() != C):
        raise ValueError(f"median: inv_mean must hold {C} float32 values")
    network =bool(N.query("mw_median_is_network", sy, sx)) and not force_generic
    with profiling.timed("median", H * W * C * (img.element_size() + out.element_size())):
        N.call("mw_median_generic" if force_generic else "mw_median", P(img), dtype_code(img), H, W, C,
               sy, sx, P(inv_mean), float(pseudoval), P(out), stream())
    MEDIAN_USED["network" if network else "generic"] += 1
    return out


def median_rows(raw: torch.Tensor, size, row_off: int, slide_H: int, r0: int, r1: int, inv_mean=None,
                pseudoval: float = 1.0, out=None, force_generic: bool = False):
    """``median`` over a row window (mw_median_rows): ``raw`` holds rows
    [row_off, row_off + len(raw)) of a slide of ``slide_H`` rows, its rows
    [r0, r1) are filtered into a compact (r1 - r0) x W x C output, and window
    rows are clamped to the slide.  ``raw`` must hold every window row of the
    requested rows (ValueError otherwise, nothing launched): size_y // 2 rows
    above r0 unless it starts the slide, size_y - 1 - size_y // 2 below r1
    unless it ends it.  Bands that tile a slide give ``median`` of the whole
    slide bit for bit."""
    H, W, C = raw.shape
    sy, sx = median_size(size)
    if not raw.is_contiguous():
        raise ValueError("median_rows: the rows must be contiguous")
    r0, r1 = int(r0), int(r1)
    if not 0 <= r0 < r1 <= H:
        raise ValueError(f"median_rows: output rows [{r0}, {r1}) of a {H}-row array")
    out_dtype = raw.dtype if inv_mean is None else torch.float32
    shape = (r1 - r0, W, C)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=raw.device)
    elif out.dtype != out_dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"median_rows: out must be a contiguous {out_dtype} tensor of shape {shape}")
    if inv_mean is not None and (inv_mean.dtype != torch.float32 or inv_mean.numel() != C):
        raise ValueError(f"median_rows: inv_mean must hold {C} float32 values")
    network = bool(N.query("mw_median_is_network", sy, sx)) and not force_generic
    with profiling.timed("median", (r1 - r0) * W * C * (raw.element_size() + out.element_size())):
        N.call("mw_median_rows", P(raw), dtype_code(raw), H, W, C, int(row_off), int(slide_H), r0, r1, sy, sx,
               1 if force_generic else 0, P(inv_mean), float(pseudoval), P(out), stream())
    MEDIAN_USED["network" if network else "generic"] += 1
    return out


BILATERAL_MAX_WIN = 25
_BILATERAL_MODES = {"constant": 0, "edge": 1}


def bilateral_args(sigma, sigma_color, win_size=None, mode="constant", cval=0.0):
    """The arguments of the bilateral filter checked on the host (no device
    call): (sigma, sigma_color, radius, mode code, cval).  ValueError: sigma or
    sigma_color not positive and finite, win_size < 1, cval not finite;
    NotImplementedError: win_size above 25, a mode other than 'constant' /
    'edge'.  win_size defaults to max(5, 2 ceil(3 sigma) + 1); the radius is
    (win_size - 1) // 2."""
    def positive(v, name):
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"bilateral {name} must be a positive finite number, got {v!r}")
        v = float(v)
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"bilateral {name} must be a positive finite number, got {v!r}")
        return v

    sigma = positive(sigma, "sigma")
    sigma_color = positive(sigma_color, "sigma_color")
    if win_size is None:
        win_size = max(5, 2 * int(np.ceil(3 * sigma)) + 1)
    if isinstance(win_size, bool) or not isinstance(win_size, (int, np.integer)):
        raise ValueError(f"bilateral win_size must be an int, got {win_size!r}")
    if win_size < 1:
        raise ValueError(f"bilateral win_size must be at least 1, got {win_size!r}")
    if win_size > BILATERAL_MAX_WIN:
        raise NotImplementedError(f"bilateral win_size {win_size} (up to {BILATERAL_MAX_WIN}: sigma up to 4 "
                                  "with the default window)")
    if mode not in _BILATERAL_MODES:
        raise NotImplementedError(f"bilateral mode {mode!r} (only 'constant' and 'edge' are implemented)")
    cval = float(cval)
    if not np.isfinite(cval):
        raise ValueError(f"bilateral cval must be finite, got {cval!r}")
    return sigma, sigma_color, (int(win_size) - 1) // 2, _BILATERAL_MODES[mode], cval


def _check_inv_mean(what, inv_mean, C):
    if inv_mean is not None and (inv_mean.dtype != torch.float32 or inv_mean.numel() != C):
        raise ValueError(f"{what}: inv_mean must hold {C} float32 values")


def image_moments(img: torch.Tensor, inv_mean=None, pseudoval: float = 1.0) -> np.ndarray:
    """Host float64 [n, mean, sum (a - mean)^2, min, max] of the HWC image
    ``a`` = ``img`` as fp32, log-normalised when ``inv_mean`` is given
    (mw_image_moments: two passes in fp64).  Synchronises on the result."""
    H, W, C = img.shape
    if not img.is_contiguous():
        raise ValueError("image_moments: the image must be contiguous")
    _check_inv_mean("image_moments", inv_mean, C)
    out = torch.empty(5, dtype=torch.float64, device=img.device)
    ws = WS.get("moments", N.query("mw_image_moments_ws_bytes"))
    with profiling.timed("image_moments", 2 * H * W * C * img.element_size()):
        N.call("mw_image_moments", P(img), dtype_code(img), H * W, C, P(inv_mean), float(pseudoval), P(out),
               P(ws), stream())
    return d2h(out)


def image_std(img: torch.Tensor, inv_mean=None, pseudoval: float = 1.0) -> float:
    """numpy's float64 population standard deviation over every element of the
    (optionally log-normalised) fp32 image: ``a.astype(float64).std()``."""
    m = image_moments(img, inv_mean, pseudoval)
    return float(np.sqrt(m[2] / m[0]))


def bilateral(img: torch.Tensor, sigma, sigma_color, win_size=None, mode="constant", cval=0.0,
              inv_mean=None, pseudoval: float = 1.0, out=None):
    """Bilateral filter of an HWC image over all channels jointly (mw_bilateral;
    the definition: DESIGN.md §17), fp32 out.  ``inv_mean``: the image is raw
    and ``lognorm`` is fused into the load: ``bilateral(lognorm(img))`` bit for
    bit.  An image whose minimum equals its maximum comes back unchanged (as
    fp32).  Arguments are checked on the host first (``bilateral_args``)."""
    sigma, sigma_color, radius, mode_code, cval = bilateral_args(sigma, sigma_color, win_size, mode, cval)
    H, W, C = img.shape
    if not img.is_contiguous():
        raise ValueError("bilateral: the image must be contiguous")
    _check_inv_mean("bilateral", inv_mean, C)
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.float32, device=img.device)
    elif out.dtype != torch.float32 or out.shape != img.shape or not out.is_contiguous():
        raise ValueError(f"bilateral: out must be a contiguous float32 tensor of shape {tuple(img.shape)}")
    if out.data_ptr() == img.data_ptr():
        raise ValueError("bilateral: the output must not alias the image")
    m = image_moments(img, inv_mean, pseudoval)
    if m[3] == m[4]:  # a constant image is returned as it is
        if inv_mean is not None:
            return lognorm(img, inv_mean, pseudoval, out=out)
        out.copy_(as_float32(img))
        return out
    with profiling.timed("bilateral", H * W * C * (img.element_size() + 4)):
        N.call("mw_bilateral", P(img), dtype_code(img), H, W, C, radius, sigma, sigma_color, mode_code, cval,
               P(inv_mean), float(pseudoval), P(out), stream())
    return out


def bilateral_rows(raw: torch.Tensor, sigma, sigma_color, row_off: int, slide_H: int, r0: int, r1: int,
                   win_size=None, mode="constant", cval=0.0, inv_mean=None, pseudoval: float = 1.0, out=None):
    """``bilateral`` over a row window (mw_bilateral_rows): ``raw`` holds rows
    [row_off, row_off + len(raw)) of a slide of ``slide_H`` rows, its rows
    [r0, r1) are filtered into a compact (r1 - r0) x W x C fp32 output, and a
    tap row is inside or outside relative to the slide.  ``raw`` must hold
    every in-slide tap row of the requested rows (ValueError otherwise,
    nothing launched): radius rows above r0 unless it starts the slide, radius
    rows below r1 unless it ends it.  Bands that tile a slide give the rows of
    mw_bilateral over the whole slide bit for bit.  The constant-image rule of
    ``bilateral`` is NOT applied: a band cannot know the slide's minimum and
    maximum, the caller owns that rule (``stream.image_moments``)."""
    sigma, sigma_color, radius, mode_code, cval = bilateral_args(sigma, sigma_color, win_size, mode, cval)
    H, W, C = raw.shape
    if not raw.is_contiguous():
        raise ValueError("bilateral_rows: the rows must be contiguous")
    _check_inv_mean("bilateral_rows", inv_mean, C)
    row_off, slide_H, r0, r1 = int(row_off), int(slide_H), int(r0), int(r1)
    if not (0 <= row_off and row_off + H <= slide_H):
        raise ValueError(f"bilateral_rows: rows [{row_off}, {row_off + H}) are not rows of a {slide_H}-row slide")
    if not 0 <= r0 < r1 <= H:
        raise ValueError(f"bilateral_rows: output rows [{r0}, {r1}) of a {H}-row array")
    if row_off > 0 and r0 < radius:
        raise ValueError(f"bilateral_rows: output row {r0} needs {radius} rows above it and the array, whose "
                         f"first row is slide row {row_off}, holds {r0}")
    if row_off + H < slide_H and H - r1 < radius:
        raise ValueError(f"bilateral_rows: output row {r1 - 1} needs {radius} rows below it and the array, "
                         f"which ends before the slide does, holds {H - r1}")
    shape = (r1 - r0, W, C)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=raw.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"bilateral_rows: out must be a contiguous float32 tensor of shape {shape}")
    if out.data_ptr() == raw.data_ptr():
        raise ValueError("bilateral_rows: the output must not alias the rows")
    with profiling.timed("bilateral", (r1 - r0) * W * C * (raw.element_size() + 4)):
        N.call("mw_bilateral_rows", P(raw), dtype_code(raw), H, W, C, row_off, slide_H, r0, r1, radius, sigma,
               sigma_color, mode_code, cval, P(inv_mean), float(pseudoval), P(out), stream())
    return out


def block_mean(img: torch.Tensor, fact: int):
    H, W, C = img.shape
    Ho, Wo = -(-H // fact), -(-W // fact)
    out = torch.empty((Ho, Wo, C), dtype=torch.float32, device=img.device)
    N.call("mw_block_mean", P(img), dtype_code(img), H, W, C, int(fact), P(out), stream())
    return out


# img.downsample's funcs (include/milwrm_amd.h: MW_REDUCE_*)
REDUCE_CODES = {"mean": 0, "sum": 1, "max": 2, "min": 3, "median": 4}
_REDUCE_FUNCS = ((np.mean, "mean"), (np.sum, "sum"), (np.max, "max"), (np.min, "min"), (np.median, "median"))


def reduce_func(func) -> str:
    """The name of a ``downsample`` func: np.mean, np.sum, np.max / np.amax,
    np.min / np.amin, np.median, or one of their names."""
    if isinstance(func, str) and func in REDUCE_CODES:
        return func
    for f, name in _REDUCE_FUNCS:
        if func is f or (name in ("max", "min") and func is getattr(np, "a" + name)):
            return name
    raise NotImplementedError("downsample supports func = np.mean, np.sum, np.max (np.amax), np.min (np.amin) "
                              f"or np.median on the device, got {func!r}")


def reduce_fact(fact) -> int:
    """``downsample``'s block size: an int >= 1."""
    if isinstance(fact, (bool, np.bool_)) or not isinstance(fact, (int, np.integer)) or fact < 1:
        raise ValueError(f"downsample: fact must be an int >= 1, got {fact!r}")
    return int(fact)


def block_reduce_rows(rows: torch.Tensor, row0: int, slide_H: int, fact: int, func, out: torch.Tensor):
    """The slide's rows [row0, row0 + len(rows)) (HWC) reduced into their rows
    of ``out``, the whole ceil(slide_H / fact) x ceil(W / fact) x C fp32
    result (mw_block_reduce_rows: ``row0`` and, unless the band ends the
    slide, its height are multiples of ``fact``)."""
    name, fact = reduce_func(func), reduce_fact(fact)
    H, W, C = rows.shape
    if not rows.is_contiguous() or not out.is_contiguous():
        raise ValueError("block_reduce_rows: the rows and the result must be contiguous")
    if tuple(out.shape) != (-(-slide_H // fact), -(-W // fact), C) or out.dtype != torch.float32:
        raise ValueError(f"block_reduce_rows: the result is {tuple(out.shape)} {out.dtype}")
    with profiling.timed("block_reduce", H * W * C * rows.element_size() + -(-H // fact) * out.shape[1] * C * 4):
        N.call("mw_block_reduce_rows", P(rows), dtype_code(rows), H, W, C, int(row0), int(slide_H), fact,
               REDUCE_CODES[name], P(out), stream())
    return out


def block_reduce(img: torch.Tensor, fact: int, func=np.mean):
    """skimage ``block_reduce(img, (fact, fact, 1), func, cval=0)`` of a
    resident HWC tensor as fp32: the one-band case of ``block_reduce_rows``."""
    fact = reduce_fact(fact)
    H, W, C = img.shape
    out = torch.empty((-(-H // fact), -(-W // fact), C), dtype=torch.float32, device=img.device)
    return block_reduce_rows(img.contiguous(), 0, H, fact, func, out)


class RankIndex:
    """The mask rank of a slide as the compact index of mw_mask_rank_index
    (per 64-pixel word: mask bits and the tissue pixels before it; ~n/6
    bytes): the kernels map a tissue rank to its pixel through it (+
    ``pix_off``, the pixel offset of a band inside a larger array)."""

    def __init__(self, buf: torch.Tensor, n_pix: int, pix_off: int = 0):
        self.buf, self.n_pix, self.pix_off = buf, int(n_pix), int(pix_off)

    def offset(self, k: int) -> "RankIndex":
        return RankIndex(self.buf, self.n_pix, self.pix_off + int(k))

    def __getitem__(self, sl):  # r2p[:M] of the table form: the index covers every rank
        return self


# The rank -> pixel table (mw_mask_rank, 4 bytes per tissue pixel: one lookup
# per draw, the faster gather -- config 2: 1.67 vs 1.81 ms) for slides up to
# RANK_TABLE_MAX_PIX pixels (1 GiB of table); the compact index above (config
# 5's 40k x 40k slide: 0.27 GB instead of 6.4 GB).  MW_RANK_TABLE=1 / 0 forces
# the table / the index.  (Round 5, MW_GATHER_PX=1 with the index: the draws
# turned into pixels beside the blur, then a lookup-free gather: gather 1.59
# -> 1.22 ms, but the 17M index lookups take 1.2 ms on the side stream and
# slow the blur by 0.65 ms: the step is unchanged, 17.65 vs 17.68 ms.)
_RT = os.environ.get("MW_RANK_TABLE")
RANK_TABLE_MAX_PIX = (1 << 62) if _RT == "1" else 0 if _RT == "0" else (1 << 28)


def mask_rank_async(mask_u8: torch.Tensor):
    """Launch the mask rank (no host sync): (the rank→pixel int32 table of
    length n -- a RankIndex above RANK_TABLE_MAX_PIX pixels --, device count
    of mask != 0)."""
    n = mask_u8.numel()
    cnt = torch.empty(1, dtype=torch.int64, device=mask_u8.device)
    ws = WS.get("mrank", N.query("mw_mask_rank_ws_bytes", n))
    if n <= RANK_TABLE_MAX_PIX:
        r2p = torch.empty(n, dtype=torch.int32, device=mask_u8.device)
        with profiling.timed("mask_rank", n):
            N.call("mw_mask_rank", P(mask_u8), n, P(r2p), P(cnt), P(ws), stream())
    else:
        buf = torch.empty(N.query("mw_rank_index_bytes", n), dtype=torch.uint8, device=mask_u8.device)
        with profiling.timed("mask_rank", n):
            N.call("mw_mask_rank_index", P(mask_u8), n, P(buf), P(cnt), P(ws), stream())
        r2p = RankIndex(buf, n)
    # the count comes back by its own copy and event, so reading it later
    # does not wait for work queued after the rank (e.g. the blur)
    slot = _PINNED.take(8)
    slot[1] = _Busy
    hv = slot[0][:8].view(torch.int64)
    hv.copy_(cnt, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return r2p, cnt, (slot, hv, ev)


def mask_rank(mask_u8: torch.Tensor, pending=None):
    """(RankIndex or rank→pixel int32 tensor of length M, M) for mask != 0
    (row-major); ``pending`` = an earlier mask_rank_async result for the same
    mask."""
    r2p, cnt, (slot, hv, ev) = mask_rank_async(mask_u8) if pending is None else pending
    ev.synchronize()
    M = int(hv[0])
    slot[1] = None
    return r2p[:M], M


def gather_rows(img_f32: torch.Tensor, feat: torch.Tensor, idx: torch.Tensor, r2p: torch.Tensor,
                X_out: torch.Tensor, stats: torch.Tensor, accumulate: bool, absmax=None,
                keep_records=False):
    """X_out[j] = img[r2p[idx[j]], feat] (``r2p`` None: idx holds the pixels,
    rank_to_pixel); Chan-merge column stats into ``stats`` = [n, mean[F],
    M2[F]] (fp64); max |x| per column maxed into ``absmax`` (fp32 [F],
    optional).  ``keep_records``: the per-block records go to a buffer of
    their own, returned as a moment segment's (rows_per_block, records)."""
    H, W, C = img_f32.shape
    S, F = X_out.shape
    if S == 0:
        return None
    ws = _records_ws(S, F, keep_records, X_out.device)
    with profiling.timed("gather", S * (F * 4 * 2 + 8)):
        if r2p is None:
            N.call("mw_gather_rows_px", P(img_f32), C, P(feat), F, P(idx), S, P(X_out), P(ws), stream())
        elif isinstance(r2p, RankIndex):
            N.call("mw_gather_rows_ri", P(img_f32), C, P(feat), F, P(idx), P(r2p.buf), r2p.n_pix, r2p.pix_off,
                   S, P(X_out), P(ws), stream())
        else:
            N.call("mw_gather_rows", P(img_f32), C, P(feat), F, P(idx), P(r2p), S, P(X_out), P(ws),
                   stream())
    N.call("mw_col_stats_finalize", P(ws), S, F, P(stats), 1 if accumulate else 0, stream())
    if absmax is not None:
        N.call("mw_col_stats_absmax", P(ws), S, F, P(absmax), 1, stream())
    return (N.query("mw_rows_per_block", S), ws) if keep_records else None


def _records_ws(S: int, F: int, keep: bool, dev):
    """The per-block record buffer of a gather / mw_col_stats_rows: the reused
    scratch, or (``keep``) a buffer of its own that outlives the call."""
    nb = N.query("mw_gather_ws_bytes", S, F)
    return torch.empty(nb, dtype=torch.uint8, device=dev) if keep else WS.get("gather", nb)


def rank_to_pixel(idx: torch.Tensor, index: "RankIndex"):
    """idx[j] (tissue ranks, int32) -> their pixels (+ index.pix_off), in place."""
    S = idx.numel()
    if S:
        with profiling.timed("rank_to_pixel", S * 8):
            N.call("mw_rank_to_pixel_ri", P(idx), S, P(index.buf), index.n_pix, index.pix_off, stream())
    return idx


def col_stats_rows(X: torch.Tensor, stats: torch.Tensor, accumulate: bool, absmax=None,
                   keep_records=False):
    """Column statistics of rows already in ``X`` (the records mw_gather_rows
    would produce for the same rows), Chan-merged into ``stats``;
    ``keep_records`` as gather_rows."""
    S, F = X.shape
    if S == 0:
        return None
    ws = _records_ws(S, F, keep_records, X.device)
    with profiling.timed("col_stats", S * F * 4):
        N.call("mw_col_stats_rows", P(X), S, F, P(ws), stream())
    N.call("mw_col_stats_finalize", P(ws), S, F, P(stats), 1 if accumulate else 0, stream())
    if absmax is not None:
        N.call("mw_col_stats_absmax", P(ws), S, F, P(absmax), 1, stream())
    return (N.query("mw_rows_per_block", S), ws) if keep_records else None


# deferred-filter paths taken (blur or median; tests read it); *_streamed: over a slide read band by band (stream.py)
FUSED_USED = {"sample": 0, "assign": 0, "assign_banded": 0, "sample_streamed": 0, "assign_streamed": 0,
              "nz_streamed": 0, "downsample_streamed": 0}
# median paths taken (tests read it): the register selection network or the generic rank search;
# rows_streamed: bands filtered from a slide that is not resident (stream.MedianBand)
MEDIAN_USED = {"network": 0, "generic": 0, "rows_streamed": 0}
# selections fed band by band from a slide that is not resident; bands rescaled on their way in
INTENSITY_USED = {"select_streamed": 0, "rescale_streamed": 0}
# bands of a slide that is not resident filtered by the deferred bilateral (stream.BilateralBand)
BILATERAL_USED = {"rows_streamed": 0}
# equalisations whose statistics were gathered band by band from a slide that is not resident
# (stream.clahe); bands equalised on their way in (stream.ClaheSource)
CLAHE_USED = {"stats_streamed": 0, "map_streamed": 0}


def defer_blur(H: int, W: int, C: int) -> bool:
    """Whether ``img.blurring`` defers the Gaussian into the fused epilogues
    (subsample gather and label pass recompute it from the raw slide, the
    fp32 blurred slide is never stored).  ``MW_FUSED_BLUR`` = 1 / 0 forces
    it; by default ("auto") only when the fp32 slide would take more than
    half of the free HBM -- at config 2 materialising is faster (the label
    pass then reads 4 bytes per element instead of recomputing 17x17 taps)."""
    mode = os.environ.get("MW_FUSED_BLUR", "auto")
    if mode in ("0", "1"):
        return mode == "1"
    free, _ = torch.cuda.mem_get_info()
    return H * W * C * 4 > free // 2


def padded_mask(mask_u8: torch.Tensor, pad: int = 256) -> torch.Tensor:
    """``mask_u8`` in a buffer readable ``pad`` bytes past its end (the fused
    assign epilogue DMAs whole 1-KB pieces of mask rows)."""
    n = mask_u8.numel()
    st = mask_u8.untyped_storage()
    if mask_u8.is_contiguous() and st.nbytes() - mask_u8.storage_offset() >= n + pad:
        return mask_u8
    buf = torch.zeros(n + pad, dtype=torch.uint8, device=mask_u8.device)
    buf[:n].copy_(mask_u8.reshape(-1))
    return buf[:n].view(mask_u8.shape)


def blur_gather_fused(img: torch.Tensor, sigma: float, inv_mean, pseudoval: float,
                      feat: torch.Tensor, idx: torch.Tensor, r2p: torch.Tensor, X_out: torch.Tensor,
                      truncate: float = 4.0) -> bool:
    """X_out[j] = blur(lognorm(img))[r2p[idx[j]], feat] without storing the
    blurred slide (stream.blur_gather over the resident slide as one band):
    sample map (per pixel its first two sample slots, later draws on an
    overflow list) → blur with the sample epilogue, which writes both table
    slots → overflow copies.  False (nothing done) when nothing is sampled."""
    from .stream import blur_gather

    return blur_gather(img, sigma, inv_mean, pseudoval, feat, idx, r2p, X_out, truncate)


def synth_slide(H, W, C, seed, mode="hard"):
    """Benchmark input generated on device (SURVEY §8d shape): uint16 HWC
    (int16 storage) + uint8 mask."""
    from .stream import _synth_params

    syx, prof, shape, bg_rows, n_seeds, n_domains = _synth_params(H, W, C, seed, mode)
    dev = device()
    d_syx = torch.from_numpy(syx.ravel()).to(dev)
    d_prof = torch.from_numpy(prof.ravel()).to(dev)
    img = torch.empty((H, W, C), dtype=torch.int16, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    N.call("mw_synth_slide", H, W, C, P(d_syx), n_seeds, P(d_prof), n_domains, shape,
           bg_rows, int(seed) & 0xFFFFFFFFFFFFFFFF, P(img), P(mask), stream())
    return img, mask
