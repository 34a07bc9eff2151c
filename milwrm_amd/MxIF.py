"""``img``: the MxIF image container of MILWRM (MxIF.py:125-589), re-designed
around HBM residency.

The pixels live on the GPU in HWC layout with a compact element type (the raw
uint8/uint16 planes as read from TIFFs, or fp32 once transformed); ``.img``
materialises the reference's float64 host array only when someone reads it.
``log_normalize`` is deferred and fused into the Gaussian blur kernel (one
HBM pass: raw → log10(x/mean+1) → 17-tap separable blur → fp32).  All
arithmetic runs in the HIP kernels of ``csrc/``; there is no CPU fallback.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import device as D
from .rng import check_total, set_global_state_after_draws, subsample_indices_device


def checktype(obj):
    """True for a non-empty iterable of str (MxIF.py:25-26)."""
    return bool(obj) and all(isinstance(elem, str) for elem in obj)


def _out_of_scope(name):
    def f(*a, **k):
        raise NotImplementedError(f"{name} is outside the MI355X hot path (plotting); use the reference "
                                  "implementation")
    f.__name__ = name
    return f


def _need_kernel_size(name):
    """The message of CLAHE / img.equalize_hist called without kernel_size=."""
    return NotImplementedError(f"{name}: pass kernel_size= (an int, a (rows, cols) pair, or None for an eighth "
                               "of the image per axis) to run the device adaptive histogram equalisation")


_CLIP_Q = (0.5, 99.5)  # clip_values' percentiles (MxIF.py:47,57)


def _lerp_quantile(a, b, n, q):
    """numpy's 'linear' percentile ``q`` of ``n`` values from its two order
    statistics: ``a`` of rank floor(v) and ``b`` of rank min(floor(v) + 1,
    n - 1), v = q/100 (n - 1).  Float64 on the host; NaN when n = 0."""
    if n < 1:
        return float("nan")
    v = float(q) / 100 * (int(n) - 1)
    t = v - np.floor(v)
    a, b = float(a), float(b)
    d = b - a
    return float(a + d * t if t < 0.5 else b - d * (1 - t))


def _clip_params(vmin, vmax):
    """rescale_intensity(x, in_range=(vmin, vmax), out_range=np.float32) as a
    D.rescale row: the output range is [0, 1], or [-1, 1] when vmin < 0."""
    omin = 0.0 if vmin >= 0 else -1.0
    mode = D.RESCALE_FLAT if vmin == vmax else D.RESCALE_CLIP
    return (vmin, vmax, omin, 1.0, mode)


def _module_call(image, op, channels, **kwargs):
    """clip_values / scale_rgb / CLAHE of a host array through a temporary ``img``."""
    a = np.asarray(image)
    im = img(a)
    getattr(im, op)(channels=channels, **kwargs)
    out = im._materialize().cpu().numpy()  # (the op may have stayed deferred: a slide over the HBM budget)
    return out if a.ndim > 2 else out[:, :, 0]


def clip_values(image, channels=None):
    """MxIF.py:29-64 on the device (``img.clip``): float32 in the pooled branch
    (``channels`` None or a 2-D image), float64 otherwise, as the reference
    gives for its float64 images."""
    out = _module_call(image, "clip", channels)
    return out if channels is None or np.ndim(image) == 2 else out.astype(np.float64)


def scale_rgb(image, channels=None):
    """MxIF.py:67-92 on the device (``img.scale``); float64."""
    return _module_call(image, "scale", channels).astype(np.float64)


def CLAHE(image=None, channels=None, **kwargs):
    """MxIF.py:95-122 on the device (``img.equalize_hist``); float64, as the
    reference's float64 copy.  Only a call that passes ``kernel_size=`` runs."""
    if "kernel_size" not in kwargs:
        raise _need_kernel_size("CLAHE")
    return _module_call(image, "equalize_hist", channels, **kwargs).astype(np.float64)


class _DeviceMask:
    """Host-side stand-in for a mask that lives in HBM (materialised on use)."""

    def __init__(self, t):
        self._t = t
        self.shape = tuple(t.shape)
        # (a mask that img.downsample reduced on the device is fractional: fp32)
        self.dtype = np.dtype(np.float32 if t.dtype == torch.float32 else np.uint8)

    def __array__(self, dtype=None, copy=None):
        a = self._t.cpu().numpy()
        return a if dtype is None else a.astype(dtype)

    def copy(self):
        return _DeviceMask(self._t.clone())


class img:
    # A gaussian blur of a resident slide with a mask writes, at first, only the
    # rows the labelling path can read (D.blur_needed): _dev_t is
    # then partly written and _blur_rest holds the completion's arguments.
    # Every read of ``_dev`` completes the image first (_finish_blur); only the
    # subsample gather and the label pass go round it (_needed_pixels).  The
    # rows written are those the mask needed when the blur ran: assigning
    # ``mask`` completes the image, but a mask array or device tensor changed
    # IN PLACE while a rest is pending is not seen -- complete first
    # (``_finish_blur()``, or read ``img``) before editing a mask in place.
    _dev_t = None
    _blur_rest = None
    _pending_clahe = None

    @property
    def _dev(self):
        if self._blur_rest is not None:
            self._finish_blur()
        return self._dev_t

    @_dev.setter
    def _dev(self, t):
        self._blur_rest = None  # (new pixels: nothing of the old ones is left to finish)
        self._dev_t = t

    def _finish_blur(self):
        """Blur the rows a partial gaussian left out (once; D.blur_rest)."""
        rest, self._blur_rest = self._blur_rest, None
        if rest is not None:
            D.blur_rest(self._dev_t, rest)
            self._count_resident()  # the raw slide is let go

    def _count_resident(self):
        """The HBM budget's count of an evictable transformed copy: its own
        bytes and, while a rest is pending, the raw slide the rest keeps."""
        from .stream import RESIDENCY

        if self._revert is None or self._dev_t is None:
            return
        n = self._dev_t.numel() * self._dev_t.element_size()
        if self._blur_rest is not None:
            raw = self._blur_rest[0]
            n += raw.numel() * raw.element_size()
        RESIDENCY.register(self, n)

    def _needed_pixels(self) -> torch.Tensor:
        """The fp32 pixels for a reader that looks only at pixels whose
        64-aligned flat tile holds a mask pixel (the subsample gather, the
        label pass): a partly blurred image stays so.  Anything pending on top
        of it applies to whole images and completes it first."""
        from .stream import RESIDENCY

        if (self._blur_rest is not None and self._pending is None and self._pending_rescale is None
                and self._pending_clahe is None and not self._filter_deferred()):
            RESIDENCY.touch(self)
            return self._dev_t
        return D.as_float32(self._materialize())

    def __init__(self, img_arr, channels=None, mask=None):
        """Same validation and attributes as MxIF.py:126-167 (``img``, ``n_ch``,
        ``ch``, ``mask``); the pixels are uploaded lazily."""
        assert img_arr.ndim > 1, "Image does not have enough dimensions: {} given".format(img_arr.ndim)
        self._ndim = img_arr.ndim
        self._host = np.asarray(img_arr)
        self._host64 = None
        self._dev = None            # HWC device tensor (authoritative when set)
        # deferred clip / scale rounds, applied before anything else pending (stream.RescaleSource):
        # (host [C, 5] D.rescale tables, the same on the device)
        self._pending_rescale = None
        # deferred equalize_hist(banded=True) rounds, applied after the clip / scale rounds and before anything
        # else pending (stream.ClaheSource): a list of (finished D.ClaheRows, kernel_size, clip_limit, nbins,
        # the round's channels), never changed in place
        self._pending_clahe = None
        self._range = None          # per-channel (lo, hi) of clipped / scaled pixels (NaN: not known), see _blur_bound
        self._pending = None        # (inv_mean fp32 device tensor, pseudoval) deferred log_normalize
        self._pending_blur = None   # (sigma, truncate) deferred gaussian (fused-epilogue mode)
        self._pending_median = None  # (size_y, size_x) deferred median (applied band by band, stream.MedianBand)
        # (sigma, sigma_color as a resolved float, win_size, mode, cval) deferred bilateral (stream.BilateralBand)
        self._pending_bilateral = None
        self._lognorm_host = None   # (inv_mean fp32 host array, pseudoval) of the pending log_normalize
        self._xbound = None         # per-channel bound on |pixel| of blur(lognorm(raw)), see _blur_bound
        self.n_ch = img_arr.shape[2] if img_arr.ndim > 2 else 1
        if channels is None:
            self.ch = ["ch_{}".format(x) for x in range(self.n_ch)]
        else:
            if not isinstance(channels, list):
                raise Exception("Channels must be given in a list")
            assert len(channels) == self.n_ch, "Number of channels must match img_arr.shape[2]"
            self.ch = channels
        if mask is not None:
            assert mask.shape == img_arr.shape[:2], \
                "Shape of mask must match the first two dimensions of img_arr"
        self.mask = mask
        self._mask_dev = None
        self._band = None  # bands.BandInfo when this img is one row band of a slide
        self._src = None   # stream.RowSource of a slide that is read band by band
        self._hsrc = None  # cached stream.HostSource over _host
        self._revert = None  # how to redo a transformed copy (_transformed / _evict)

    # ----------------------------------------------------------- residency
    # The raw pixels of a host-backed image are uploaded whole while they fit
    # the HBM budget (stream.RESIDENCY, least recently used out); otherwise
    # every pass that needs them streams them in row bands (milwrm_amd.stream)
    @property
    def shape(self):
        if self._dev_t is not None:
            return tuple(self._dev_t.shape) if self._ndim > 2 else tuple(self._dev_t.shape[:2])
        if self._host is None and self._src is not None:
            return self._src.shape if self._ndim > 2 else self._src.shape[:2]
        return self._host.shape

    def _raw_nbytes(self) -> int:
        from .stream import device_dtype_of

        a = self._host
        memo = getattr(self, "_rawb", None)
        if memo is None or memo[0] is not a:
            elem = torch.empty(0, dtype=device_dtype_of(a)).element_size()
            memo = self._rawb = (a, int(a.size) * elem)
        return memo[1]

    def _elem_size(self) -> int:
        """Bytes per element of the pixels as the device holds (or would hold) them."""
        from .stream import device_dtype_of

        if self._pending_rescale is not None or self._pending_clahe is not None:
            return 4
        if self._dev_t is not None:
            return self._dev_t.element_size()
        t = self._src.dtype if self._host is None else device_dtype_of(self._host)
        return torch.empty(0, dtype=t).element_size()

    def _device(self) -> torch.Tensor:
        """HWC device tensor (uploads on first use; a host-backed upload may
        first evict older resident copies, stream.RESIDENCY)."""
        from .stream import RESIDENCY

        if self._dev is None:
            if self._host is None and self._src is not None:
                src = self._src
                self._fits_whole(src.H * src.row_bytes)
                self._dev = src.materialize()  # an explicit whole-slide read
            else:
                a = self._host if self._host.ndim > 2 else self._host[:, :, None]
                if not RESIDENCY.admit(self, self._raw_nbytes()):
                    self._fits_whole(self._raw_nbytes())  # over the budget: only if HBM holds it
                self._dev = D.to_device_image(a)
            RESIDENCY.register(self, self._dev.numel() * self._dev.element_size())
        else:
            RESIDENCY.touch(self)
        return self._dev

    def _fits_whole(self, nbytes: int):
        """Raise a MemoryError naming the streamed alternative when a
        whole-slide device copy of ``nbytes`` cannot be had even after evicting
        every other resident slide (instead of an allocator failure deep in a
        pass)."""
        from .stream import RESIDENCY, alloc_bytes

        RESIDENCY.release(nbytes + (256 << 20))
        have = alloc_bytes()
        if nbytes + (256 << 20) > have:
            raise MemoryError(
                f"this operation needs the whole raw slide in HBM ({nbytes / 2**30:.1f} GiB) and "
                f"{have / 2**30:.1f} GiB can be allocated: the slide is streamed in row bands instead by "
                f"the passes that take bands (clip and scale of raw or clipped / scaled pixels, "
                f"equalize_hist(banded=True) of those, calculate_non_zero_mean, log_normalize + blurring with the "
                f"default batch mean, subsample_pixels, create_tissue_mask, downsample, label_tissue_regions, "
                f"confidence_score_images; not clip, scale or equalize_hist after a log_normalize or a filter, "
                f"nor clip or scale after a deferred equalize_hist)")

    def _source(self):
        """None when the pixels are resident (or the raw ones are admitted now:
        the caller then takes ``_device()``); else the ``stream.RowSource`` to
        read them from band by band.  With clip / scale or equalize_hist rounds
        deferred that is always a source: the raw one -- the resident raw
        slide, if it is -- seen through the clip / scale rounds
        (``stream.RescaleSource``), then through one ``stream.ClaheSource``
        per equalize_hist round."""
        from .stream import ClaheSource, DeviceSource, RescaleSource

        src = self._raw_source()
        if self._pending_rescale is None and self._pending_clahe is None:
            return src
        if src is None:
            src = DeviceSource(self._device())
        if self._pending_rescale is not None:
            src = RescaleSource(src, self._pending_rescale[1])
        for rnd in self._pending_clahe or ():
            src = ClaheSource(src, rnd[0])
        return src

    def _raw_source(self):
        """``_source`` of the raw pixels (before any deferred clip / scale)."""
        from .stream import RESIDENCY, HostSource

        if self._dev_t is not None:
            RESIDENCY.touch(self)
            return None
        if self._band is not None:  # a slide band (milwrm_amd.bands) stays resident
            return None
        if self._host is None:
            return self._src
        if RESIDENCY.admit(self, self._raw_nbytes()):
            return None
        if self._hsrc is None:
            self._hsrc = HostSource(self._host)
        return self._hsrc

    def _may_hold(self, nbytes: int) -> bool:
        """Whether a device copy of ``nbytes`` may be kept for this image: any
        for an image born on the device; within the HBM budget (evicting older
        copies) for one a host array or a source backs."""
        from .stream import RESIDENCY

        if self._host is None and self._src is None:
            return True
        return RESIDENCY.admit(self, nbytes)

    @classmethod
    def from_source(cls, src, mask=None, channels=None) -> "img":
        """An image whose raw pixels come from a ``stream.RowSource`` band by
        band (never resident whole): a slide reader, a host array, or the
        benchmark's synthetic generator.  ``mask``: host or device H x W
        (default: the source's own mask)."""
        obj = cls.__new__(cls)
        obj._ndim = 3
        obj._host = None
        obj._host64 = None
        obj._dev = None
        obj._pending_rescale = None
        obj._pending_clahe = None
        obj._range = None
        obj._pending = None
        obj._pending_blur = None
        obj._pending_median = None
        obj._pending_bilateral = None
        obj._lognorm_host = None
        obj._xbound = None
        obj._src = src
        obj._hsrc = None
        obj._revert = None
        obj.n_ch = int(src.C)
        obj.ch = channels if channels is not None else ["ch_{}".format(x) for x in range(obj.n_ch)]
        obj._mask = None
        obj._mask_dev = None
        obj._mrank = None
        obj._band = None
        if mask is None:
            mask = src.mask_device()
        if isinstance(mask, torch.Tensor):
            obj._mask = _DeviceMask(mask)
            obj._mask_dev = D.padded_mask((mask != 0).to(torch.uint8) if mask.dtype != torch.uint8 else mask)
        elif mask is not None:
            assert tuple(mask.shape) == (src.H, src.W), \
                "Shape of mask must match the first two dimensions of img_arr"
            obj._mask = mask
        return obj

    def _materialize(self) -> torch.Tensor:
        """Apply a deferred blur (with its log_normalize fused), a deferred
        median (the log_normalize as its epilogue), a deferred bilateral (the
        log_normalize as its load) or a deferred log_normalize (standalone
        kernel).  Deferred clip / scale rounds apply first, then deferred
        equalize_hist rounds, then what else is pending on their fp32 result,
        as one evictable transform."""
        if self._pending_rescale is not None or self._pending_clahe is not None:
            rng = self._range if self._pending is None and not self._filter_deferred() else None
            self._transformed(self._apply_rescaled)
            self._range = rng
            return self._device()
        if self._pending_bilateral is not None:
            sigma, sigma_color, win_size, mode, cval = self._pending_bilateral
            inv, p = self._pending if self._pending is not None else (None, 1.0)

            def make():
                # (a slide that is not resident and does not fit: _device()'s MemoryError)
                src = self._device()
                # the one-band case of the bands' kernel; the constant-image rule was settled at call time
                return D.bilateral_rows(src, sigma, sigma_color, 0, src.shape[0], 0, src.shape[0],
                                        win_size=win_size, mode=mode, cval=cval, inv_mean=inv, pseudoval=p)

            self._transformed(make)
        if self._pending_median is not None:
            size = self._pending_median
            inv, p = self._pending if self._pending is not None else (None, 1.0)
            # (a slide that is not resident and does not fit: _device()'s MemoryError)
            self._transformed(lambda: D.median(self._device(), size, inv_mean=inv, pseudoval=p))
        if self._pending_blur is not None:
            sigma, truncate = self._pending_blur
            inv, p = self._pending
            self._transformed(lambda: D.blur(self._device(), sigma, inv_mean=inv, pseudoval=p,
                                             truncate=truncate))
        if self._pending is not None:
            inv, p = self._pending
            if inv is None:
                self._pending = None
            else:
                self._transformed(lambda: D.lognorm(self._device(), inv, p))
        return self._device()

    def _apply_rescaled(self) -> torch.Tensor:
        """The pixels with everything pending applied, the deferred clip /
        scale rounds first, then the deferred equalize_hist rounds (each whole,
        D.clahe: the banded form's bits): the calls of the resident path, in
        its order."""
        t = self._device()  # (a slide that is not resident and does not fit: _device()'s MemoryError)
        for i, tab in enumerate(self._pending_rescale[1] if self._pending_rescale is not None else ()):
            t = D.rescale(t, tab, out=t if i else None)
        for _, kernel_size, clip_limit, nbins, chs in self._pending_clahe or ():
            t = D.clahe(t, kernel_size, clip_limit, nbins, enable=chs)
        inv, p = self._pending if self._pending is not None else (None, 1.0)
        if self._pending_bilateral is not None:
            sigma, sigma_color, win_size, mode, cval = self._pending_bilateral
            return D.bilateral_rows(t, sigma, sigma_color, 0, t.shape[0], 0, t.shape[0], win_size=win_size,
                                    mode=mode, cval=cval, inv_mean=inv, pseudoval=p)
        if self._pending_median is not None:
            return D.median(t, self._pending_median, inv_mean=inv, pseudoval=p)
        if self._pending_blur is not None:
            sigma, truncate = self._pending_blur
            return D.blur(t, sigma, inv_mean=inv, pseudoval=p, truncate=truncate)
        return t if inv is None else D.lognorm(t, inv, p)

    def _transformed(self, make):
        """Replace the pixels by ``make()`` (the pending transforms applied).
        An image backed by a host array or a source keeps how to redo it: its
        transformed copy stays evictable (``_evict`` returns it to the
        deferred state, which gives the same bits, stream.py)."""
        from .stream import RESIDENCY

        backed = self._host is not None or self._src is not None
        state = (self._host, self._src, self._pending, self._pending_blur,
                 self._pending_median, self._pending_bilateral, self._pending_rescale, self._pending_clahe,
                 self._range) if backed else None
        out = make()
        self._pending_rescale = None
        self._pending_clahe = None
        self._pending = None
        self._pending_blur = None
        self._pending_median = None
        self._pending_bilateral = None
        self._set_device(out)
        if state is not None:
            self._revert = state
            RESIDENCY.register(self, out.numel() * out.element_size())

    def _set_device(self, t: torch.Tensor):
        """The image's pixels are now ``t`` (not a raw copy that could be read
        again: not evictable unless ``_transformed`` records how to redo it)."""
        from .stream import RESIDENCY

        RESIDENCY.forget(self)
        self._dev = t
        self._host64 = None
        self._host = None
        self._src = None
        self._hsrc = None
        self._revert = None
        self._range = None

    def _evict(self):
        """Drop the device copy: the raw copy of a host array / source, or a
        transformed copy back to its deferred state."""
        rv = getattr(self, "_revert", None)
        if rv is not None:
            (self._host, self._src, self._pending, self._pending_blur, self._pending_median,
             self._pending_bilateral, self._pending_rescale, self._pending_clahe, self._range) = rv
            self._revert = None
            self._host64 = None
        self._dev = None

    @property
    def img(self) -> np.ndarray:
        """The reference's float64 HWC array (materialised from HBM on read)."""
        if self._host64 is None:
            if (self._dev is None and self._host is not None and self._pending is None
                    and self._pending_blur is None and self._pending_median is None
                    and self._pending_bilateral is None and self._pending_rescale is None
                    and self._pending_clahe is None):
                self._host64 = self._host.astype("float64")
            else:
                t = self._materialize()
                a = D.to_host_float64(t)
                self._host64 = a if self._ndim > 2 else a[:, :, 0]
        return self._host64

    @img.setter
    def img(self, value):
        from .stream import RESIDENCY

        value = np.asarray(value)
        RESIDENCY.forget(self)
        self._ndim = value.ndim
        self._host = value
        self._host64 = None
        self._dev = None
        self._src = None
        self._hsrc = None
        self._pending_rescale = None
        self._pending_clahe = None
        self._range = None
        self._pending = None
        self._pending_blur = None
        self._pending_median = None
        self._pending_bilateral = None
        self._lognorm_host = None
        self._xbound = None

    def _filter_deferred(self) -> bool:
        """Whether a filter (gaussian, median or bilateral) is deferred: the
        passes that need pixels recompute it band by band (milwrm_amd.stream)."""
        return (self._pending_blur is not None or self._pending_median is not None
                or self._pending_bilateral is not None)

    @property
    def mask(self):
        return self._mask

    @mask.setter
    def mask(self, m):
        self._finish_blur()  # (a partly blurred image holds the rows the old mask needs)
        self._mask = m
        self._mask_dev = None
        self._mrank = None

    def _mask_device(self) -> torch.Tensor:
        if self._mask_dev is None:
            if self._mask is None:
                raise AssertionError("No tissue mask available")
            m = np.ascontiguousarray(np.asarray(self._mask) != 0, dtype=np.uint8)
            self._mask_dev = D.padded_mask(torch.from_numpy(m).to(D.device()))
        return self._mask_dev

    def _prefetch_mask_rank(self):
        """Queue the mask rank on the stream without waiting for it (it only
        depends on the mask): it then overlaps the host work between
        calculate_non_zero_mean and subsample_pixels."""
        if getattr(self, "_mrank", None) is None and self._mask is not None:
            self._mrank = D.mask_rank_async(self._mask_device().reshape(-1))

    def _mask_rank(self):
        """(rank→pixel, M) of the current mask, from the prefetched launch if any."""
        pending = getattr(self, "_mrank", None)
        self._mrank = None
        return D.mask_rank(self._mask_device().reshape(-1), pending)

    # -------------------------------------------------------------- basics
    def __repr__(self) -> str:
        descr = "img object with {} of {} and shape {}px x {}px\n".format(
            np.ndarray, np.dtype("float64"), self.shape[0], self.shape[1]
        ) + "{} image channels:\n\t{}".format(self.n_ch, self.ch)
        if self.mask is not None:
            descr += "\n\ntissue mask {} of {} and shape {}px x {}px".format(
                type(self.mask), self.mask.dtype, self.mask.shape[0], self.mask.shape[1])
        return descr

    def copy(self) -> "img":
        new = img.__new__(img)
        new.__dict__.update(self.__dict__)
        new.ch = list(self.ch)
        new._host = None if self._host is None else self._host.copy()
        new._host64 = None if self._host64 is None else self._host64.copy()
        new._dev = None if self._dev is None else self._dev.clone()
        new._hsrc = None
        new._mask = None if self._mask is None else self._mask.copy()
        new._mask_dev = None
        new._mrank = None
        return new

    def _features(self, features):
        if isinstance(features, int):
            features = [features]
        if isinstance(features, str):
            features = [self.ch.index(features)]
        if checktype(features):
            features = [self.ch.index(x) for x in features]
        if features is None:
            features = [x for x in range(self.n_ch)]
        features = [int(f) for f in features]
        for f in features:  # checked on the host: the kernels index channels with them
            if not -self.n_ch <= f < self.n_ch:
                raise IndexError(f"index {f} is out of bounds for axis 2 with size {self.n_ch}")
        return [f % self.n_ch for f in features]

    def __getitem__(self, channels):
        return self.img[:, :, self._features(channels)]

    @classmethod
    def from_device(cls, tensor, mask=None, channels=None) -> "img":
        """Wrap an HWC image already resident in HBM (uint8 / uint16-as-int16 /
        fp32) and an optional device mask (nonzero = tissue).  The mask tensor
        is kept by reference: it must not be changed in place between a
        gaussian ``blurring`` and the passes that follow it (the blur writes
        the rows that mask needs first)."""
        assert tensor.dim() == 3, "device image must be H x W x C"
        obj = cls.__new__(cls)
        obj._ndim = 3
        obj._host = None
        obj._host64 = None
        obj._dev = tensor
        obj._pending_rescale = None
        obj._pending_clahe = None
        obj._range = None
        obj._pending = None
        obj._pending_blur = None
        obj._pending_median = None
        obj._pending_bilateral = None
        obj._lognorm_host = None
        obj._xbound = None
        obj.n_ch = int(tensor.shape[2])
        obj.ch = channels if channels is not None else ["ch_{}".format(x) for x in range(obj.n_ch)]
        obj._mask = None
        obj._mask_dev = None
        obj._mrank = None
        obj._band = None
        obj._src = None
        obj._hsrc = None
        obj._revert = None
        if mask is not None:
            obj._mask = _DeviceMask(mask)
            obj._mask_dev = (mask != 0).to(torch.uint8) if mask.dtype != torch.uint8 else mask
        return obj

    # ----------------------------------------------------------------- I/O
    @classmethod
    def from_tiffs(cls, tiffdir, channels, common_strings=None, mask=None):
        """MxIF.py:211-283 (needs an installed TIFF reader: skimage.io)."""
        try:
            from skimage.io import imread
        except ImportError as e:  # pragma: no cover - image has no skimage
            raise ImportError("img.from_tiffs needs scikit-image (skimage.io.imread)") from e
        if common_strings is not None and isinstance(common_strings, str):
            common_strings = [common_strings]
        A = []
        for channel in channels:
            if common_strings is None:
                f = [f for f in os.listdir(tiffdir) if channel in f]
            else:
                f = [f for f in os.listdir(tiffdir) if all(x in f for x in common_strings + [channel])]
            assert len(f) != 0, "No file found with channel {}".format(channel)
            assert len(f) == 1, "More than one match found for file with channel {}".format(channel)
            A.append(imread(os.path.join(tiffdir, f[0])))
        A_arr = np.dstack(A)
        A_mask = None
        if mask is not None:
            f = [f for f in os.listdir(tiffdir) if mask in f]
            assert len(f) != 0, "No tissue mask file found"
            assert len(f) == 1, "More than one match found for tissue mask file"
            A_mask = imread(os.path.join(tiffdir, f[0]))
            assert A_mask.shape == A_arr.shape[:2], \
                "Mask (shape: {}) is not the same shape as marker images (shape: {})".format(
                    A_mask.shape, A_arr.shape[:2])
        return cls(img_arr=A_arr, channels=channels, mask=A_mask)

    @classmethod
    def from_npz(cls, file):
        """MxIF.py:285-309 (no pickles: allow_pickle stays False)."""
        print("Loading img object from {}...".format(file))
        tmp = np.load(file)
        assert "img" in tmp.files, \
            "Unexpected files in .npz: {}, expected ['img','mask','ch'].".format(tmp.files)
        A_mask = tmp["mask"] if "mask" in tmp.files else None
        A_ch = list(tmp["ch"]) if "ch" in tmp.files else None
        return cls(img_arr=tmp["img"], channels=A_ch, mask=A_mask)

    def to_npz(self, file):
        """MxIF.py:311-328."""
        print("Saving img object to {}...".format(file))
        if self.mask is None:
            np.savez_compressed(file, img=self.img, ch=self.ch)
        else:
            np.savez_compressed(file, img=self.img, ch=self.ch, mask=self.mask)

    # ----------------------------------------------------------- intensity
    def _channel_rounds(self, channels):
        """``channels`` of clip / scale / equalize_hist as rounds of distinct
        plane indices: [None] (every plane at once) for None or a 2-D image;
        a channel listed twice is in two rounds."""
        if channels is None or self._ndim == 2:
            return [None]
        if isinstance(channels, (int, np.integer, str)):
            channels = (channels,)
        todo = self._features(list(channels))
        rounds = []
        while todo:
            uniq = list(dict.fromkeys(todo))
            rounds.append(uniq)
            for c in uniq:
                todo.remove(c)
        return rounds

    def _intensity(self, channels, q, skip_pooled, rows_of):
        """clip / scale: per round one exact selection of the percentiles ``q``
        (D.quantiles, one host read of its few numbers; ``skip_pooled``: the
        pooled selection leaves out -99999) and one rescale pass.
        ``rows_of(record)`` turns a channel's record into its D.rescale row and
        whether the rescaled plane's range is known.  A channel listed twice
        is processed twice, as the reference's loop does.

        Raw pixels (or ones whose only pending state is earlier clip / scale
        rounds) that are not resident, or whose fp32 result may not be held
        (the HBM budget), keep the rounds deferred (``_pending_rescale``): the
        selection reads the slide band by band (stream.quantiles) and every
        pass that needs pixels rescales each band as it reads it
        (stream.RescaleSource), before a later log_normalize or filter: the
        resident bits.  With a log_normalize or a filter already pending the
        pixels are materialised first (MemoryError when they do not fit), and
        so are deferred equalize_hist rounds; a row band of a slide split over
        ranks is refused."""
        from . import stream

        if getattr(self, "_band", None) is not None:
            raise NotImplementedError("clip / scale of a row band of a slide: the percentiles are the "
                                      "whole slide's")
        rounds = self._channel_rounds(channels)
        deferred = False
        rng = np.full((2, self.n_ch), np.nan)  # after a log_normalize or a filter: not known
        if self._pending is None and not self._filter_deferred() and self._pending_clahe is None:
            rng = self._range_now()
            H, W = self.shape[0], self.shape[1]
            deferred = self._source() is not None or not self._may_hold(H * W * self.n_ch * 4)
        if deferred:
            C = self.n_ch
            base = self._raw_source()
            if base is None:
                base = stream.DeviceSource(self._device())
            host, dev = ([], []) if self._pending_rescale is None else (list(x) for x in self._pending_rescale)
        else:
            t = self._materialize()  # a slide that is not resident: _device()'s MemoryError
            C = int(t.shape[2])
        lo, hi = rng[0].copy(), rng[1].copy()
        for chs in rounds:
            pooled = chs is None
            params = np.zeros((C, 5), dtype=np.float64)  # mode 0: the value itself
            if deferred:
                rec = stream.quantiles(stream.RescaleSource(base, dev) if dev else base, q, pooled=pooled,
                                       skip_sentinel=pooled and skip_pooled)
            else:
                rec = D.quantiles(t, q, pooled=pooled, skip_sentinel=pooled and skip_pooled)
            st = D.d2h(rec)
            for c in range(C) if pooled else chs:
                params[c], known = rows_of(st[0 if pooled else c])
                lo[c], hi[c] = (params[c, 2], params[c, 3]) if known else (np.nan, np.nan)
            if deferred:
                host.append(params)
                dev.append(D.h2d(params, D.device()))
            else:
                t = D.rescale(t, params)
        if deferred:
            self._pending_rescale = (host, dev)
            self._host64 = None
        else:
            self._set_device(t)
        self._range = np.stack([lo, hi])
        self._xbound = None
        self._lognorm_host = None

    def _range_now(self):
        """[2, n_ch] (lo, hi) of the current pixels, NaN where not known: what
        earlier clip / scale rounds left, or a raw integer slide's type range."""
        if self._range is not None:
            return self._range
        mx = self._raw_int_max()
        if mx is None:
            return np.full((2, self.n_ch), np.nan)
        return np.stack([np.zeros(self.n_ch), np.full(self.n_ch, mx)])

    def clip(self, channels=None):
        """MxIF.py:330-343 / clip_values (MxIF.py:29-64): rescale to the 0.5 and
        99.5 percentiles (NaNs left out) as skimage's rescale_intensity(...,
        out_range=np.float32) does.  ``channels`` None (or a 2-D image): one
        pair over all channels, elements equal to -99999 left out as well;
        else a tuple of channel indices (or names), each plane with its own
        pair, the others unchanged.  The pixels become fp32.  A slide that is
        not resident (or whose fp32 result may not be held) keeps the clip
        deferred, see ``_intensity``; out of that scope, as before: a
        log_normalize or a filter already pending materialises first, a row
        band of a split slide raises."""
        def rows_of(st):
            n = int(st[0, 2])
            row = _clip_params(_lerp_quantile(st[0, 0], st[0, 1], n, _CLIP_Q[0]),
                               _lerp_quantile(st[1, 0], st[1, 1], n, _CLIP_Q[1]))
            return row, n > 0 and st[0, 3] == 0  # (a NaN pixel stays NaN: no bound)

        self._intensity(channels, _CLIP_Q, True, rows_of)

    def scale(self, channels=None):
        """MxIF.py:345-358 / scale_rgb (MxIF.py:67-92): (x - min) / (max - min),
        one min / max over everything (``channels`` None or a 2-D image) or per
        listed plane.  As numpy's min(): a plane holding a NaN becomes NaN, and
        a constant plane gives 0/0 = NaN.  The pixels become fp32.  Deferred
        for a slide that is not resident, as ``clip``."""
        def rows_of(st):
            nan = float("nan")
            lo, hi = (st[0, 0], st[1, 1]) if st[0, 3] == 0 and st[0, 2] > 0 else (nan, nan)
            return (lo, hi, 0.0, 1.0, D.RESCALE_SCALE), bool(hi > lo)  # (else the plane is NaN: no bound)

        self._intensity(channels, (0.0, 100.0), False, rows_of)

    def equalize_hist(self=None, channels=None, **kwargs):
        """MxIF.py:360-373 / CLAHE (MxIF.py:95-122): contrast-limited adaptive
        histogram equalisation per plane (D.clahe; the definition, and how it
        relates to skimage's equalize_adapthist: DESIGN.md §21).  Only a call
        that passes ``kernel_size=`` runs: an int, a (rows, cols) pair, or
        None for an eighth of the image per axis; ``clip_limit`` (0.01) and
        ``nbins`` (256, at most 256) as skimage's.  ``channels`` as ``clip``:
        None (or a 2-D image) means every plane, else indices or names, the
        other planes unchanged; a plane listed twice is equalised twice.  The
        pixels become fp32.

        ``banded=False``: the slide must be resident: deferred clip / scale
        rounds are materialised first (MemoryError when that does not fit).
        ``banded=True`` permits the banded form: raw pixels (or
        ones whose only pending state is earlier clip / scale / equalize_hist
        rounds) that are not resident, or whose fp32 result may not be held
        (the HBM budget), keep the rounds deferred (``_pending_clahe``).  The
        call reads the slide three times per round (the planes' ranges, the
        tiles' histograms, the extremes of the blend: stream.clahe) and keeps
        the tables in HBM (MemoryError when they do not fit: a larger
        ``kernel_size`` makes them smaller); every pass that needs pixels then
        equalises each band as it reads it (stream.ClaheSource), before a
        later log_normalize or filter, with the resident bits.  A resident
        slide whose result may be held is equalised at once, exactly as with
        ``banded=False``; so is one with a log_normalize or a filter already
        pending (materialised first, MemoryError when it does not fit)."""
        if "kernel_size" not in kwargs:  # also for the unbound call with no arguments at all
            raise _need_kernel_size("img.equalize_hist")
        kernel_size = kwargs.pop("kernel_size")
        clip_limit = kwargs.pop("clip_limit", 0.01)
        nbins = kwargs.pop("nbins", 256)
        banded = bool(kwargs.pop("banded", False))
        if kwargs:
            raise NotImplementedError(f"equalize_hist options {kwargs} (kernel_size, clip_limit, nbins and banded "
                                      "are implemented)")
        if getattr(self, "_band", None) is not None:
            raise NotImplementedError("equalize_hist of a row band of a slide: the tiles and the extremes are the "
                                      "whole slide's")
        H, W = self.shape[0], self.shape[1]
        kh, kw, clip_limit, nbins = D.clahe_args(H, W, kernel_size, clip_limit, nbins)  # before any device call
        if banded and self._pending is None and not self._filter_deferred():
            src = self._source()
            if src is not None or not self._may_hold(H * W * self.n_ch * 4):
                self._equalize_deferred(src, channels, (kh, kw), clip_limit, nbins)
                return
        t = self._materialize()  # a slide that is not resident: _device()'s MemoryError
        for chs in self._channel_rounds(channels):
            t = D.clahe(t, kernel_size, clip_limit, nbins, enable=chs)
        self._set_device(t)
        self._xbound = None
        self._lognorm_host = None

    def _equalize_deferred(self, src, channels, kernel, clip_limit, nbins):
        """The banded form of ``equalize_hist``: per round the statistics now,
        band by band over ``src`` (None: the resident raw slide as a source)
        seen through the rounds before it, then the round stays deferred.
        ``_range`` is left as the resident call leaves it: not known."""
        from . import stream

        if src is None:
            src = stream.DeviceSource(self._device())
        rounds = list(self._pending_clahe or ())
        for chs in self._channel_rounds(channels):
            state = stream.clahe(src, kernel, clip_limit, nbins, enable=chs)
            rounds.append((state, kernel, clip_limit, nbins, chs))
            src = stream.ClaheSource(src, state)
        self._pending_clahe = rounds
        self._host64 = None
        self._range = None
        self._xbound = None
        self._lognorm_host = None

    show = _out_of_scope("img.show")

    def histogram(self, channels=None, bins=100, range=None, mask_out=False):
        """np.histogram of the current pixels of the planes ``channels`` (None:
        all; indices or names, a plane listed twice comes back twice; a 2-D
        image is one plane), each as float64 -- what ``self.img[:, :, c]``
        holds, everything pending applied -- counted on the device (D.histogram;
        the definition: DESIGN.md §27).  ``bins``: an int >= 1 (up to 4096);
        ``range``: a finite (lo, hi) for every plane (elements outside are left
        out), or None for each plane's own (nanmin, nanmax), as matplotlib's
        ``hist`` takes it; NaNs are never counted.  ``mask_out``: only pixels
        of the tissue mask take part, in the range too.  Returns (counts int64
        [n, bins], edges float64 [n, bins + 1]) as host arrays.

        A reader: the pixels do not change.  A slide that is not resident is
        read band by band (stream.histogram: twice, once with a range given),
        any pending log_normalize or deferred filter applied to each band and
        nothing pending cleared; otherwise the pixels are materialised as
        ``img`` does.  ValueError: ``bins`` below 1, a range that is not finite
        or has lo > hi, a plane without an element that is not NaN or with an
        infinite extreme (range None), ``mask_out`` without a mask."""
        from . import stream

        if getattr(self, "_band", None) is not None:
            raise NotImplementedError("histogram of a row band of a slide split over ranks: the counts are the "
                                      "whole slide's")
        bins, range = D.histogram_args(bins, range)  # before any device call
        feats = self._features(channels)
        names = [self.ch[f] for f in feats]
        mask = None
        if mask_out:
            if self._mask is None:
                raise ValueError("histogram(mask_out=True): the image has no tissue mask")
            mask = self._mask_device()
        src = self._source()
        if src is None and self._filter_deferred():
            # a resident slide whose filter stayed deferred (its fp32 copy may not be held): filtered band by band
            src = stream.DeviceSource(self._device())
        if src is not None:
            filt = stream.band_filter(self)
            if filt is None and self._pending is not None and self._pending[0] is not None:
                filt = stream.LogNormBand(*self._pending)
            return stream.histogram(src, feats, bins, range, mask, filt, names=names)
        return D.histogram(self._materialize(), feats, bins, range, mask, names=names)

    def plot_image_histogram(self=None, channels=None, ncols=4, save_to=None, **kwargs):
        """MxIF.py:733-774: one histogram of 100 bins per channel of
        ``channels`` (indices or names) on a grid of ``ncols`` columns, drawn
        from the device counts (``histogram``; no float64 copy of the slide).
        ``range=`` is the histogram's as well as the drawing's, ``mask_out=``
        the histogram's; every other keyword goes to ``Axes.hist`` (density,
        log, color, ...).  Saves the figure to ``save_to`` if given and returns
        the GridSpec.  ``channels`` must be given (the reference fails without
        them too)."""
        if self is None or channels is None:
            raise NotImplementedError("img.plot_image_histogram: pass channels= (a list of channel indices or names) "
                                      "to draw the device histograms")
        import matplotlib.pyplot as plt
        from matplotlib import gridspec

        if isinstance(channels, (int, np.integer, str)):
            channels = [channels]
        channels = list(channels)
        mask_out = bool(kwargs.pop("mask_out", False))
        n = len(channels)
        n_cols = n if n <= ncols else ncols
        n_rows = -(-n // n_cols) if n else 1
        fig = plt.figure(figsize=(ncols * n_cols, ncols * n_rows))
        gs = gridspec.GridSpec(n_rows, max(n_cols, 1), figure=fig)
        for i, channel in enumerate(channels):
            ax = plt.subplot(gs[i])
            counts, edges = self.histogram(channel, bins=100, range=kwargs.get("range"), mask_out=mask_out)
            ax.hist(edges[0][:-1], bins=edges[0], weights=counts[0], **kwargs)
            ax.set_title(channel, fontweight="bold", fontsize=16)
        fig.tight_layout()
        plt.show()
        if save_to:
            fig.savefig(save_to, dpi=300, bbox_inches="tight")
        return gs

    # ------------------------------------------------------- preprocessing
    def blurring(self, filter_name="gaussian", sigma=2, **kwargs):
        """MxIF.py:375-414.  'gaussian' runs the fused lognorm+blur kernel."""
        if filter_name == "gaussian":
            print("Applying gaussian filter")
            truncate = float(kwargs.pop("truncate", 4.0))
            eager = bool(kwargs.pop("_eager", False))  # private: blur every row now (tests)
            mode = kwargs.pop("mode", "nearest")
            kwargs.pop("preserve_range", None)
            if mode != "nearest" or kwargs:
                raise NotImplementedError(f"gaussian options {dict(mode=mode, **kwargs)} "
                                          "(only mode='nearest' is implemented)")
            if self._pending_median is not None or self._pending_bilateral is not None:
                self._materialize()  # a second filter: the deferred one applies first
            bound = self._blur_bound()
            self._blur_(float(sigma), truncate, eager)
            self._xbound = bound
        elif filter_name == "median" and "size" in kwargs:
            # what the reference's branch evidently means: skimage's
            # filters.median(plane, np.ones((k, k))) per channel, on the device
            size = D.median_size(kwargs.pop("size"))
            if kwargs:
                raise NotImplementedError(f"median options {kwargs} (only size is implemented)")
            print("Applying median filter")
            self.median_filter(size)
        elif filter_name == "median":
            # The reference's median branch calls np.ones(sigma, sigma), which
            # raises for any integer sigma (MxIF.py:403); keep that behaviour.
            print("Applying median filter")
            if isinstance(sigma, float):
                sigma = int(sigma)
            np.ones(sigma, sigma)
            raise NotImplementedError("median filter")
        elif filter_name == "bilateral" and "sigma_color" in kwargs:
            # only sigma_color= selects the device filter (as size= selects the
            # median): the bare call keeps raising, below
            sigma_color = kwargs.pop("sigma_color")
            opts = {k: kwargs.pop(k) for k in ("win_size", "bins", "mode", "cval", "banded") if k in kwargs}
            if kwargs:
                raise NotImplementedError(f"bilateral options {kwargs} (sigma_color, win_size, bins, mode, "
                                          "cval and banded are implemented)")
            print("Applying bilateral filter")
            self.bilateral_filter(sigma, sigma_color, **opts)
        elif filter_name == "bilateral":
            raise NotImplementedError("bilateral filter: pass sigma_color= (a number, or 'std' for the "
                                      "standard deviation of the whole image) to run the device filter")
        else:
            raise Exception("filter name should be either gaussian, median or bilateral")

    def median_filter(self, size):
        """Median filter per channel over a ``size`` window (an int or (rows,
        cols), up to 15), edges replicated: skimage's filters.median(plane,
        np.ones(size)) on every plane, exact (D.median).  A pending
        log_normalize alone is applied to the selected raw elements in the
        kernel's epilogue (selection commutes with the non-decreasing map:
        the same bits as normalising first); anything else pending is applied
        first.  A slide that is not resident, or whose filtered copy may not
        be held (the HBM budget), keeps the filter deferred
        (``_pending_median``): every pass that needs pixels applies it band by
        band (stream.MedianBand: the subsample, the label pass, the QC sums),
        which gives the resident filter's bits; ``_materialize`` applies it
        over the whole slide when that fits."""
        size = D.median_size(size)
        if getattr(self, "_band", None) is not None:
            raise NotImplementedError("median filter of a row band of a slide: the window needs the "
                                      "neighbour rows across the band edge")
        # an element of the window is within any bound on the window's elements
        bound = self._blur_bound()
        if bound is None and self._pending is None and self._pending_blur is None:
            bound = self._xbound
        if self._pending_median is not None or self._pending_bilateral is not None:
            self._materialize()  # a second filter: the deferred one applies first
        fused = self._pending is not None and self._pending[0] is not None and self._pending_blur is None
        if fused or self._pending is None:  # raw pixels (and a log_normalize): the state that can stay deferred
            H, W = self.shape[0], self.shape[1]
            if self._source() is not None or not self._may_hold(
                    H * W * self.n_ch * (4 if fused else self._elem_size())):
                self._pending_median = size
                self._host64 = None
                self._xbound = bound
                return
        if fused:
            inv, p = self._pending
            out = D.median(self._device(), size, inv_mean=inv, pseudoval=p)
        else:
            out = D.median(self._materialize(), size)
        self._pending = None
        self._pending_blur = None
        self._set_device(out)
        self._xbound = bound

    def bilateral_filter(self, sigma, sigma_color, win_size=None, bins=None, mode="constant", cval=0,
                         banded=False):
        """Bilateral filter over all channels jointly (D.bilateral; the
        definition and how it differs from skimage's denoise_bilateral:
        DESIGN.md §17).  ``sigma_color``: a positive number, or "std" for the
        float64 standard deviation of the whole image (the reference's
        default).  ``win_size`` defaults to max(5, 2 ceil(3 sigma) + 1), up to
        25; ``mode`` "constant" (``cval`` outside the image) or "edge";
        ``bins`` is accepted and ignored (the weight is exact, the limit of
        skimage's table).  A pending log_normalize alone is fused into the
        kernel's load (the same bits as normalising first); a pending gaussian
        or median is applied first.  The pixels become fp32.

        ``banded=False``: the slide must be resident and its fp32 result must
        fit the HBM budget (MemoryError otherwise).  ``banded=True`` permits
        the banded form: a slide that is not resident, or whose
        fp32 result may not be held, keeps the filter deferred
        (``_pending_bilateral``) and every pass that needs pixels -- the
        subsample, the label pass and the QC sums, each of them -- recomputes
        it band by band (stream.BilateralBand), with the resident filter's
        bits.  The bilateral is the heaviest stage per pixel, so a deferred one
        costs about three whole-slide filters per fit instead of one, plus one
        or two reads of the slide at the call for the whole-slide minimum,
        maximum and ("std") standard deviation (stream.image_moments): the
        caller chooses that knowingly.  A resident slide whose result may be
        held is filtered at once, exactly as with ``banded=False``."""
        std = isinstance(sigma_color, str) and sigma_color == "std"
        D.bilateral_args(sigma, 1.0 if std else sigma_color, win_size, mode, cval)  # before any device call
        if getattr(self, "_band", None) is not None:
            raise NotImplementedError("bilateral filter of a row band of a slide: the window needs the "
                                      "neighbour rows across the band edge")
        # the output is a convex combination of window elements and cval
        bound = self._blur_bound()
        if bound is None and self._pending is None and self._pending_blur is None:
            bound = self._xbound
        if bound is not None:
            bound = np.maximum(bound, abs(float(cval)))
        if self._filter_deferred():
            self._materialize()  # a second filter: the deferred one applies first
        H, W = self.shape[0], self.shape[1]
        rsrc = self._source()
        if rsrc is not None or not self._may_hold(H * W * self.n_ch * 4):
            if not banded:
                raise MemoryError("bilateral filter: the slide is not resident in HBM, or its fp32 result may "
                                  "not be held under the HBM budget; pass banded=True for the banded form of "
                                  "the bilateral filter (every pass that needs pixels then recomputes it band "
                                  "by band)")
            self._bilateral_deferred(rsrc, sigma, sigma_color, std, win_size, mode, cval, bound)
            return
        inv, p = self._pending if self._pending is not None else (None, 1.0)
        src = self._device()
        if std:
            sigma_color = D.image_std(src, inv_mean=inv, pseudoval=p)
            if not sigma_color > 0:  # a constant image: returned unchanged whatever the weight
                sigma_color = 1.0
        out = D.bilateral(src, sigma, sigma_color, win_size=win_size, mode=mode, cval=cval, inv_mean=inv,
                          pseudoval=p)
        self._pending = None
        self._set_device(out)
        self._xbound = bound

    def _bilateral_deferred(self, rsrc, sigma, sigma_color, std, win_size, mode, cval, bound):
        """The banded form of ``bilateral_filter``: the whole-slide moments now
        (over the source, or over the resident raw slide as a source: the same
        bits either way), then the filter stays deferred.  A constant slide is
        left as it is -- the filter is the identity by definition -- with a
        pending log_normalize still pending."""
        from . import stream

        inv, p = self._pending if self._pending is not None else (None, 1.0)
        m = stream.image_moments(rsrc if rsrc is not None else self._device(), inv, p, m2=std)
        if m[3] == m[4]:
            return
        if std:
            sigma_color = float(np.sqrt(m[2] / m[0]))
            if not sigma_color > 0:
                sigma_color = 1.0
        self._pending_bilateral = (float(sigma), float(sigma_color), win_size, mode, float(cval))
        self._host64 = None
        self._xbound = bound

    def _raw_int_max(self):
        """The largest value the current pixels' element type holds when they
        are a raw uint8 / uint16 slide (device, host or streamed), else None."""
        if self._pending_blur is not None or self._pending_bilateral is not None:
            return None
        if self._pending_rescale is not None or self._pending_clahe is not None:
            return None
        if self._dev_t is not None:
            t = self._dev_t.dtype
        elif self._host is not None:
            t = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16}.get(self._host.dtype)
        elif self._src is not None:
            t = self._src.dtype
        else:
            return None
        return {torch.uint8: 255.0, torch.int16: 65535.0}.get(t)  # int16 storage = uint16 bits

    def _blur_bound(self):
        """Per-channel bound on |x| of blur(lognorm(raw)) for a raw integer
        slide, known before any pixel is blurred: log10(x inv + p) is monotone
        in x in [0, dtype max], and the gaussian is a convex combination, so
        |x| <= max(|log10 p|, |log10(max inv + p)|) (max itself without a
        log_normalize), with slack for the fp32 arithmetic.  The exact QC sums
        take their fixed point from it (milwrm_amd.assign._DomainSSE): the
        label pass can then add each band's sums as it labels it, and the
        standalone estimators give the same bits without a first pass for the
        column maxima.  Clipped and scaled pixels are known as well, resident
        or deferred (``_range``): a clipped channel lies in [0, 1] ([-1, 1] when
        its lower percentile is negative), a scaled one in [0, 1], an untouched
        one keeps its raw type's range; a log_normalize on top needs every
        lower end >= 0.  None when the pixels are neither (a plane that scale
        turned into NaN, a channel with NaN pixels, untouched fp32)."""
        mx = self._raw_int_max()
        if mx is None:
            return self._range_bound()
        if self._pending is None:
            return np.full(self.n_ch, mx * (1 + 1e-3))
        if self._lognorm_host is None:
            return None
        inv, p = self._lognorm_host
        if not (np.isfinite(p) and p > 0):
            return None
        with np.errstate(invalid="ignore", over="ignore"):
            hi = np.log10(mx * inv.astype(np.float64) + p)
        return np.maximum(abs(np.log10(p)), np.abs(hi)) * (1 + 1e-3) + 1e-30

    def _range_bound(self):
        """``_blur_bound`` of clipped / scaled pixels (``_range``)."""
        if self._range is None or self._pending_blur is not None or self._pending_bilateral is not None:
            return None
        lo, hi = self._range
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            return None
        if self._pending is None:
            return np.maximum(np.abs(lo), np.abs(hi)) * (1 + 1e-3)
        if self._lognorm_host is None or (lo < 0).any():
            return None
        inv, p = self._lognorm_host
        if not (np.isfinite(p) and p > 0):
            return None
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            a = np.log10(lo * inv.astype(np.float64) + p)
            b = np.log10(hi * inv.astype(np.float64) + p)
        return np.maximum(np.abs(a), np.abs(b)) * (1 + 1e-3) + 1e-30

    def _blur_(self, sigma: float, truncate: float, eager: bool = False):
        """The gaussian branch of ``blurring``: deferred (streamed slide, or the
        fp32 copy would not fit) or materialised.  A materialised blur of a
        whole slide with a mask writes only the rows the labelling path can
        read and leaves the rest pending (``_blur_rest``) unless ``eager``."""
        if self._pending_median is not None or self._pending_bilateral is not None:
            self._materialize()  # a second filter: the deferred one applies first
        if self._pending_blur is None and self._source() is not None:
            # not resident: the blur runs inside every pass over the
            # streamed bands (stream.blur_gather, the banded label pass)
            self._pending_blur = (sigma, truncate)
            if self._pending is None:
                self._pending = (None, 1.0)  # no log-normalise before this blur
            self._host64 = None
            return
        src = self._materialize() if self._pending_blur is not None else self._device()
        if self._pending is not None and src.dim() == 3 and (
                D.defer_blur(*src.shape) or not self._may_hold(src.numel() * 4)):
            # fused-epilogue mode: the subsample gather and the label pass
            # recompute the blur from the raw slide (D.defer_blur, or the
            # fp32 copy of a host-backed slide would exceed the HBM budget)
            self._pending_blur = (sigma, truncate)
            self._host64 = None
            return
        self._pending_blur = (sigma, truncate)
        if self._pending is None:
            self._pending = (None, 1.0)
        inv, p = self._pending
        # the pending rest keeps the raw slide next to the fp32 one: only within the budget
        # (a row band of a slide gathers through whole-image reads: blurred whole)
        partial = (not eager and self._mask is not None and src.dim() == 3 and self._band is None
                   and self._may_hold(src.numel() * (4 + src.element_size())))
        rest = []

        def make():
            if not partial:
                return D.blur(src, sigma, inv_mean=inv, pseudoval=p, truncate=truncate)
            out, r = D.blur_needed(src, sigma, self._mask_device(), inv_mean=inv, pseudoval=p, truncate=truncate)
            rest.append(r)
            return out

        self._transformed(make)
        self._blur_rest = rest[0] if rest else None
        self._count_resident()

    def log_normalize(self, pseudoval=1, mean=None, mask=True):
        """MxIF.py:416-455: log10(x/mean_c + pseudoval) on every pixel.  The
        transform is deferred and fused into the next blur (or materialised
        when ``.img`` is read).  Deferred clip / scale rounds stay deferred:
        they apply before it."""
        if mask:
            assert self.mask is not None, "No tissue mask available"
        else:
            print("WARNING: Performing normalization without a tissue mask.")
        if mean is None:
            print("mean calculated to perform log normalization")
            s, _ = self._nz_stats()  # zeros add nothing: channel sum over all pixels
            n = self.shape[0] * self.shape[1]
            mean = s.cpu().numpy() / n
        elif self._pending is not None or self._pending_blur is not None or self._pending_bilateral is not None:
            # a transform already pending applies first (the median commutes with the
            # log and stays deferred; the bilateral does not)
            self._materialize()
        mean = np.asarray(mean, dtype=np.float64)
        with np.errstate(divide="ignore"):
            inv = (1.0 / mean).astype(np.float32)
        # a raw integer slide's bound survives a pending log_normalize (_blur_bound)
        raw = ((self._raw_int_max() is not None or self._range is not None) and self._pending is None
               and self._pending_blur is None and self._pending_bilateral is None)
        self._pending = (D.h2d(inv, D.device()), float(pseudoval))
        self._lognorm_host = (inv, float(pseudoval)) if raw else None
        self._xbound = None
        self._host64 = None

    def _subsample_device(self, features, fract=0.2, random_state=16, X_out=None, stats=None,
                          accumulate=False):
        """Device subsample: mask rank → legacy-RNG indices → row gather into
        ``X_out`` (fp32) with column statistics folded into ``stats``."""
        from .stream import bilateral_gather, blur_gather, median_gather

        features = self._features(features)
        np.random.seed(random_state)  # the reference's global-RNG side effect (MxIF.py:484)
        deferred = self._filter_deferred()
        src = None if deferred else self._needed_pixels()  # gather_rows reads mask pixels only
        r2p, M = self._mask_rank()
        dev = D.device()
        d_idx, total = subsample_indices_device(M, fract, random_state, dev)
        S = d_idx.shape[0]
        if X_out is None:
            X_out = torch.empty((S, len(features)), dtype=torch.float32, device=dev)
        if stats is None:
            stats = torch.zeros(1 + 2 * len(features), dtype=torch.float64, device=dev)
        if S:
            feat = D.h2d(np.asarray(features, dtype=np.int32), dev)
            if deferred:  # rows straight from the filter (resident or streamed slide)
                inv, p = self._pending if self._pending is not None else (None, 1.0)
                if self._pending_median is not None:
                    median_gather(self._source() or self._device(), self._pending_median, inv, p, feat,
                                  d_idx, r2p, X_out)
                elif self._pending_bilateral is not None:
                    bilateral_gather(self._source() or self._device(), self._pending_bilateral, inv, p, feat,
                                     d_idx, r2p, X_out)
                else:
                    sigma, truncate = self._pending_blur
                    blur_gather(self._source() or self._device(), sigma, inv, p, feat, d_idx, r2p, X_out,
                                truncate)
                D.col_stats_rows(X_out, stats, accumulate)
            else:
                D.gather_rows(src, feat, d_idx, r2p, X_out, stats, accumulate)
            check_total(total, S)
            set_global_state_after_draws()
        return X_out, stats

    def subsample_pixels(self, features, fract=0.2, random_state=16):
        """MxIF.py:457-492 — returns the float64 (S x F) host array."""
        X, _ = self._subsample_device(features, fract, random_state)
        return X.double().cpu().numpy()

    def downsample(self, fact, func=np.mean):
        """MxIF.py:494-517: skimage ``block_reduce(img, (fact, fact, 1), func,
        cval=0)`` for func = np.mean, np.sum, np.max, np.min or np.median (zero
        padded, the pad's zeros take part); the mask goes through the same
        func, as in the reference (np.mean: it becomes fractional).  A slide
        that is not resident is reduced band by band (stream.downsample), any
        pending log_normalize or deferred filter applied to each band first:
        the bits are the resident slide's.  A host mask comes back as a float64
        array; a device mask stays on the device as fp32."""
        from . import stream

        func = D.reduce_func(func)
        fact = D.reduce_fact(fact)
        if getattr(self, "_band", None) is not None:
            raise NotImplementedError("downsample of a row band of a slide split over ranks "
                                      "(the blocks straddle the bands)")
        src = self._source()
        if src is not None:
            filt = stream.band_filter(self)
            if filt is None and self._pending is not None and self._pending[0] is not None:
                filt = stream.LogNormBand(*self._pending)
            out = stream.downsample(src, fact, func, filt)
            self._pending = self._pending_blur = self._pending_median = self._pending_bilateral = None
            self._pending_rescale = None
            self._pending_clahe = None
            self._lognorm_host = None
        else:
            out = D.block_reduce(self._materialize(), fact, func)
        m = self._mask
        if isinstance(m, _DeviceMask):
            t = m._t if m._t.dtype in (torch.uint8, torch.float32) else m._t.to(torch.float32)
            small = D.block_reduce(t.contiguous()[:, :, None], fact, func)[:, :, 0]
            self.mask = _DeviceMask(small)
            self._mask_dev = D.padded_mask((small != 0).to(torch.uint8))
        elif m is not None:
            t = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)[:, :, None]).to(D.device())
            self.mask = D.block_reduce(t, fact, func)[:, :, 0].double().cpu().numpy()
        self._set_device(out)
        self._xbound = None

    def _nz_stats(self):
        """Per-channel non-zero (sum, count) of the current pixels: band by
        band when the raw slide is not resident (stream.nz_stats: exact
        integer sums for uint8 / uint16, the whole-slide bits)."""
        from . import stream

        src = self._source() if self._pending is None and not self._filter_deferred() else None
        if src is not None:
            D.FUSED_USED["nz_streamed"] += 1
            return stream.nz_stats(src)
        return D.nz_stats(self._materialize())

    def calculate_non_zero_mean(self, comm=None):
        """MxIF.py:519-541: ([mean_c * pixels], pixels) with pixels = non-zero
        elements over all channels.  A row band of a slide (milwrm_amd.bands)
        sums its band rows and all-reduces the exact integer-valued sums over
        ``comm``: every band returns the whole slide's values."""
        if getattr(self, "_band", None) is not None:
            s, c = D.nz_stats(self._materialize()[self._band.rows].contiguous())
            if comm is not None and comm.sharded():
                comm.all_reduce_(s)
                comm.all_reduce_(c)
            s, c = D.d2h(s, c)
            pixels = int(c.sum())
            with np.errstate(invalid="ignore", divide="ignore"):
                means = s / c
            return [float(m) * pixels for m in means], pixels
        s, c = self._nz_stats()
        pending = D.d2h_async(s, c)
        # the mask rank queued behind the copies: it runs while the host waits
        # for them and does the work that follows (the blur needs its result
        # only later), instead of before them
        self._prefetch_mask_rank()
        s, c = pending.wait()
        pixels = int(c.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            means = s / c
        return [float(m) * pixels for m in means], pixels

    def create_tissue_mask(self, features=None, fract=0.2):
        """MxIF.py:543-589 on the device kernels: log-normalise (global channel
        means), Gaussian sigma=2, subsample ``features``, KMeans(2,
        random_state=18) on the UNscaled samples, predict every pixel on ALL
        channels (as the reference's ``kmeans.predict(image_ar_reshape)``, so a
        feature subset raises sklearn's feature-count error), background flip."""
        from .assign import assign_image, banded_assign_image
        from .kmeans import DeviceRows, KMeans
        from .stream import band_filter

        cp = self.copy()
        H, W = cp.shape[0], cp.shape[1]
        if cp._source() is not None:
            # a slide read band by band: the all-ones mask lives on the device (as float64 on
            # the host it would be 8 bytes per pixel of a slide too large to hold)
            ones = torch.ones((H, W), dtype=torch.uint8, device=D.device())
            cp.mask = _DeviceMask(ones)
            cp._mask_dev = D.padded_mask(ones)
        else:
            cp.mask = np.ones((H, W))
        cp.log_normalize()
        cp.blurring("gaussian", sigma=2)
        X, st = cp._subsample_device(features, fract)
        stats = st.cpu().numpy()
        F = X.shape[1]
        var = stats[1 + F:] / stats[0]
        km = KMeans(n_clusters=2, random_state=18).fit(DeviceRows(X, feature_var=var))
        d = cp.n_ch
        if d != F:
            raise ValueError(f"X has {d} features, but KMeans is expecting {F} features as input.")
        res = None
        if cp._filter_deferred():
            # the blur was deferred (a slide that is not resident, or whose fp32 copy would not fit):
            # labelled band by band, the whole-slide bits (assign.banded_assign_image)
            res = banded_assign_image(cp._source() or cp._device(), band_filter(cp), list(range(d)), np.zeros(F),
                                      np.ones(F), km.cluster_centers_, cp._mask_device())
        if res is None:
            res = assign_image(D.as_float32(cp._materialize()), list(range(d)), np.zeros(F),
                               np.ones(F), km.cluster_centers_, cp._mask_device())
        tID = res[0].cpu().numpy().astype(float)
        scores = km.cluster_centers_
        z = (scores - scores.mean()) / scores.std()
        if z[0].mean() > 0:
            tID = np.where(tID == 0.0, 0.5, tID)
            tID = np.where(tID == 1.0, 0.0, tID)
            tID = np.where(tID == 0.5, 1.0, tID)
        self.mask = tID
