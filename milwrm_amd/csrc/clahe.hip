// Contrast-limited adaptive histogram equalisation on MI355X (gfx950).
//
//   clahe   img.equalize_hist / CLAHE -> skimage equalize_adapthist   MxIF.py:95-122, 360-373
//
// The definition is DESIGN.md §21.  Five stages on one stream, nothing returns
// to the host in between:
//   range   per-channel minimum and maximum as monotone uint32 keys
//   hist    the image streamed once with 16-byte loads, quantised in fp64,
//           counted into per-(tile, channel) LDS tables (the skewed 257-word
//           tables of intensity.hip) and merged into global memory with
//           integer atomics, once per workgroup
//   lut     one wave per histogram: clip, redistribute (the sequential loop of
//           the definition, a wave-wide count and a strided masked increment
//           per index), cumulative sum, look-up table, in place
//   map     per element the bin again, the four table entries (staged in LDS
//           per cell of pixels that share them where the tile is large enough,
//           else read from global memory), fp64 weights, the fp32 sum in the
//           defined order, the plane's extremes of the sum by integer atomics
//           on the fp32 bits
//   rescale mw_rescale in place with rows made on the device from the extremes
//
// The same stages over a slide handed over in bands of rows (mw_clahe_rows_*,
// DESIGN.md §26): the state is mw_clahe's workspace, kept between the calls.
// A band holds its own rows only, so its histogram pass is driven by the
// source rows (a row counts into its own tile row and, reflected, at most once
// more into the last), the blend's extremes are taken by a map pass that
// stores nothing, and the map pass proper writes the final pixels.  A band may
// start anywhere: the kernels get the 16-byte-aligned address below it and
// the elements in between as an offset.
#include <math.h>

#include <type_traits>

#include "common.h"

// the fp64 expressions must round as numpy's elementwise operations do
#pragma clang fp contract(off)

namespace mw {

constexpr int kClSlots = 32;       // 256-bin LDS tables per workgroup of the histogram pass (32 KB)
constexpr int kClTabStride = 257;  // words between tables: equal bins of different channels in different banks
constexpr int kClMaxC = 256;
constexpr int kClMaxBins = 256;
constexpr int kClLevels = 16384;   // G
constexpr int kClTilePixels = 8192;  // pixels of a tile per histogram workgroup: the merge costs nbins atomics
                                     // per table, 3 % of the LDS adds at 256 bins
constexpr int kClMapSeg = 16384;   // elements of a row per workgroup of the generic map pass (a multiple of 4)
constexpr int kClLdsEntSmall = 7680;    // (channel, bin) entries of the staged map pass: 60 KB, 30 channels x 256
constexpr int kClLdsEntLarge = 16384;   // 128 KB, one workgroup per CU: 64 channels x 256
constexpr int kClCellPixels = 4096;     // pixels of a cell per workgroup of the staged map pass

struct ClEnable { uint32_t w[kClMaxC / 32]; };
__device__ __forceinline__ bool cl_enabled(const ClEnable& en, int c) { return (en.w[c >> 5] >> (c & 31)) & 1u; }

template <typename T, int N>
struct alignas(sizeof(T) * N) ClPack { T v[N]; };

// monotone key of an element (-0.0 orders as +0.0) and its value back
template <typename T>
__device__ __forceinline__ uint32_t cl_key(T v) { return (uint32_t)v; }
template <>
__device__ __forceinline__ uint32_t cl_key<float>(float v) {
  uint32_t b = __float_as_uint(v);
  if (v == 0.0f) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
template <typename T>
__device__ __forceinline__ double cl_value(uint32_t key) { return (double)key; }
template <>
__device__ __forceinline__ double cl_value<float>(uint32_t key) {
  const uint32_t b = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  return (double)__uint_as_float(b);
}

// Step 1: rint((x - lo) / d * (G - 1)) // binsz; M = ceil(2^32 / binsz), and
// v M >> 32 = v / binsz for v < 2^14 as v (M binsz - 2^32) < 2^14 binsz < 2^32.
// The clamp changes no defined value: it keeps a NaN inside the table.
__device__ __forceinline__ int cl_bin(double x, double lo, double d, uint32_t M) {
  double r = rint((x - lo) / d * (double)(kClLevels - 1));
  r = fmin(fmax(r, 0.0), (double)(kClLevels - 1));
  return (int)__umulhi((uint32_t)r, M);
}

// The elements [sb, se) of one image row, spread over `nl` lanes: whole
// aligned vectors of V elements, and the fewer than V elements before the
// first and after the last of them one per lane.  f(e, values, n) gets the
// flat index of its first element; n is an integral_constant, 1 or V.  (f may
// store to the elements it was given: an fp32 band mapped in place.)
template <typename T, int V, typename F>
__device__ __forceinline__ void cl_walk(const T* img, int64_t sb, int64_t se, int lane, int nl, F&& f) {
  int64_t a0 = (sb + V - 1) / V * V;
  if (a0 > se) a0 = se;
  const int64_t a1 = a0 + (se - a0) / V * V;
  if (lane < a0 - sb) {
    const T v = img[sb + lane];
    f(sb + lane, &v, std::integral_constant<int, 1>{});
  }
  if (lane < se - a1) {
    const T v = img[a1 + lane];
    f(a1 + lane, &v, std::integral_constant<int, 1>{});
  }
  const int64_t stride = (int64_t)nl * V;
  int64_t e = a0 + (int64_t)lane * V;
  for (; e + stride < a1; e += 2 * stride) {  // two independent loads in flight
    const ClPack<T, V> p = *reinterpret_cast<const ClPack<T, V>*>(img + e);
    const ClPack<T, V> q = *reinterpret_cast<const ClPack<T, V>*>(img + e + stride);
    f(e, p.v, std::integral_constant<int, V>{});
    f(e + stride, q.v, std::integral_constant<int, V>{});
  }
  if (e < a1) {
    const ClPack<T, V> p = *reinterpret_cast<const ClPack<T, V>*>(img + e);
    f(e, p.v, std::integral_constant<int, V>{});
  }
}

// ------------------------------------------------------------------ range
// Workgroups take rows in turn.  An LDS cell is read before it is updated:
// after the first few elements almost no atomic is issued.  Row 0 starts `off`
// elements after the aligned `img` (0 for a whole image).
template <typename T>
__global__ void __launch_bounds__(256) clahe_range_kernel(const T* __restrict__ img, int64_t off, int H, int W,
                                                          int C, uint32_t* __restrict__ kmin,
                                                          uint32_t* __restrict__ kmax) {
  constexpr int V = 16 / sizeof(T);
  __shared__ uint32_t s_min[kClMaxC], s_max[kClMaxC];
  const int t = threadIdx.x;
  for (int c = t; c < C; c += 256) { s_min[c] = 0xffffffffu; s_max[c] = 0u; }
  __syncthreads();
  const int64_t rowlen = (int64_t)W * C;
  for (int y = blockIdx.x; y < H; y += gridDim.x) {
    const int64_t rowbase = off + (int64_t)y * rowlen;
    cl_walk<T, V>(img, rowbase, rowbase + rowlen, t, 256, [&](int64_t e, const T* v, auto nn) {
      constexpr int n = decltype(nn)::value;
      int c = (int)(e - rowbase) % C;
#pragma unroll
      for (int k = 0; k < n; ++k) {
        const uint32_t key = cl_key<T>(v[k]);
        if (key < *(volatile uint32_t*)&s_min[c]) atomicMin(&s_min[c], key);
        if (key > *(volatile uint32_t*)&s_max[c]) atomicMax(&s_max[c], key);
        if (++c == C) c = 0;
      }
    });
  }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    atomicMin(&kmin[c], s_min[c]);
    atomicMax(&kmax[c], s_max[c]);
  }
}

// ------------------------------------------------------------------ histograms
// The virtual rows [r0, r1) of tile (ti, tj), every channel, in rounds of
// kClSlots channels.  The four waves take the rows in turn.  A row past the
// image is the reflected row; the columns of the last tile column past the
// image are the contiguous run [2 W - 1 - (j + 1) kw, W - 1) of the same row
// (the order inside a histogram does not matter), so no address outside the
// image is formed.  `img` holds the slide's rows from `yb` on, the first of
// them `off` elements after it; the caller passes only rows it holds.
template <typename T>
__device__ __forceinline__ void cl_hist_tile(const T* __restrict__ img, int64_t off, int yb, int ti, int tj, int r0,
                                             int r1, int H, int W, int C, int kw, int nby, int nbx, int nbins,
                                             uint32_t M, const uint32_t* __restrict__ kmin,
                                             const uint32_t* __restrict__ kmax, const ClEnable& en,
                                             uint32_t* __restrict__ hist) {
  constexpr int V = 16 / sizeof(T);
  __shared__ unsigned int tab[kClSlots * kClTabStride];
  __shared__ double s_lo[kClMaxC], s_d[kClMaxC];
  __shared__ int s_off[kClMaxC];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int xs = tj * kw, xe = min(W, xs + kw);
  const bool over = xs + kw > W;
  const int fs = over ? 2 * W - 1 - (xs + kw) : 0, fe = over ? W - 1 : 0;
  for (int c = t; c < C; c += 256) {
    const double lo = cl_value<T>(kmin[c]);
    s_lo[c] = lo;
    s_d[c] = cl_value<T>(kmax[c]) - lo;
  }
  __syncthreads();
  const int groups = (C + kClSlots - 1) / kClSlots;
  for (int g = 0; g < groups; ++g) {
    for (int q = t; q < kClSlots * kClTabStride; q += 256) tab[q] = 0u;
    for (int c = t; c < C; c += 256) {
      const int rel = c - g * kClSlots;
      const bool live = rel >= 0 && rel < kClSlots && cl_enabled(en, c) && s_d[c] > 0.0;
      s_off[c] = live ? rel * kClTabStride : -1;
    }
    __syncthreads();
    for (int r = r0 + wid; r < r1; r += 4) {
      const int ys = r < H ? r : 2 * H - 2 - r;
      const int64_t rowbase = off + (int64_t)(ys - yb) * W * C;
      auto take = [&](int64_t e, const T* v, auto nn) {
        constexpr int n = decltype(nn)::value;
        int c = (int)(e - rowbase) % C;
#pragma unroll
        for (int k = 0; k < n; ++k) {
          const int off_c = s_off[c];
          if (off_c >= 0) atomicAdd(&tab[off_c + cl_bin((double)v[k], s_lo[c], s_d[c], M)], 1u);
          if (++c == C) c = 0;
        }
      };
      cl_walk<T, V>(img, rowbase + (int64_t)xs * C, rowbase + (int64_t)xe * C, lane, 64, take);
      if (fe > fs) cl_walk<T, V>(img, rowbase + (int64_t)fs * C, rowbase + (int64_t)fe * C, lane, 64, take);
    }
    __syncthreads();
    const int here = min(kClSlots, C - g * kClSlots);
    for (int q = t; q < here * nbins; q += 256) {
      const int rel = q / nbins, b = q - rel * nbins;
      const unsigned int v = tab[rel * kClTabStride + b];
      if (v) atomicAdd(&hist[(((size_t)(g * kClSlots + rel) * nby + ti) * nbx + tj) * nbins + b], v);
    }
    __syncthreads();
  }
}

// The whole image.  Workgroup (chunk, i, j): rows [i kh + chunk rpc, ... + rpc)
// of tile (i, j), the rows past the image among them.
template <typename T>
__global__ void __launch_bounds__(256) clahe_hist_kernel(const T* __restrict__ img, int H, int W, int C, int kh,
                                                         int kw, int nby, int nbx, int rpc, int nbins, uint32_t M,
                                                         const uint32_t* __restrict__ kmin,
                                                         const uint32_t* __restrict__ kmax, ClEnable en,
                                                         uint32_t* __restrict__ hist) {
  int bid = blockIdx.x;
  const int tj = bid % nbx;
  bid /= nbx;
  const int ti = bid % nby;
  const int chunk = bid / nby;
  const int r0 = ti * kh + chunk * rpc, r1 = min((ti + 1) * kh, r0 + rpc);
  cl_hist_tile<T>(img, 0, 0, ti, tj, r0, r1, H, W, C, kw, nby, nbx, nbins, M, kmin, kmax, en, hist);
}

// A band, driven by its source rows.  The virtual rows [v0, v1) are either the
// band's own rows [yb, yb + rows) or the rows r in [H, nby kh) whose source
// 2 H - 2 - r lies in the band (all of them in tile row nby - 1).  Workgroup
// (chunk, i, j): the rows of [v0, v1) in tile row t0 + i, from its first on in
// chunks of rpc, of tile column j.  The counts are integer atomics: the totals
// over all bands are clahe_hist_kernel's.
template <typename T>
__global__ void __launch_bounds__(256) clahe_hist_rows_kernel(const T* __restrict__ img, int64_t off, int yb, int v0,
                                                              int v1, int t0, int nt, int H, int W, int C, int kh,
                                                              int kw, int nby, int nbx, int rpc, int nbins,
                                                              uint32_t M, const uint32_t* __restrict__ kmin,
                                                              const uint32_t* __restrict__ kmax, ClEnable en,
                                                              uint32_t* __restrict__ hist) {
  int bid = blockIdx.x;
  const int tj = bid % nbx;
  bid /= nbx;
  const int ti = t0 + bid % nt;
  const int chunk = bid / nt;
  const int r0 = max(v0, ti * kh) + chunk * rpc, r1 = min(min(v1, (ti + 1) * kh), r0 + rpc);
  if (r0 >= r1) return;  // the whole workgroup
  cl_hist_tile<T>(img, off, yb, ti, tj, r0, r1, H, W, C, kw, nby, nbx, nbins, M, kmin, kmax, en, hist);
}

// ------------------------------------------------------------------ clip + map
// One wave per histogram, bins 4 lane .. 4 lane + 3 in the lane.  The counts
// become the look-up table in place.
__global__ void __launch_bounds__(256) clahe_lut_kernel(uint32_t* __restrict__ hist, int64_t n_hist, int nbins,
                                                        int clim, double scale, int* __restrict__ luts_out) {
  const int lane = threadIdx.x & 63;
  const int64_t id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (id >= n_hist) return;
  uint32_t* hp = hist + (size_t)id * nbins;
  int h[4];
  bool real[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    real[r] = lane * 4 + r < nbins;
    h[r] = real[r] ? (int)hp[lane * 4 + r] : 0;
  }
  long long part = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (real[r] && h[r] > clim) { part += h[r] - clim; h[r] = clim; }
  long long n_ex = wave_sum(part);
  const int incr = (int)(n_ex / nbins), upper = clim - incr;
  int low = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (real[r] && h[r] < upper) { h[r] += incr; ++low; }
  n_ex -= (long long)wave_sum(low) * incr;
  part = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (real[r] && h[r] >= upper && h[r] < clim) { part += h[r] - clim; h[r] = clim; }
  n_ex += wave_sum(part);
  while (n_ex > 0) {
    const long long prev = n_ex;
    for (int index = 0; index < nbins; ++index) {
      int under = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) under += real[r] && h[r] < clim;
      under = wave_sum(under);
      const int step = n_ex >= under ? 1 : under / (int)n_ex;  // max(1, under // n_ex)
      int add = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rel = lane * 4 + r - index;
        if (real[r] && rel >= 0 && h[r] < clim && (step == 1 || rel % step == 0)) { ++h[r]; ++add; }
      }
      n_ex -= wave_sum(add);
      if (n_ex <= 0) break;
    }
    if (prev == n_ex) break;
  }
  unsigned long long s = 0ull;
#pragma unroll
  for (int r = 0; r < 4; ++r) s += (unsigned long long)h[r];
  unsigned long long incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  unsigned long long run = incl - s;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    run += (unsigned long long)h[r];
    if (real[r]) {
      const int v = (int)fmin((double)run * scale, (double)(kClLevels - 1));
      hp[lane * 4 + r] = (uint32_t)v;
      if (luts_out) luts_out[(size_t)id * nbins + lane * 4 + r] = v;
    }
  }
}

// ------------------------------------------------------------------ map
// Step 5's sum: fp32 terms of fp64 products, added in the defined order
__device__ __forceinline__ float cl_blend(int v00, int v01, int v10, int v11, double w00, double w01, double w10,
                                          double w11) {
  float res = (float)((double)v00 * w00);
  res += (float)((double)v01 * w01);
  res += (float)((double)v10 * w10);
  res += (float)((double)v11 * w11);
  return res;
}

// What a map kernel does with the blend.  kClWhole (mw_clahe): stores it and
// keeps its extremes, mw_rescale follows.  The bands: kClExtremes keeps the
// extremes and stores nothing; kClFinal, after clahe_params_kernel, stores the
// final pixels, the blend through its plane's rescale row as rescale_kernel
// evaluates it: (float)(((double)res - lo) / (hi - lo)) in mode 3, 0 in mode
// 2, the value itself in mode 0.
enum { kClWhole = 0, kClExtremes = 1, kClFinal = 2 };

// The per-channel tables of a map kernel in LDS.  mode 0: the value itself,
// 1: zero (a constant plane; kClFinal: also a constant blend), 2: equalised.
struct ClMapChan {
  double lo[kClMaxC], d[kClMaxC];      // the plane's minimum and extent
  double rlo[kClMaxC], rd[kClMaxC];    // kClFinal: the blend's minimum and extent
  uint32_t mn[kClMaxC], mx[kClMaxC];   // else: the extremes of the blend seen by this workgroup
  int mode[kClMaxC];
};

template <typename T, int kPass>
__device__ __forceinline__ void cl_map_chan_init(ClMapChan& s, int C, int t, int nt,
                                                 const uint32_t* __restrict__ kmin,
                                                 const uint32_t* __restrict__ kmax, const ClEnable& en,
                                                 const double* __restrict__ params) {
  for (int c = t; c < C; c += nt) {
    const double lo = cl_value<T>(kmin[c]), d = cl_value<T>(kmax[c]) - lo;
    s.lo[c] = lo;
    s.d[c] = d;
    if constexpr (kPass == kClFinal) {
      const int pm = (int)params[c * 5 + 4];
      s.mode[c] = pm == 0 ? 0 : (pm == 3 ? 2 : 1);
      s.rlo[c] = params[c * 5 + 0];
      s.rd[c] = params[c * 5 + 1] - params[c * 5 + 0];
    } else {
      s.mode[c] = !cl_enabled(en, c) ? 0 : (d > 0.0 ? 2 : 1);
      s.mn[c] = 0xffffffffu;
      s.mx[c] = 0u;
    }
  }
}

// an element of a plane with mode != 0: the blend `res` (0 unless mode 2) to its extremes or to the final pixel
template <int kPass>
__device__ __forceinline__ float cl_map_finish(ClMapChan& s, int c, int mode, float res) {
  if constexpr (kPass == kClFinal) {
    return mode == 2 ? (float)(((double)res - s.rlo[c]) / s.rd[c]) : 0.0f;
  } else {
    const uint32_t bits = __float_as_uint(res);  // res >= 0: the bits order as the values
    if (bits < *(volatile uint32_t*)&s.mn[c]) atomicMin(&s.mn[c], bits);
    if (bits > *(volatile uint32_t*)&s.mx[c]) atomicMax(&s.mx[c], bits);
    return res;
  }
}

// n = 1 or 4 pixels' elements to out[at ..]; a band's vector may start off the 16-byte grid
template <int kPass, int n>
__device__ __forceinline__ void cl_map_store(float* out, int64_t at, const float* o) {
  if constexpr (kPass == kClExtremes) {
    return;
  } else if constexpr (n == 1) {
    out[at] = o[0];
  } else if constexpr (kPass == kClWhole) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 ov;
#pragma unroll
    for (int k = 0; k < 4; ++k) ov[k] = o[k];
    *reinterpret_cast<f4*>(out + at) = ov;
  } else {
    struct __attribute__((packed, aligned(4))) F4u { float v[4]; };
    F4u ov;
#pragma unroll
    for (int k = 0; k < 4; ++k) ov.v[k] = o[k];
    *reinterpret_cast<F4u*>(out + at) = ov;
  }
}

template <int kPass>
__device__ __forceinline__ void cl_map_merge(ClMapChan& s, int C, int t, int nt, uint32_t* __restrict__ rmin,
                                             uint32_t* __restrict__ rmax) {
  if constexpr (kPass != kClFinal) {
    for (int c = t; c < C; c += nt)
      if (s.mode[c] != 0 && s.mx[c] >= s.mn[c]) {
        atomicMin(&rmin[c], s.mn[c]);
        atomicMax(&rmax[c], s.mx[c]);
      }
  }
}

// The generic form, for tiles too small to pay for staging their tables (or
// tables too large for LDS): the four table entries are read from global
// memory.  Workgroup (y, part): kClMapSeg elements of row yb + y.  `img`
// holds the `rows` rows from slide row `yb` on, the first of them `off`
// elements after it, and `out` those rows' pixels (it may be the band itself:
// a thread writes the elements it has read); the whole image is yb = off = 0.
template <typename T, int kPass>
__global__ void __launch_bounds__(256) clahe_map_kernel(const T* img, int64_t off, int yb, float* out, int W, int C,
                                                        int kh, int kw, int nby, int nbx, int nbins, int parts,
                                                        uint32_t M, const uint32_t* __restrict__ kmin,
                                                        const uint32_t* __restrict__ kmax, ClEnable en,
                                                        const int* __restrict__ lut,
                                                        const double* __restrict__ params,
                                                        uint32_t* __restrict__ rmin, uint32_t* __restrict__ rmax) {
  constexpr int V = 4;
  __shared__ ClMapChan s;
  const int t = threadIdx.x;
  cl_map_chan_init<T, kPass>(s, C, t, 256, kmin, kmax, en, params);
  __syncthreads();
  const int yl = blockIdx.x / parts, part = blockIdx.x - yl * parts, y = yb + yl;
  const int64_t rowlen = (int64_t)W * C, rowbase = off + (int64_t)yl * rowlen;
  const int64_t sb = rowbase + (int64_t)part * kClMapSeg, se = min(rowbase + rowlen, sb + kClMapSeg);
  const int py = y + kh / 2, ti = py / kh;
  const double ry = (double)(py - ti * kh) / (double)kh;
  const double wy0 = 1.0 - ry, wy1 = ry;
  const int i0 = min(max(ti - 1, 0), nby - 1), i1 = min(ti, nby - 1);
  const size_t plane = (size_t)nby * nbx * nbins;
  cl_walk<T, V>(img, sb, se, t, 256, [&](int64_t e, const T* v, auto nn) {
    constexpr int n = decltype(nn)::value;
    const int er = (int)(e - rowbase);
    int x = er / C, c = er - x * C;
    size_t o00, o01, o10, o11;
    double w00, w01, w10, w11;
    auto column = [&]() {
      const int px = x + kw / 2, tj = px / kw;
      const double rx = (double)(px - tj * kw) / (double)kw;
      const double wx0 = 1.0 - rx, wx1 = rx;
      const int j0 = min(max(tj - 1, 0), nbx - 1), j1 = min(tj, nbx - 1);
      o00 = (size_t)(i0 * nbx + j0) * nbins;
      o01 = (size_t)(i0 * nbx + j1) * nbins;
      o10 = (size_t)(i1 * nbx + j0) * nbins;
      o11 = (size_t)(i1 * nbx + j1) * nbins;
      w00 = wy0 * wx0;
      w01 = wy0 * wx1;
      w10 = wy1 * wx0;
      w11 = wy1 * wx1;
    };
    column();
    float o[n];
#pragma unroll
    for (int k = 0; k < n; ++k) {
      const int mode = s.mode[c];
      float res = (float)v[k];
      if (mode != 0) {
        res = 0.0f;
        if (mode == 2) {
          const int* p = lut + (size_t)c * plane + cl_bin((double)v[k], s.lo[c], s.d[c], M);
          res = cl_blend(p[o00], p[o01], p[o10], p[o11], w00, w01, w10, w11);
        }
        res = cl_map_finish<kPass>(s, c, mode, res);
      }
      o[k] = res;
      if (++c == C) {
        c = 0;
        ++x;
        if (k + 1 < n) column();
      }
    }
    cl_map_store<kPass, n>(out, e - off, o);
  });
  __syncthreads();
  cl_map_merge<kPass>(s, C, t, 256, rmin, rmax);
}

// The staged form.  The pixels whose four nearest tile centres are the same
// form a cell: rows with (y + kh / 2) / kh = ci, columns likewise.  Workgroup
// (chunk, ci, cj) stages the cell's four tables of every channel in LDS, one
// 8-byte entry of four uint16 (a table value is below 2^14) per (channel,
// bin), so an element costs one LDS read where the generic form makes four
// scattered global reads; then its eight waves take the rows of its chunk of
// the cell in turn.  `img`, `off`, `out` as clahe_map_kernel: the slide rows
// [yb, ye) (the whole image: [0, H)), whose cell rows are ci0 .. ci0 + ncy - 1;
// a cell the band cuts is clipped to the band's rows.
template <typename T, int kEnt, int kPass>
__global__ void __launch_bounds__(512) clahe_map_lds_kernel(const T* img, int64_t off, int yb, int ye, float* out,
                                                            int W, int C, int kh, int kw, int nby, int nbx,
                                                            int nbins, int ci0, int ncy, int ncx, int rpc,
                                                            uint32_t M, const uint32_t* __restrict__ kmin,
                                                            const uint32_t* __restrict__ kmax, ClEnable en,
                                                            const int* __restrict__ lut,
                                                            const double* __restrict__ params,
                                                            uint32_t* __restrict__ rmin,
                                                            uint32_t* __restrict__ rmax) {
  constexpr int V = 4;
  __shared__ uint2 s_lut[kEnt];
  __shared__ ClMapChan s;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  int bid = blockIdx.x;
  const int cj = bid % ncx;
  bid /= ncx;
  const int ci = ci0 + bid % ncy;
  const int chunk = bid / ncy;
  const int y0 = max(yb, ci * kh - kh / 2) + chunk * rpc, y1 = min(min(ye, (ci + 1) * kh - kh / 2), y0 + rpc);
  if (y0 >= y1) return;  // the whole workgroup
  const int x0 = max(0, cj * kw - kw / 2), x1 = min(W, (cj + 1) * kw - kw / 2);
  const int i0 = min(max(ci - 1, 0), nby - 1), i1 = min(ci, nby - 1);
  const int j0 = min(max(cj - 1, 0), nbx - 1), j1 = min(cj, nbx - 1);
  cl_map_chan_init<T, kPass>(s, C, t, 512, kmin, kmax, en, params);
  {
    const size_t plane = (size_t)nby * nbx * nbins;
    const size_t o00 = (size_t)(i0 * nbx + j0) * nbins, o01 = (size_t)(i0 * nbx + j1) * nbins;
    const size_t o10 = (size_t)(i1 * nbx + j0) * nbins, o11 = (size_t)(i1 * nbx + j1) * nbins;
    for (int q = t; q < C * nbins; q += 512) {
      const int c = q / nbins;
      const int* p = lut + (size_t)c * plane + (q - c * nbins);
      s_lut[q] = make_uint2((uint32_t)p[o00] | ((uint32_t)p[o01] << 16), (uint32_t)p[o10] | ((uint32_t)p[o11] << 16));
    }
  }
  __syncthreads();
  for (int y = y0 + wid; y < y1; y += 8) {
    const int64_t rowbase = off + (int64_t)(y - yb) * W * C;
    const double ry = (double)(y + kh / 2 - ci * kh) / (double)kh;
    const double wy0 = 1.0 - ry, wy1 = ry;
    cl_walk<T, V>(img, rowbase + (int64_t)x0 * C, rowbase + (int64_t)x1 * C, lane, 64,
                  [&](int64_t e, const T* v, auto nn) {
      constexpr int n = decltype(nn)::value;
      const int er = (int)(e - rowbase);
      int x = er / C, c = er - x * C;
      double w00, w01, w10, w11;
      auto column = [&]() {
        const double rx = (double)(x + kw / 2 - cj * kw) / (double)kw;
        const double wx0 = 1.0 - rx, wx1 = rx;
        w00 = wy0 * wx0;
        w01 = wy0 * wx1;
        w10 = wy1 * wx0;
        w11 = wy1 * wx1;
      };
      column();
      float o[n];
#pragma unroll
      for (int k = 0; k < n; ++k) {
        const int mode = s.mode[c];
        float res = (float)v[k];
        if (mode != 0) {
          res = 0.0f;
          if (mode == 2) {
            const uint2 q = s_lut[c * nbins + cl_bin((double)v[k], s.lo[c], s.d[c], M)];
            res = cl_blend((int)(q.x & 0xffffu), (int)(q.x >> 16), (int)(q.y & 0xffffu), (int)(q.y >> 16), w00, w01,
                           w10, w11);
          }
          res = cl_map_finish<kPass>(s, c, mode, res);
        }
        o[k] = res;
        if (++c == C) {
          c = 0;
          ++x;
          if (k + 1 < n) column();
        }
      }
      cl_map_store<kPass, n>(out, e - off, o);
    });
  }
  __syncthreads();
  cl_map_merge<kPass>(s, C, t, 512, rmin, rmax);
}

// mw_rescale's rows from the extremes of the blend: (res - rmin) / (rmax -
// rmin) (mode 3), 0 for a plane whose blend is constant (mode 2 clipped to
// [0, 0]), the value itself for a plane that is not enabled (mode 0)
__global__ void clahe_params_kernel(int C, ClEnable en, const uint32_t* __restrict__ rmin,
                                    const uint32_t* __restrict__ rmax, double* __restrict__ params) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double lo = 0.0, hi = 0.0, mode = 0.0;
  if (cl_enabled(en, c)) {
    if (rmin[c] < rmax[c]) {
      lo = (double)__uint_as_float(rmin[c]);
      hi = (double)__uint_as_float(rmax[c]);
      mode = 3.0;
    } else {
      mode = 2.0;
    }
  }
  params[c * 5 + 0] = lo;
  params[c * 5 + 1] = hi;
  params[c * 5 + 2] = 0.0;
  params[c * 5 + 3] = mode == 3.0 ? 1.0 : 0.0;
  params[c * 5 + 4] = mode;
}

static inline size_t cl_al16(size_t n) { return (n + 15) & ~(size_t)15; }

struct ClLayout { size_t mins, maxs, params, hist, total; };
static ClLayout cl_layout(int H, int W, int C, int kh, int kw, int nbins) {
  const size_t nby = ((size_t)H + kh - 1) / kh, nbx = ((size_t)W + kw - 1) / kw;
  ClLayout o;
  size_t at = 0;
  o.mins = at;   at += cl_al16((size_t)2 * C * 4);  // key minima, then the blend's minima
  o.maxs = at;   at += cl_al16((size_t)2 * C * 4);
  o.params = at; at += cl_al16((size_t)C * 5 * 8);
  o.hist = at;   at += cl_al16((size_t)C * nby * nbx * nbins * 4);  // counts, then the tables in place
  o.total = at;
  return o;
}

// MW_OK, or the status of the first argument that cannot be served (no device call)
static int cl_check(int dtype, int H, int W, int C, int kh, int kw, double clip_limit, int nbins) {
  MW_CHECK_ARG(H >= 2 && W >= 2 && C >= 1, "mw_clahe: bad shape H=%d W=%d C=%d (H and W at least 2)", H, W, C);
  MW_CHECK_ARG(kh >= 1 && kh <= H && kw >= 1 && kw <= W,
               "mw_clahe: kernel %d x %d outside 1..%d x 1..%d (the image's extent)", kh, kw, H, W);
  MW_CHECK_ARG(isfinite(clip_limit) && clip_limit > 0.0, "mw_clahe: clip_limit=%g must be positive and finite",
               clip_limit);
  MW_CHECK_ARG(nbins >= 2, "mw_clahe: nbins=%d below 2", nbins);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_clahe: bad dtype %d", dtype);
  if (nbins > kClMaxBins) {
    set_error("mw_clahe: nbins=%d (up to %d)", nbins, kClMaxBins);
    return MW_EUNSUPPORTED;
  }
  if (C > kClMaxC) {
    set_error("mw_clahe: %d channels (up to %d)", C, kClMaxC);
    return MW_EUNSUPPORTED;
  }
  const int64_t nby = ((int64_t)H + kh - 1) / kh, nbx = ((int64_t)W + kw - 1) / kw;
  const int64_t parts = ((int64_t)W * C + kClMapSeg - 1) / kClMapSeg;
  if ((int64_t)W * C >= ((int64_t)1 << 31) || (int64_t)kh * kw >= ((int64_t)1 << 31) ||
      nby * nbx * kh >= ((int64_t)1 << 31) || (int64_t)H * parts >= ((int64_t)1 << 31)) {
    set_error("mw_clahe: H=%d W=%d C=%d kernel %d x %d: a row, a tile or a grid of 2^31 or more", H, W, C, kh, kw);
    return MW_EUNSUPPORTED;
  }
  return MW_OK;
}

static ClEnable cl_enable_of(const int* h_enable, int C) {
  ClEnable en;
  for (int i = 0; i < kClMaxC / 32; ++i) en.w[i] = 0u;
  for (int c = 0; c < C; ++c)
    if (!h_enable || h_enable[c]) en.w[c >> 5] |= 1u << (c & 31);
  return en;
}

// The geometry of one equalisation and the sections of its workspace (the
// state of the mw_clahe_rows_* calls)
struct ClPlan {
  int H, W, C, kh, kw, nby, nbx, nbins;
  uint32_t M;
  ClEnable en;
  uint32_t *kmin, *kmax, *rmin, *rmax, *hist;
  double* params;
};
static ClPlan cl_plan(int H, int W, int C, const int* h_enable, int kh, int kw, int nbins, void* d_ws) {
  const ClLayout lay = cl_layout(H, W, C, kh, kw, nbins);
  char* ws = reinterpret_cast<char*>(d_ws);
  ClPlan p;
  p.H = H; p.W = W; p.C = C; p.kh = kh; p.kw = kw; p.nbins = nbins;
  p.nby = (H + kh - 1) / kh;
  p.nbx = (W + kw - 1) / kw;
  const uint32_t binsz = 1u + (uint32_t)(kClLevels / nbins);
  p.M = 0xffffffffu / binsz + 1u;
  p.en = cl_enable_of(h_enable, C);
  p.kmin = reinterpret_cast<uint32_t*>(ws + lay.mins);
  p.kmax = reinterpret_cast<uint32_t*>(ws + lay.maxs);
  p.rmin = p.kmin + C;
  p.rmax = p.kmax + C;
  p.params = reinterpret_cast<double*>(ws + lay.params);
  p.hist = reinterpret_cast<uint32_t*>(ws + lay.hist);
  return p;
}

static int cl_clear(const ClPlan& p, void* d_ws, hipStream_t s) {
  const ClLayout lay = cl_layout(p.H, p.W, p.C, p.kh, p.kw, p.nbins);
  char* ws = reinterpret_cast<char*>(d_ws);
  MW_HIP(hipMemsetAsync(ws + lay.mins, 0xff, lay.maxs - lay.mins, s));
  MW_HIP(hipMemsetAsync(ws + lay.maxs, 0, lay.total - lay.maxs, s));
  return MW_OK;
}

static inline int cl_hist_rpc(const ClPlan& p) {
  const int rpc = (kClTilePixels + p.kw - 1) / p.kw;
  return std::min(p.kh, (rpc + 3) / 4 * 4);
}

static int cl_luts(const ClPlan& p, double clip_limit, int* d_luts_out, hipStream_t s) {
  const double area = (double)p.kh * (double)p.kw;
  double climd = clip_limit * (double)p.kh * (double)p.kw;  // in the definition's order
  if (!(climd >= 1.0)) climd = 1.0;
  const int clim = (int)(climd < area ? climd : area);  // a limit above the tile's count clips nothing
  const double scale = (double)(kClLevels - 1) / area;
  const int64_t n_hist = (int64_t)p.C * p.nby * p.nbx;
  hipLaunchKernelGGL(clahe_lut_kernel, dim3((unsigned)((n_hist + 3) / 4)), dim3(256), 0, s, p.hist, n_hist, p.nbins,
                     clim, scale, d_luts_out);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

// The map pass over the slide rows [yb, yb + rows) at img + off (the whole
// image: yb = off = 0, rows = H): staged where the tables fit LDS and a cell
// has at least two elements per table word it stages, else generic
template <typename T, int kPass>
static int cl_map(const ClPlan& p, const T* img, int64_t off, int yb, int rows, float* d_out, hipStream_t s) {
  const int* lut = reinterpret_cast<const int*>(p.hist);
  const int ci0 = (yb + p.kh / 2) / p.kh, ncy = (yb + rows - 1 + p.kh / 2) / p.kh - ci0 + 1;
  const int ncx = (p.W - 1 + p.kw / 2) / p.kw + 1;
  int mrpc = (kClCellPixels + p.kw - 1) / p.kw;
  mrpc = std::min(p.kh, (mrpc + 7) / 8 * 8);
  const int mchunks = (std::min(p.kh, rows) + mrpc - 1) / mrpc;
  const int64_t cells = (int64_t)ncy * ncx * mchunks;
  const int ent = p.C * p.nbins;
  if (ent <= kClLdsEntLarge && (int64_t)p.kh * p.kw >= (int64_t)8 * p.nbins && cells < ((int64_t)1 << 31)) {
    if (ent <= kClLdsEntSmall)
      hipLaunchKernelGGL((clahe_map_lds_kernel<T, kClLdsEntSmall, kPass>), dim3((unsigned)cells), dim3(512), 0, s,
                         img, off, yb, yb + rows, d_out, p.W, p.C, p.kh, p.kw, p.nby, p.nbx, p.nbins, ci0, ncy, ncx,
                         mrpc, p.M, p.kmin, p.kmax, p.en, lut, p.params, p.rmin, p.rmax);
    else
      hipLaunchKernelGGL((clahe_map_lds_kernel<T, kClLdsEntLarge, kPass>), dim3((unsigned)cells), dim3(512), 0, s,
                         img, off, yb, yb + rows, d_out, p.W, p.C, p.kh, p.kw, p.nby, p.nbx, p.nbins, ci0, ncy, ncx,
                         mrpc, p.M, p.kmin, p.kmax, p.en, lut, p.params, p.rmin, p.rmax);
  } else {
    const int parts = (int)(((int64_t)p.W * p.C + kClMapSeg - 1) / kClMapSeg);
    hipLaunchKernelGGL((clahe_map_kernel<T, kPass>), dim3((unsigned)(rows * parts)), dim3(256), 0, s, img, off, yb,
                       d_out, p.W, p.C, p.kh, p.kw, p.nby, p.nbx, p.nbins, parts, p.M, p.kmin, p.kmax, p.en, lut,
                       p.params, p.rmin, p.rmax);
  }
  MW_LAUNCH_CHECK();
  return MW_OK;
}

template <typename T>
static int run_clahe(const void* d_img, const ClPlan& p, double clip_limit, float* d_out, int* d_luts_out,
                     hipStream_t s) {
  const T* img = reinterpret_cast<const T*>(d_img);
  hipLaunchKernelGGL(clahe_range_kernel<T>, dim3(std::min(p.H, 2048)), dim3(256), 0, s, img, (int64_t)0, p.H, p.W,
                     p.C, p.kmin, p.kmax);
  MW_LAUNCH_CHECK();
  const int rpc = cl_hist_rpc(p);
  const int chunks = (p.kh + rpc - 1) / rpc;
  hipLaunchKernelGGL(clahe_hist_kernel<T>, dim3((unsigned)(p.nbx * p.nby * chunks)), dim3(256), 0, s, img, p.H, p.W,
                     p.C, p.kh, p.kw, p.nby, p.nbx, rpc, p.nbins, p.M, p.kmin, p.kmax, p.en, p.hist);
  MW_LAUNCH_CHECK();
  int st = cl_luts(p, clip_limit, d_luts_out, s);
  if (st != MW_OK) return st;
  st = cl_map<T, kClWhole>(p, img, 0, 0, p.H, d_out, s);
  if (st != MW_OK) return st;
  hipLaunchKernelGGL(clahe_params_kernel, dim3(1), dim3(256), 0, s, p.C, p.en, p.rmin, p.rmax, p.params);
  MW_LAUNCH_CHECK();
  return mw_rescale(d_out, MW_F32, (int64_t)p.H * p.W, p.C, p.params, d_out, s);
}

// ------------------------------------------------------------------ bands
// A band's pointer as the 16-byte-aligned address at or below it and the
// elements in between: cl_walk takes its vector phase from the element index
// relative to an aligned base, so the phase follows the address
template <typename T>
struct ClBand { const T* base; int64_t off; };
template <typename T>
static ClBand<T> cl_band(const void* d_rows) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(d_rows);
  return {reinterpret_cast<const T*>(a & ~(uintptr_t)15), (int64_t)((a & 15) / sizeof(T))};
}

static inline size_t cl_elem(int dtype) { return dtype == MW_U8 ? 1 : (dtype == MW_U16 ? 2 : 4); }

// the arguments every band entry shares (no device call)
static int cl_rows_check(const void* d_rows, int dtype, int y0, int rows, int H, int W, int C, int kh, int kw,
                         int nbins, const void* d_state) {
  const int bad = cl_check(dtype, H, W, C, kh, kw, 1.0, nbins);
  if (bad != MW_OK) return bad;
  MW_CHECK_ARG(rows >= 1 && y0 >= 0 && (int64_t)y0 + rows <= H,
               "mw_clahe_rows: the band's rows [%d, %d + %d) are not rows of the %d-row slide", y0, y0, rows, H);
  MW_CHECK_ARG(d_rows && d_state, "mw_clahe_rows: null pointer");
  MW_CHECK_ARG(((uintptr_t)d_state & 15) == 0, "mw_clahe_rows: the state must be 16-byte aligned");
  MW_CHECK_ARG((uintptr_t)d_rows % cl_elem(dtype) == 0, "mw_clahe_rows: the band must be aligned to its element type");
  return MW_OK;
}

template <typename T>
static int cl_hist_rows(const ClPlan& p, const void* d_rows, int y0, int rows, hipStream_t s) {
  const ClBand<T> b = cl_band<T>(d_rows);
  const int rpc = cl_hist_rpc(p);
  auto launch = [&](int v0, int v1) {
    const int t0 = v0 / p.kh, nt = (v1 - 1) / p.kh - t0 + 1;
    const int chunks = (std::min(p.kh, v1 - v0) + rpc - 1) / rpc;
    hipLaunchKernelGGL(clahe_hist_rows_kernel<T>, dim3((unsigned)(p.nbx * nt * chunks)), dim3(256), 0, s, b.base,
                       b.off, y0, v0, v1, t0, nt, p.H, p.W, p.C, p.kh, p.kw, p.nby, p.nbx, rpc, p.nbins, p.M, p.kmin,
                       p.kmax, p.en, p.hist);
  };
  launch(y0, y0 + rows);
  MW_LAUNCH_CHECK();
  // the rows past the image that reflect into this band: r with y0 <= 2 H - 2 - r < y0 + rows, H <= r < nby kh
  const int64_t ra = std::max<int64_t>(p.H, (int64_t)2 * p.H - 1 - y0 - rows);
  const int64_t rb = std::min<int64_t>((int64_t)p.nby * p.kh, (int64_t)2 * p.H - 1 - y0);
  if (ra < rb) {
    launch((int)ra, (int)rb);
    MW_LAUNCH_CHECK();
  }
  return MW_OK;
}

template <typename T, int kPass>
static int cl_map_rows(const ClPlan& p, const void* d_rows, int y0, int rows, float* d_out, hipStream_t s) {
  const ClBand<T> b = cl_band<T>(d_rows);
  return cl_map<T, kPass>(p, b.base, b.off, y0, rows, d_out, s);
}

}  // namespace mw

using namespace mw;

#define CL_BY_DTYPE(dtype, call_u8, call_u16, call_f32) \
  switch (dtype) {                                      \
    case MW_U8: return call_u8;                         \
    case MW_U16: return call_u16;                       \
    default: return call_f32;                           \
  }

extern "C" {

size_t mw_clahe_ws_bytes(int H, int W, int C, int kh, int kw, int nbins) {
  if (H < 1 || W < 1 || C < 1 || kh < 1 || kw < 1 || nbins < 1) return 0;
  return cl_layout(H, W, C, kh, kw, nbins).total + 256;
}

int mw_clahe(const void* d_img, int dtype, int H, int W, int C, const int* h_enable, int kh, int kw,
             double clip_limit, int nbins, float* d_out, void* d_ws, int* d_luts_out, void* stream) {
  const int bad = cl_check(dtype, H, W, C, kh, kw, clip_limit, nbins);
  if (bad != MW_OK) return bad;
  MW_CHECK_ARG(d_img && d_out && d_ws, "mw_clahe: null pointer");
  MW_CHECK_ARG(((uintptr_t)d_img & 15) == 0 && ((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_ws & 15) == 0,
               "mw_clahe: image, output and workspace must be 16-byte aligned");
  MW_CHECK_ARG(d_img != (const void*)d_out, "mw_clahe: the output must not alias the image");
  hipStream_t s = as_stream(stream);
  const ClPlan p = cl_plan(H, W, C, h_enable, kh, kw, nbins, d_ws);
  const int st = cl_clear(p, d_ws, s);
  if (st != MW_OK) return st;
  CL_BY_DTYPE(dtype, run_clahe<uint8_t>(d_img, p, clip_limit, d_out, d_luts_out, s),
              run_clahe<uint16_t>(d_img, p, clip_limit, d_out, d_luts_out, s),
              run_clahe<float>(d_img, p, clip_limit, d_out, d_luts_out, s));
}

int mw_clahe_rows_begin(int dtype, int H, int W, int C, int kh, int kw, double clip_limit, int nbins, void* d_state,
                        void* stream) {
  const int bad = cl_check(dtype, H, W, C, kh, kw, clip_limit, nbins);
  if (bad != MW_OK) return bad;
  MW_CHECK_ARG(d_state && ((uintptr_t)d_state & 15) == 0, "mw_clahe_rows_begin: the state must be 16-byte aligned");
  return cl_clear(cl_plan(H, W, C, nullptr, kh, kw, nbins, d_state), d_state, as_stream(stream));
}

int mw_clahe_rows_range(const void* d_rows, int dtype, int rows, int W, int C, void* d_state, void* stream) {
  MW_CHECK_ARG(rows >= 1 && W >= 2 && C >= 1, "mw_clahe_rows_range: bad band rows=%d W=%d C=%d", rows, W, C);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_clahe_rows_range: bad dtype %d", dtype);
  if (C > kClMaxC || (int64_t)W * C >= ((int64_t)1 << 31)) {
    set_error("mw_clahe_rows_range: W=%d C=%d (up to %d channels, a row below 2^31 elements)", W, C, kClMaxC);
    return MW_EUNSUPPORTED;
  }
  MW_CHECK_ARG(d_rows && d_state, "mw_clahe_rows_range: null pointer");
  MW_CHECK_ARG(((uintptr_t)d_state & 15) == 0, "mw_clahe_rows_range: the state must be 16-byte aligned");
  MW_CHECK_ARG((uintptr_t)d_rows % cl_elem(dtype) == 0,
               "mw_clahe_rows_range: the band must be aligned to its element type");
  hipStream_t s = as_stream(stream);
  // the minima and maxima head the state whatever the kernel (cl_layout)
  const ClPlan p = cl_plan(2, W, C, nullptr, 1, 1, 2, d_state);
  const unsigned grid = (unsigned)std::min(rows, 2048);
  switch (dtype) {
    case MW_U8: {
      const ClBand<uint8_t> b = cl_band<uint8_t>(d_rows);
      hipLaunchKernelGGL(clahe_range_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, b.base, b.off, rows, W, C, p.kmin,
                         p.kmax);
      break;
    }
    case MW_U16: {
      const ClBand<uint16_t> b = cl_band<uint16_t>(d_rows);
      hipLaunchKernelGGL(clahe_range_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, b.base, b.off, rows, W, C, p.kmin,
                         p.kmax);
      break;
    }
    default: {
      const ClBand<float> b = cl_band<float>(d_rows);
      hipLaunchKernelGGL(clahe_range_kernel<float>, dim3(grid), dim3(256), 0, s, b.base, b.off, rows, W, C, p.kmin,
                         p.kmax);
    }
  }
  MW_LAUNCH_CHECK();
  return MW_OK;
}

int mw_clahe_rows_hist(const void* d_rows, int dtype, int y0, int rows, int H, int W, int C, const int* h_enable,
                       int kh, int kw, int nbins, void* d_state, void* stream) {
  const int bad = cl_rows_check(d_rows, dtype, y0, rows, H, W, C, kh, kw, nbins, d_state);
  if (bad != MW_OK) return bad;
  hipStream_t s = as_stream(stream);
  const ClPlan p = cl_plan(H, W, C, h_enable, kh, kw, nbins, d_state);
  CL_BY_DTYPE(dtype, cl_hist_rows<uint8_t>(p, d_rows, y0, rows, s), cl_hist_rows<uint16_t>(p, d_rows, y0, rows, s),
              cl_hist_rows<float>(p, d_rows, y0, rows, s));
}

int mw_clahe_rows_luts(int H, int W, int C, int kh, int kw, double clip_limit, int nbins, void* d_state,
                       int* d_luts_out, void* stream) {
  const int bad = cl_check(MW_U8, H, W, C, kh, kw, clip_limit, nbins);
  if (bad != MW_OK) return bad;
  MW_CHECK_ARG(d_state && ((uintptr_t)d_state & 15) == 0, "mw_clahe_rows_luts: the state must be 16-byte aligned");
  return cl_luts(cl_plan(H, W, C, nullptr, kh, kw, nbins, d_state), clip_limit, d_luts_out, as_stream(stream));
}

int mw_clahe_rows_extremes(const void* d_rows, int dtype, int y0, int rows, int H, int W, int C,
                           const int* h_enable, int kh, int kw, int nbins, void* d_state, void* stream) {
  const int bad = cl_rows_check(d_rows, dtype, y0, rows, H, W, C, kh, kw, nbins, d_state);
  if (bad != MW_OK) return bad;
  hipStream_t s = as_stream(stream);
  const ClPlan p = cl_plan(H, W, C, h_enable, kh, kw, nbins, d_state);
  CL_BY_DTYPE(dtype, (cl_map_rows<uint8_t, kClExtremes>(p, d_rows, y0, rows, nullptr, s)),
              (cl_map_rows<uint16_t, kClExtremes>(p, d_rows, y0, rows, nullptr, s)),
              (cl_map_rows<float, kClExtremes>(p, d_rows, y0, rows, nullptr, s)));
}

int mw_clahe_rows_finish(int C, const int* h_enable, void* d_state, void* stream) {
  MW_CHECK_ARG(C >= 1 && C <= kClMaxC, "mw_clahe_rows_finish: %d channels outside 1..%d", C, kClMaxC);
  MW_CHECK_ARG(d_state && ((uintptr_t)d_state & 15) == 0, "mw_clahe_rows_finish: the state must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  const ClPlan p = cl_plan(2, 2, C, h_enable, 1, 1, 2, d_state);  // the rows head the state whatever the kernel
  hipLaunchKernelGGL(clahe_params_kernel, dim3(1), dim3(256), 0, s, C, p.en, p.rmin, p.rmax, p.params);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

int mw_clahe_rows_map(const void* d_rows, int dtype, int y0, int rows, int H, int W, int C, const int* h_enable,
                      int kh, int kw, int nbins, void* d_state, float* d_out, void* stream) {
  const int bad = cl_rows_check(d_rows, dtype, y0, rows, H, W, C, kh, kw, nbins, d_state);
  if (bad != MW_OK) return bad;
  MW_CHECK_ARG(d_out && ((uintptr_t)d_out & 3) == 0, "mw_clahe_rows_map: the output must be a float pointer");
  MW_CHECK_ARG((const void*)d_out == d_rows ? dtype == MW_F32 : true,
               "mw_clahe_rows_map: only an fp32 band may be mapped in place");
  hipStream_t s = as_stream(stream);
  const ClPlan p = cl_plan(H, W, C, h_enable, kh, kw, nbins, d_state);
  CL_BY_DTYPE(dtype, (cl_map_rows<uint8_t, kClFinal>(p, d_rows, y0, rows, d_out, s)),
              (cl_map_rows<uint16_t, kClFinal>(p, d_rows, y0, rows, d_out, s)),
              (cl_map_rows<float, kClFinal>(p, d_rows, y0, rows, d_out, s)));
}

}  // extern "C"

