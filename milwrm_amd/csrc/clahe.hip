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
// flat index of its first element; n is an integral_constant, 1 or V.
template <typename T, int V, typename F>
__device__ __forceinline__ void cl_walk(const T* __restrict__ img, int64_t sb, int64_t se, int lane, int nl, F&& f) {
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
// after the first few elements almost no atomic is issued.
template <typename T>
__global__ void __launch_bounds__(256) clahe_range_kernel(const T* __restrict__ img, int H, int W, int C,
                                                          uint32_t* __restrict__ kmin, uint32_t* __restrict__ kmax) {
  constexpr int V = 16 / sizeof(T);
  __shared__ uint32_t s_min[kClMaxC], s_max[kClMaxC];
  const int t = threadIdx.x;
  for (int c = t; c < C; c += 256) { s_min[c] = 0xffffffffu; s_max[c] = 0u; }
  __syncthreads();
  const int64_t rowlen = (int64_t)W * C;
  for (int y = blockIdx.x; y < H; y += gridDim.x) {
    const int64_t rowbase = (int64_t)y * rowlen;
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
// Workgroup (chunk, i, j): rows [i kh + chunk rpc, ... + rpc) of tile (i, j),
// every channel, in rounds of kClSlots channels.  The four waves take the rows
// in turn.  A row past the image is the reflected row; the columns of the last
// tile column past the image are the contiguous run [2 W - 1 - (j + 1) kw,
// W - 1) of the same row (the order inside a histogram does not matter), so no
// address outside the image is formed.
template <typename T>
__global__ void __launch_bounds__(256) clahe_hist_kernel(const T* __restrict__ img, int H, int W, int C, int kh,
                                                         int kw, int nby, int nbx, int rpc, int nbins, uint32_t M,
                                                         const uint32_t* __restrict__ kmin,
                                                         const uint32_t* __restrict__ kmax, ClEnable en,
                                                         uint32_t* __restrict__ hist) {
  constexpr int V = 16 / sizeof(T);
  __shared__ unsigned int tab[kClSlots * kClTabStride];
  __shared__ double s_lo[kClMaxC], s_d[kClMaxC];
  __shared__ int s_off[kClMaxC];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  int bid = blockIdx.x;
  const int tj = bid % nbx;
  bid /= nbx;
  const int ti = bid % nby;
  const int chunk = bid / nby;
  const int r0 = ti * kh + chunk * rpc, r1 = min((ti + 1) * kh, r0 + rpc);
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
      const int64_t rowbase = (int64_t)ys * W * C;
      auto take = [&](int64_t e, const T* v, auto nn) {
        constexpr int n = decltype(nn)::value;
        int c = (int)(e - rowbase) % C;
#pragma unroll
        for (int k = 0; k < n; ++k) {
          const int off = s_off[c];
          if (off >= 0) atomicAdd(&tab[off + cl_bin((double)v[k], s_lo[c], s_d[c], M)], 1u);
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

// The generic form, for tiles too small to pay for staging their tables (or
// tables too large for LDS): the four table entries are read from global
// memory.  Workgroup (y, part): kClMapSeg elements of row y.
template <typename T>
__global__ void __launch_bounds__(256) clahe_map_kernel(const T* __restrict__ img, float* __restrict__ out, int H,
                                                        int W, int C, int kh, int kw, int nby, int nbx, int nbins,
                                                        int parts, uint32_t M, const uint32_t* __restrict__ kmin,
                                                        const uint32_t* __restrict__ kmax, ClEnable en,
                                                        const int* __restrict__ lut, uint32_t* __restrict__ rmin,
                                                        uint32_t* __restrict__ rmax) {
  constexpr int V = 4;
  __shared__ double s_lo[kClMaxC], s_d[kClMaxC];
  __shared__ uint32_t s_min[kClMaxC], s_max[kClMaxC];
  __shared__ int s_mode[kClMaxC];  // 0: the value itself, 1: a constant plane, 2: equalised
  const int t = threadIdx.x;
  for (int c = t; c < C; c += 256) {
    const double lo = cl_value<T>(kmin[c]), d = cl_value<T>(kmax[c]) - lo;
    s_lo[c] = lo;
    s_d[c] = d;
    s_mode[c] = !cl_enabled(en, c) ? 0 : (d > 0.0 ? 2 : 1);
    s_min[c] = 0xffffffffu;
    s_max[c] = 0u;
  }
  __syncthreads();
  const int y = blockIdx.x / parts, part = blockIdx.x - y * parts;
  const int64_t rowlen = (int64_t)W * C, rowbase = (int64_t)y * rowlen;
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
      const int mode = s_mode[c];
      float res = (float)v[k];
      if (mode != 0) {
        res = 0.0f;
        if (mode == 2) {
          const int* p = lut + (size_t)c * plane + cl_bin((double)v[k], s_lo[c], s_d[c], M);
          res = cl_blend(p[o00], p[o01], p[o10], p[o11], w00, w01, w10, w11);
        }
        const uint32_t bits = __float_as_uint(res);  // res >= 0: the bits order as the values
        if (bits < *(volatile uint32_t*)&s_min[c]) atomicMin(&s_min[c], bits);
        if (bits > *(volatile uint32_t*)&s_max[c]) atomicMax(&s_max[c], bits);
      }
      o[k] = res;
      if (++c == C) {
        c = 0;
        ++x;
        if (k + 1 < n) column();
      }
    }
    if constexpr (n == V) {
      typedef float f4 __attribute__((ext_vector_type(4)));
      f4 ov;
#pragma unroll
      for (int k = 0; k < V; ++k) ov[k] = o[k];
      *reinterpret_cast<f4*>(out + e) = ov;
    } else {
      out[e] = o[0];
    }
  });
  __syncthreads();
  for (int c = t; c < C; c += 256)
    if (s_mode[c] != 0 && s_max[c] >= s_min[c]) {
      atomicMin(&rmin[c], s_min[c]);
      atomicMax(&rmax[c], s_max[c]);
    }
}

// The staged form.  The pixels whose four nearest tile centres are the same
// form a cell: rows with (y + kh / 2) / kh = ci, columns likewise.  Workgroup
// (chunk, ci, cj) stages the cell's four tables of every channel in LDS, one
// 8-byte entry of four uint16 (a table value is below 2^14) per (channel,
// bin), so an element costs one LDS read where the generic form makes four
// scattered global reads; then its eight waves take the rows of its chunk of
// the cell in turn.
template <typename T, int kEnt>
__global__ void __launch_bounds__(512) clahe_map_lds_kernel(const T* __restrict__ img, float* __restrict__ out,
                                                            int H, int W, int C, int kh, int kw, int nby, int nbx,
                                                            int nbins, int ncy, int ncx, int rpc, uint32_t M,
                                                            const uint32_t* __restrict__ kmin,
                                                            const uint32_t* __restrict__ kmax, ClEnable en,
                                                            const int* __restrict__ lut,
                                                            uint32_t* __restrict__ rmin,
                                                            uint32_t* __restrict__ rmax) {
  constexpr int V = 4;
  __shared__ uint2 s_lut[kEnt];
  __shared__ double s_lo[kClMaxC], s_d[kClMaxC];
  __shared__ uint32_t s_min[kClMaxC], s_max[kClMaxC];
  __shared__ int s_mode[kClMaxC];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  int bid = blockIdx.x;
  const int cj = bid % ncx;
  bid /= ncx;
  const int ci = bid % ncy;
  const int chunk = bid / ncy;
  const int y0 = max(0, ci * kh - kh / 2) + chunk * rpc, y1 = min(min(H, (ci + 1) * kh - kh / 2), y0 + rpc);
  if (y0 >= y1) return;  // the whole workgroup
  const int x0 = max(0, cj * kw - kw / 2), x1 = min(W, (cj + 1) * kw - kw / 2);
  const int i0 = min(max(ci - 1, 0), nby - 1), i1 = min(ci, nby - 1);
  const int j0 = min(max(cj - 1, 0), nbx - 1), j1 = min(cj, nbx - 1);
  for (int c = t; c < C; c += 512) {
    const double lo = cl_value<T>(kmin[c]), d = cl_value<T>(kmax[c]) - lo;
    s_lo[c] = lo;
    s_d[c] = d;
    s_mode[c] = !cl_enabled(en, c) ? 0 : (d > 0.0 ? 2 : 1);
    s_min[c] = 0xffffffffu;
    s_max[c] = 0u;
  }
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
    const int64_t rowbase = (int64_t)y * W * C;
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
        const int mode = s_mode[c];
        float res = (float)v[k];
        if (mode != 0) {
          res = 0.0f;
          if (mode == 2) {
            const uint2 q = s_lut[c * nbins + cl_bin((double)v[k], s_lo[c], s_d[c], M)];
            res = cl_blend((int)(q.x & 0xffffu), (int)(q.x >> 16), (int)(q.y & 0xffffu), (int)(q.y >> 16), w00, w01,
                           w10, w11);
          }
          const uint32_t bits = __float_as_uint(res);
          if (bits < *(volatile uint32_t*)&s_min[c]) atomicMin(&s_min[c], bits);
          if (bits > *(volatile uint32_t*)&s_max[c]) atomicMax(&s_max[c], bits);
        }
        o[k] = res;
        if (++c == C) {
          c = 0;
          ++x;
          if (k + 1 < n) column();
        }
      }
      if constexpr (n == V) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        f4 ov;
#pragma unroll
        for (int k = 0; k < V; ++k) ov[k] = o[k];
        *reinterpret_cast<f4*>(out + e) = ov;
      } else {
        out[e] = o[0];
      }
    });
  }
  __syncthreads();
  for (int c = t; c < C; c += 512)
    if (s_mode[c] != 0 && s_max[c] >= s_min[c]) {
      atomicMin(&rmin[c], s_min[c]);
      atomicMax(&rmax[c], s_max[c]);
    }
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

template <typename T>
static int run_clahe(const void* d_img, int H, int W, int C, const ClEnable& en, int kh, int kw, double clip_limit,
                     int nbins, float* d_out, char* ws, const ClLayout& lay, int* d_luts_out, hipStream_t s) {
  const T* img = reinterpret_cast<const T*>(d_img);
  const int nby = (H + kh - 1) / kh, nbx = (W + kw - 1) / kw;
  uint32_t* kmin = reinterpret_cast<uint32_t*>(ws + lay.mins);
  uint32_t* kmax = reinterpret_cast<uint32_t*>(ws + lay.maxs);
  uint32_t* rmin = kmin + C;
  uint32_t* rmax = kmax + C;
  double* params = reinterpret_cast<double*>(ws + lay.params);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + lay.hist);
  const uint32_t binsz = 1u + (uint32_t)(kClLevels / nbins);
  const uint32_t M = 0xffffffffu / binsz + 1u;
  const double area = (double)kh * (double)kw;
  double climd = clip_limit * (double)kh * (double)kw;  // in the definition's order
  if (!(climd >= 1.0)) climd = 1.0;
  const int clim = (int)(climd < area ? climd : area);  // a limit above the tile's count clips nothing
  const double scale = (double)(kClLevels - 1) / area;

  hipLaunchKernelGGL(clahe_range_kernel<T>, dim3(std::min(H, 2048)), dim3(256), 0, s, img, H, W, C, kmin, kmax);
  MW_LAUNCH_CHECK();
  int rpc = (kClTilePixels + kw - 1) / kw;
  rpc = std::min(kh, (rpc + 3) / 4 * 4);
  const int chunks = (kh + rpc - 1) / rpc;
  hipLaunchKernelGGL(clahe_hist_kernel<T>, dim3((unsigned)(nbx * nby * chunks)), dim3(256), 0, s, img, H, W, C, kh,
                     kw, nby, nbx, rpc, nbins, M, kmin, kmax, en, hist);
  MW_LAUNCH_CHECK();
  const int64_t n_hist = (int64_t)C * nby * nbx;
  hipLaunchKernelGGL(clahe_lut_kernel, dim3((unsigned)((n_hist + 3) / 4)), dim3(256), 0, s, hist, n_hist, nbins, clim,
                     scale, d_luts_out);
  MW_LAUNCH_CHECK();
  const int* lut = reinterpret_cast<const int*>(hist);
  // staged where the tables fit LDS and a cell has at least two elements per table word it stages
  const int ncy = (H - 1 + kh / 2) / kh + 1, ncx = (W - 1 + kw / 2) / kw + 1;
  int mrpc = (kClCellPixels + kw - 1) / kw;
  mrpc = std::min(kh, (mrpc + 7) / 8 * 8);
  const int mchunks = (kh + mrpc - 1) / mrpc;
  const int64_t cells = (int64_t)ncy * ncx * mchunks;
  const int ent = C * nbins;
  if (ent <= kClLdsEntLarge && (int64_t)kh * kw >= (int64_t)8 * nbins && cells < ((int64_t)1 << 31)) {
    if (ent <= kClLdsEntSmall)
      hipLaunchKernelGGL((clahe_map_lds_kernel<T, kClLdsEntSmall>), dim3((unsigned)cells), dim3(512), 0, s, img,
                         d_out, H, W, C, kh, kw, nby, nbx, nbins, ncy, ncx, mrpc, M, kmin, kmax, en, lut, rmin, rmax);
    else
      hipLaunchKernelGGL((clahe_map_lds_kernel<T, kClLdsEntLarge>), dim3((unsigned)cells), dim3(512), 0, s, img,
                         d_out, H, W, C, kh, kw, nby, nbx, nbins, ncy, ncx, mrpc, M, kmin, kmax, en, lut, rmin, rmax);
  } else {
    const int parts = (int)(((int64_t)W * C + kClMapSeg - 1) / kClMapSeg);
    hipLaunchKernelGGL(clahe_map_kernel<T>, dim3((unsigned)(H * parts)), dim3(256), 0, s, img, d_out, H, W, C, kh,
                       kw, nby, nbx, nbins, parts, M, kmin, kmax, en, lut, rmin, rmax);
  }
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(clahe_params_kernel, dim3(1), dim3(256), 0, s, C, en, rmin, rmax, params);
  MW_LAUNCH_CHECK();
  return mw_rescale(d_out, MW_F32, (int64_t)H * W, C, params, d_out, s);
}

}  // namespace mw

using namespace mw;

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
  ClEnable en;
  for (int i = 0; i < kClMaxC / 32; ++i) en.w[i] = 0u;
  for (int c = 0; c < C; ++c)
    if (!h_enable || h_enable[c]) en.w[c >> 5] |= 1u << (c & 31);
  hipStream_t s = as_stream(stream);
  const ClLayout lay = cl_layout(H, W, C, kh, kw, nbins);
  char* ws = reinterpret_cast<char*>(d_ws);
  MW_HIP(hipMemsetAsync(ws + lay.mins, 0xff, lay.maxs - lay.mins, s));
  MW_HIP(hipMemsetAsync(ws + lay.maxs, 0, lay.total - lay.maxs, s));
  switch (dtype) {
    case MW_U8:
      return run_clahe<uint8_t>(d_img, H, W, C, en, kh, kw, clip_limit, nbins, d_out, ws, lay, d_luts_out, s);
    case MW_U16:
      return run_clahe<uint16_t>(d_img, H, W, C, en, kh, kw, clip_limit, nbins, d_out, ws, lay, d_luts_out, s);
    default:
      return run_clahe<float>(d_img, H, W, C, en, kh, kw, clip_limit, nbins, d_out, ws, lay, d_luts_out, s);
  }
}

}  // extern "C"
