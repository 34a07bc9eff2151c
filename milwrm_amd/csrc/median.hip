// Median filter of the MILWRM MxIF container on MI355X (gfx950).
//
//   median   img.blurring('median', size=k)   MxIF.py:395-405 as intended:
//            skimage.filters.median(plane, np.ones((sy, sx))) per channel =
//            scipy.ndimage.median_filter(footprint=ones, mode='nearest')
//
// The window of pixel (y, x) covers rows y - sy/2 .. y + sy - 1 - sy/2 and
// columns x - sx/2 .. x + sx - 1 - sx/2, coordinates clamped to the image; the
// output is the element of rank (sy sx) / 2 (from 0) of the window sorted
// ascending.  It is an element of the input, so the filter is exact.
//
// Everything runs on monotone unsigned keys with integer min / max and
// compares: the value itself for uint8 / uint16 (16-bit keys, two channels per
// 32-bit word, so the network's compare-exchanges are packed v_pk_min_u16 /
// v_pk_max_u16), the order-preserving bit transform for fp32 (32-bit keys; no
// floating-point min / max ever touches a pixel, so subnormals and +-0 come
// through bit for bit).
//
// One workgroup = kMedTH output rows x TW output pixels x one chunk of up to
// 16 words of channels.  The tile with its halo is staged once in LDS as keys,
// [row][pixel][word] (every coordinate clamped BEFORE the load: no address
// outside the image is formed); consecutive lanes then take consecutive words
// of a tile row, and the window of a word is sy x sx words at a fixed stride.
//   network path (2x2, 3x3, 5x5): the window in registers, a forgetful
//     selection of min / max compare-exchanges, fully unrolled;
//   generic path (every size up to 15x15): per output a bitwise rank search,
//     one round per key bit (8 / 16 / 32), counting the window elements below
//     the candidate key.
// Optional epilogue: the selected raw value goes through lognorm1 (the
// standalone mw_lognorm's arithmetic) and is written as fp32 once.
//
// Row window (mw_median_rows): the array holds rows [row_off, row_off + H) of a
// slide of slide_H rows, rows [r0, r1) of the array are filtered into a compact
// (r1 - r0)-row output, and window rows are clamped to the SLIDE.  The entry
// refuses an array that lacks a window row of a requested output row, so for
// every row that is written the slide clamp and the clamp to the array pick
// the same row: the kernel clamps to the array (no address outside it is
// formed, also for the unwritten rows of a last partial tile) and only needs
// r0 and r1.  A value's window holds the same elements whichever band reads
// them, and the selection is exact: bands tile to one whole-slide call bit for
// bit.  mw_median is the one-band case (row_off 0, slide_H = H, rows [0, H)).
#include "common.h"
#include "blur.h"  // lognorm1

namespace mw {

constexpr int kMedTH = 16;        // output rows per tile
constexpr int kMedMaxTW = 64;     // output pixels per tile, at most
constexpr int kMedMinTW = 16;
constexpr int kMedMaxWC = 16;     // words of channels per chunk
constexpr int kMedMaxSize = 15;
constexpr int kMedThreads = 256;

struct MedPlan {
  int H, W, C, sy, sx;
  int r0, r1;   // output rows [r0, r1) of the array; the output starts at row r0
  int TW;       // output pixels per tile
  int WC;       // words per pixel in a chunk
  int KC;       // channels per chunk (pad included): WC * keys per word
  int chunks, tiles_x;
  uint32_t m_kc, m_wc, m_rw, m_lrow;  // ceil(2^32 / d) of KC, WC, TW * WC, (TW + sx - 1) * KC
};

template <typename T> struct MedKey;
template <> struct MedKey<uint8_t> {
  using K = uint16_t;
  static constexpr int BITS = 8;
  static __device__ __forceinline__ K key(uint8_t v) { return (K)v; }
  static __device__ __forceinline__ uint8_t val(uint32_t k) { return (uint8_t)k; }
};
template <> struct MedKey<uint16_t> {
  using K = uint16_t;
  static constexpr int BITS = 16;
  static __device__ __forceinline__ K key(uint16_t v) { return v; }
  static __device__ __forceinline__ uint16_t val(uint32_t k) { return (uint16_t)k; }
};
// the monotone key of intensity.hip's selection, without folding -0.0 into
// +0.0: the transform must give the element's own bits back
template <> struct MedKey<float> {
  using K = uint32_t;
  static constexpr int BITS = 32;
  static __device__ __forceinline__ K key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  static __device__ __forceinline__ float val(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  }
};

typedef unsigned short med_u16x2 __attribute__((ext_vector_type(2)));

// compare-exchange of two words: a <- min, b <- max, per key
template <int KPW>
__device__ __forceinline__ void med_ce(uint32_t& a, uint32_t& b) {
  if constexpr (KPW == 2) {
    const med_u16x2 x = __builtin_bit_cast(med_u16x2, a), y = __builtin_bit_cast(med_u16x2, b);
    a = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, y));
    b = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(x, y));
  } else {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
  }
}

// Forgetful selection of the element of rank R (from 0) among N: v[LO, HI) is
// the working set, v[HI, TOT) has not been looked at, N = TOT - LO.  The
// minimum of M elements has at least M - 1 elements above it, so its rank is
// at most N - M: it goes when M > N - R; the maximum has rank at least M - 1
// and goes when M > R + 1.  The set grows by one unseen element until both
// hold (or nothing is left), then loses both ends: pairs first (M / 2
// exchanges leave the minimum in the lower half and the maximum in the upper),
// then one scan of each half.  All indices are compile-time constants.
template <int KPW, int LO, int HI, int TOT, int R>
__device__ __forceinline__ uint32_t med_select(uint32_t* v) {
  constexpr int N = TOT - LO, M = HI - LO;
  if constexpr (N == 1) {
    return v[LO];
  } else {
    constexpr bool drop_min = M > N - R, drop_max = M > R + 1;
    if constexpr (HI < TOT && !(drop_min && drop_max)) {
      return med_select<KPW, LO, HI + 1, TOT, R>(v);
    } else if constexpr (drop_min && drop_max) {
      constexpr int half = M / 2, low_end = LO + (M + 1) / 2;  // an odd middle element joins both scans
#pragma unroll
      for (int i = 0; i < half; ++i) med_ce<KPW>(v[LO + i], v[HI - 1 - i]);
#pragma unroll
      for (int i = LO + 1; i < low_end; ++i) med_ce<KPW>(v[LO], v[i]);
#pragma unroll
      for (int i = LO + half; i < HI - 1; ++i) med_ce<KPW>(v[i], v[HI - 1]);
      if constexpr (M > 2) {  // the maximum beside the minimum, out of the set
        const uint32_t t = v[LO + 1];
        v[LO + 1] = v[HI - 1];
        v[HI - 1] = t;
      }
      return med_select<KPW, LO + 2, HI, TOT, R - 1>(v);
    } else if constexpr (drop_min) {
#pragma unroll
      for (int i = LO + 1; i < HI; ++i) med_ce<KPW>(v[LO], v[i]);
      return med_select<KPW, LO + 1, HI, TOT, R - 1>(v);
    } else {
#pragma unroll
      for (int i = LO + 1; i < HI; ++i) med_ce<KPW>(v[i], v[LO]);
      return med_select<KPW, LO + 1, HI, TOT, R>(v);
    }
  }
}

__device__ __forceinline__ uint32_t med_div(uint32_t n, uint32_t magic, uint32_t d) {
  // n / d for n d < 2^32 with magic = ceil(2^32 / d); d = 1: magic does not fit, n itself
  return d == 1u ? n : __umulhi(n, magic);
}

// S > 0: the S x S network; S = 0: the generic search over p.sy x p.sx
template <typename T, int S, bool EPI>
__global__ void __launch_bounds__(kMedThreads) median_kernel(const T* __restrict__ img, MedPlan p,
                                                              const float* __restrict__ inv_mean,
                                                              float pseudo, void* __restrict__ out_v) {
  using MK = MedKey<T>;
  using K = typename MK::K;
  constexpr int KPW = 4 / (int)sizeof(K);  // keys per word
  extern __shared__ uint32_t med_tile[];
  K* tk = reinterpret_cast<K*>(med_tile);
  const int t = threadIdx.x;
  uint32_t b = blockIdx.x;
  const int chunk = (int)(b % (uint32_t)p.chunks);
  b /= (uint32_t)p.chunks;
  const int tx = (int)(b % (uint32_t)p.tiles_x), ty = (int)(b / (uint32_t)p.tiles_x);
  const int x0 = tx * p.TW, y0 = p.r0 + ty * kMedTH, c0 = chunk * p.KC;
  const int sy = S ? S : p.sy, sx = S ? S : p.sx;
  const int hy = sy / 2, hx = sx / 2;
  const int LW = p.TW + sx - 1, LH = kMedTH + sy - 1;

  // the tile and its halo as keys; element i is [row][pixel][channel of the chunk]
  const uint32_t lrow = (uint32_t)(LW * p.KC), n_el = (uint32_t)LH * lrow;
  for (uint32_t i = t; i < n_el; i += kMedThreads) {
    const uint32_t ry = med_div(i, p.m_lrow, lrow), rem = i - ry * lrow;
    const uint32_t cx = med_div(rem, p.m_kc, (uint32_t)p.KC), k = rem - cx * (uint32_t)p.KC;
    const int y = min(max(y0 - hy + (int)ry, 0), p.H - 1);
    const int x = min(max(x0 - hx + (int)cx, 0), p.W - 1);
    const int c = c0 + (int)k;
    K key = 0;
    if (c < p.C) key = MK::key(img[((int64_t)y * p.W + x) * p.C + c]);
    tk[i] = key;
  }
  __syncthreads();

  const uint32_t RW = (uint32_t)(p.TW * p.WC), n_items = (uint32_t)kMedTH * RW;
  const int rstride = LW * p.WC;  // words between tile rows
  for (uint32_t i = t; i < n_items; i += kMedThreads) {
    const uint32_t row = med_div(i, p.m_rw, RW), rem = i - row * RW;
    const uint32_t px = med_div(rem, p.m_wc, (uint32_t)p.WC), w = rem - px * (uint32_t)p.WC;
    const int y = y0 + (int)row, x = x0 + (int)px;
    if (y >= p.r1 || x >= p.W) continue;
    const uint32_t* win = med_tile + (int)row * rstride + (int)rem;  // the window's top left word
    uint32_t res;
    if constexpr (S > 0) {
      uint32_t v[S * S];
#pragma unroll
      for (int dy = 0; dy < S; ++dy)
#pragma unroll
        for (int dx = 0; dx < S; ++dx) v[dy * S + dx] = win[dy * rstride + dx * p.WC];
      res = med_select<KPW, 0, 1, S * S, (S * S) / 2>(v);
    } else {
      const uint32_t rank = (uint32_t)(sy * sx) / 2u;
      if constexpr (KPW == 2) {
        uint32_t r0 = 0u, r1 = 0u;
        for (int bit = MK::BITS - 1; bit >= 0; --bit) {
          const uint32_t q0 = r0 | (1u << bit), q1 = r1 | (1u << bit);
          uint32_t n0 = 0u, n1 = 0u;
          for (int dy = 0; dy < sy; ++dy) {
            const uint32_t* wr = win + dy * rstride;
            for (int dx = 0; dx < sx; ++dx) {
              const uint32_t e = wr[dx * p.WC];
              n0 += (e & 0xffffu) < q0 ? 1u : 0u;
              n1 += (e >> 16) < q1 ? 1u : 0u;
            }
          }
          // the element of rank r is >= q exactly when at most r elements lie below q
          if (n0 <= rank) r0 = q0;
          if (n1 <= rank) r1 = q1;
        }
        res = r0 | (r1 << 16);
      } else {
        uint32_t r0 = 0u;
        for (int bit = MK::BITS - 1; bit >= 0; --bit) {
          const uint32_t q0 = r0 | (1u << bit);
          uint32_t n0 = 0u;
          for (int dy = 0; dy < sy; ++dy) {
            const uint32_t* wr = win + dy * rstride;
            for (int dx = 0; dx < sx; ++dx) n0 += wr[dx * p.WC] < q0 ? 1u : 0u;
          }
          if (n0 <= rank) r0 = q0;
        }
        res = r0;
      }
    }
    const int64_t o = ((int64_t)(y - p.r0) * p.W + x) * p.C + c0 + (int)w * KPW;
#pragma unroll
    for (int h = 0; h < KPW; ++h) {
      const int c = c0 + (int)w * KPW + h;
      if (c >= p.C) break;
      const T val = MK::val(KPW == 2 ? ((res >> (16 * h)) & 0xffffu) : res);
      if constexpr (EPI)
        reinterpret_cast<float*>(out_v)[o + h] = lognorm1((float)val, inv_mean[c], pseudo);
      else
        reinterpret_cast<T*>(out_v)[o + h] = val;
    }
  }
}

static inline uint32_t med_magic(uint32_t d) {  // ceil(2^32 / d), d >= 2 (d = 1 is not divided)
  return d < 2u ? 0u : (uint32_t)((((uint64_t)1 << 32) + d - 1) / d);
}

static inline bool med_network(int sy, int sx) { return sy == sx && (sy == 2 || sy == 3 || sy == 5); }

template <typename T, bool EPI>
static int launch_median(const char* fn, const void* d_img, int H, int W, int C, int r0, int r1, int sy,
                         int sx, bool network, const float* d_inv_mean, float pseudoval, void* d_out, hipStream_t s) {
  constexpr int KPW = 4 / (int)sizeof(typename MedKey<T>::K);
  MedPlan p;
  p.H = H; p.W = W; p.C = C; p.sy = sy; p.sx = sx; p.r0 = r0; p.r1 = r1;
  const int words = (C + KPW - 1) / KPW;
  p.chunks = (words + kMedMaxWC - 1) / kMedMaxWC;
  p.WC = (words + p.chunks - 1) / p.chunks;  // even chunks, at most kMedMaxWC words
  p.KC = p.WC * KPW;
  p.TW = std::min(kMedMaxTW, std::max(kMedMinTW, kMedThreads / p.WC));
  p.tiles_x = (W + p.TW - 1) / p.TW;
  const int64_t tiles_y = ((int64_t)(r1 - r0) + kMedTH - 1) / kMedTH;  // the requested rows only
  const int64_t blocks = (int64_t)p.tiles_x * tiles_y * p.chunks;
  if (blocks > 0x7fffffffll) {
    set_error("%s: %lld workgroups (image too large for one launch)", fn, (long long)blocks);
    return MW_EUNSUPPORTED;
  }
  const int LW = p.TW + sx - 1, LH = kMedTH + sy - 1;
  const size_t lds = (size_t)LH * LW * p.WC * 4;
  if (lds > 65536) {
    set_error("%s: tile of %zu bytes does not fit in LDS", fn, lds);
    return MW_EUNSUPPORTED;
  }
  p.m_kc = med_magic((uint32_t)p.KC);
  p.m_wc = med_magic((uint32_t)p.WC);
  p.m_rw = med_magic((uint32_t)(p.TW * p.WC));
  p.m_lrow = med_magic((uint32_t)(LW * p.KC));
  const T* img = reinterpret_cast<const T*>(d_img);
  const dim3 grid((unsigned)blocks), block(kMedThreads);
#define MW_MED_LAUNCH(S_)                                                                          \
  hipLaunchKernelGGL((median_kernel<T, S_, EPI>), grid, block, lds, s, img, p, d_inv_mean, pseudoval, d_out)
  if (network && sy == 2) MW_MED_LAUNCH(2);
  else if (network && sy == 3) MW_MED_LAUNCH(3);
  else if (network && sy == 5) MW_MED_LAUNCH(5);
  else MW_MED_LAUNCH(0);
#undef MW_MED_LAUNCH
  MW_LAUNCH_CHECK();
  return MW_OK;
}

static int median_entry(const char* fn, const void* d_img, int dtype, int H, int W, int C, int64_t row_off,
                        int64_t slide_H, int r0, int r1, int sy, int sx, bool generic,
                        const float* d_inv_mean, float pseudoval, void* d_out, void* stream) {
  MW_CHECK_ARG(d_img && d_out, "%s: null pointer", fn);
  MW_CHECK_ARG(H >= 1 && W >= 1 && C >= 1, "%s: bad shape %d x %d x %d", fn, H, W, C);
  MW_CHECK_ARG(sy >= 1 && sx >= 1, "%s: size %d x %d (each must be at least 1)", fn, sy, sx);
  MW_CHECK_ARG(d_out != d_img, "%s: the output must not alias the image", fn);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "%s: bad dtype %d", fn, dtype);
  MW_CHECK_ARG(row_off >= 0 && row_off + H <= slide_H, "%s: rows [%lld, %lld) are not rows of a %lld-row slide",
               fn, (long long)row_off, (long long)row_off + H, (long long)slide_H);
  MW_CHECK_ARG(0 <= r0 && r0 < r1 && r1 <= H, "%s: output rows [%d, %d) of a %d-row array", fn, r0, r1, H);
  if (sy > kMedMaxSize || sx > kMedMaxSize) {
    set_error("%s: size %d x %d (up to %d per axis)", fn, sy, sx, kMedMaxSize);
    return MW_EUNSUPPORTED;
  }
  // every window row of every requested output row, clamped to the slide, must be in the array
  const int hy = sy / 2, below = sy - 1 - hy;
  MW_CHECK_ARG(row_off == 0 || r0 >= hy, "%s: output row %d needs %d rows above it and the array, whose first row "
               "is slide row %lld, holds %d", fn, r0, hy, (long long)row_off, r0);
  MW_CHECK_ARG(row_off + H == slide_H || H - r1 >= below, "%s: output row %d needs %d rows below it and the array, "
               "which ends before the slide does, holds %d", fn, r1 - 1, below, H - r1);
  hipStream_t s = as_stream(stream);
  const bool net = !generic && med_network(sy, sx);
  const bool epi = d_inv_mean != nullptr;
#define MW_MED_DTYPE(T_)                                                                                         \
  (epi ? launch_median<T_, true>(fn, d_img, H, W, C, r0, r1, sy, sx, net, d_inv_mean, pseudoval, d_out, s)       \
       : launch_median<T_, false>(fn, d_img, H, W, C, r0, r1, sy, sx, net, d_inv_mean, pseudoval, d_out, s))
  switch (dtype) {
    case MW_U8: return MW_MED_DTYPE(uint8_t);
    case MW_U16: return MW_MED_DTYPE(uint16_t);
    default: return MW_MED_DTYPE(float);
  }
#undef MW_MED_DTYPE
}

}  // namespace mw

using namespace mw;

extern "C" {

int mw_median_is_network(int size_y, int size_x) { return med_network(size_y, size_x) ? 1 : 0; }

int mw_median(const void* d_img, int dtype, int H, int W, int C, int size_y, int size_x,
              const float* d_inv_mean, float pseudoval, void* d_out, void* stream) {
  return median_entry("mw_median", d_img, dtype, H, W, C, 0, H, 0, H, size_y, size_x, false, d_inv_mean,
                      pseudoval, d_out, stream);
}

int mw_median_generic(const void* d_img, int dtype, int H, int W, int C, int size_y, int size_x,
                      const float* d_inv_mean, float pseudoval, void* d_out, void* stream) {
  return median_entry("mw_median", d_img, dtype, H, W, C, 0, H, 0, H, size_y, size_x, true, d_inv_mean,
                      pseudoval, d_out, stream);
}

int mw_median_rows(const void* d_img, int dtype, int H, int W, int C, int64_t row_off, int64_t slide_H,
                   int r0, int r1, int size_y, int size_x, int force_generic, const float* d_inv_mean,
                   float pseudoval, void* d_out, void* stream) {
  return median_entry("mw_median_rows", d_img, dtype, H, W, C, row_off, slide_H, r0, r1, size_y, size_x,
                      force_generic != 0, d_inv_mean, pseudoval, d_out, stream);
}

}  // extern "C"
