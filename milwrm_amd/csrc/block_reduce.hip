// img.downsample(fact, func) (MxIF.py:494-517) on a slide or a row band of it:
// skimage.measure.block_reduce(x, (f, f, 1), func, cval=0) for func in
// {mean, sum, max, min, median}, HWC u8 / u16 / f32 in, HWC fp32 out.
//
// The pad (zeros below the slide's last row and right of its last column)
// takes part in every func.  Every output value is computed by one lane from
// its own f x f block in one order, so the result has the same bits whatever
// row bands the slide arrives in (a band holds whole block rows):
//
//   mean, sum  fp64 sum, block rows top to bottom, within a row left to
//              right (block_mean_kernel's order: mean gives mw_block_mean's
//              bits), mean times the fp64 1 / f^2, rounded once to fp32
//   max, min   exact; a NaN in the block gives NaN
//   median     exact selection by bisection over the monotone uint32 keys of
//              the elements (the keys of intensity.hip): per key bit one
//              count of the block's elements below the trial key, 8 / 16 / 32
//              rounds for u8 / u16 / f32 over a block that sits in cache, no
//              per-lane array; an even count averages the two middle order
//              statistics in fp64.  fact <= 16.
//
// mean / sum / max / min read every input element once: a lane owns N
// consecutive channels of one output pixel (N elements = the widest naturally
// aligned vector that divides C, up to 16 bytes) and walks its f x f block
// with vector loads, up to four of a block row in flight.
#include <math.h>

#include "common.h"

namespace mw {

namespace {

constexpr int kMedianMaxFact = 16;

template <typename T, int N>
using RVec = T __attribute__((ext_vector_type(N)));

template <int N>
struct alignas(N >= 4 ? 16 : 4 * N) FVec { float v[N]; };

enum { OP_SUM = 0, OP_MAX = 1, OP_MIN = 2 };

template <int OP> struct Acc { using type = float; };
template <> struct Acc<OP_SUM> { using type = double; };

template <int OP, typename A>
__device__ __forceinline__ A fold(A acc, float v) {
  if constexpr (OP == OP_SUM) return acc + (A)v;
  else if constexpr (OP == OP_MAX) return (v > acc || v != v) ? v : acc;  // a NaN stays (acc != acc: no v replaces it)
  else return (v < acc || v != v) ? v : acc;
}

// in: the slide's rows [row0, row0 + rows); out: the band's first output row
// (slide output row row0 / f).  One lane per N output channels of a pixel.
template <typename T, int N, int OP>
__global__ void __launch_bounds__(256) block_reduce_kernel(const T* __restrict__ in, int rows, int W, int C,
                                                           int row0, int slide_H, int f, double scale,
                                                           int Hob, int Wo, float* __restrict__ out) {
  using A = typename Acc<OP>::type;
  using V = RVec<T, N>;
  const int Cv = C / N;
  const int64_t n = (int64_t)Hob * Wo * Cv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const int cv = (int)(e % Cv);
    const int64_t p = e / Cv;
    const int ox = (int)(p % Wo), oy = (int)(p / Wo);
    const int y0 = oy * f, x0 = ox * f;
    const int ny = min(f, rows - y0), nx = min(f, W - x0);  // the block's rows / columns inside the slide
    A acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = OP == OP_SUM ? A(0) : OP == OP_MAX ? A(-INFINITY) : A(INFINITY);
    for (int dy = 0; dy < ny; ++dy) {
      const T* row = in + ((int64_t)(y0 + dy) * W + x0) * C + (int64_t)cv * N;
      int dx = 0;
      for (; dx + 4 <= nx; dx += 4) {
        V q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = ld_stream(reinterpret_cast<const V*>(row + (int64_t)(dx + u) * C));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int i = 0; i < N; ++i) acc[i] = fold<OP>(acc[i], (float)q[u][i]);
      }
      for (; dx < nx; ++dx) {
        const V q = ld_stream(reinterpret_cast<const V*>(row + (int64_t)dx * C));
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = fold<OP>(acc[i], (float)q[i]);
      }
    }
    // the pad's zeros (rows below the slide, columns right of it) take part
    const bool padded = row0 + y0 + f > slide_H || x0 + f > W;
    FVec<N> r;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if constexpr (OP == OP_SUM) r.v[i] = (float)(acc[i] * scale);
      else r.v[i] = padded ? fold<OP>(acc[i], 0.0f) : acc[i];
    }
    *reinterpret_cast<FVec<N>*>(out + p * C + (int64_t)cv * N) = r;
  }
}

// ---- median: monotone keys (as intensity.hip's sel_key / sel_value) ----
template <typename T>
__device__ __forceinline__ uint32_t med_key(T v) { return (uint32_t)v; }
template <>
__device__ __forceinline__ uint32_t med_key<float>(float v) {
  uint32_t b = __float_as_uint(v);
  if (v == 0.0f) b = 0u;  // -0.0 orders (and is returned) as +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
template <typename T>
__device__ __forceinline__ double med_value(uint32_t key) { return (double)key; }
template <>
__device__ __forceinline__ double med_value<float>(uint32_t key) {
  const uint32_t b = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  return (double)__uint_as_float(b);
}
template <typename T> struct KeyBits { static constexpr int N = 8 * sizeof(T); };

// One lane per output element.  The order statistic of rank k (0-based) is the
// largest key K with |{elements < K}| <= k, built bit by bit from the top.
template <typename T>
__global__ void __launch_bounds__(256) block_median_kernel(const T* __restrict__ in, int rows, int W, int C,
                                                           int f, int Hob, int Wo, float* __restrict__ out) {
  const int64_t n = (int64_t)Hob * Wo * C;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int cnt = f * f;
  const int k = (cnt - 1) / 2;  // the middle (odd count) or the lower middle (even)
  const uint32_t key0 = med_key<T>(T(0));
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const int c = (int)(e % C);
    const int64_t p = e / C;
    const int ox = (int)(p % Wo), oy = (int)(p / Wo);
    const int y0 = oy * f, x0 = ox * f;
    const int ny = min(f, rows - y0), nx = min(f, W - x0);
    const int npad = cnt - ny * nx;  // zeros of the pad: ranked with the rest
    const T* base = in + ((int64_t)y0 * W + x0) * C + c;
    bool nan = false;
    if constexpr (sizeof(T) == 4) {
      for (int dy = 0; dy < ny; ++dy)
        for (int dx = 0; dx < nx; ++dx) {
          const T v = base[((int64_t)dy * W + dx) * C];
          nan |= v != v;
        }
    }
    uint32_t key = 0;
    for (int bit = KeyBits<T>::N - 1; bit >= 0; --bit) {
      const uint32_t trial = key | (1u << bit);
      int below = key0 < trial ? npad : 0;
      for (int dy = 0; dy < ny; ++dy)
        for (int dx = 0; dx < nx; ++dx) below += med_key<T>(base[((int64_t)dy * W + dx) * C]) < trial ? 1 : 0;
      if (below <= k) key = trial;
    }
    double r = med_value<T>(key);
    if ((cnt & 1) == 0) {
      // rank k + 1: the same key when more than k + 1 elements are <= it, else the next key up
      int le = key0 <= key ? npad : 0;
      uint32_t next = (npad && key0 > key) ? key0 : 0xffffffffu;
      for (int dy = 0; dy < ny; ++dy)
        for (int dx = 0; dx < nx; ++dx) {
          const uint32_t q = med_key<T>(base[((int64_t)dy * W + dx) * C]);
          le += q <= key ? 1 : 0;
          if (q > key && q < next) next = q;
        }
      const double hi = le >= k + 2 ? r : med_value<T>(next);
      r = (r + hi) * 0.5;
    }
    out[e] = nan ? __uint_as_float(0x7fc00000u) : (float)r;
  }
}

static inline int reduce_grid(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 1 << 20); }

template <typename T, int N>
int launch_reduce_n(const T* in, int rows, int W, int C, int row0, int slide_H, int f, int func, int Hob, int Wo,
                    float* out, hipStream_t st) {
  const int grid = reduce_grid((int64_t)Hob * Wo * (C / N));
  const double scale = func == MW_REDUCE_MEAN ? 1.0 / ((double)f * f) : 1.0;
  switch (func) {
    case MW_REDUCE_MEAN:
    case MW_REDUCE_SUM:
      hipLaunchKernelGGL((block_reduce_kernel<T, N, OP_SUM>), dim3(grid), dim3(256), 0, st, in, rows, W, C, row0,
                         slide_H, f, scale, Hob, Wo, out);
      break;
    case MW_REDUCE_MAX:
      hipLaunchKernelGGL((block_reduce_kernel<T, N, OP_MAX>), dim3(grid), dim3(256), 0, st, in, rows, W, C, row0,
                         slide_H, f, scale, Hob, Wo, out);
      break;
    default:
      hipLaunchKernelGGL((block_reduce_kernel<T, N, OP_MIN>), dim3(grid), dim3(256), 0, st, in, rows, W, C, row0,
                         slide_H, f, scale, Hob, Wo, out);
      break;
  }
  MW_LAUNCH_CHECK();
  return MW_OK;
}

template <typename T>
int launch_reduce(const T* in, int rows, int W, int C, int row0, int slide_H, int f, int func, int Hob, int Wo,
                  float* out, hipStream_t st) {
  if (func == MW_REDUCE_MEDIAN) {
    const int grid = reduce_grid((int64_t)Hob * Wo * C);
    hipLaunchKernelGGL(block_median_kernel<T>, dim3(grid), dim3(256), 0, st, in, rows, W, C, f, Hob, Wo, out);
    MW_LAUNCH_CHECK();
    return MW_OK;
  }
  // the widest vector (up to 16 bytes) that divides a pixel's C elements and
  // is naturally aligned in both arrays: every pixel then starts on it
  constexpr int kMaxN = 16 / (int)sizeof(T);
  int nvec = 1;
  for (int cand = kMaxN; cand > 1; cand >>= 1) {
    const uintptr_t ob = (uintptr_t)(cand >= 4 ? 16 : 4 * cand);
    if (C % cand == 0 && (uintptr_t)in % (cand * sizeof(T)) == 0 && (uintptr_t)out % ob == 0) {
      nvec = cand;
      break;
    }
  }
#define MW_REDUCE_CASE(NN) \
  case NN: return launch_reduce_n<T, NN>(in, rows, W, C, row0, slide_H, f, func, Hob, Wo, out, st)
  switch (nvec) {
    MW_REDUCE_CASE(1);
    MW_REDUCE_CASE(2);
    MW_REDUCE_CASE(4);
    default:
      if constexpr (kMaxN >= 8) {
        if (nvec == 8) return launch_reduce_n<T, 8>(in, rows, W, C, row0, slide_H, f, func, Hob, Wo, out, st);
      }
      if constexpr (kMaxN >= 16) {
        if (nvec == 16) return launch_reduce_n<T, 16>(in, rows, W, C, row0, slide_H, f, func, Hob, Wo, out, st);
      }
      set_error("mw_block_reduce_rows: vector width %d", nvec);
      return MW_EINVAL;
  }
#undef MW_REDUCE_CASE
}

}  // namespace

}  // namespace mw

using namespace mw;

extern "C" int mw_block_reduce_rows(const void* d_rows, int dtype, int rows, int W, int C, int row0, int slide_H,
                                    int fact, int func, float* d_out, void* stream) {
  const char* fn = "mw_block_reduce_rows";
  MW_CHECK_ARG(d_rows && d_out, "%s: null pointer", fn);
  MW_CHECK_ARG(rows > 0 && W > 0 && C > 0 && fact > 0 && slide_H > 0, "%s: bad shape", fn);
  MW_CHECK_ARG(func >= MW_REDUCE_MEAN && func <= MW_REDUCE_MEDIAN, "%s: bad func %d", fn, func);
  MW_CHECK_ARG(row0 >= 0 && (int64_t)row0 + rows <= slide_H, "%s: rows [%d, %lld) of a %d-row slide", fn, row0,
               (long long)row0 + rows, slide_H);
  MW_CHECK_ARG(row0 % fact == 0, "%s: the band starts at row %d, not a multiple of fact = %d", fn, row0, fact);
  MW_CHECK_ARG(rows % fact == 0 || row0 + rows == slide_H,
               "%s: a band of %d rows that does not end the slide is not a multiple of fact = %d", fn, rows, fact);
  if (func == MW_REDUCE_MEDIAN && fact > kMedianMaxFact) {
    set_error("%s: median of fact = %d (up to %d)", fn, fact, kMedianMaxFact);
    return MW_EUNSUPPORTED;
  }
  const int Wo = (W + fact - 1) / fact;
  const int Hob = (rows + fact - 1) / fact;  // output rows of this band
  float* out = d_out + (int64_t)(row0 / fact) * Wo * C;
  hipStream_t st = as_stream(stream);
  switch (dtype) {
    case MW_U8: return launch_reduce<uint8_t>((const uint8_t*)d_rows, rows, W, C, row0, slide_H, fact, func, Hob, Wo, out, st);
    case MW_U16: return launch_reduce<uint16_t>((const uint16_t*)d_rows, rows, W, C, row0, slide_H, fact, func, Hob, Wo, out, st);
    case MW_F32: return launch_reduce<float>((const float*)d_rows, rows, W, C, row0, slide_H, fact, func, Hob, Wo, out, st);
    default: set_error("%s: bad dtype %d", fn, dtype); return MW_EINVAL;
  }
}
