// Bilateral filter of the MILWRM MxIF container on MI355X (gfx950).
//
//   bilateral   img.blurring('bilateral', sigma=s, sigma_color=v)   MxIF.py:406-410
//
// The definition (skimage's documented algorithm without its
// colour look-up table): a = the image as fp32 (raw uint8 / uint16 through
// lognorm1 when a log_normalize is fused into the load), r the radius,
//   out[y, x, c] = sum_t w_t q_t[c] / sum_t w_t      over the (2r + 1)^2 taps t = (dy, dx),
//   q_t = a[y + dy, x + dx, :]  (outside the image: cval in every channel in
//         mode 'constant', the pixel at the clamped coordinates in mode 'edge'),
//   w_t = exp(-(dy^2 + dx^2) / (2 sigma^2)) exp(-|q_t - a[y, x, :]|^2 / (2 sigma_color^2)).
// The spatial factor is g[|dy|] g[|dx|] from a table of r + 1 fp32 values made
// on the host in fp64; the colour factor is one v_exp_f32 of an fp32 squared
// distance over ALL channels.  The centre tap has weight exactly 1.
//
// One workgroup = 8 output rows x 32 output pixels, one thread per pixel, all
// channels.  A tap's weight needs every channel of the tap before any channel
// can be accumulated, so a thread keeps its centre pixel, the tap and the
// accumulators in registers, in a compile-time number NQ of 4-channel groups
// (4 NQ >= C; the pad channels are zero in both, so they add nothing to the
// distance).  The taps come from LDS: the tile with its column halo is staged
// as fp32 [row][pixel][4 NQ] (every coordinate clamped BEFORE the load: no
// address outside the image is formed), a pixel is NQ 16-byte reads, and with
// NQ odd the 16 lanes of a ds_read_b128 group (consecutive pixels of one tile
// row) fall on 16 different bank quads.  25 x 25 x 64 fp32 values do not fit
// in LDS, and the weight of a tap depends on no other tap: the window's rows
// are therefore taken in bands of RB rows (LDS holds 8 + RB - 1 tile rows, the
// accumulators stay in registers across bands), RB sized by the host so that
// two workgroups share a CU's LDS where the shape allows it.  Staging costs
// one load (and lognorm1) per staged element against 3 (2 r + 1) RB packed
// operations per thread and channel pair, so the re-staged halo is cheap.
//
// Row window (mw_bilateral_rows): the array holds rows [row_off, row_off + H)
// of a slide of slide_H rows, rows [r0, r1) of the array are filtered into a
// compact (r1 - r0)-row output, and a tap row is inside or outside relative to
// the SLIDE.  The entry refuses an array that lacks an in-slide tap row of a
// requested output row, so for every row that is written the clamp to the
// array picks the row the clamp to the slide would: the kernel clamps its
// addresses to the array (no address outside it is formed, also for the
// centre pixel of the unwritten rows of a last partial tile) and only needs
// r0, r1 and the slide's rows as array coordinates [ylo, yhi).  A pixel's taps
// are visited in one order (window-row groups of RB, RB a function of C and r
// alone), whichever tile or band computes it: bands tile to one whole-slide
// call bit for bit.  mw_bilateral is the one-band case (row_off 0, slide_H =
// H, rows [0, H)).
#include <math.h>

#include "common.h"
#include "blur.h"  // lognorm1, bf2

namespace mw {

constexpr int kBilTH = 8;          // output rows per tile
constexpr int kBilTW = 32;         // output pixels per tile row (half a wave: one ds_read_b128 group is one row)
constexpr int kBilThreads = kBilTH * kBilTW;
constexpr int kBilMaxR = 12;       // win_size 25
constexpr int kBilMaxC = 64;
constexpr int kBilLdsShared = 80 * 1024;   // two workgroups per CU
constexpr int kBilLdsWhole = 160 * 1024;
constexpr int kBilModeConstant = 0, kBilModeEdge = 1;

struct BilPlan {
  int H, W, C, r;
  int r0, r1;      // output rows [r0, r1) of the array; the output starts at row r0
  int ylo, yhi;    // the slide's rows in array coordinates: [-row_off, slide_H - row_off)
  int RB;          // window rows per band
  int LW;          // staged pixels per tile row: kBilTW + 2 r
  int tiles_x;
  int mode;
  float cval;
  float k2;        // -log2(e) / (2 sigma_color^2): w_colour = 2^(k2 d^2)
  uint32_t m_c;    // ceil(2^32 / C)
  float g[kBilMaxR + 1];  // exp(-d^2 / (2 sigma^2)), d = 0 .. r
};

template <typename T, bool LOGN>
__device__ __forceinline__ float bil_load(const T* __restrict__ p, int64_t i, int c,
                                          const float* __restrict__ inv_mean, float pseudo) {
  const float v = (float)p[i];
  if constexpr (LOGN) return lognorm1(v, inv_mean[c], pseudo);
  else return v;
}

__device__ __forceinline__ uint32_t bil_div(uint32_t n, uint32_t magic, uint32_t d) {
  // n / d for n d < 2^32 with magic = ceil(2^32 / d); d = 1: magic does not fit, n itself
  return d == 1u ? n : __umulhi(n, magic);
}

template <typename T, bool LOGN, int NQ>
__global__ void __launch_bounds__(kBilThreads) bilateral_kernel(const T* __restrict__ img, BilPlan p,
                                                                 const float* __restrict__ inv_mean,
                                                                 float pseudo, float* __restrict__ out) {
  constexpr int CP = 4 * NQ;  // fp32 per staged pixel
  constexpr int CP2 = 2 * NQ;
  extern __shared__ __attribute__((aligned(16))) float bil_tile[];
  const int t = threadIdx.x, tx = t & (kBilTW - 1), ty = t / kBilTW;
  const int bx = (int)(blockIdx.x % (uint32_t)p.tiles_x), by = (int)(blockIdx.x / (uint32_t)p.tiles_x);
  const int x0 = bx * kBilTW, y0 = p.r0 + by * kBilTH;
  const int r = p.r, n = 2 * r + 1, C = p.C, LW = p.LW;
  const int LR = kBilTH + p.RB - 1;
  float* sg = bil_tile + LR * LW * CP;  // g[|j - r|], j = 0 .. 2r

  // the pad channels of every staged pixel stay zero; the spatial table
  {
    const int n_el = LR * LW * CP;
    for (int i = t; i < n_el; i += kBilThreads) bil_tile[i] = 0.f;
    if (t < n) {
      const int d = t < r ? r - t : t - r;
      float gv = 0.f;
#pragma unroll
      for (int k = 0; k <= kBilMaxR; ++k) gv = d == k ? p.g[k] : gv;
      sg[t] = gv;
    }
  }

  // this thread's pixel (a thread past the rows asked for or the image keeps a clamped one and does not store)
  const int y = y0 + ty, x = x0 + tx;
  const bool live = y < p.r1 && x < p.W;
  bf2 ctr[CP2], acc[CP2];
  {
    const int64_t base = ((int64_t)min(y, p.H - 1) * p.W + min(x, p.W - 1)) * C;
#pragma unroll
    for (int c = 0; c < CP; c += 2) {
      const float v0 = c < C ? bil_load<T, LOGN>(img, base + c, c, inv_mean, pseudo) : 0.f;
      const float v1 = c + 1 < C ? bil_load<T, LOGN>(img, base + c + 1, c + 1, inv_mean, pseudo) : 0.f;
      ctr[c / 2] = bf2{v0, v1};
      acc[c / 2] = bf2{0.f, 0.f};
    }
  }
  float wsum = 0.f;

  const uint32_t row_el = (uint32_t)(LW * C);
  for (int b0 = 0; b0 < n; b0 += p.RB) {
    const int rb = min(p.RB, n - b0);
    const int rows = kBilTH + rb - 1;
    __syncthreads();  // the band before has been read (first band: the zeros are written)
    for (int lr = 0; lr < rows; ++lr) {
      const int gy = y0 - r + b0 + lr;
      const bool yin = gy >= p.ylo && gy < p.yhi;  // a row of the slide (the array may hold less)
      const T* __restrict__ srow = img + (int64_t)min(max(gy, 0), p.H - 1) * p.W * C;
      float* drow = bil_tile + lr * LW * CP;
      for (uint32_t j = t; j < row_el; j += kBilThreads) {
        const uint32_t px = bil_div(j, p.m_c, (uint32_t)C), c = j - px * (uint32_t)C;
        const int gx = x0 - r + (int)px;
        const bool in = yin && gx >= 0 && gx < p.W;
        float v = p.cval;
        if (in || p.mode == kBilModeEdge)
          v = bil_load<T, LOGN>(srow, (int64_t)min(max(gx, 0), p.W - 1) * C + (int)c, (int)c, inv_mean, pseudo);
        drow[px * CP + c] = v;
      }
    }
    __syncthreads();
    for (int k = 0; k < rb; ++k) {
      const float gy_w = sg[b0 + k];
      const float4* rowp = reinterpret_cast<const float4*>(bil_tile + ((ty + k) * LW + tx) * CP);
      for (int j = 0; j < n; ++j) {
        const float4* q4 = rowp + j * NQ;
        bf2 q[CP2];
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
          const float4 v = q4[i];
          q[2 * i] = bf2{v.x, v.y};
          q[2 * i + 1] = bf2{v.z, v.w};
        }
        bf2 d2 = bf2{0.f, 0.f};
#pragma unroll
        for (int i = 0; i < CP2; ++i) {
          const bf2 d = q[i] - ctr[i];
          d2 = __builtin_elementwise_fma(d, d, d2);
        }
        const float w = (gy_w * sg[j]) * __builtin_amdgcn_exp2f(p.k2 * (d2.x + d2.y));
        wsum += w;
        const bf2 ww = bf2{w, w};
#pragma unroll
        for (int i = 0; i < CP2; ++i) acc[i] = __builtin_elementwise_fma(ww, q[i], acc[i]);
      }
    }
  }
  if (live) {
    const float inv = 1.0f / wsum;  // wsum >= 1: the centre tap
    float* o = out + ((int64_t)(y - p.r0) * p.W + x) * C;
#pragma unroll
    for (int c = 0; c < CP; c += 2) {
      if (c < C) o[c] = acc[c / 2].x * inv;
      if (c + 1 < C) o[c + 1] = acc[c / 2].y * inv;
    }
  }
}

static inline int bil_nq(int C) {  // 4-channel groups per pixel: odd (bank quads), 4 NQ >= C
  const int need = (C + 3) / 4;
  for (int nq : {1, 3, 5, 7, 9, 13, 17})
    if (nq >= need) return nq;
  return 0;
}

template <typename T, bool LOGN>
static int launch_bilateral(const char* fn, const T* img, BilPlan& p, const float* d_inv_mean, float pseudoval,
                            float* d_out, hipStream_t s) {
  const int NQ = bil_nq(p.C);
  const int n = 2 * p.r + 1;
  const size_t row_bytes = (size_t)p.LW * 4 * NQ * sizeof(float), extra = (size_t)((n + 3) & ~3) * sizeof(float);
  size_t budget = kBilLdsShared;
  if (extra + kBilTH * row_bytes > budget) budget = kBilLdsWhole;
  if (NQ == 0 || extra + kBilTH * row_bytes > budget) {
    set_error("%s: a tile of C=%d r=%d does not fit in LDS", fn, p.C, p.r);
    return MW_EUNSUPPORTED;
  }
  const int rb_max = std::min<int>(n, (int)((budget - extra) / row_bytes) - kBilTH + 1);
  const int bands = (n + rb_max - 1) / rb_max;
  p.RB = (n + bands - 1) / bands;  // even bands
  const size_t lds = (size_t)(kBilTH + p.RB - 1) * row_bytes + extra;
  const int64_t blocks = (int64_t)p.tiles_x * ((p.r1 - p.r0 + kBilTH - 1) / kBilTH);
  if (blocks > 0x7fffffffll) {
    set_error("%s: %lld workgroups (image too large for one launch)", fn, (long long)blocks);
    return MW_EUNSUPPORTED;
  }
  const dim3 grid((unsigned)blocks), block(kBilThreads);
#define MW_BIL_LAUNCH(NQ_)                                                                                   \
  case NQ_:                                                                                                  \
    hipLaunchKernelGGL((bilateral_kernel<T, LOGN, NQ_>), grid, block, lds, s, img, p, d_inv_mean, pseudoval, \
                       d_out);                                                                               \
    break;
  switch (NQ) {
    MW_BIL_LAUNCH(1) MW_BIL_LAUNCH(3) MW_BIL_LAUNCH(5) MW_BIL_LAUNCH(7) MW_BIL_LAUNCH(9) MW_BIL_LAUNCH(13)
    MW_BIL_LAUNCH(17)
  }
#undef MW_BIL_LAUNCH
  MW_LAUNCH_CHECK();
  return MW_OK;
}

// ------------------------------------------------------------------ moments
// count, mean, centred second moment, minimum and maximum of the (optionally
// log-normalised) image in fp64, two passes: the sum, then the squared
// deviations from the mean.  A block takes whole pixels (so a thread's channel
// advances by 256 mod C per step); every sum is a fixed tree: deterministic.
constexpr int kMomThreads = 256;
constexpr int kMomMaxBlocks = 1024;

struct MomPart { double sum, m2; float lo, hi; };

// the total of part[].sum (M2 = false) or part[].m2 in thread 0, the same tree in every block
template <bool M2>
__device__ __forceinline__ double mom_total(const MomPart* __restrict__ part, int G, double* scratch) {
  double s = 0.0;
  for (int i = threadIdx.x; i < G; i += kMomThreads) s += M2 ? part[i].m2 : part[i].sum;
  return block_sum(s, scratch);
}

// PASS 0: block partials (sum, min, max); PASS 1: block partials of sum (x - mean)^2
template <typename T, bool LOGN, int PASS>
__global__ void __launch_bounds__(kMomThreads) moments_kernel(const T* __restrict__ img, int64_t n_pix, int C,
                                                               int64_t pix_per_block,
                                                               const float* __restrict__ inv_mean, float pseudo,
                                                               MomPart* __restrict__ part) {
  __shared__ double scratch[kMomThreads / 64];
  __shared__ float lo_sh[kMomThreads / 64], hi_sh[kMomThreads / 64];
  __shared__ double mean_sh;
  double mean = 0.0;
  if constexpr (PASS == 1) {
    const double tot = mom_total<false>(part, (int)gridDim.x, scratch);
    if (threadIdx.x == 0) mean_sh = tot / ((double)n_pix * (double)C);
    __syncthreads();
    mean = mean_sh;
  }
  const int64_t p0 = (int64_t)blockIdx.x * pix_per_block, p1 = min(n_pix, p0 + pix_per_block);
  const int64_t e1 = p1 * C;
  const int step = kMomThreads % C;
  int c = (int)threadIdx.x % C;
  double s = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t e = p0 * C + threadIdx.x; e < e1; e += kMomThreads) {
    const float v = bil_load<T, LOGN>(img, e, c, inv_mean, pseudo);
    if constexpr (PASS == 0) {
      s += (double)v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    } else {
      const double d = (double)v - mean;
      s += d * d;
    }
    c += step;
    c = c >= C ? c - C : c;
  }
  if constexpr (PASS == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, o, 64));
      hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      lo_sh[threadIdx.x >> 6] = lo;
      hi_sh[threadIdx.x >> 6] = hi;
    }
  }
  const double tot = block_sum(s, scratch);  // its barriers order lo_sh / hi_sh too
  if (threadIdx.x == 0) {
    if constexpr (PASS == 0) {
      for (int w = 1; w < kMomThreads / 64; ++w) {
        lo = fminf(lo, lo_sh[w]);
        hi = fmaxf(hi, hi_sh[w]);
      }
      part[blockIdx.x].sum = tot;
      part[blockIdx.x].lo = lo;
      part[blockIdx.x].hi = hi;
    } else {
      part[blockIdx.x].m2 = tot;
    }
  }
}

__global__ void __launch_bounds__(kMomThreads) moments_final_kernel(const MomPart* __restrict__ part, int G,
                                                                     double n, double* __restrict__ out) {
  __shared__ double scratch[kMomThreads / 64];
  const double sum = mom_total<false>(part, G, scratch);
  const double m2 = mom_total<true>(part, G, scratch);
  if (threadIdx.x == 0) {
    float lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < G; ++i) {
      lo = fminf(lo, part[i].lo);
      hi = fmaxf(hi, part[i].hi);
    }
    out[0] = n;
    out[1] = sum / n;  // the division every PASS 1 block made
    out[2] = m2;
    out[3] = (double)lo;
    out[4] = (double)hi;
  }
}

template <typename T, bool LOGN>
static int launch_moments(const T* img, int64_t n_pix, int C, const float* d_inv_mean, float pseudoval,
                          double* d_out, void* d_ws, hipStream_t s) {
  MomPart* part = reinterpret_cast<MomPart*>(d_ws);
  const int64_t n_el = n_pix * C;
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(kMomMaxBlocks, (n_el + kMomThreads * 16 - 1) / (kMomThreads * 16)));
  const int64_t ppb = (n_pix + want - 1) / want;
  const int G = (int)((n_pix + ppb - 1) / ppb);
  hipLaunchKernelGGL((moments_kernel<T, LOGN, 0>), dim3(G), dim3(kMomThreads), 0, s, img, n_pix, C, ppb,
                     d_inv_mean, pseudoval, part);
  hipLaunchKernelGGL((moments_kernel<T, LOGN, 1>), dim3(G), dim3(kMomThreads), 0, s, img, n_pix, C, ppb,
                     d_inv_mean, pseudoval, part);
  hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(kMomThreads), 0, s, part, G, (double)n_el, d_out);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

// ---------------------------------------------------------- moments by rows
// The same five numbers from a slide that arrives in row bands, with bits that
// do not depend on the bands: every slide row is reduced by ONE workgroup
// (element e of the row by thread e % 256, block_sum's tree) into entry
// [slide row] of a slide_H-long table -- PASS 0 the row's (sum, min, max),
// PASS 1 its sum (a - mean)^2 with the mean PASS 0's table gave -- and one
// workgroup reduces the table (entry i by thread i % 256, the same tree).
// Workspace: RowMomHead, then the table.
struct RowMomHead { double mean; double pad; };

template <typename T, bool LOGN, int PASS>
__global__ void __launch_bounds__(kMomThreads) moments_rows_kernel(const T* __restrict__ img, int row_el, int C,
                                                                    const float* __restrict__ inv_mean,
                                                                    float pseudo,
                                                                    const RowMomHead* __restrict__ head,
                                                                    MomPart* __restrict__ part) {
  __shared__ double scratch[kMomThreads / 64];
  __shared__ float lo_sh[kMomThreads / 64], hi_sh[kMomThreads / 64];
  const T* __restrict__ row = img + (int64_t)blockIdx.x * row_el;
  double mean = 0.0;
  if constexpr (PASS == 1) mean = head->mean;
  const int step = kMomThreads % C;
  int c = (int)threadIdx.x % C;
  double s = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int e = threadIdx.x; e < row_el; e += kMomThreads) {
    const float v = bil_load<T, LOGN>(row, e, c, inv_mean, pseudo);
    if constexpr (PASS == 0) {
      s += (double)v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    } else {
      const double d = (double)v - mean;
      s += d * d;
    }
    c += step;
    c = c >= C ? c - C : c;
  }
  if constexpr (PASS == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, o, 64));
      hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      lo_sh[threadIdx.x >> 6] = lo;
      hi_sh[threadIdx.x >> 6] = hi;
    }
  }
  const double tot = block_sum(s, scratch);  // its barriers order lo_sh / hi_sh too
  if (threadIdx.x == 0) {
    if constexpr (PASS == 0) {
      for (int w = 1; w < kMomThreads / 64; ++w) {
        lo = fminf(lo, lo_sh[w]);
        hi = fmaxf(hi, hi_sh[w]);
      }
      part[blockIdx.x].sum = tot;
      part[blockIdx.x].lo = lo;
      part[blockIdx.x].hi = hi;
    } else {
      part[blockIdx.x].m2 = tot;
    }
  }
}

// the table's totals: the mean into the head (what PASS 1 subtracts), the five numbers into out;
// with_m2 == 0 (PASS 1 has not run): out[2] is NaN
__global__ void __launch_bounds__(kMomThreads) moments_rows_final_kernel(const MomPart* __restrict__ part,
                                                                          int64_t G, double n, int with_m2,
                                                                          RowMomHead* __restrict__ head,
                                                                          double* __restrict__ out) {
  __shared__ double scratch[kMomThreads / 64];
  __shared__ float lo_sh[kMomThreads / 64], hi_sh[kMomThreads / 64];
  double s = 0.0, q = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = threadIdx.x; i < G; i += kMomThreads) {
    s += part[i].sum;
    if (with_m2) q += part[i].m2;
    lo = fminf(lo, part[i].lo);
    hi = fmaxf(hi, part[i].hi);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    lo_sh[threadIdx.x >> 6] = lo;
    hi_sh[threadIdx.x >> 6] = hi;
  }
  const double sum = block_sum(s, scratch);
  const double m2 = block_sum(q, scratch);
  if (threadIdx.x == 0) {
    for (int w = 1; w < kMomThreads / 64; ++w) {
      lo = fminf(lo, lo_sh[w]);
      hi = fmaxf(hi, hi_sh[w]);
    }
    const double mean = sum / n;
    head->mean = mean;
    out[0] = n;
    out[1] = mean;
    out[2] = with_m2 ? m2 : (double)NAN;
    out[3] = (double)lo;
    out[4] = (double)hi;
  }
}

template <typename T, bool LOGN>
static int launch_moments_rows(const T* img, int H, int row_el, int C, int pass, const float* d_inv_mean,
                               float pseudoval, const RowMomHead* head, MomPart* part, hipStream_t s) {
  if (pass == 0)
    hipLaunchKernelGGL((moments_rows_kernel<T, LOGN, 0>), dim3(H), dim3(kMomThreads), 0, s, img, row_el, C,
                       d_inv_mean, pseudoval, head, part);
  else
    hipLaunchKernelGGL((moments_rows_kernel<T, LOGN, 1>), dim3(H), dim3(kMomThreads), 0, s, img, row_el, C,
                       d_inv_mean, pseudoval, head, part);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

static int bilateral_entry(const char* fn, const void* d_img, int dtype, int H, int W, int C, int64_t row_off,
                           int64_t slide_H, int r0, int r1, int radius, double sigma_spatial,
                           double sigma_color, int mode, float cval, const float* d_inv_mean, float pseudoval,
                           float* d_out, void* stream) {
  MW_CHECK_ARG(d_img && d_out, "%s: null pointer", fn);
  MW_CHECK_ARG(H >= 1 && W >= 1 && C >= 1, "%s: bad shape %d x %d x %d", fn, H, W, C);
  MW_CHECK_ARG((const void*)d_out != d_img, "%s: the output must not alias the image", fn);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "%s: bad dtype %d", fn, dtype);
  MW_CHECK_ARG(radius >= 0, "%s: radius %d", fn, radius);
  MW_CHECK_ARG(row_off >= 0 && row_off + H <= slide_H, "%s: rows [%lld, %lld) are not rows of a %lld-row slide",
               fn, (long long)row_off, (long long)row_off + H, (long long)slide_H);
  MW_CHECK_ARG(0 <= r0 && r0 < r1 && r1 <= H, "%s: output rows [%d, %d) of a %d-row array", fn, r0, r1, H);
  MW_CHECK_ARG(std::isfinite(sigma_spatial) && sigma_spatial > 0, "%s: sigma_spatial %g (must be "
               "positive and finite)", fn, sigma_spatial);
  MW_CHECK_ARG(std::isfinite(sigma_color) && sigma_color > 0, "%s: sigma_color %g (must be positive "
               "and finite)", fn, sigma_color);
  MW_CHECK_ARG(mode == kBilModeConstant || mode == kBilModeEdge, "%s: mode %d (0 constant, 1 edge)", fn, mode);
  MW_CHECK_ARG(std::isfinite(cval), "%s: cval %g", fn, (double)cval);
  if (radius > kBilMaxR || C > kBilMaxC) {
    set_error("%s: radius %d, %d channels (up to radius %d and %d channels)", fn, radius, C, kBilMaxR,
              kBilMaxC);
    return MW_EUNSUPPORTED;
  }
  if ((int64_t)W * C > 0x7fffffffll - 64 * kBilMaxC) {
    set_error("%s: rows of %d x %d elements", fn, W, C);
    return MW_EUNSUPPORTED;
  }
  // every tap row of every requested output row that is a row of the slide must be in the array
  MW_CHECK_ARG(row_off == 0 || r0 >= radius, "%s: output row %d needs %d rows above it and the array, whose first "
               "row is slide row %lld, holds %d", fn, r0, radius, (long long)row_off, r0);
  MW_CHECK_ARG(row_off + H == slide_H || H - r1 >= radius, "%s: output row %d needs %d rows below it and the "
               "array, which ends before the slide does, holds %d", fn, r1 - 1, radius, H - r1);
  BilPlan p;
  p.r0 = r0; p.r1 = r1;
  // the slide's rows as array rows; a tap row lies within [-radius, H + radius + 7], so the clips lose nothing
  p.ylo = (int)std::max<int64_t>(-row_off, -(int64_t)(1 << 20));
  p.yhi = (int)std::min<int64_t>(slide_H - row_off, (int64_t)0x7fffffff);
  p.H = H; p.W = W; p.C = C; p.r = radius; p.RB = 1;
  p.LW = kBilTW + 2 * radius;
  p.tiles_x = (W + kBilTW - 1) / kBilTW;
  p.mode = mode;
  p.cval = cval;
  p.k2 = (float)(-0.5 * 1.4426950408889634 / (sigma_color * sigma_color));
  MW_CHECK_ARG(std::isfinite(p.k2), "%s: sigma_color %g is too small for fp32 weights", fn, sigma_color);
  p.m_c = C < 2 ? 0u : (uint32_t)((((uint64_t)1 << 32) + (uint32_t)C - 1) / (uint32_t)C);
  for (int d = 0; d <= kBilMaxR; ++d)
    p.g[d] = d <= radius ? (float)exp(-0.5 * (double)(d * d) / (sigma_spatial * sigma_spatial)) : 0.f;
  hipStream_t s = as_stream(stream);
  const bool logn = d_inv_mean != nullptr;
#define MW_BIL_DTYPE(T_)                                                                                   \
  (logn ? launch_bilateral<T_, true>(fn, (const T_*)d_img, p, d_inv_mean, pseudoval, d_out, s)             \
        : launch_bilateral<T_, false>(fn, (const T_*)d_img, p, d_inv_mean, pseudoval, d_out, s))
  switch (dtype) {
    case MW_U8: return MW_BIL_DTYPE(uint8_t);
    case MW_U16: return MW_BIL_DTYPE(uint16_t);
    default: return MW_BIL_DTYPE(float);
  }
#undef MW_BIL_DTYPE
}

}  // namespace mw

using namespace mw;

extern "C" {

int mw_bilateral(const void* d_img, int dtype, int H, int W, int C, int radius, double sigma_spatial,
                 double sigma_color, int mode, float cval, const float* d_inv_mean, float pseudoval,
                 float* d_out, void* stream) {
  return bilateral_entry("mw_bilateral", d_img, dtype, H, W, C, 0, H, 0, H, radius, sigma_spatial, sigma_color,
                         mode, cval, d_inv_mean, pseudoval, d_out, stream);
}

int mw_bilateral_rows(const void* d_img, int dtype, int H, int W, int C, int64_t row_off, int64_t slide_H,
                      int r0, int r1, int radius, double sigma_spatial, double sigma_color, int mode,
                      float cval, const float* d_inv_mean, float pseudoval, float* d_out, void* stream) {
  return bilateral_entry("mw_bilateral_rows", d_img, dtype, H, W, C, row_off, slide_H, r0, r1, radius,
                         sigma_spatial, sigma_color, mode, cval, d_inv_mean, pseudoval, d_out, stream);
}

size_t mw_image_moments_rows_ws_bytes(int64_t slide_H) {
  return sizeof(RowMomHead) + (size_t)std::max<int64_t>(slide_H, 0) * sizeof(MomPart);
}

int mw_image_moments_rows(const void* d_img, int dtype, int H, int W, int C, int64_t row_off, int64_t slide_H,
                          int pass, const float* d_inv_mean, float pseudoval, void* d_ws, void* stream) {
  MW_CHECK_ARG(d_img && d_ws, "mw_image_moments_rows: null pointer");
  MW_CHECK_ARG(H >= 1 && W >= 1 && C >= 1, "mw_image_moments_rows: bad shape %d x %d x %d", H, W, C);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_image_moments_rows: bad dtype %d", dtype);
  MW_CHECK_ARG(pass == 0 || pass == 1, "mw_image_moments_rows: pass %d (0: sums, minimum, maximum; 1: squared "
               "deviations)", pass);
  MW_CHECK_ARG(row_off >= 0 && row_off + H <= slide_H, "mw_image_moments_rows: rows [%lld, %lld) are not rows of "
               "a %lld-row slide", (long long)row_off, (long long)row_off + H, (long long)slide_H);
  if ((int64_t)W * C > 0x7fffffffll - kMomThreads) {
    set_error("mw_image_moments_rows: rows of %d x %d elements", W, C);
    return MW_EUNSUPPORTED;
  }
  hipStream_t s = as_stream(stream);
  const RowMomHead* head = reinterpret_cast<const RowMomHead*>(d_ws);
  MomPart* part = reinterpret_cast<MomPart*>(reinterpret_cast<char*>(d_ws) + sizeof(RowMomHead)) + row_off;
  const bool logn = d_inv_mean != nullptr;
#define MW_MOMR_DTYPE(T_)                                                                                       \
  (logn ? launch_moments_rows<T_, true>((const T_*)d_img, H, W * C, C, pass, d_inv_mean, pseudoval, head, part, s)  \
        : launch_moments_rows<T_, false>((const T_*)d_img, H, W * C, C, pass, d_inv_mean, pseudoval, head, part, s))
  switch (dtype) {
    case MW_U8: return MW_MOMR_DTYPE(uint8_t);
    case MW_U16: return MW_MOMR_DTYPE(uint16_t);
    default: return MW_MOMR_DTYPE(float);
  }
#undef MW_MOMR_DTYPE
}

int mw_image_moments_rows_final(int64_t slide_H, int W, int C, int with_m2, void* d_ws, double* d_out,
                                void* stream) {
  MW_CHECK_ARG(d_ws && d_out, "mw_image_moments_rows_final: null pointer");
  MW_CHECK_ARG(slide_H >= 1 && W >= 1 && C >= 1, "mw_image_moments_rows_final: bad shape %lld x %d x %d",
               (long long)slide_H, W, C);
  RowMomHead* head = reinterpret_cast<RowMomHead*>(d_ws);
  const MomPart* part = reinterpret_cast<const MomPart*>(reinterpret_cast<char*>(d_ws) + sizeof(RowMomHead));
  hipLaunchKernelGGL(moments_rows_final_kernel, dim3(1), dim3(kMomThreads), 0, as_stream(stream), part, slide_H,
                     (double)slide_H * (double)W * (double)C, with_m2 != 0 ? 1 : 0, head, d_out);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

size_t mw_image_moments_ws_bytes(void) { return (size_t)kMomMaxBlocks * sizeof(MomPart); }

int mw_image_moments(const void* d_img, int dtype, int64_t n_pix, int C, const float* d_inv_mean,
                     float pseudoval, double* d_out, void* d_ws, void* stream) {
  MW_CHECK_ARG(d_img && d_out && d_ws, "mw_image_moments: null pointer");
  MW_CHECK_ARG(n_pix >= 1 && C >= 1, "mw_image_moments: bad shape %lld x %d", (long long)n_pix, C);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_image_moments: bad dtype %d", dtype);
  hipStream_t s = as_stream(stream);
  const bool logn = d_inv_mean != nullptr;
#define MW_MOM_DTYPE(T_)                                                                          \
  (logn ? launch_moments<T_, true>((const T_*)d_img, n_pix, C, d_inv_mean, pseudoval, d_out, d_ws, s)  \
        : launch_moments<T_, false>((const T_*)d_img, n_pix, C, d_inv_mean, pseudoval, d_out, d_ws, s))
  switch (dtype) {
    case MW_U8: return MW_MOM_DTYPE(uint8_t);
    case MW_U16: return MW_MOM_DTYPE(uint16_t);
    default: return MW_MOM_DTYPE(float);
  }
#undef MW_MOM_DTYPE
}

}  // extern "C"
