// Intensity utilities of the MILWRM MxIF container on MI355X (gfx950).
//
//   quantiles  clip_values' np.nanpercentile / scale_rgb's min, max   MxIF.py:29-92
//   rescale    skimage rescale_intensity / (x - min) / (max - min)     MxIF.py:29-92
//
// quantiles is an exact order-statistic selection: a radix select over
// monotone uint32 keys, 8-bit digits, most significant first.  Every pass
// streams the HWC image once and histograms the digit of the elements whose
// higher digits equal one of the channel's live prefixes (pass 1: all kept
// elements) into LDS tables of 256 counters (up to 56 per workgroup), merged
// into global memory once per workgroup.  Between passes a one-workgroup
// kernel picks, per channel and rank, the digit that holds the rank; ranks
// come from the histogram's own sum, so nothing returns to the host before
// the last pass has written the order statistics.  A pass may be fed in pieces
// (mw_quantiles_rows_*): the counts are integer adds into global memory, so
// counting a slide band after band gives the whole slide's histograms.
#include <math.h>

#include "common.h"

// rescale's fp64 expression must round as numpy's elementwise operations do
#pragma clang fp contract(off)

namespace mw {

constexpr int kSelBlocks = 1024;  // streaming workgroups (4 per CU)
constexpr int kSlotsFirst = 56;   // 256-bin tables per workgroup, pass 1: 56 KB of LDS
constexpr int kSlotsNext = 44;    // later passes: 44 KB beside the live prefixes
constexpr int kTabStride = 257;   // words between tables
constexpr int kRegPrefixes = 4;   // live prefixes per channel held in registers (two percentiles)
constexpr int kMaxQ = 8;          // percentiles per call
constexpr int kMaxSelC = 256;     // channels of a per-channel selection
constexpr int kPrefLds = kMaxSelC * 2 * kMaxQ;  // every live prefix of a pass (16 KB)
constexpr int kChoiceThreads = 1024;

struct QList { double q[kMaxQ]; };  // q / 100

template <typename T> struct SelVec;
template <> struct SelVec<uint8_t> { static constexpr int N = 16; };
template <> struct SelVec<uint16_t> { static constexpr int N = 8; };
template <> struct SelVec<float> { static constexpr int N = 4; };

template <typename T, int N>
struct alignas(sizeof(T) * N) SelPack { T v[N]; };

// monotone key of an element and whether it takes part
template <typename T>
__device__ __forceinline__ uint32_t sel_key(T v, bool skip, bool& kept, bool& isnan) {
  kept = true;
  isnan = false;
  return (uint32_t)v;
}
template <>
__device__ __forceinline__ uint32_t sel_key<float>(float v, bool skip, bool& kept, bool& isnan) {
  isnan = v != v;
  kept = !isnan && !(skip && v == -99999.0f);
  uint32_t b = __float_as_uint(v);
  if (v == 0.0f) b = 0u;  // -0.0 orders (and is returned) as +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename T>
__device__ __forceinline__ double sel_value(uint32_t key) { return (double)key; }
template <>
__device__ __forceinline__ double sel_value<float>(uint32_t key) {
  const uint32_t b = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  return (double)__uint_as_float(b);
}

// Selection state in the workspace (device pointers)
struct SelState {
  unsigned long long* nan_cnt;   // [Ceff]
  unsigned long long* n_kept;    // [Ceff]
  uint32_t* rank_prefix;         // [Ceff * L] digits chosen so far of rank r
  unsigned long long* rank_rem;  // [Ceff * L] rank among the elements sharing that prefix
  int* rank_slot;                // [Ceff * L] table of the rank in the next pass (-1: no element)
  int* nuniq;                    // [Ceff] live prefixes of the channel
  int* slot_base;                // [Ceff] first table of the channel
  uint32_t* uprefix;             // [Ceff * L] the live prefixes
  int* n_slots;                  // tables in use in the next pass
};

// Workgroup b owns elements [b*epb, (b+1)*epb) of the flat HWC array; epb is a
// multiple of V*teff with V*teff % C == 0, so the V channels of a lane are the
// same for all its loads.  The LDS tables: kTabStride = 257 words apart, so
// equal digits of different tables (the tied top digits of every channel of a
// slide) fall into different banks; and while the pass needs at most half of
// the tables, R replicas of each, picked by lane, which spreads the adds of
// lanes that share a channel (all of them, in the pooled selection).  Later
// passes compare against the live prefixes of the lane's channels: in
// registers while a channel has at most kRegPrefixes of them (LREG; two
// percentiles, as clip and scale ask), else in LDS beside the tables, where
// the dependent LDS reads of every element bound the pass.
//
// A band of rows need not start on a 16-byte boundary: img is the band's start
// rounded down to one, the band's elements are [off, n_elem) of it (off < V, so
// only the first vector of workgroup 0 holds elements before the band: its
// lane takes it element by element) and flat element e belongs to channel
// (e + phase) % C, phase = (C - off % C) % C.
template <typename T, bool FIRST, bool LREG>
__global__ void __launch_bounds__(256) select_count_kernel(const T* __restrict__ img, int64_t n_elem,
                                                           int C, int L, int teff, int64_t epb,
                                                           int shift, int skip, int off, int phase,
                                                           SelState st,
                                                           unsigned long long* __restrict__ hist) {
  constexpr int V = SelVec<T>::N;
  constexpr int S = FIRST ? kSlotsFirst : kSlotsNext;
  __shared__ unsigned int tab[S * kTabStride];
  __shared__ unsigned long long s_nan[FIRST ? kMaxSelC : 1];
  __shared__ uint32_t s_pref[FIRST || LREG ? 1 : kPrefLds];
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * epb;
  const int64_t hi = min(n_elem, lo + epb);
  const int n_slots = FIRST ? C : *st.n_slots;
  const int groups = (n_slots + S - 1) / S;
  int R = 1;
  if (groups == 1)
    while (R < 32 && 2 * R * n_slots <= S) R *= 2;
  const int rep = t & (R - 1);

  int chn[V], nu[V], sb[V];
  unsigned int nanc[V];
  uint32_t pr[LREG ? V : 1][kRegPrefixes];  // no prefix has its top byte set: ~0 matches none
#pragma unroll
  for (int i = 0; i < V; ++i) {
    chn[i] = (int)(((int64_t)t * V + i + phase) % C);
    nanc[i] = 0u;
    if constexpr (FIRST) {
      nu[i] = 1;
      sb[i] = chn[i];
    } else {
      nu[i] = t < teff ? st.nuniq[chn[i]] : 0;
      sb[i] = t < teff ? st.slot_base[chn[i]] : 0;
      if constexpr (LREG) {
#pragma unroll
        for (int j = 0; j < kRegPrefixes; ++j) pr[i][j] = j < nu[i] ? st.uprefix[chn[i] * L + j] : ~0u;
      }
    }
  }
  if constexpr (FIRST) {
    for (int c = t; c < kMaxSelC; c += 256) s_nan[c] = 0ull;
  } else {
    if constexpr (!LREG)
      for (int i = t; i < C * L; i += 256) s_pref[i] = st.uprefix[i];
  }

  for (int g = 0; g < groups; ++g) {
    for (int i = t; i < S * kTabStride; i += 256) tab[i] = 0u;
    __syncthreads();
    const int s0 = g * S;
    int tb[V];  // FIRST: the lane's table of channel i in this group (-1: another group's)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int rel = sb[i] - s0;
      tb[i] = (rel >= 0 && rel < S) ? (rel * R + rep) * kTabStride : -1;
    }
    auto take = [&](T v, int i) {
      bool kept, isnan;
      const uint32_t key = sel_key<T>(v, skip != 0, kept, isnan);
      const int digit = (int)((key >> shift) & 255u);
      if constexpr (FIRST) {
        if (g == 0 && isnan) nanc[i] += 1u;
        if (kept && tb[i] >= 0) atomicAdd(&tab[tb[i] + digit], 1u);
      } else {
        const uint32_t pf = key >> (shift + 8);
        int rel = -1;
        if constexpr (LREG) {
#pragma unroll
          for (int j = 0; j < kRegPrefixes; ++j)
            if (pr[i][j] == pf) rel = sb[i] + j - s0;
        } else {
          const int base = chn[i] * L;
          for (int j = 0; j < nu[i]; ++j)
            if (s_pref[base + j] == pf) rel = sb[i] + j - s0;
        }
        if (kept && rel >= 0 && rel < S) atomicAdd(&tab[(rel * R + rep) * kTabStride + digit], 1u);
      }
    };
    if (t < teff) {
      const int64_t stride = (int64_t)teff * V;
      int64_t e = lo + (int64_t)t * V;
      if (off > 0 && e == 0) {  // the vector that straddles the band's start
#pragma unroll
        for (int i = 0; i < V; ++i)
          if (i >= off && i < hi) take(img[i], i);
        e += stride;
      }
      // four independent 16-B loads in flight per iteration
      for (; e + 3 * stride + V <= hi; e += 4 * stride) {
        SelPack<T, V> p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = *reinterpret_cast<const SelPack<T, V>*>(img + e + u * stride);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int i = 0; i < V; ++i) take(p[u].v[i], i);
      }
      for (; e + V <= hi; e += stride) {
        const SelPack<T, V> p = *reinterpret_cast<const SelPack<T, V>*>(img + e);
#pragma unroll
        for (int i = 0; i < V; ++i) take(p.v[i], i);
      }
      if (e < hi) {  // partial vector: same lane, same channels
#pragma unroll
        for (int i = 0; i < V; ++i)
          if (e + i < hi) take(img[e + i], i);
      }
    }
    __syncthreads();
    // the group's tables (their replicas summed) into global memory, once
    const int here = min(S / R, n_slots - s0);
    for (int i = t; i < here * 256; i += 256) {
      const int rel = i >> 8, d = i & 255;
      unsigned int v = 0u;
      for (int r = 0; r < R; ++r) v += tab[(rel * R + r) * kTabStride + d];
      if (v) atomicAdd(&hist[(size_t)(s0 + rel) * 256 + d], (unsigned long long)v);
    }
    __syncthreads();
  }
  if constexpr (FIRST) {
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (nanc[i]) atomicAdd(&s_nan[chn[i]], (unsigned long long)nanc[i]);
    __syncthreads();
    for (int c = t; c < C; c += 256)
      if (s_nan[c]) atomicAdd(&st.nan_cnt[c], s_nan[c]);
  }
}

// One workgroup.  first: the kept counts and the ranks of the percentiles.
// Then per channel and rank the digit that holds the rank and the rank inside
// it; then either the channel's distinct prefixes and their tables for the
// next pass, or (last) the order statistics.
template <typename T>
__global__ void __launch_bounds__(kChoiceThreads) select_choose_kernel(
    int C, int nq, int first, int last, QList qf, const unsigned long long* __restrict__ hist,
    SelState st, double* __restrict__ out) {
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  constexpr int kWaves = kChoiceThreads / 64;
  const int L = 2 * nq;
  if (first) {
    for (int c = wid; c < C; c += kWaves) {
      unsigned long long s = 0ull;
      for (int b = lane; b < 256; b += 64) s += hist[(size_t)c * 256 + b];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) st.n_kept[c] = s;
      if (lane < L) {
        unsigned long long rank = 0ull;
        if (s) {
          const double v = qf.q[lane >> 1] * (double)(s - 1ull);
          const unsigned long long fl = (unsigned long long)floor(v);
          const unsigned long long up = fl + 1ull;
          rank = (lane & 1) ? (up < s ? up : s - 1ull) : (fl < s ? fl : s - 1ull);
        }
        st.rank_prefix[c * L + lane] = 0u;
        st.rank_rem[c * L + lane] = rank;
        st.rank_slot[c * L + lane] = s ? c : -1;
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  for (int pr = wid; pr < C * L; pr += kWaves) {
    const int slot = st.rank_slot[pr];
    if (slot < 0) continue;
    const unsigned long long rem = st.rank_rem[pr];
    unsigned long long h[4], s = 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) { h[i] = hist[(size_t)slot * 256 + lane * 4 + i]; s += h[i]; }
    unsigned long long incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    unsigned long long cum = incl - s;
    if (rem >= cum && rem < incl) {  // one lane
      int d = lane * 4;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (rem >= cum + h[i] && d == lane * 4 + i) { cum += h[i]; d += 1; }
      st.rank_prefix[pr] = (st.rank_prefix[pr] << 8) | (uint32_t)d;
      st.rank_rem[pr] = rem - cum;
    }
  }
  __threadfence_block();
  __syncthreads();
  if (last) {
    for (int i = t; i < C * nq; i += kChoiceThreads) {
      const int c = i / nq, qi = i - c * nq;
      const unsigned long long n = st.n_kept[c];
      const double nanv = __longlong_as_double(0x7ff8000000000000ll);
      out[(size_t)i * 4 + 0] = n ? sel_value<T>(st.rank_prefix[c * L + 2 * qi]) : nanv;
      out[(size_t)i * 4 + 1] = n ? sel_value<T>(st.rank_prefix[c * L + 2 * qi + 1]) : nanv;
      out[(size_t)i * 4 + 2] = (double)n;
      out[(size_t)i * 4 + 3] = (double)st.nan_cnt[c];
    }
    return;
  }
  for (int c = t; c < C; c += kChoiceThreads) {
    int nuq = 0;
    if (st.n_kept[c]) {
      for (int r = 0; r < L; ++r) {
        const uint32_t pf = st.rank_prefix[c * L + r];
        int j = 0;
        while (j < nuq && st.uprefix[c * L + j] != pf) ++j;
        if (j == nuq) { st.uprefix[c * L + j] = pf; ++nuq; }
        st.rank_slot[c * L + r] = j;  // within the channel; the base is added below
      }
    }
    st.nuniq[c] = nuq;
  }
  __threadfence_block();
  __syncthreads();
  if (t == 0) {
    int base = 0;
    for (int c = 0; c < C; ++c) { st.slot_base[c] = base; base += st.nuniq[c]; }
    *st.n_slots = base;
  }
  __threadfence_block();
  __syncthreads();
  for (int i = t; i < C * L; i += kChoiceThreads) {
    const int c = i / L;
    if (st.n_kept[c]) st.rank_slot[i] += st.slot_base[c];
  }
}

// ------------------------------------------------------------------ rescale
template <typename T>
using Vec4 = T __attribute__((ext_vector_type(4)));

template <typename T>
__global__ void __launch_bounds__(256) rescale_kernel(const T* img, int64_t n_elem, int C, int teff,
                                                      int64_t epb, const double* __restrict__ params,
                                                      float* out) {
  constexpr int V = 4;
  const int t = threadIdx.x;
  if (t >= teff) return;
  const int64_t lo_e = (int64_t)blockIdx.x * epb;
  const int64_t hi_e = min(n_elem, lo_e + epb);
  double lo[V], hi[V], omin[V], omax[V];
  int mode[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = (int)(((int64_t)t * V + i) % C);
    lo[i] = params[c * 5 + 0];
    hi[i] = params[c * 5 + 1];
    omin[i] = params[c * 5 + 2];
    omax[i] = params[c * 5 + 3];
    mode[i] = (int)params[c * 5 + 4];
  }
  auto f = [&](T v, int i) -> float {
    if (mode[i] == 0) return (float)v;
    const double x = (double)v;
    if (mode[i] == 3) return (float)((x - lo[i]) / (hi[i] - lo[i]));
    if (x != x) return (float)x;
    if (mode[i] == 2) return (float)fmin(fmax(x, omin[i]), omax[i]);
    const double xc = fmin(fmax(x, lo[i]), hi[i]);
    return (float)((xc - lo[i]) / (hi[i] - lo[i]) * (omax[i] - omin[i]) + omin[i]);
  };
  const int64_t stride = (int64_t)teff * V;
  int64_t e = lo_e + (int64_t)t * V;
  for (; e + V <= hi_e; e += stride) {
    const Vec4<T> p = ld_stream(reinterpret_cast<const Vec4<T>*>(img + e));
    Vec4<float> o;
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = f(p[i], i);
    __builtin_nontemporal_store(o, reinterpret_cast<Vec4<float>*>(out + e));
  }
  if (e < hi_e) {
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (e + i < hi_e) out[e + i] = f(img[e + i], i);
  }
}

static inline int sel_gcd(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

struct SelPlan { int teff; int64_t epb; int G; };
static SelPlan sel_plan(int64_t n_elem, int C, int V, int max_blocks) {
  const int unit = C / sel_gcd(V, C);  // lanes per channel period (<= C <= 256)
  SelPlan p;
  p.teff = (256 / unit) * unit;
  const int64_t chunk = (int64_t)p.teff * V;  // a multiple of C and of V
  const int64_t chunks = (n_elem + chunk - 1) / chunk;
  int G = (int)(chunks < max_blocks ? chunks : max_blocks);
  if (G < 1) G = 1;
  p.epb = ((chunks + G - 1) / G) * chunk;
  p.G = (int)((n_elem + p.epb - 1) / p.epb);
  if (p.G < 1) p.G = 1;
  return p;
}

static inline size_t al16(size_t n) { return (n + 15) & ~(size_t)15; }

struct SelLayout {
  size_t hist, nan_cnt, n_kept, rank_prefix, rank_rem, rank_slot, nuniq, slot_base, uprefix, n_slots, total;
};
static SelLayout sel_layout(int C, int nq) {
  const size_t L = 2 * (size_t)nq, cl = (size_t)C * L;
  SelLayout o;
  size_t at = 0;
  o.hist = at;        at += al16(4 * cl * 256 * sizeof(unsigned long long));  // one region per pass
  o.nan_cnt = at;     at += al16((size_t)C * 8);
  o.n_kept = at;      at += al16((size_t)C * 8);
  o.rank_prefix = at; at += al16(cl * 4);
  o.rank_rem = at;    at += al16(cl * 8);
  o.rank_slot = at;   at += al16(cl * 4);
  o.nuniq = at;       at += al16((size_t)C * 4);
  o.slot_base = at;   at += al16((size_t)C * 4);
  o.uprefix = at;     at += al16(cl * 4);
  o.n_slots = at;     at += 16;
  o.total = at;
  return o;
}

static SelState sel_state(const SelLayout& lay, char* ws) {
  SelState st;
  st.nan_cnt = reinterpret_cast<unsigned long long*>(ws + lay.nan_cnt);
  st.n_kept = reinterpret_cast<unsigned long long*>(ws + lay.n_kept);
  st.rank_prefix = reinterpret_cast<uint32_t*>(ws + lay.rank_prefix);
  st.rank_rem = reinterpret_cast<unsigned long long*>(ws + lay.rank_rem);
  st.rank_slot = reinterpret_cast<int*>(ws + lay.rank_slot);
  st.nuniq = reinterpret_cast<int*>(ws + lay.nuniq);
  st.slot_base = reinterpret_cast<int*>(ws + lay.slot_base);
  st.uprefix = reinterpret_cast<uint32_t*>(ws + lay.uprefix);
  st.n_slots = reinterpret_cast<int*>(ws + lay.n_slots);
  return st;
}

static inline unsigned long long* sel_hist(const SelLayout& lay, char* ws, int Ce, int nq, int ps) {
  return reinterpret_cast<unsigned long long*>(ws + lay.hist) + (size_t)ps * Ce * 2 * nq * 256;
}

static inline int sel_passes(int dtype) { return dtype == MW_U8 ? 1 : dtype == MW_U16 ? 2 : dtype == MW_F32 ? 4 : 0; }

// Pass ps of the selection over the elements [off, n_elem) of the 16-byte
// aligned img: added to the pass's histograms.
template <typename T>
static int run_count(const void* d_img, int64_t n_elem, int off, int Ce, int nq, int ps, int passes, int skip,
                     const SelLayout& lay, char* ws, hipStream_t s) {
  const int L = 2 * nq;
  const SelState st = sel_state(lay, ws);
  const SelPlan p = sel_plan(n_elem, Ce, SelVec<T>::N, kSelBlocks);
  const T* img = reinterpret_cast<const T*>(d_img);
  const int shift = 8 * (passes - 1 - ps);
  const int phase = (Ce - off % Ce) % Ce;
  unsigned long long* hist = sel_hist(lay, ws, Ce, nq, ps);
  if (ps == 0)
    hipLaunchKernelGGL((select_count_kernel<T, true, false>), dim3(p.G), dim3(256), 0, s, img, n_elem, Ce,
                       L, p.teff, p.epb, shift, skip, off, phase, st, hist);
  else if (L <= kRegPrefixes)
    hipLaunchKernelGGL((select_count_kernel<T, false, true>), dim3(p.G), dim3(256), 0, s, img, n_elem, Ce,
                       L, p.teff, p.epb, shift, skip, off, phase, st, hist);
  else
    hipLaunchKernelGGL((select_count_kernel<T, false, false>), dim3(p.G), dim3(256), 0, s, img, n_elem, Ce,
                       L, p.teff, p.epb, shift, skip, off, phase, st, hist);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

template <typename T>
static int run_choose(int Ce, int nq, int ps, int passes, const QList& qf, const SelLayout& lay, char* ws,
                      double* d_out, hipStream_t s) {
  hipLaunchKernelGGL(select_choose_kernel<T>, dim3(1), dim3(kChoiceThreads), 0, s, Ce, nq, ps == 0 ? 1 : 0,
                     ps == passes - 1 ? 1 : 0, qf, sel_hist(lay, ws, Ce, nq, ps), sel_state(lay, ws), d_out);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

static int sel_count(const void* d_img, int dtype, int64_t n_elem, int off, int Ce, int nq, int ps, int skip,
                     const SelLayout& lay, char* ws, hipStream_t s) {
  switch (dtype) {
    case MW_U8: return run_count<uint8_t>(d_img, n_elem, off, Ce, nq, ps, 1, 0, lay, ws, s);
    case MW_U16: return run_count<uint16_t>(d_img, n_elem, off, Ce, nq, ps, 2, 0, lay, ws, s);
    default: return run_count<float>(d_img, n_elem, off, Ce, nq, ps, 4, skip, lay, ws, s);
  }
}

static int sel_choose(int dtype, int Ce, int nq, int ps, const QList& qf, const SelLayout& lay, char* ws,
                      double* d_out, hipStream_t s) {
  switch (dtype) {
    case MW_U8: return run_choose<uint8_t>(Ce, nq, ps, 1, qf, lay, ws, d_out, s);
    case MW_U16: return run_choose<uint16_t>(Ce, nq, ps, 2, qf, lay, ws, d_out, s);
    default: return run_choose<float>(Ce, nq, ps, 4, qf, lay, ws, d_out, s);
  }
}

// the percentiles as fractions; false: one lies outside [0, 100]
static bool sel_qlist(const double* h_q, int nq, QList& qf, int& bad) {
  for (int i = 0; i < kMaxQ; ++i) qf.q[i] = 0.0;
  for (int i = 0; i < nq; ++i) {
    if (!(h_q[i] >= 0.0 && h_q[i] <= 100.0)) { bad = i; return false; }
    qf.q[i] = h_q[i] / 100.0;
  }
  return true;
}

}  // namespace mw

using namespace mw;

extern "C" {

size_t mw_quantiles_ws_bytes(int C, int nq) {
  if (C < 1 || nq < 1 || nq > kMaxQ) return 0;
  return sel_layout(C, nq).total + 256;
}

int mw_quantiles(const void* d_img, int dtype, int64_t n_pix, int C, int pooled, const double* h_q,
                 int nq, int skip_sentinel, double* d_out, void* d_ws, void* stream) {
  MW_CHECK_ARG(d_img && h_q && d_out && d_ws, "mw_quantiles: null pointer");
  MW_CHECK_ARG(C >= 1 && n_pix >= 1, "mw_quantiles: bad shape n_pix=%lld C=%d", (long long)n_pix, C);
  MW_CHECK_ARG(n_pix <= ((int64_t)1 << 40) / C, "mw_quantiles: more than 2^40 elements");
  MW_CHECK_ARG(nq >= 1 && nq <= kMaxQ, "mw_quantiles: nq=%d outside 1..%d", nq, kMaxQ);
  MW_CHECK_ARG(((uintptr_t)d_img & 15) == 0 && ((uintptr_t)d_ws & 15) == 0,
               "mw_quantiles: image and workspace must be 16-byte aligned");
  QList qf;
  int bad = 0;
  MW_CHECK_ARG(sel_qlist(h_q, nq, qf, bad), "mw_quantiles: q[%d]=%g outside [0, 100]", bad, h_q[bad]);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_quantiles: bad dtype %d", dtype);
  const int Ce = pooled ? 1 : C;
  if (Ce > kMaxSelC) {
    set_error("mw_quantiles: %d channels (per-channel selection takes up to %d)", C, kMaxSelC);
    return MW_EUNSUPPORTED;
  }
  hipStream_t s = as_stream(stream);
  // the layout of the advertised size (C channels) also holds the pooled one
  const SelLayout lay = sel_layout(Ce, nq);
  MW_HIP(hipMemsetAsync(d_ws, 0, lay.total, s));
  const int64_t n_elem = n_pix * C;
  char* ws = reinterpret_cast<char*>(d_ws);
  const int passes = sel_passes(dtype);
  for (int ps = 0; ps < passes; ++ps) {
    int rc = sel_count(d_img, dtype, n_elem, 0, Ce, nq, ps, skip_sentinel, lay, ws, s);
    if (rc != MW_OK) return rc;
    rc = sel_choose(dtype, Ce, nq, ps, qf, lay, ws, d_out, s);
    if (rc != MW_OK) return rc;
  }
  return MW_OK;
}

int mw_quantiles_passes(int dtype) { return sel_passes(dtype); }

int mw_quantiles_rows_begin(int C, int pooled, int nq, void* d_ws, void* stream) {
  MW_CHECK_ARG(d_ws, "mw_quantiles_rows_begin: null pointer");
  MW_CHECK_ARG(C >= 1, "mw_quantiles_rows_begin: bad shape C=%d", C);
  MW_CHECK_ARG(nq >= 1 && nq <= kMaxQ, "mw_quantiles_rows_begin: nq=%d outside 1..%d", nq, kMaxQ);
  MW_CHECK_ARG(((uintptr_t)d_ws & 15) == 0, "mw_quantiles_rows_begin: the workspace must be 16-byte aligned");
  const int Ce = pooled ? 1 : C;
  if (Ce > kMaxSelC) {
    set_error("mw_quantiles_rows_begin: %d channels (per-channel selection takes up to %d)", C, kMaxSelC);
    return MW_EUNSUPPORTED;
  }
  MW_HIP(hipMemsetAsync(d_ws, 0, sel_layout(Ce, nq).total, as_stream(stream)));
  return MW_OK;
}

int mw_quantiles_rows_count(const void* d_rows, int dtype, int64_t n_pix, int C, int pooled, int nq,
                            int skip_sentinel, int pass, void* d_ws, void* stream) {
  MW_CHECK_ARG(d_rows && d_ws, "mw_quantiles_rows_count: null pointer");
  MW_CHECK_ARG(C >= 1 && n_pix >= 1, "mw_quantiles_rows_count: bad shape n_pix=%lld C=%d", (long long)n_pix, C);
  MW_CHECK_ARG(n_pix <= ((int64_t)1 << 40) / C, "mw_quantiles_rows_count: more than 2^40 elements");
  MW_CHECK_ARG(nq >= 1 && nq <= kMaxQ, "mw_quantiles_rows_count: nq=%d outside 1..%d", nq, kMaxQ);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_quantiles_rows_count: bad dtype %d",
               dtype);
  MW_CHECK_ARG(pass >= 0 && pass < sel_passes(dtype), "mw_quantiles_rows_count: pass %d outside 0..%d", pass,
               sel_passes(dtype) - 1);
  const uintptr_t p = (uintptr_t)d_rows;
  const int elem = dtype == MW_U8 ? 1 : dtype == MW_U16 ? 2 : 4;
  MW_CHECK_ARG(p % elem == 0 && ((uintptr_t)d_ws & 15) == 0,
               "mw_quantiles_rows_count: rows must be element aligned, the workspace 16-byte aligned");
  const int Ce = pooled ? 1 : C;
  if (Ce > kMaxSelC) {
    set_error("mw_quantiles_rows_count: %d channels (per-channel selection takes up to %d)", C, kMaxSelC);
    return MW_EUNSUPPORTED;
  }
  // the band from the 16-byte boundary at or below its start: the elements
  // before it are loaded with the first vector and left out
  const int off = (int)((p & 15) / elem);
  const void* base = reinterpret_cast<const void*>(p & ~(uintptr_t)15);
  return sel_count(base, dtype, n_pix * C + off, off, Ce, nq, pass, skip_sentinel, sel_layout(Ce, nq),
                   reinterpret_cast<char*>(d_ws), as_stream(stream));
}

int mw_quantiles_rows_choose(int dtype, int C, int pooled, const double* h_q, int nq, int pass, double* d_out,
                             void* d_ws, void* stream) {
  MW_CHECK_ARG(h_q && d_out && d_ws, "mw_quantiles_rows_choose: null pointer");
  MW_CHECK_ARG(C >= 1, "mw_quantiles_rows_choose: bad shape C=%d", C);
  MW_CHECK_ARG(nq >= 1 && nq <= kMaxQ, "mw_quantiles_rows_choose: nq=%d outside 1..%d", nq, kMaxQ);
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_quantiles_rows_choose: bad dtype %d",
               dtype);
  MW_CHECK_ARG(pass >= 0 && pass < sel_passes(dtype), "mw_quantiles_rows_choose: pass %d outside 0..%d", pass,
               sel_passes(dtype) - 1);
  MW_CHECK_ARG(((uintptr_t)d_ws & 15) == 0, "mw_quantiles_rows_choose: the workspace must be 16-byte aligned");
  QList qf;
  int bad = 0;
  MW_CHECK_ARG(sel_qlist(h_q, nq, qf, bad), "mw_quantiles_rows_choose: q[%d]=%g outside [0, 100]", bad, h_q[bad]);
  const int Ce = pooled ? 1 : C;
  if (Ce > kMaxSelC) {
    set_error("mw_quantiles_rows_choose: %d channels (per-channel selection takes up to %d)", C, kMaxSelC);
    return MW_EUNSUPPORTED;
  }
  return sel_choose(dtype, Ce, nq, pass, qf, sel_layout(Ce, nq), reinterpret_cast<char*>(d_ws), d_out,
                    as_stream(stream));
}

int mw_rescale(const void* d_img, int dtype, int64_t n_pix, int C, const double* d_params, float* d_out,
               void* stream) {
  MW_CHECK_ARG(d_img && d_params && d_out, "mw_rescale: null pointer");
  MW_CHECK_ARG(C >= 1 && n_pix >= 1, "mw_rescale: bad shape n_pix=%lld C=%d", (long long)n_pix, C);
  MW_CHECK_ARG(n_pix <= ((int64_t)1 << 40) / C, "mw_rescale: more than 2^40 elements");
  MW_CHECK_ARG(((uintptr_t)d_img & 15) == 0 && ((uintptr_t)d_out & 15) == 0,
               "mw_rescale: image and output must be 16-byte aligned");
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_rescale: bad dtype %d", dtype);
  if (C > kMaxSelC) {
    set_error("mw_rescale: %d channels (up to %d)", C, kMaxSelC);
    return MW_EUNSUPPORTED;
  }
  MW_CHECK_ARG(dtype == MW_F32 || d_img != (const void*)d_out, "mw_rescale: only an fp32 image may alias out");
  hipStream_t s = as_stream(stream);
  const int64_t n_elem = n_pix * C;
  // more, smaller workgroups than the selection: nothing is merged per workgroup
  const SelPlan p = sel_plan(n_elem, C, 4, 16 * kSelBlocks);
  switch (dtype) {
    case MW_U8:
      hipLaunchKernelGGL(rescale_kernel<uint8_t>, dim3(p.G), dim3(256), 0, s, (const uint8_t*)d_img, n_elem,
                         C, p.teff, p.epb, d_params, d_out);
      break;
    case MW_U16:
      hipLaunchKernelGGL(rescale_kernel<uint16_t>, dim3(p.G), dim3(256), 0, s, (const uint16_t*)d_img,
                         n_elem, C, p.teff, p.epb, d_params, d_out);
      break;
    default:
      hipLaunchKernelGGL(rescale_kernel<float>, dim3(p.G), dim3(256), 0, s, (const float*)d_img, n_elem, C,
                         p.teff, p.epb, d_params, d_out);
      break;
  }
  MW_LAUNCH_CHECK();
  return MW_OK;
}

}  // extern "C"
