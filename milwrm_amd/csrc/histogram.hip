// Whole-slide intensity histograms of the MILWRM MxIF container on MI355X
// (gfx950): img.histogram / img.plot_image_histogram (MxIF.py:733-774).
//
// Per selected channel the counts of numpy's uniform-bin histogram of the
// plane as float64 (numpy/lib/_histograms_impl.py:840-867), bit for bit:
//   keep lo <= x <= hi (a NaN fails both);  i = (int)(((x - lo) / (hi - lo)) * bins);
//   i == bins: i -= 1;  x < edges[i]: i -= 1;  else x >= edges[i + 1] and
//   i != bins - 1: i += 1
// all in fp64 without contraction, against the caller's np.linspace edge
// table.  The image is read once per pass in the radix select's layout
// (intensity.hip): workgroup b owns a run of whole channel periods of the flat
// HWC array, so the channels of a lane's vector slots never change.  A pass
// may be fed in bands of rows (mw_hist_rows_*): every reduction is an integer
// one (32-bit LDS adds, 64-bit global adds; minima and maxima on monotone
// integer keys), so the totals are the whole slide's whatever the bands.
//
// Contention: a slide's background is one value in millions of pixels.  Each
// lane keeps, per vector slot (one channel), the bin of its last element and
// how often it came in a row, and issues one LDS add per run instead of one per
// element; and while LDS allows, every channel has R tables picked by lane, so
// the lanes of a wave that share a channel and a bin spread over R addresses.
#include <math.h>

#include "common.h"

// the index expression must round as numpy's elementwise operations do
#pragma clang fp contract(off)

namespace mw {

constexpr int kHistBlocks = 1024;     // streaming workgroups (4 per CU)
constexpr int kHistMaxC = 256;        // channels of the image
constexpr int kHistMaxBins = 4096;    // one channel's table and edges stay within kHistLds
constexpr int kHistLds = 60 * 1024;   // bytes of LDS a workgroup takes at most
constexpr int kHistLdsRep = 40 * 1024;  // ... for more than one table per channel (four workgroups per CU)
constexpr int kHistMaxRep = 8;        // tables per channel

template <typename T> struct HistVec;
template <> struct HistVec<uint8_t> { static constexpr int N = 16; };
template <> struct HistVec<uint16_t> { static constexpr int N = 8; };
template <> struct HistVec<float> { static constexpr int N = 4; };

template <typename T, int N>
struct alignas(sizeof(T) * N) HistPack { T v[N]; };

// selected slot of every channel (-1: not selected), by value to the kernels
struct HistSlots { short s[kHistMaxC]; };

// monotone key of an element for the extremes; NaN takes no part
template <typename T>
__device__ __forceinline__ uint32_t hist_key(T v, bool& isnan) {
  isnan = false;
  return (uint32_t)v;
}
template <>
__device__ __forceinline__ uint32_t hist_key<float>(float v, bool& isnan) {
  isnan = v != v;
  uint32_t b = __float_as_uint(v);
  if (v == 0.0f) b = 0u;  // -0.0 orders (and is returned) as +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename T>
__device__ __forceinline__ double hist_value(uint32_t key) { return (double)key; }
template <>
__device__ __forceinline__ double hist_value<float>(uint32_t key) {
  const uint32_t b = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  return (double)__uint_as_float(b);
}

// State in the workspace (device pointers)
struct HistState {
  uint32_t* kmin;               // [C] smallest key (all ones: none yet)
  uint32_t* kmax;               // [C] largest key
  unsigned long long* n_ok;     // [C] non-NaN elements of the range pass
  unsigned long long* n_nan;    // [C] NaN elements of the range pass
  unsigned long long* counts;   // [C * bins], by selected slot
};

// The elements [off, n_elem) of the 16-byte aligned img that workgroup
// blockIdx.x owns ([b * epb, (b + 1) * epb)), lane t taking the vectors t,
// t + teff, ...; teff * V is a multiple of C, so slot i of the lane always
// holds channel (t * V + i + phase) % C.  off < V: only the first vector of
// workgroup 0 holds elements before the band, its lane takes it element by
// element, as the partial last vector.  MASKED: an element takes part when the
// mask byte of its pixel ((e - off) / C, the band's first pixel is mask[0]) is
// not zero; the pixel of slot i is that of slot 0 plus a per-lane constant,
// because every vector of the lane starts at the same offset in the channel
// period.  take(v, i) is called, with i a compile-time slot, for the slots
// with use(i) (the mask byte of another slot is not loaded).
template <typename T, bool MASKED, typename U, typename F>
__device__ __forceinline__ void hist_walk(const T* __restrict__ img, int64_t n_elem, int C, int teff,
                                          int64_t epb, int off, const uint8_t* __restrict__ mask, U use,
                                          F take) {
  constexpr int V = HistVec<T>::N;
  const int t = threadIdx.x;
  if (t >= teff) return;
  const int64_t lo = (int64_t)blockIdx.x * epb;
  const int64_t hi = min(n_elem, lo + epb);
  const int64_t stride = (int64_t)teff * V;
  const int64_t ppv = stride / C;  // pixels between a lane's vectors
  int64_t e = lo + (int64_t)t * V;
  int dl[MASKED ? V : 1];
  if constexpr (MASKED) {
    // (e - off may be negative only for the vector that straddles the band's start, taken apart below)
    const int r0 = (int)(((e - off) % C + C) % C);
#pragma unroll
    for (int i = 0; i < V; ++i) dl[i] = (r0 + i) / C;
  }
  auto pix0 = [&](int64_t ee) -> int64_t { return (ee - off) / C; };  // ee >= off
  if (off > 0 && e == 0) {  // the vector that straddles the band's start
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (i >= off && i < hi) {
        bool on = use(i);
        if constexpr (MASKED) on = on && mask[(i - off) / C] != 0;
        if (on) take(img[i], i);
      }
    e += stride;
  }
  // four independent 16-B loads in flight per iteration
  for (; e + 3 * stride + V <= hi; e += 4 * stride) {
    HistPack<T, V> p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) p[u] = *reinterpret_cast<const HistPack<T, V>*>(img + e + u * stride);
    const int64_t px = MASKED ? pix0(e) : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) {
        bool on = use(i);
        if constexpr (MASKED) on = on && mask[px + u * ppv + dl[i]] != 0;
        if (on) take(p[u].v[i], i);
      }
  }
  for (; e + V <= hi; e += stride) {
    const HistPack<T, V> p = *reinterpret_cast<const HistPack<T, V>*>(img + e);
    const int64_t px = MASKED ? pix0(e) : 0;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      bool on = use(i);
      if constexpr (MASKED) on = on && mask[px + dl[i]] != 0;
      if (on) take(p.v[i], i);
    }
  }
  if (e < hi) {  // partial vector: same lane, same channels
    const int64_t px = MASKED ? pix0(e) : 0;
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (e + i < hi) {
        bool on = use(i);
        if constexpr (MASKED) on = on && mask[px + dl[i]] != 0;
        if (on) take(img[e + i], i);
      }
  }
}

// Extremes and NaN / non-NaN counts of the selected channels: per lane in
// registers, per workgroup in LDS, then one global atomic per channel.
template <typename T, bool MASKED>
__global__ void __launch_bounds__(256) hist_range_kernel(const T* __restrict__ img, int64_t n_elem, int C,
                                                         int teff, int64_t epb, int off, int phase,
                                                         HistSlots slots, const uint8_t* __restrict__ mask,
                                                         HistState st) {
  constexpr int V = HistVec<T>::N;
  __shared__ uint32_t s_min[kHistMaxC], s_max[kHistMaxC];
  __shared__ unsigned long long s_ok[kHistMaxC], s_nan[kHistMaxC];
  const int t = threadIdx.x;
  for (int c = t; c < C; c += 256) { s_min[c] = ~0u; s_max[c] = 0u; s_ok[c] = 0ull; s_nan[c] = 0ull; }
  __syncthreads();
  int chn[V];
  bool sel[V];
  uint32_t kmin[V], kmax[V], nok[V], nnan[V];  // a lane sees far fewer than 2^32 elements
  bool any = false;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    chn[i] = (int)(((int64_t)t * V + i + phase) % C);
    sel[i] = slots.s[chn[i]] >= 0;
    any |= sel[i];
    kmin[i] = ~0u; kmax[i] = 0u; nok[i] = 0u; nnan[i] = 0u;
  }
  if (any) {
    hist_walk<T, MASKED>(img, n_elem, C, teff, epb, off, mask, [&](int i) { return sel[i]; }, [&](T v, int i) {
      bool isnan;
      const uint32_t key = hist_key<T>(v, isnan);
      nnan[i] += isnan ? 1u : 0u;
      kmin[i] = isnan ? kmin[i] : min(kmin[i], key);
      kmax[i] = isnan ? kmax[i] : max(kmax[i], key);
      nok[i] += isnan ? 0u : 1u;
    });
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (nok[i]) {
        atomicMin(&s_min[chn[i]], kmin[i]);
        atomicMax(&s_max[chn[i]], kmax[i]);
        atomicAdd(&s_ok[chn[i]], (unsigned long long)nok[i]);
      }
      if (nnan[i]) atomicAdd(&s_nan[chn[i]], (unsigned long long)nnan[i]);
    }
  }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    if (s_ok[c]) {
      atomicMin(&st.kmin[c], s_min[c]);
      atomicMax(&st.kmax[c], s_max[c]);
      atomicAdd(&st.n_ok[c], s_ok[c]);
    }
    if (s_nan[c]) atomicAdd(&st.n_nan[c], s_nan[c]);
  }
}

// The counts of the selected slots [s0, s0 + gn).  Dynamic LDS: the slots'
// edges (gn * (bins + 1) doubles), then gn * R tables of ts = bins | 1 words
// (an odd stride: equal bins of different tables fall into different banks).
template <typename T, bool MASKED>
__global__ void __launch_bounds__(256) hist_count_kernel(const T* __restrict__ img, int64_t n_elem, int C,
                                                         int teff, int64_t epb, int off, int phase,
                                                         HistSlots slots, int bins, int s0, int gn, int R,
                                                         const double* __restrict__ edges,
                                                         const uint8_t* __restrict__ mask,
                                                         unsigned long long* __restrict__ counts) {
  constexpr int V = HistVec<T>::N;
  extern __shared__ double s_hist[];
  double* s_edge = s_hist;
  const int ne = bins + 1, ts = bins | 1;
  unsigned int* tab = reinterpret_cast<unsigned int*>(s_hist + (size_t)gn * ne);
  const int t = threadIdx.x;
  for (int i = t; i < gn * ne; i += 256) s_edge[i] = edges[(size_t)s0 * ne + i];
  for (int i = t; i < gn * R * ts; i += 256) tab[i] = 0u;
  __syncthreads();
  const int rep = t & (R - 1);
  int tb[V], eb[V];  // the lane's table and edges of slot i (-1: the channel is not in this launch)
  double lo[V], hi[V];
  int rb[V];           // run: the table word of the slot's last element (-1: none) ...
  unsigned int rc[V];  // ... and how many elements in a row fell into it
  bool any = false;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = (int)(((int64_t)t * V + i + phase) % C);
    const int rel = (int)slots.s[c] - s0;
    const bool in = slots.s[c] >= 0 && rel >= 0 && rel < gn;
    tb[i] = in ? (rel * R + rep) * ts : -1;
    eb[i] = in ? rel * ne : 0;
    lo[i] = in ? s_edge[eb[i]] : 0.0;
    hi[i] = in ? s_edge[eb[i] + bins] : 0.0;
    rb[i] = -1;
    rc[i] = 0u;
    any |= in;
  }
  if (any) {
    hist_walk<T, MASKED>(img, n_elem, C, teff, epb, off, mask, [&](int i) { return tb[i] >= 0; }, [&](T v, int i) {
      const double x = (double)v;
      if (!(x >= lo[i] && x <= hi[i])) return;  // (a NaN fails both)
      const double f = ((x - lo[i]) / (hi[i] - lo[i])) * (double)bins;
      int b = f < (double)bins ? (int)f : bins - 1;  // (also f == bins: the last bin holds its right edge)
      if (x < s_edge[eb[i] + b]) b -= 1;
      else if (x >= s_edge[eb[i] + b + 1] && b != bins - 1) b += 1;
      b = max(b, 0);
      const int w = tb[i] + b;
      if (w == rb[i]) {
        rc[i] += 1u;
      } else {
        if (rc[i]) atomicAdd(&tab[rb[i]], rc[i]);
        rb[i] = w;
        rc[i] = 1u;
      }
    });
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (rc[i]) atomicAdd(&tab[rb[i]], rc[i]);
  }
  __syncthreads();
  // the tables (their replicas summed) into global memory, once
  for (int i = t; i < gn * bins; i += 256) {
    const int rel = i / bins, b = i - rel * bins;
    unsigned int v = 0u;
    for (int r = 0; r < R; ++r) v += tab[(rel * R + r) * ts + b];
    if (v) atomicAdd(&counts[(size_t)(s0 + rel) * bins + b], (unsigned long long)v);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) hist_finish_kernel(int C, HistSlots slots, int bins, HistState st,
                                                          long long* __restrict__ d_counts,
                                                          double* __restrict__ d_record) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  int n_sel = 0;
  for (int c = 0; c < C; ++c) n_sel += slots.s[c] >= 0;
  if (d_counts)
    for (int i = t; i < n_sel * bins; i += gridDim.x * 256) d_counts[i] = (long long)st.counts[i];
  if (d_record && blockIdx.x == 0)
    for (int c = threadIdx.x; c < C; c += 256) {
      const int s = slots.s[c];
      if (s < 0) continue;
      const unsigned long long n = st.n_ok[c];
      const double nanv = __longlong_as_double(0x7ff8000000000000ll);
      d_record[s * 4 + 0] = n ? hist_value<T>(st.kmin[c]) : nanv;
      d_record[s * 4 + 1] = n ? hist_value<T>(st.kmax[c]) : nanv;
      d_record[s * 4 + 2] = (double)n;
      d_record[s * 4 + 3] = (double)st.n_nan[c];
    }
}

static inline int hist_gcd(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

struct HistPlan { int teff; int64_t epb; int G; };
static HistPlan hist_plan(int64_t n_elem, int C, int V) {
  const int unit = C / hist_gcd(V, C);  // lanes per channel period (<= C <= 256)
  HistPlan p;
  p.teff = (256 / unit) * unit;
  const int64_t chunk = (int64_t)p.teff * V;  // a multiple of C and of V
  const int64_t chunks = (n_elem + chunk - 1) / chunk;
  int G = (int)(chunks < kHistBlocks ? chunks : kHistBlocks);
  if (G < 1) G = 1;
  p.epb = ((chunks + G - 1) / G) * chunk;
  p.G = (int)((n_elem + p.epb - 1) / p.epb);
  if (p.G < 1) p.G = 1;
  return p;
}

static inline size_t hist_al16(size_t n) { return (n + 15) & ~(size_t)15; }

struct HistLayout { size_t kmin, kmax, n_ok, n_nan, counts, total; };
static HistLayout hist_layout(int C, int bins) {
  HistLayout o;
  size_t at = 0;
  o.kmin = at;   at += hist_al16((size_t)C * 4);
  o.kmax = at;   at += hist_al16((size_t)C * 4);
  o.n_ok = at;   at += hist_al16((size_t)C * 8);
  o.n_nan = at;  at += hist_al16((size_t)C * 8);
  o.counts = at; at += hist_al16((size_t)C * bins * 8);
  o.total = at;
  return o;
}

static HistState hist_state(const HistLayout& lay, char* ws) {
  HistState st;
  st.kmin = reinterpret_cast<uint32_t*>(ws + lay.kmin);
  st.kmax = reinterpret_cast<uint32_t*>(ws + lay.kmax);
  st.n_ok = reinterpret_cast<unsigned long long*>(ws + lay.n_ok);
  st.n_nan = reinterpret_cast<unsigned long long*>(ws + lay.n_nan);
  st.counts = reinterpret_cast<unsigned long long*>(ws + lay.counts);
  return st;
}

// the selected slots of the channels (h_enable null: all of them); their number
static int hist_slots(int C, const int* h_enable, HistSlots& sl) {
  int n = 0;
  for (int c = 0; c < kHistMaxC; ++c) sl.s[c] = (short)((c < C && (!h_enable || h_enable[c])) ? n++ : -1);
  return n;
}

// LDS bytes of gn slots with R tables each
static inline size_t hist_lds(int gn, int R, int bins) {
  return (size_t)gn * (bins + 1) * 8 + (size_t)gn * R * (bins | 1) * 4;
}

struct HistBand { const void* base; int64_t n_elem; int off, phase; };
// the band from the 16-byte boundary at or below its start: the elements
// before it are loaded with the first vector and left out
static HistBand hist_band(const void* d_rows, int elem, int64_t n_pix, int C) {
  const uintptr_t p = (uintptr_t)d_rows;
  HistBand b;
  b.off = (int)((p & 15) / elem);
  b.base = reinterpret_cast<const void*>(p & ~(uintptr_t)15);
  b.n_elem = n_pix * C + b.off;
  b.phase = (C - b.off % C) % C;
  return b;
}

template <typename T>
static int run_range(const HistBand& b, int C, const HistSlots& sl, const uint8_t* mask, const HistState& st,
                     hipStream_t s) {
  const HistPlan p = hist_plan(b.n_elem, C, HistVec<T>::N);
  const T* img = reinterpret_cast<const T*>(b.base);
  if (mask)
    hipLaunchKernelGGL((hist_range_kernel<T, true>), dim3(p.G), dim3(256), 0, s, img, b.n_elem, C, p.teff, p.epb,
                       b.off, b.phase, sl, mask, st);
  else
    hipLaunchKernelGGL((hist_range_kernel<T, false>), dim3(p.G), dim3(256), 0, s, img, b.n_elem, C, p.teff, p.epb,
                       b.off, b.phase, sl, mask, st);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

// The selected slots in groups that fit the LDS: one launch (one read of the
// band) per group; a single group takes as many tables per channel as fit.
template <typename T>
static int run_count(const HistBand& b, int C, const HistSlots& sl, int n_sel, int bins, const double* d_edges,
                     const uint8_t* mask, const HistState& st, hipStream_t s) {
  const HistPlan p = hist_plan(b.n_elem, C, HistVec<T>::N);
  const T* img = reinterpret_cast<const T*>(b.base);
  int per = (int)(kHistLds / hist_lds(1, 1, bins));  // >= 1: bins <= kHistMaxBins
  if (per > n_sel) per = n_sel;
  int R = 1;
  if (per == n_sel)
    while (R < kHistMaxRep && hist_lds(n_sel, 2 * R, bins) <= (size_t)kHistLdsRep) R *= 2;
  for (int s0 = 0; s0 < n_sel; s0 += per) {
    const int gn = n_sel - s0 < per ? n_sel - s0 : per;
    const size_t lds = hist_lds(gn, R, bins);
    if (mask)
      hipLaunchKernelGGL((hist_count_kernel<T, true>), dim3(p.G), dim3(256), lds, s, img, b.n_elem, C, p.teff,
                         p.epb, b.off, b.phase, sl, bins, s0, gn, R, d_edges, mask, st.counts);
    else
      hipLaunchKernelGGL((hist_count_kernel<T, false>), dim3(p.G), dim3(256), lds, s, img, b.n_elem, C, p.teff,
                         p.epb, b.off, b.phase, sl, bins, s0, gn, R, d_edges, mask, st.counts);
    MW_LAUNCH_CHECK();
  }
  return MW_OK;
}

template <typename T>
static int run_finish(int C, const HistSlots& sl, int n_sel, int bins, const HistState& st, int64_t* d_counts,
                      double* d_record, hipStream_t s) {
  const int64_t n = (int64_t)n_sel * bins;
  int G = (int)((n + 255) / 256);
  if (G > 256) G = 256;
  if (G < 1) G = 1;
  hipLaunchKernelGGL(hist_finish_kernel<T>, dim3(G), dim3(256), 0, s, C, sl, bins, st,
                     reinterpret_cast<long long*>(d_counts), d_record);
  MW_LAUNCH_CHECK();
  return MW_OK;
}

}  // namespace mw

using namespace mw;

#define MW_HIST_CHECK_SHAPE(who)                                                                    \
  MW_CHECK_ARG(C >= 1 && bins >= 1, who ": bad shape C=%d bins=%d", C, bins);                       \
  if (C > kHistMaxC || bins > kHistMaxBins) {                                                       \
    set_error(who ": C=%d bins=%d (up to %d channels, %d bins)", C, bins, kHistMaxC, kHistMaxBins); \
    return MW_EUNSUPPORTED;                                                                         \
  }

#define MW_HIST_CHECK_ROWS(who)                                                                              \
  MW_CHECK_ARG(d_rows && d_ws, who ": null pointer");                                                        \
  MW_CHECK_ARG(n_pix >= 1, who ": bad shape n_pix=%lld", (long long)n_pix);                                  \
  MW_CHECK_ARG(n_pix <= ((int64_t)1 << 40) / C, who ": more than 2^40 elements");                            \
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, who ": bad dtype %d", dtype);           \
  MW_CHECK_ARG((uintptr_t)d_rows % (dtype == MW_U8 ? 1 : dtype == MW_U16 ? 2 : 4) == 0 &&                    \
                   ((uintptr_t)d_ws & 15) == 0,                                                              \
               who ": rows must be element aligned, the workspace 16-byte aligned")

extern "C" {

size_t mw_hist_ws_bytes(int C, int bins) {
  if (C < 1 || C > kHistMaxC || bins < 1 || bins > kHistMaxBins) return 0;
  return hist_layout(C, bins).total + 256;
}

int mw_hist_max_bins(void) { return kHistMaxBins; }

int mw_hist_rows_begin(int C, int bins, void* d_ws, void* stream) {
  MW_CHECK_ARG(d_ws, "mw_hist_rows_begin: null pointer");
  MW_HIST_CHECK_SHAPE("mw_hist_rows_begin");
  MW_CHECK_ARG(((uintptr_t)d_ws & 15) == 0, "mw_hist_rows_begin: the workspace must be 16-byte aligned");
  const HistLayout lay = hist_layout(C, bins);
  char* ws = reinterpret_cast<char*>(d_ws);
  hipStream_t s = as_stream(stream);
  MW_HIP(hipMemsetAsync(ws, 0, lay.total, s));
  MW_HIP(hipMemsetAsync(ws + lay.kmin, 0xff, (size_t)C * 4, s));  // no minimum yet
  return MW_OK;
}

int mw_hist_rows_range(const void* d_rows, int dtype, int64_t n_pix, int C, const int* h_enable, int bins,
                       const uint8_t* d_mask_rows, void* d_ws, void* stream) {
  MW_HIST_CHECK_SHAPE("mw_hist_rows_range");
  MW_HIST_CHECK_ROWS("mw_hist_rows_range");
  HistSlots sl;
  MW_CHECK_ARG(hist_slots(C, h_enable, sl) >= 1, "mw_hist_rows_range: no channel is enabled");
  const HistState st = hist_state(hist_layout(C, bins), reinterpret_cast<char*>(d_ws));
  hipStream_t s = as_stream(stream);
  switch (dtype) {
    case MW_U8: return run_range<uint8_t>(hist_band(d_rows, 1, n_pix, C), C, sl, d_mask_rows, st, s);
    case MW_U16: return run_range<uint16_t>(hist_band(d_rows, 2, n_pix, C), C, sl, d_mask_rows, st, s);
    default: return run_range<float>(hist_band(d_rows, 4, n_pix, C), C, sl, d_mask_rows, st, s);
  }
}

int mw_hist_rows_count(const void* d_rows, int dtype, int64_t n_pix, int C, const int* h_enable, int bins,
                       const double* d_edges, const uint8_t* d_mask_rows, void* d_ws, void* stream) {
  MW_HIST_CHECK_SHAPE("mw_hist_rows_count");
  MW_HIST_CHECK_ROWS("mw_hist_rows_count");
  MW_CHECK_ARG(d_edges && ((uintptr_t)d_edges & 7) == 0, "mw_hist_rows_count: the edges must be 8-byte aligned");
  HistSlots sl;
  const int n_sel = hist_slots(C, h_enable, sl);
  MW_CHECK_ARG(n_sel >= 1, "mw_hist_rows_count: no channel is enabled");
  const HistState st = hist_state(hist_layout(C, bins), reinterpret_cast<char*>(d_ws));
  hipStream_t s = as_stream(stream);
  switch (dtype) {
    case MW_U8:
      return run_count<uint8_t>(hist_band(d_rows, 1, n_pix, C), C, sl, n_sel, bins, d_edges, d_mask_rows, st, s);
    case MW_U16:
      return run_count<uint16_t>(hist_band(d_rows, 2, n_pix, C), C, sl, n_sel, bins, d_edges, d_mask_rows, st, s);
    default:
      return run_count<float>(hist_band(d_rows, 4, n_pix, C), C, sl, n_sel, bins, d_edges, d_mask_rows, st, s);
  }
}

int mw_hist_rows_finish(int dtype, int C, const int* h_enable, int bins, int64_t* d_counts, double* d_record,
                        void* d_ws, void* stream) {
  MW_CHECK_ARG(d_ws && (d_counts || d_record), "mw_hist_rows_finish: null pointer");
  MW_HIST_CHECK_SHAPE("mw_hist_rows_finish");
  MW_CHECK_ARG(dtype == MW_U8 || dtype == MW_U16 || dtype == MW_F32, "mw_hist_rows_finish: bad dtype %d", dtype);
  MW_CHECK_ARG(((uintptr_t)d_ws & 15) == 0, "mw_hist_rows_finish: the workspace must be 16-byte aligned");
  HistSlots sl;
  const int n_sel = hist_slots(C, h_enable, sl);
  MW_CHECK_ARG(n_sel >= 1, "mw_hist_rows_finish: no channel is enabled");
  const HistState st = hist_state(hist_layout(C, bins), reinterpret_cast<char*>(d_ws));
  hipStream_t s = as_stream(stream);
  switch (dtype) {
    case MW_U8: return run_finish<uint8_t>(C, sl, n_sel, bins, st, d_counts, d_record, s);
    case MW_U16: return run_finish<uint16_t>(C, sl, n_sel, bins, st, d_counts, d_record, s);
    default: return run_finish<float>(C, sl, n_sel, bins, st, d_counts, d_record, s);
  }
}

}  // extern "C"
