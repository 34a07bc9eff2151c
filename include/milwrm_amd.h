/*
 * milwrm_amd — C ABI of the MI355X-native MILWRM pixel-clustering hot path.
 *
 * Plain pointers and sizes only (no torch types).  Every pointer named d_* is
 * device memory (HBM) owned by the caller; h_* is host memory.  `stream` is a
 * hipStream_t passed as void*.  All launches are asynchronous on `stream`
 * unless a function says it synchronises.  Workspace buffers (d_ws) are
 * caller-allocated; their sizes come from the matching *_ws_bytes() query.
 * The library never frees caller memory and never allocates inside a launch
 * function.  Status: 0 = ok, < 0 = error; mw_last_error() gives the text.
 *
 * Reference interfaces replaced (file:line in codyheiser/MILWRM unless noted;
 * sklearn/scipy paths are the pinned third-party engines the reference calls):
 *   mw_nz_stats        img.calculate_non_zero_mean        MxIF.py:519-541
 *   mw_lognorm         img.log_normalize                  MxIF.py:416-455
 *   mw_blur            img.blurring('gaussian') → skimage.filters.gaussian →
 *                      scipy.ndimage.gaussian_filter       MxIF.py:375-394
 *   mw_clahe,
 *   mw_clahe_rows_*    img.equalize_hist → skimage equalize_adapthist
 *                                                          MxIF.py:95-122, 360-373
 *   mw_block_mean,
 *   mw_block_reduce_rows img.downsample → skimage block_reduce MxIF.py:494-517
 *   mw_mask_rank,
 *   mw_gather_rows     img.subsample_pixels (mask gather + fancy index)
 *                                                          MxIF.py:457-492
 *   mw_legacy_randint_* np.random.seed(16); np.random.choice(M, S)
 *                                                          MxIF.py:484,490
 *   mw_col_stats_finalize StandardScaler.fit               MILWRM.py:1742-1745
 *   mw_kpp_*           sklearn _kmeans_plusplus            _kmeans.py:174-272
 *   mw_lloyd_pass      sklearn lloyd_iter_chunked_dense    _k_means_lloyd.pyx:23-218
 *                      (+ _inertia_dense                   _k_means_common.pyx:94-124)
 *   mw_farthest        sklearn _relocate_empty_clusters_dense _k_means_common.pyx:181-226
 *   mw_assign_conf     KMeans.predict + estimate_confidence_score_mxif
 *                                                          MILWRM.py:237-277, 389-450
 */
#ifndef MILWRM_AMD_H
#define MILWRM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define MW_OK 0
#define MW_EINVAL (-1)      /* bad argument (ValueError on the Python side) */
#define MW_EHIP (-2)        /* HIP runtime error */
#define MW_EUNSUPPORTED (-3) /* shape/parameter outside what the kernels take */

/* element types of image planes */
#define MW_U8 0
#define MW_U16 1
#define MW_F32 2

int mw_version(void);
const char* mw_last_error(void);
/* Number of streaming workgroups the reductions use for `n` rows; partial
 * buffers are sized from it.  Fixed per n (not per device) so results are
 * identical across runs and shard layouts. */
int mw_stream_blocks(int64_t n);
/* Rows of each of those workgroups (whole 256-row tiles): block b of the
 * gather's and mw_col_stats_rows' records covers rows [b * R, (b + 1) * R). */
int64_t mw_rows_per_block(int64_t n);

/* ---- img.calculate_non_zero_mean (MxIF.py:519-541) --------------------------
 * HWC image of n_pix pixels x C channels.  Outputs per channel: sum of the
 * non-zero values (fp64) and their count (int64).  Deterministic. */
size_t mw_nz_stats_ws_bytes(int64_t n_pix, int C);
int mw_nz_stats(const void* d_img, int dtype, int64_t n_pix, int C,
                double* d_sum, int64_t* d_cnt, void* d_ws, void* stream);

/* ---- img.log_normalize (MxIF.py:416-455) ------------------------------------
 * out = log10(x * inv_mean[c] + pseudoval), HWC, fp32 out. */
int mw_lognorm(const void* d_img, int dtype, int64_t n_pix, int C,
               const float* d_inv_mean, float pseudoval, float* d_out, void* stream);

/* ---- img.clip / img.scale (MxIF.py:29-92, 330-358) ---------------------------
 * Exact order statistics of an HWC image by a most-significant-digit-first
 * radix select (8-bit digits over monotone uint32 keys: 1 pass for u8, 2 for
 * u16, 4 for fp32; no host synchronisation between the passes).  NaNs are left
 * out and counted; -0.0 orders equal to +0.0 and is returned as +0.0.
 * pooled = 0: every channel on its own; pooled = 1: the image as one channel
 * of n_pix * C elements, without the elements equal to -99999 when
 * skip_sentinel is set.  h_q: nq percentiles in [0, 100] (host, nq <= 8).
 * d_out (device, [channels][nq][4] doubles): for numpy's 'linear' rule on the
 * n kept values, v = q/100 (n-1), the order statistics of rank floor(v) and
 * min(floor(v)+1, n-1), then n and the NaN count (NaN, NaN, 0, NaNs when
 * n = 0).  The caller interpolates on the host.  The image must be 16-byte
 * aligned; C <= 256 per-channel (MW_EUNSUPPORTED above). */
size_t mw_quantiles_ws_bytes(int C, int nq);
int mw_quantiles(const void* d_img, int dtype, int64_t n_pix, int C,
                 int pooled, const double* h_q, int nq, int skip_sentinel,
                 double* d_out, void* d_ws, void* stream);
/* The same selection over a slide that is handed over in bands of rows (a
 * slide streamed from the host, stream.quantiles): mw_quantiles is
 * begin, then per pass one count and one choose.
 *   mw_quantiles_passes      passes of a dtype (1 u8, 2 u16, 4 fp32; 0: bad dtype)
 *   mw_quantiles_rows_begin  zeroes the workspace (mw_quantiles_ws_bytes(C, nq))
 *   mw_quantiles_rows_count  adds the n_pix pixels at d_rows to the histograms
 *                            of pass `pass` (and, in pass 0, to the NaN counts);
 *                            once per band, every band in every pass
 *   mw_quantiles_rows_choose once per pass after its last band: the digit of
 *                            every rank; the last pass writes d_out as
 *                            mw_quantiles does
 * The counts are integer adds, so the record is bit for bit mw_quantiles' of
 * the whole slide whatever the bands and their order.  d_rows must start a
 * pixel (element 0 = channel 0) and be aligned to its element type only: a
 * band that is a view into a resident slide starts at y * W * C elements,
 * and the kernel leaves out what precedes it in its first 16-byte vector
 * (up to 15 bytes below d_rows are loaded, inside the same aligned 16 bytes).
 * pooled, skip_sentinel, nq, h_q and C as mw_quantiles, the same values in
 * every call of one selection.  Nothing returns to the host between the calls;
 * all of them on one stream (or ordered by the caller). */
int mw_quantiles_passes(int dtype);
int mw_quantiles_rows_begin(int C, int pooled, int nq, void* d_ws, void* stream);
int mw_quantiles_rows_count(const void* d_rows, int dtype, int64_t n_pix, int C,
                            int pooled, int nq, int skip_sentinel, int pass,
                            void* d_ws, void* stream);
int mw_quantiles_rows_choose(int dtype, int C, int pooled, const double* h_q,
                             int nq, int pass, double* d_out, void* d_ws,
                             void* stream);
/* Elementwise intensity rescale, fp32 out (may alias an fp32 in).  d_params
 * (device, [C][5] doubles): lo, hi, omin, omax, mode with mode 0 = the value
 * itself, 1 = (clip(x, lo, hi) - lo) / (hi - lo) * (omax - omin) + omin,
 * 2 = clip(x, omin, omax), 3 = (x - lo) / (hi - lo); evaluated in fp64 without
 * contraction and rounded once to fp32.  NaN stays NaN in modes 0-2. */
int mw_rescale(const void* d_img, int dtype, int64_t n_pix, int C,
               const double* d_params, float* d_out, void* stream);

/* ---- img.histogram / img.plot_image_histogram (MxIF.py:733-774) ---------------
 * numpy's uniform-bin histogram of every enabled plane of an HWC image, as
 * np.histogram(plane.astype(float64), bins, range=(lo, hi)) counts it, bit for
 * bit.  d_edges (device, [n_sel][bins + 1] doubles, one row per enabled channel
 * in channel order): np.linspace(lo, hi, bins + 1) computed by the caller, lo =
 * row[0] < hi = row[bins].  Per element x of an enabled channel, all in fp64
 * without contraction: kept when lo <= x <= hi (a NaN fails both);
 * i = (int)(((x - lo) / (hi - lo)) * bins); i == bins: i -= 1; x < edges[i]:
 * i -= 1; then x >= edges[i + 1] and i != bins - 1: i += 1.
 * The slide is handed over in bands of rows (the whole image is one band):
 *   mw_hist_rows_begin   resets the state (mw_hist_ws_bytes(C, bins)): the
 *                        channels' extremes, NaN / non-NaN counts, 64-bit counts
 *   mw_hist_rows_range   folds the band's NaN-skipping minimum and maximum and
 *                        its NaN / non-NaN counts into the enabled channels'
 *                        (atomic minima / maxima on monotone integer keys; -0.0
 *                        counts as +0.0); needed only when the caller takes the
 *                        range from the data
 *   mw_hist_rows_count   adds the band's elements to the counts (32-bit LDS
 *                        tables per workgroup, flushed with 64-bit global adds);
 *                        once per band
 *   mw_hist_rows_finish  writes d_counts ([n_sel][bins] int64; may be null) and
 *                        d_record ([n_sel][4] doubles: minimum, maximum, non-NaN
 *                        count, NaN count of the range pass -- NaN, NaN, 0, NaNs
 *                        when no element was not NaN; may be null); it changes
 *                        no state, so the caller may read the record after the
 *                        range pass, make the edges, and go on with the counts
 * h_enable (host, C ints; null: every channel) and bins are the same in every
 * call of one histogram.  d_mask_rows (device uint8, the band's pixels, first
 * pixel first; null: every pixel): only pixels whose byte is not zero take
 * part, in the range and in the counts.  d_rows must start a pixel and be
 * aligned to its element type only, as mw_quantiles_rows_count's.  Every
 * reduction is an integer one, so the results are the whole slide's whatever
 * the bands and their order.  When the enabled channels' tables and edges
 * exceed a workgroup's LDS they are counted in groups, one read of the band
 * per group (100 bins: 50 channels a read; 1000 bins: 5).  Nothing returns
 * to the host between the calls; all of them on one stream (or ordered by the
 * caller).  C <= 256, bins <= 4096 = mw_hist_max_bins() (MW_EUNSUPPORTED above).
 * A slide is read once by the range pass and once per group by the count pass.
 * 10k x 10k x 30 uint16 on one MI355X: range pass 1.01 ms, count
 * pass 4.0-4.3 ms at 100 bins (mw_nz_stats of the same tensor: 0.99 ms), 37.8 ms
 * at 1000 bins (six groups). */
size_t mw_hist_ws_bytes(int C, int bins);
int mw_hist_max_bins(void);
int mw_hist_rows_begin(int C, int bins, void* d_ws, void* stream);
int mw_hist_rows_range(const void* d_rows, int dtype, int64_t n_pix, int C,
                       const int* h_enable, int bins, const uint8_t* d_mask_rows,
                       void* d_ws, void* stream);
int mw_hist_rows_count(const void* d_rows, int dtype, int64_t n_pix, int C,
                       const int* h_enable, int bins, const double* d_edges,
                       const uint8_t* d_mask_rows, void* d_ws, void* stream);
int mw_hist_rows_finish(int dtype, int C, const int* h_enable, int bins,
                        int64_t* d_counts, double* d_record, void* d_ws, void* stream);

/* ---- img.equalize_hist(kernel_size=k) / CLAHE (MxIF.py:95-122, 360-373) ------
 * Contrast-limited adaptive histogram equalisation of every enabled plane of
 * an HWC image, fp32 out; the definition (the published equalize_adapthist
 * procedure restated, G = 16384 grey levels) is DESIGN.md §21.  Per plane:
 * the minimum and maximum; bins b = rint((a - lo) / (hi - lo) (G - 1)) //
 * (1 + G / nbins) in fp64; the histogram of every kh x kw tile (tile (i, j)
 * starts at pixel (i kh, j kw); coordinates past the image are reflected
 * without repeating the edge); each histogram clipped at
 * int(max(clip_limit kh kw, 1)) with the excess redistributed (integers
 * only), summed and scaled into a look-up table of nbins int32 in [0, G - 1];
 * every pixel the bilinear blend of the tables of the four nearest tile
 * centres (fp64 weights, fp32 terms summed in a fixed order); the plane
 * finally rescaled by its own minimum and maximum, (res - rmin) / (rmax -
 * rmin) in fp64 rounded once.  A constant plane, or one whose blend is
 * constant, becomes 0.  NaN input is undefined.  Nothing returns to the host
 * between the stages.
 * h_enable (host, C ints, or NULL for every plane): planes with 0 are written
 * as the fp32 conversion of their values.  d_luts_out (device, may be NULL):
 * the tables, [C][nby][nbx][nbins] int32 with nby = ceil(H / kh), nbx =
 * ceil(W / kw); zeros for planes that are not enabled or constant.
 * d_img, d_out and d_ws must be 16-byte aligned; d_out must not alias d_img.
 * MW_EINVAL: H or W < 2, C < 1, kh outside [1, H], kw outside [1, W],
 * clip_limit not finite or not positive, nbins < 2, a bad dtype, a null or
 * misaligned pointer.  MW_EUNSUPPORTED: nbins > 256, C > 256, W * C or
 * kh * kw of 2^31 or more.  All of them are found before any device call. */
size_t mw_clahe_ws_bytes(int H, int W, int C, int kh, int kw, int nbins);
int mw_clahe(const void* d_img, int dtype, int H, int W, int C, const int* h_enable,
             int kh, int kw, double clip_limit, int nbins, float* d_out,
             void* d_ws, int* d_luts_out, void* stream);
/* The same equalisation of a slide that is handed over in bands of rows (a
 * slide streamed from the host, stream.clahe / stream.ClaheSource; DESIGN.md
 * §26).  d_state: mw_clahe_ws_bytes(H, W, C, kh, kw, nbins) bytes, 16-byte
 * aligned, kept from begin until the last map (the key minima and maxima, the
 * [C][nby][nbx][nbins] counts that become the tables in place, the blend's
 * extremes, the rescale rows).  In this order, every band once per loop:
 *   mw_clahe_rows_begin     checks the arguments as mw_clahe, clears the state
 *   mw_clahe_rows_range     adds a band to the planes' minima and maxima
 *   mw_clahe_rows_hist      counts a band into the tiles' histograms: slide row
 *                           y into tile row y / kh and, when r = 2 H - 2 - y
 *                           lies in [H, nby kh), once more into tile row
 *                           nby - 1 (the rows past the image reflect; as
 *                           nby kh - H < kh <= H a row reflects at most once)
 *   mw_clahe_rows_luts      after the last band: the counts become the tables
 *                           (d_luts_out as mw_clahe's, may be NULL)
 *   mw_clahe_rows_extremes  the map pass of a band without a store: only the
 *                           minimum and maximum of every plane's blend are kept
 *   mw_clahe_rows_finish    after the last band: the rescale rows
 *   mw_clahe_rows_map       writes a band's final fp32 pixels to d_out (rows x
 *                           W x C): the blend and the rescale in one kernel,
 *                           the rescale evaluated as mw_rescale's mode 3
 * The minima, maxima and counts are integer atomics (the blend's extremes
 * integer atomics on fp32 bits), the tables and the map are mw_clahe's code, so
 * tables and pixels are bit for bit mw_clahe's of the whole slide whatever the
 * bands and their order.  d_rows: the slide's rows [y0, y0 + rows), contiguous,
 * aligned to its element type only (a band that is a view into a resident
 * slide starts anywhere; the kernels take their vector phase from the
 * address); d_out: aligned to 4 bytes, and it may be d_rows itself for an fp32
 * band (no other overlap).  dtype, H, W, C, h_enable, kh, kw, clip_limit and
 * nbins as mw_clahe, the same values in every call of one equalisation.
 * MW_EINVAL also for rows < 1, y0 < 0, y0 + rows > H and a null state;
 * MW_EUNSUPPORTED as mw_clahe; all found before any device call.  Nothing
 * returns to the host between the calls; all of them on one stream (or
 * ordered by the caller). */
int mw_clahe_rows_begin(int dtype, int H, int W, int C, int kh, int kw, double clip_limit,
                        int nbins, void* d_state, void* stream);
int mw_clahe_rows_range(const void* d_rows, int dtype, int rows, int W, int C,
                        void* d_state, void* stream);
int mw_clahe_rows_hist(const void* d_rows, int dtype, int y0, int rows, int H, int W, int C,
                       const int* h_enable, int kh, int kw, int nbins, void* d_state,
                       void* stream);
int mw_clahe_rows_luts(int H, int W, int C, int kh, int kw, double clip_limit, int nbins,
                       void* d_state, int* d_luts_out, void* stream);
int mw_clahe_rows_extremes(const void* d_rows, int dtype, int y0, int rows, int H, int W,
                           int C, const int* h_enable, int kh, int kw, int nbins,
                           void* d_state, void* stream);
int mw_clahe_rows_finish(int C, const int* h_enable, void* d_state, void* stream);
int mw_clahe_rows_map(const void* d_rows, int dtype, int y0, int rows, int H, int W, int C,
                      const int* h_enable, int kh, int kw, int nbins, void* d_state,
                      float* d_out, void* stream);

/* ---- img.blurring('median', size=k) (MxIF.py:395-405 as intended) -----------
 * Median filter per channel over a size_y x size_x window (rows y - size_y/2
 * .. y + size_y - 1 - size_y/2, columns likewise; coordinates clamped to the
 * image, scipy's mode='nearest'): the element of rank (size_y size_x) / 2,
 * from 0, of the window sorted ascending (the upper median of an even count)
 * = scipy.ndimage.median_filter(plane, footprint=ones((size_y, size_x)),
 * mode='nearest').  HWC in; exact: the output is an element of the input
 * (fp32 subnormals unchanged; windows holding a NaN are undefined).
 * d_inv_mean == NULL: d_out has the input's dtype.  Otherwise d_out is fp32
 * and holds mw_lognorm's value of the selected raw element, bit for bit
 * (selection commutes with the non-decreasing map, so the filter runs on the
 * compact raw type and writes fp32 once).  Sizes 1..15 per axis: 2x2, 3x3 and
 * 5x5 take a register selection network, every other size a bitwise rank
 * search (mw_median_generic: that search for every size;
 * mw_median_is_network: which of the two mw_median takes).  size < 1 or
 * d_out == d_img: MW_EINVAL; a size above 15: MW_EUNSUPPORTED (nothing
 * launched).  No workspace. */
int mw_median_is_network(int size_y, int size_x);
int mw_median(const void* d_img, int dtype, int H, int W, int C, int size_y, int size_x,
              const float* d_inv_mean, float pseudoval, void* d_out, void* stream);
int mw_median_generic(const void* d_img, int dtype, int H, int W, int C, int size_y, int size_x,
                      const float* d_inv_mean, float pseudoval, void* d_out, void* stream);
/* The row-window form (a slide streamed in row bands, milwrm_amd.stream):
 * d_img holds the H rows [row_off, row_off + H) of a slide of slide_H rows;
 * only the array's rows [r0, r1) are filtered, into a compact d_out of
 * (r1 - r0) x W x C (the input's dtype, or fp32 with the lognorm epilogue).
 * Window rows are clamped to the SLIDE, [0, slide_H - 1], not to the array;
 * columns to [0, W - 1].  The array must hold every clamped window row of
 * every requested output row: r0 >= size_y / 2 when row_off > 0, and H - r1 >=
 * size_y - 1 - size_y / 2 when row_off + H < slide_H; otherwise MW_EINVAL,
 * as for rows outside the slide or r0 >= r1 (nothing launched, d_out
 * untouched).  Rows outside [r0, r1) are read, never computed or written, and
 * no address outside the array is formed.  Calls over bands that tile a slide
 * write exactly the rows of one mw_median over the whole slide, bit for bit;
 * mw_median / mw_median_generic are the one-band case (row_off 0, slide_H =
 * H, rows [0, H)) of the same kernel.  force_generic != 0: the rank search
 * for every size.  Every other argument and error as mw_median. */
int mw_median_rows(const void* d_img, int dtype, int H, int W, int C,
                   int64_t row_off, int64_t slide_H, int r0, int r1,
                   int size_y, int size_x, int force_generic,
                   const float* d_inv_mean, float pseudoval,
                   void* d_out, void* stream);

/* ---- img.blurring('bilateral', sigma, sigma_color=v) (MxIF.py:406-410) -------
 * Bilateral filter over all channels jointly.  a = the image as fp32: the
 * element itself, or mw_lognorm's value of it when d_inv_mean != NULL (the
 * log-normalise fused into the load).  For output pixel (y, x) and every tap
 * (dy, dx) in [-radius, radius]^2, q = a[y + dy, x + dx, :]; outside the image
 * q is cval in every channel (mode 0, 'constant') or the pixel at the clamped
 * coordinates (mode 1, 'edge');
 *   w = exp(-(dy^2 + dx^2) / (2 sigma_spatial^2) - |q - a[y, x, :]|^2 / (2 sigma_color^2)),
 *   d_out[y, x, c] = sum w q[c] / sum w          (fp32; the centre tap has w = 1).
 * This is skimage's documented denoise_bilateral without its colour look-up
 * table, its shift of negative images and its release-specific index quirks
 * (DESIGN.md §17).  The spatial factor comes from a table made in fp64, the
 * colour factor and the sums are fp32.  NaN input is undefined.  The kernel
 * filters every image; returning a constant image unchanged is the caller's
 * rule (milwrm_amd.device.bilateral, from mw_image_moments' min and max).
 * radius 0..12 and C <= 64 (beyond either: MW_EUNSUPPORTED, nothing launched);
 * sigma_spatial or sigma_color not positive and finite, radius < 0, a mode
 * other than 0 / 1, cval not finite or d_out == d_img: MW_EINVAL.  No
 * workspace. */
int mw_bilateral(const void* d_img, int dtype, int H, int W, int C, int radius,
                 double sigma_spatial, double sigma_color, int mode, float cval,
                 const float* d_inv_mean, float pseudoval, float* d_out, void* stream);
/* The row-window form (a slide streamed in row bands, milwrm_amd.stream):
 * d_img holds the H rows [row_off, row_off + H) of a slide of slide_H rows;
 * only the array's rows [r0, r1) are filtered, into a compact fp32 d_out of
 * (r1 - r0) x W x C.  A tap row is inside or outside relative to the SLIDE:
 * mode 0 takes cval for a tap row outside [0, slide_H), mode 1 clamps tap rows
 * to [0, slide_H - 1]; columns as mw_bilateral.  The array must hold every
 * in-slide tap row of every requested output row: r0 >= radius when row_off >
 * 0, and H - r1 >= radius when row_off + H < slide_H; otherwise MW_EINVAL, as
 * for rows outside the slide or r0 >= r1 (nothing launched, d_out untouched).
 * Rows outside [r0, r1) are read, never computed or written, and no address
 * outside the array is formed.  A pixel's taps are summed in one order
 * whichever tile or band computes it: calls over bands that tile a slide
 * write exactly the rows of one mw_bilateral over the whole slide, bit for
 * bit; mw_bilateral is the one-band case (row_off 0, slide_H = H, rows
 * [0, H)) of the same kernel.  Every other argument and error as
 * mw_bilateral. */
int mw_bilateral_rows(const void* d_img, int dtype, int H, int W, int C,
                      int64_t row_off, int64_t slide_H, int r0, int r1, int radius,
                      double sigma_spatial, double sigma_color, int mode, float cval,
                      const float* d_inv_mean, float pseudoval, float* d_out, void* stream);
/* d_out (device, 5 doubles): the element count n_pix * C, the mean, the
 * centred second moment sum (a - mean)^2, the minimum and the maximum of the
 * image a (the load transform of mw_bilateral), in fp64 by two passes (the
 * sum, then the squared deviations) over fixed reduction trees: deterministic,
 * and sqrt(d_out[2] / d_out[0]) is numpy's a.astype(float64).std() to about
 * 1e-15 relative.  d_ws: mw_image_moments_ws_bytes() bytes. */
size_t mw_image_moments_ws_bytes(void);
int mw_image_moments(const void* d_img, int dtype, int64_t n_pix, int C,
                     const float* d_inv_mean, float pseudoval, double* d_out,
                     void* d_ws, void* stream);
/* The same five numbers of a slide that arrives in row bands, with bits that
 * do not depend on the bands (they differ from mw_image_moments' in the
 * summation order only).  d_ws: mw_image_moments_rows_ws_bytes(slide_H)
 * bytes, a table with one entry per slide row, kept by the caller from the
 * first call to the last.  mw_image_moments_rows reduces each of the H rows
 * [row_off, row_off + H) held by d_img with one workgroup into its entry:
 * pass 0 the row's sum, minimum and maximum; pass 1 its sum (a - mean)^2, mean
 * as the last mw_image_moments_rows_final left it.  Once every slide row has
 * been through a pass, mw_image_moments_rows_final reduces the table by a
 * fixed tree into d_out and keeps the mean in d_ws: with_m2 == 0 after pass 0
 * (d_out[2] is NaN), != 0 after pass 1.  So: pass 0 over all bands, final(0),
 * and for the second moment pass 1 over all bands, final(1).  Rows that are
 * not rows of the slide, a pass other than 0 / 1: MW_EINVAL. */
size_t mw_image_moments_rows_ws_bytes(int64_t slide_H);
int mw_image_moments_rows(const void* d_img, int dtype, int H, int W, int C,
                          int64_t row_off, int64_t slide_H, int pass,
                          const float* d_inv_mean, float pseudoval, void* d_ws, void* stream);
int mw_image_moments_rows_final(int64_t slide_H, int W, int C, int with_m2,
                                void* d_ws, double* d_out, void* stream);

/* ---- img.blurring('gaussian', sigma) (MxIF.py:375-394) ----------------------
 * Separable Gaussian, per channel, edge-replicate ('nearest'), radius r =
 * int(4*sigma+0.5) <= 32, taps h_w[0..2r] (scipy _gaussian_kernel1d).
 * Optional fused log-normalise prologue when d_inv_mean != NULL.  HWC in,
 * HWC fp32 out (out must not alias in).  Even C and r <= 12: single
 * streaming pass (register ring); otherwise two passes through d_ws
 * (mw_blur_ws_bytes). */
size_t mw_blur_ws_bytes(int H, int W, int C, int radius);
int mw_blur(const void* d_img, int dtype, int H, int W, int C,
            const float* d_inv_mean, float pseudoval,
            const float* h_w, int radius, float* d_out, void* d_ws, void* stream);

/* The blur in two parts: first the rows the labelling path can read, the rest
 * only if something else reads the image (no reference counterpart).  A pixel
 * is needed when its 64-aligned flat tile (p >> 6, p = y W + x) holds a mask
 * pixel: the tiles mw_assign_conf loads, which cover the pixels a gather over
 * the mask reads.  mw_blur_rows_table writes, per workgroup tile of the
 * matrix-core kernel (mw_blur_rows_tiles(H, W) of them, 64 columns x 512 rows,
 * column band fastest), the hull [a, b) of its output rows that hold a needed
 * pixel into d_table[2 t], d_table[2 t + 1] (a = b: none); d_mask is H x W
 * bytes, nonzero = tissue.  mw_blur_part blurs, with mw_blur's arguments, the
 * rows of the hulls (part 1) or the rows outside them (part 2) and leaves the
 * other rows of d_out untouched: part 1 then part 2 write mw_blur's d_out, bit
 * for bit.  MW_EUNSUPPORTED, nothing launched, for shapes the matrix-core
 * kernel does not take (odd C, C > 64, radius > 8, MW_BLUR_IMPL=v): those are
 * blurred whole by mw_blur.  The table stays on the device. */
int mw_blur_rows_tiles(int H, int W);
int mw_blur_rows_table(const uint8_t* d_mask, int H, int W, int32_t* d_table, void* stream);
int mw_blur_part(const void* d_img, int dtype, int H, int W, int C,
                 const float* d_inv_mean, float pseudoval, const float* h_w, int radius,
                 float* d_out, const int32_t* d_table, int part, void* stream);

/* ---- img.downsample(fact, np.mean) (MxIF.py:494-517) ------------------------
 * block mean over fact x fact, zero padded to a multiple of fact, pad zeros
 * included.  HWC in, fp32 HWC out of ceil(H/f) x ceil(W/f) x C. */
int mw_block_mean(const void* d_img, int dtype, int H, int W, int C, int fact,
                  float* d_out, void* stream);

/* ---- img.downsample(fact, func) on a slide or a row band of it --------------
 * skimage block_reduce(x, (fact, fact, 1), func, cval=0): the pad (zeros below
 * the slide's last row and right of its last column) takes part in every func.
 * d_rows holds the slide's rows [row0, row0 + rows), HWC; d_out is the whole
 * ceil(slide_H / fact) x ceil(W / fact) x C fp32 result, of which the call
 * writes the output rows from row0 / fact on.  row0 must be a multiple of
 * fact, and so must rows unless the band ends at slide_H (MW_EINVAL
 * otherwise); a resident slide is the one-band case.  Every output value is
 * computed from its own block in one order, so the result has the same bits
 * whatever the band split: mean and sum in fp64, block rows top to bottom and
 * within a row left to right, rounded once (mean: the bits of the block-mean
 * entry above); max and min exact, a NaN in the block gives NaN; median the
 * exact middle order statistic, an even count the fp64 average of the middle
 * two, any NaN gives NaN, fact <= 16 (MW_EUNSUPPORTED above, nothing
 * launched). */
#define MW_REDUCE_MEAN 0
#define MW_REDUCE_SUM 1
#define MW_REDUCE_MAX 2
#define MW_REDUCE_MIN 3
#define MW_REDUCE_MEDIAN 4
int mw_block_reduce_rows(const void* d_rows, int dtype, int rows, int W, int C,
                         int row0, int slide_H, int fact, int func,
                         float* d_out, void* stream);

/* ---- mask row-major rank → pixel (MxIF.py:486-488) --------------------------
 * d_rank2pix[r] = flat index of the r-th pixel with mask != 0.  d_count gets
 * the number of such pixels (int64 on device). */
size_t mw_mask_rank_ws_bytes(int64_t n_pix);
int mw_mask_rank(const uint8_t* d_mask, int64_t n_pix, uint32_t* d_rank2pix,
                 int64_t* d_count, void* d_ws, void* stream);

/* The same rank as a compact index (img.subsample_pixels' mask gather,
 * MxIF.py:486-488, without a rank -> pixel table): per 64-pixel word its mask
 * bits and the tissue pixels before it, per 64 ranks the word holding the
 * first: mw_rank_index_bytes(n_pix) bytes (~n_pix / 6), d_count = M.  The *_ri
 * forms below look a rank up in it (+ pix_off: the index of a slide band
 * inside a larger array) -- the random lookups of a subsample then stay in
 * the on-die caches instead of reading an HBM line per draw. */
size_t mw_rank_index_bytes(int64_t n_pix);
int mw_mask_rank_index(const uint8_t* d_mask, int64_t n_pix, void* d_index, int64_t* d_count, void* d_ws,
                       void* stream);

/* ---- subsample gather (MxIF.py:490-491) -------------------------------------
 * X[j, f] = img[rank2pix[idx[j]], feat[f]] as fp32 rows (S x F), plus per
 * block column statistics (count, mean, M2 in fp64) for StandardScaler.
 * d_img is fp32 HWC with C channels. */
size_t mw_gather_ws_bytes(int64_t S, int F);
int mw_gather_rows(const float* d_img, int C, const int32_t* d_feat, int F,
                   const int32_t* d_idx, const uint32_t* d_rank2pix, int64_t S,
                   float* d_X, void* d_ws, void* stream);
int mw_gather_rows_ri(const float* d_img, int C, const int32_t* d_feat, int F, const int32_t* d_idx,
                      const void* d_index, int64_t n_pix, int64_t pix_off, int64_t S, float* d_X, void* d_ws,
                      void* stream);
/* The draws as pixels: d_idx[j] = pixel of rank d_idx[j] (+ pix_off) through
 * the rank index, in place -- a pass over the draws that keeps the random
 * lookups in the on-die caches (it runs beside the blur); then
 * mw_gather_rows_px reads X[j, f] = img[d_pix[j], feat[f]] with no lookup.
 * Same rows and records as mw_gather_rows over the same draws. */
int mw_rank_to_pixel_ri(int32_t* d_idx, int64_t S, const void* d_index, int64_t n_pix, int64_t pix_off,
                        void* stream);
int mw_gather_rows_px(const float* d_img, int C, const int32_t* d_feat, int F, const int32_t* d_pix, int64_t S,
                      float* d_X, void* d_ws, void* stream);
/* Column statistics of rows already in X (same per-block records as
 * mw_gather_rows, same order: identical numbers for identical rows); then
 * mw_col_stats_finalize. */
int mw_col_stats_rows(const float* d_X, int64_t S, int F, void* d_ws, void* stream);

/* ---- fused blur + subsample (MxIF.py:375-394 + 457-492, MILWRM.py:1716-1733)
 * The subsample rows are written by the blur itself, so the blurred slide is
 * never stored:
 *   mw_sample_map:      slots[2p], slots[2p+1] = the first two sample slots j
 *                       of pixel p (rank2pix[idx[j]] == p; -1 where absent;
 *                       d_slots holds mw_sample_slot_elems(n_pix) int32), the
 *                       later slots of p on the overflow list d_ovf (S + 1
 *                       int32: [0] = count, then the slots);
 *   mw_blur_sample:     lognorm + blur of the slide; X[j, f] = blurred[p,
 *                       feat[f]] for both table slots j of every sampled p;
 *   mw_sample_overflow: X[j] = X[slots[2p]] for the overflow slots;
 * then mw_col_stats_rows.  X ends up equal to mw_blur + mw_gather_rows.
 * mw_blur_sample returns MW_EUNSUPPORTED (nothing launched) for shapes the
 * fused kernel does not take (odd C, C > 64, radius 0 or > 8, F > C rounded
 * up to 16, no log-normalise); the caller then materialises the blur. */
size_t mw_sample_slot_elems(int64_t n_pix);
int mw_sample_map(const int32_t* d_idx, const uint32_t* d_rank2pix, int64_t S, int64_t n_pix,
                  int32_t* d_slots, int32_t* d_ovf, void* stream);
int mw_blur_sample(const void* d_img, int dtype, int H, int W, int C, const float* d_inv_mean,
                   float pseudoval, const float* h_weights, int radius, const int32_t* d_slots,
                   int64_t S, const int32_t* d_feat, int F, float* d_X, void* stream);
int mw_sample_overflow(const int32_t* d_idx, const uint32_t* d_rank2pix, const int32_t* d_slots,
                       const int32_t* d_ovf, int64_t S, int F, float* d_X, void* stream);
int mw_sample_map_ri(const int32_t* d_idx, const void* d_index, int64_t n_index, int64_t pix_off, int64_t S,
                     int64_t n_pix, int32_t* d_slots, int32_t* d_ovf, void* stream);
int mw_sample_overflow_ri(const int32_t* d_idx, const void* d_index, int64_t n_index, int64_t pix_off,
                          const int32_t* d_slots, const int32_t* d_ovf, int64_t S, int F, float* d_X,
                          void* stream);
/* Row-window form for a slide streamed in row bands (img.subsample_pixels over a
 * slide that is not resident in HBM, MxIF.py:457-492): d_img holds the H rows
 * [row_off, row_off + H) of the slide (a band and its +-radius halo rows);
 * only its rows [r0, r1) are blurred into samples, d_slots is the whole
 * slide's table (indexed by slide pixel).  Calling it for bands that tile the
 * slide writes exactly the rows of one mw_blur_sample over the whole slide. */
int mw_blur_sample_rows(const void* d_img, int dtype, int H, int W, int C, int64_t row_off, int r0, int r1,
                        const float* d_inv_mean, float pseudoval, const float* h_weights, int radius,
                        const int32_t* d_slots, int64_t S, const int32_t* d_feat, int F, float* d_X,
                        void* stream);
/* The same rows from a band already blurred into fp32 (any shape the fused
 * kernel does not take): d_band = n_pix HWC fp32 pixels, slide pixels
 * [pix_off, pix_off + n_pix); X[j] = band[p - pix_off, feat] for both table
 * slots j of every sampled pixel p of the band. */
int mw_slot_gather(const float* d_band, int C, int64_t n_pix, int64_t pix_off, const int32_t* d_slots,
                   int64_t S, const int32_t* d_feat, int F, float* d_X, void* stream);

/* Chan-merge the per-block stats of the last gather(s) into d_stats =
 * [n, mean[F], M2[F]] (fp64).  `n_parts` gathers may be accumulated: pass
 * the workspace of each; merged in call order. */
int mw_col_stats_finalize(const void* d_ws, int64_t S, int F, double* d_stats,
                          int accumulate, void* stream);
/* Column max |x| of the same rows (fp32 d_out[F]; maxed into d_out when
 * accumulating): the fixed-point exponents of mw_lloyd_pass come from it
 * (replaces a separate mw_col_absmax pass over the rows). */
int mw_col_stats_absmax(const void* d_ws, int64_t S, int F, float* d_out, int accumulate,
                        void* stream);

/* ---- legacy MT19937 subsample indices (MxIF.py:484,490) ---------------------
 * Bit-exact np.random.RandomState(seed).randint(0, high, size) (== choice),
 * masked rejection on MT19937.  Host implementation (single thread). */
int mw_legacy_randint_host(uint32_t seed, int64_t high, int64_t size, int32_t* h_out);

/* ---- device MT19937 with jump-ahead (bit-exact legacy randint) -------------
 * One-time host tables: h_j(t) = t^(L*2^j) mod phi(t), j < J (312 uint64 per
 * polynomial; phi = characteristic polynomial of the MT19937 transition,
 * found by Berlekamp-Massey).  The device builds the start state of every
 * L-word segment by a parallel prefix of jumps (block Horner), then every
 * workgroup regenerates, tempers and filters its segment; accepted draws are
 * compacted in stream order.  Output identical to mw_legacy_randint_host. */
int mw_mt_jump_tables(int64_t L, int J, uint64_t* h_tables);
int mw_mt_jump_host(const uint32_t* h_state_in, const uint64_t* h_poly, uint32_t* h_state_out);
int mw_mt_seed_state(uint32_t seed, uint32_t* h_state);
size_t mw_legacy_randint_ws_bytes(int64_t high, int64_t size, int64_t L);
int mw_legacy_randint_device(uint32_t seed, int64_t high, int64_t size, const uint64_t* d_tables,
                             int J, int64_t L, int32_t* d_out, int64_t* d_total, void* d_ws,
                             void* stream);
/* The same in two halves.  The segment start states depend only on (seed, L):
 * every image of a batch reseeds with 16 (MxIF.py:484), so a caller may build
 * them once (mw_mt_segment_states, W x 624 uint32 in d_states) and draw any
 * (high, size) needing at most W segments from them
 * (mw_legacy_randint_from_states; workspace mw_legacy_randint_gen_ws_bytes). */
int64_t mw_legacy_randint_segments(int64_t high, int64_t size, int64_t L);
int mw_mt_segment_states(uint32_t seed, int64_t W, const uint64_t* d_tables, int J,
                         uint32_t* d_states, void* stream);
size_t mw_legacy_randint_gen_ws_bytes(int64_t high, int64_t size, int64_t L);
int mw_legacy_randint_from_states(const uint32_t* d_states, int64_t W_avail, int64_t high,
                                  int64_t size, int64_t L, int32_t* d_out, int64_t* d_total,
                                  void* d_ws, void* stream);

/* ---- k-means++ (sklearn _kmeans.py:174-272) ---------------------------------
 * Rows are scaled on the fly: x' = (x - mu) * inv_sigma  (fp64 affine).
 * The workspace keeps the closest distance of every row (fp64) and per-block
 * / per-64-row-tile sums of the step's T trial arrays (the arrays themselves
 * are recomputed where the search needs them, never stored).
 * Single device: mw_kpp_init + (k-1) x mw_kpp_step + mw_kpp_indices keep all
 * state on the device (no host synchronisation between steps).
 * Row-sharded (one shard per rank): mw_kpp_init, then per step c
 * mw_kpp_pots → (host all-gather, global argmin, targets) → mw_kpp_search
 * with explicit local targets → (host all-reduce of candidate rows) →
 * mw_kpp_trial. */
size_t mw_kpp_ws_bytes(int64_t S, int T);
/* distances to one center row (raw fp32 features, device) */
int mw_kpp_init(const float* d_X, int64_t S, int F, const double* d_mu,
                const double* d_inv, const float* d_center_row, int T, void* d_ws,
                void* stream);
/* mw_kpp_init and step 1 (mw_kpp_step with c = 1, draws h_u[T]) without the
 * init's pass over the rows, for rows whose producer left per-block moment
 * records (mw_gather_rows* / mw_col_stats_rows: [n, mean[F], M2[F], max|x|[F]]
 * fp64 per block of rows_per_block consecutive rows; mw_rows_per_block).  X is
 * n_seg <= 16 segments in row order (one per gathered image), h_segs a host
 * array; each segment's records stay valid until the stream has run the call.
 * The sum of d(x, c0) over a block comes from its record, step 1's targets are
 * located in the scan of those sums and only the located blocks' rows are read;
 * step 1's pass takes cur = d(x, c0) from the row it holds.  The workspace
 * after the call (cur, block and tile sums, candidates) is bit for bit what
 * mw_kpp_init followed by mw_kpp_step(c = 1) leave when both locate the same
 * candidate rows; the record sums differ from the summed distances by
 * rounding, so a target within that rounding of a block boundary may land on
 * the neighbouring row.  Go on with mw_kpp_step for c = 2.. and
 * mw_kpp_indices. */
typedef struct mw_kpp_seg {
  int64_t row_start;       /* first row of the segment in X */
  int64_t n_rows;
  int64_t rows_per_block;  /* rows per record (the last block may be short) */
  const double* d_records; /* ceil(n_rows / rows_per_block) records of 1 + 3 F fp64 (device) */
} mw_kpp_seg;
int mw_kpp_init_moments(const float* d_X, int64_t S, int F, const double* d_mu, const double* d_inv,
                        const float* d_center_row, const double* h_u, int T, int n_seg,
                        const mw_kpp_seg* h_segs, void* d_ws, void* stream);
/* byte offsets of the workspace's sections and its grid, for tests: out[7] =
 * cur, block sums, tile sums, moment block sums (then their scan), blocks,
 * tiles, capacity in moment blocks */
void mw_kpp_ws_sections(int64_t S, int T, int64_t* out);
/* single-device step for center c (1..k-1); h_u = the T uniform draws */
int mw_kpp_step(const float* d_X, int64_t S, int F, const double* d_mu,
                const double* d_inv, int c, const double* h_u, int T,
                void* d_ws, void* stream);
/* single-device: chosen indices (int64 [k]) into d_idx_out */
int mw_kpp_indices(const void* d_ws, int64_t S, int T, int k, int64_t* d_idx_out,
                   void* stream);
/* single-device last step (c = k-1 >= 2, mw_kpp_fold_supported) with the
 * first Lloyd E-step folded into its pass (opt-in: MW_KPP_FOLD=1; no
 * reference counterpart: it replaces the pass over the rows that sklearn's
 * first lloyd_iter_chunked_dense makes after _kmeans_plusplus, _kmeans.py:
 * 624-752): besides the step's trial sums, every row gets its label among the
 * k-1 centers so far (labels), distance bounds valid whichever candidate wins
 * (ub, lb), the bits "moves to the new center if candidate t wins" (moved,
 * S bytes) and the base cluster sums as Lloyd block records (d_rec,
 * mw_kpp_fold_rec_bytes) folded into d_rec_out (mw_lloyd_rec_len(k, F) fp64).
 * first = the first center's row; d_a32 / d_b32 / d_qexp as mw_lloyd_pass;
 * d_centers_img = 8 KB of device scratch.  After mw_kpp_indices, the winner's
 * moved rows are listed (mw_lloyd_list_moved) and a mode-0 mw_lloyd_pass of
 * kind 8 over the k final centers moves them: its record plus d_rec_out's
 * sums and counts are those of a kind-0 first pass, bit for bit. */
int mw_kpp_step_fold(const float* d_X, int64_t S, int F, const double* d_mu, const double* d_inv, int c,
                     const double* h_u, int T, void* d_ws, int64_t first, const float* d_a32,
                     const float* d_b32, const int32_t* d_qexp, uint8_t* d_labels, float* d_ub, float* d_lb,
                     uint8_t* d_moved, void* d_centers_img, double* d_rec, double* d_rec_out, void* stream);
size_t mw_kpp_fold_rec_bytes(int64_t S, int k, int F);
/* 1 when mw_kpp_step_fold takes (k, F, T): 3 <= k <= 16, T <= 4, F <= 32 and
 * its LDS fits two blocks per CU */
int mw_kpp_fold_supported(int k, int F, int T);
/* device address of the k-means++ workspace's selected-array index (int) */
const int* mw_kpp_best_ptr(const void* d_ws, int64_t S, int T);
/* sharded: local potentials (fp64) of the arrays finished before step c
 * (1 array after init, T after a trial) */
int mw_kpp_pots(const void* d_ws, int64_t S, int T, int c, double* d_pots, void* stream);
/* sharded: search array `best` of step c-1 (recomputed from the rows where
 * needed) for local targets d_rv[T] (fp64, < 0 = not on this shard); local
 * row indices (int64, -1 if skipped) */
int mw_kpp_search(const float* d_X, int64_t S, int F, void* d_ws, int T, int c, int best,
                  const double* d_rv, int64_t* d_local_idx, void* stream);
/* sharded: pass of step c against candidate rows d_rows (T x F raw fp32),
 * after folding in array `best` of step c-1 */
int mw_kpp_trial(const float* d_X, int64_t S, int F, const double* d_mu,
                 const double* d_inv, int c, int best, const float* d_rows, int T,
                 void* d_ws, void* stream);

/* ---- Lloyd iteration (sklearn lloyd_iter_chunked_dense, _k_means_lloyd.pyx:23-218;
 *      _inertia_dense, _k_means_common.pyx:94-124) -----------------------------
 * One pass over S rows for n independent fits (n = 1 for KMeans.fit, all k of
 * the find_optimal_k sweep, MILWRM.py:29-90, batched).  Rows x' = x*a[f] +
 * b[f] (fp32, the folded StandardScaler); labels = argmin of the direct
 * squared distance, lowest index on ties.  Per fit the caller owns:
 *   centers   k x F fp32 (scaled space)
 *   labels    S uint8 (255 = none yet; k <= 64)
 *   ub, lb    S fp32 distance bounds (mode 0; contents ignored where label = 255)
 *   drift     k fp32 |c_j - c_j(previous pass)|, rounded up (0 on the first pass)
 *   half_sep  k fp32 0.5 * min_{i != j} |c_i - c_j|, rounded down (+inf for k = 1)
 *   drift_max max_j drift[j]
 *   ws        mw_lloyd_ws_bytes(S, k, F) bytes of per-block records and row lists
 *             (mw_lloyd_ws_bytes_kinds(S, k, F, 0): records only, no kind 4)
 *   out       mw_lloyd_rec_len(k, F) fp64, the fixed-order fold of the records:
 *             [dQ_hi k*F | dQ_lo k*F | dcount k | changed | recomputed | in_hi | in_lo]
 *             (mode 0: in_hi * 2^32 + in_lo = the rows whose features the pass
 *             read -- all of them for kinds 0 / 1, the queued or listed ones
 *             for kinds 2 / 4; 0 for the dense kinds)
 * mode 0: E-step (rows whose bounds prove the label skip the distances) and
 *         the M-step change of the per-cluster sums: every raw value rounds
 *         once to q = rint(x * 2^qexp[f]) (|q| < 2^41) and a relabelled row
 *         moves its q from the old cluster to the new one; dQ = dQ_hi * 2^32 +
 *         dQ_lo (exact integers), dcount the change of the cluster sizes.
 * mode 1: full E-step (labels updated) and inertia = (in_hi * 2^32 + in_lo) *
 *         2^-inertia_exp of the new labels (each distance rounded once to that
 *         fixed point);  mode 2: inertia of the given labels.
 * Every sum is an integer sum: identical for any row order or sharding.
 * `kind` (mode 0): 0 = first pass (every label 255: sums of all rows on the
 * fp64 matrix cores), 1 = stream every row, the bounds skip the E-step per
 * row (most rows undecided), 2 = stream the row state only and read just the
 * undecided rows (few undecided), chunk by chunk in one kernel, 4 = the same
 * as two kernels: the bound test over the whole row state lists the undecided
 * rows, then a second launch reads only those (falls back to 2 when S >= 2^31;
 * ws then also holds the lists).  Same results for any kind.
 * k <= 64, F <= 64, n <= 24.  h_fits is a host array. */
typedef struct mw_lloyd_fit {
  const float* centers;
  const float* drift;
  const float* half_sep;
  uint8_t* labels;
  float* ub;
  float* lb;
  void* ws;
  double* out;
  int k;
  float drift_max;
  int inertia_exp;  /* modes 1 / 2: inertia fixed point 2^-inertia_exp */
} mw_lloyd_fit;
int mw_lloyd_rec_len(int k, int F);
size_t mw_lloyd_ws_bytes(int64_t S, int k, int F);
/* The workspace without the kList row lists (4 bytes per row) when with_list
 * is 0 or S >= 2^31 (kind 4 falls back to kind 2 there): a fit whose passes
 * never take kind 4 (MW_LLOYD_LIST=0) needs only its per-block records. */
size_t mw_lloyd_ws_bytes_kinds(int64_t S, int k, int F, int with_list);
/* kind 8 = kind 4 over row lists written beforehand into ws: the rows of
 * d_moved (mw_kpp_step_fold) whose bit *d_best is set (S < 2^31) */
int mw_lloyd_list_moved(const uint8_t* d_moved, const int* d_best, int64_t S, int F, int k, void* d_ws,
                        void* stream);
int mw_lloyd_pass(const float* d_X, int64_t S, int F, const float* d_a, const float* d_b,
                  const int32_t* d_qexp, int n, const mw_lloyd_fit* h_fits, int mode, int kind,
                  void* stream);
/* per-column max |x| of S x F fp32 rows (F <= 16384), fp32 out */
int mw_col_absmax(const float* d_X, int64_t S, int F, float* d_out, void* stream);
/* The same maxima folded into d_out (fp32 [F], >= 0) without resetting it:
 * the column maxima of a slide processed band after band. */
int mw_col_absmax_acc(const float* d_X, int64_t S, int F, float* d_out, void* stream);

/* Per pass of the calling thread's last mw_kmeans_fit / mw_kmeans_fit_async
 * (k-means++ passes excluded): 4 int64 each -- kind (0..8; 10 + mode for the
 * final pass), rows relabelled, rows recomputed, rows whose features the pass
 * read -- up to cap passes into out; returns the number of passes.  For the
 * measurement of the bytes a pruned fit really reads (bench.py). */
int mw_kmeans_fit_history(int64_t* out, int cap);

/* ---- whole fit: sklearn KMeans(algorithm="lloyd").fit (_kmeans.py:1427-1554)
 * Replaces the reference's `KMeans(n_clusters=k, random_state=seed).fit(X)`
 * (MILWRM.py:706-737 find_tissue_regions; MILWRM.py:29-54 kMeansRes) for a
 * caller of the C ABI; KMeans.fit of the Python package runs through it too
 * (single process, one k-means++ init from an int seed or an explicit init).
 * Rows: S x F raw fp32 on the device, scaled on the fly x' = (x - mu) * inv
 * (fp64 host arrays; mu = 0, inv = 1 for rows that are already standardised).
 * k-means++ seeded from RandomState(seed) (or the k x F scaled centers
 * h_init, then no seeding), Lloyd with sklearn's strict and tolerance
 * convergence (tol relative: tol * mean of the scaled rows' per-feature
 * variance, from h_feature_var[F] when given, else computed on the device),
 * empty-cluster relocation, the extra E-step and inertia.  h_xmax[F]: the
 * rows' column max |x| when the producer already has it (else one pass).
 * Outputs: d_labels (S uint8, device), h_centers (k x F fp64, scaled space),
 * *h_inertia, *h_n_iter, h_init_idx (k int64, may be NULL; untouched with
 * h_init).  d_ws: mw_kmeans_fit_ws_bytes(S, F, k) bytes of device workspace
 * (NULL: allocated and freed inside).  Caps: 1 <= k <= 64 (uint8 labels,
 * centers in LDS / scalar registers), 1 <= F <= 64 (one feature per lane of
 * a wave); S >= k.  Synchronises `stream` before returning. */
size_t mw_kmeans_fit_ws_bytes(int64_t S, int F, int k);
int mw_kmeans_fit(const float* d_X, int64_t S, int F, const double* h_mu,
                  const double* h_inv, const double* h_feature_var, const float* h_xmax,
                  int k, const double* h_init, uint32_t seed, int max_iter, double tol,
                  uint8_t* d_labels, double* h_centers, double* h_inertia, int* h_n_iter,
                  int64_t* h_init_idx, void* d_ws, size_t ws_bytes, void* stream);
/* The same fit with an asynchronous end: returns once the final E-step
 * (labels, inertia) is queued on `stream`, so the caller can queue the label
 * pass behind it without a host round trip (the centers, n_iter and k-means++
 * indices are final at return; d_labels is stream-ordered).  The final pass's
 * record (mw_lloyd_rec_len(k, F) fp64) is copied to the caller's PAGE-LOCKED
 * h_final_rec when the stream gets there; after synchronising the stream the
 * inertia is (rec[rl - 2] * 2^32 + rec[rl - 1]) * 2^-(*h_inertia_exp).  A
 * d_ws of NULL (workspace allocated inside) makes the end synchronous, with
 * the same outputs. */
int mw_kmeans_fit_async(const float* d_X, int64_t S, int F, const double* h_mu,
                        const double* h_inv, const double* h_feature_var, const float* h_xmax,
                        int k, const double* h_init, uint32_t seed, int max_iter, double tol,
                        uint8_t* d_labels, double* h_centers, int* h_n_iter, int64_t* h_init_idx,
                        void* d_ws, size_t ws_bytes, double* h_final_rec, int* h_inertia_exp,
                        void* stream);
/* mw_kmeans_fit_async for rows that come with their producer's moment records
 * (h_segs[n_seg], see mw_kpp_init_moments): a k-means++ seeding of k >= 2
 * centers then starts with mw_kpp_init_moments instead of the init pass; the
 * same indices, centers, labels and inertia.  n_seg = 0: mw_kmeans_fit_async. */
int mw_kmeans_fit_async_moments(const float* d_X, int64_t S, int F, const double* h_mu,
                                const double* h_inv, const double* h_feature_var, const float* h_xmax,
                                int k, const double* h_init, uint32_t seed, int max_iter, double tol,
                                uint8_t* d_labels, double* h_centers, int* h_n_iter, int64_t* h_init_idx,
                                void* d_ws, size_t ws_bytes, double* h_final_rec, int* h_inertia_exp,
                                int n_seg, const mw_kpp_seg* h_segs, void* stream);
/* mw_kmeans_fit_async_moments without the final pass: everything up to and
 * including the last Lloyd iteration.  h_centers, *h_n_iter and h_init_idx
 * are final at return and *h_strict says whether the fit converged strictly
 * (no label changed in its last iteration); `stream` is synchronised.
 * d_labels then holds the LAST ITERATION's labels: sklearn's labels_ only when
 * *h_strict is 1.  The labels under the final centers and the inertia are
 * mw_kmeans_fit_finish's, whenever (and if) the caller wants them; a caller
 * that needs only the centers (the label pass over the slides) never pays
 * that pass over the rows.  mw_kmeans_fit_history lists what the fit read: no
 * final-pass entry. */
int mw_kmeans_fit_deferred(const float* d_X, int64_t S, int F, const double* h_mu,
                           const double* h_inv, const double* h_feature_var, const float* h_xmax,
                           int k, const double* h_init, uint32_t seed, int max_iter, double tol,
                           uint8_t* d_labels, double* h_centers, int* h_n_iter, int64_t* h_init_idx,
                           void* d_ws, size_t ws_bytes, int n_seg, const mw_kpp_seg* h_segs,
                           int* h_strict, void* stream);
/* The final pass of a fit that mw_kmeans_fit_deferred left out, over the same
 * rows, scaler and column maxima (h_xmax[F], required) with the fit's
 * h_centers, strict flag and d_labels: the extra E-step (strict = 0; d_labels
 * rewritten) or none (strict = 1), and the inertia.  Bit for bit the labels
 * and inertia of the eager entries.  The pass is queued on `stream` and its
 * record copied to the caller's PAGE-LOCKED h_final_rec as by
 * mw_kmeans_fit_async (inertia = (rec[rl - 2] * 2^32 + rec[rl - 1]) *
 * 2^-(*h_inertia_exp) once the stream got there).  d_ws:
 * mw_kmeans_fit_finish_ws_bytes(S, F, k) bytes of its own (required; nothing
 * of the fit's workspace is read).  The fit history is left alone.
 * MW_EINVAL before any launch: a null pointer, k or F outside [1, 64], S < k,
 * a short workspace. */
size_t mw_kmeans_fit_finish_ws_bytes(int64_t S, int F, int k);
int mw_kmeans_fit_finish(const float* d_X, int64_t S, int F, const double* h_mu, const double* h_inv,
                         const float* h_xmax, int k, const double* h_centers, int strict,
                         uint8_t* d_labels, void* d_ws, size_t ws_bytes, double* h_final_rec,
                         int* h_inertia_exp, void* stream);

/* ---- batched fits: the find_optimal_k sweep's Lloyd iterations ----------------
 * Replaces kMeansRes' per-k `KMeans(n_clusters=k, random_state=seed).fit(X)`
 * (MILWRM.py:29-54, called per k by find_optimal_k MILWRM.py:659-704) for n
 * fits over the same rows, from given k x F scaled initial centers (h_init,
 * the fits' blocks concatenated; the caller seeds them with mw_kpp_*): one
 * iteration = one mw_lloyd_pass per pass kind for every fit still running,
 * one record download; each fit returns exactly what mw_kmeans_fit returns
 * for it alone (strict / tolerance convergence, tol absolute here,
 * relocation, the extra E-step, inertia).  Rows as mw_lloyd_pass (d_a32,
 * d_b32, d_qexp on the device; h_a32, h_b32, h_qexp, the column max |x|
 * h_xmax[F] and the scaler h_mu / h_inv on the host).  Per fit g the caller
 * owns d_labels[g] (S uint8, filled with 255), d_ub[g], d_lb[g] (S fp32) and
 * d_ws[g] (mw_lloyd_ws_bytes); d_par: sum of (k F + 2k) fp32, d_out: sum of
 * mw_lloyd_rec_len(k, F) fp64.  Pass-kind policy: first_kind (0 or 3),
 * queue_kind (2 or 4) below queue_below of the rows recomputed, the dense pass
 * while >= dense_min fits run (< 0: never), nobound != 0: no bound ever holds.
 * Outputs: h_centers (the fits' k x F fp64 blocks), h_inertia[n],
 * h_n_iter[n]; h_hist (may be NULL): per fit hist_cap x (changed, recomputed)
 * int64, h_hist_len[n] entries; h_timing (may be NULL, 30 doubles): 9 x
 * (launches, ms, algorithmic bytes) of the passes by mode-0 kind 0..6, mode 1,
 * mode 2, then (host intervals, their host ms: from a pass's records arriving
 * to the next pass queued, ms inside the caller's collectives).
 * Synchronises `stream`. */
int mw_lloyd_fits(const float* d_X, int64_t S, int F, const float* d_a32, const float* d_b32,
                  const int32_t* d_qexp, const float* h_a32, const float* h_b32,
                  const int32_t* h_qexp, const float* h_xmax, const double* h_mu,
                  const double* h_inv, int n, const int* h_k, const double* h_init,
                  uint8_t* const* d_labels, float* const* d_ub, float* const* d_lb,
                  void* const* d_ws, float* d_par, double* d_out, int max_iter, double tol,
                  int first_kind, int queue_kind, double queue_below, int dense_min,
                  int nobound, double* h_centers, double* h_inertia, int* h_n_iter,
                  int64_t* h_hist, int hist_cap, int* h_hist_len, double* h_timing,
                  void* stream);

/* ---- the same fits over row shards (one process per GPU) ----------
 * Replaces the per-iteration loop of the row-sharded fit (MILWRM.py:706-737
 * find_tissue_regions, MILWRM.py:29-90 the k sweep, with the pixels of a
 * cohort split over the GPUs of a node): mw_lloyd_fits where each rank holds
 * its S rows (ranks hold consecutive row ranges, `row_offset` its first global
 * row, `rows_total` all of them) and the caller supplies the collectives.  Per
 * pass ONE in-place sum over the ranks of the fits' records (exact
 * fixed-point limbs, so the centers, labels, n_iter and inertia are bitwise
 * those of one process over all rows); a rare empty-cluster relocation adds
 * one all-gather of 2n values and one all-sum of n (F + 1) values.  Every
 * rank calls with the same n, k, init, tolerances and policy, and S >= 1.
 * The messages live in the caller's device buffer d_msg (fp64, msg_len >=
 * mw_lloyd_fits_msg_len(sum of mw_lloyd_rec_len, F, world) elements), with
 * d_out == d_msg (the records at offset 0); the callbacks address it by
 * element offsets, return 0 on success, and must order the collective after
 * the work queued on `stream` and the later work on `stream` after it (the
 * Python package binds them to torch.distributed: RCCL on the current
 * stream, or gloo through host copies; a C caller to ncclAllReduce /
 * ncclAllGather on `stream`).  A failing callback ends the call with MW_EHIP. */
typedef struct mw_fit_comm {
  void* ctx;
  int world;
  int rank;
  int64_t rows_total;
  int64_t row_offset;
  double* d_msg;
  int64_t msg_len;
  /* d_msg[off, off + n) <- its sum over the ranks */
  int (*all_reduce_sum)(void* ctx, int64_t off, int64_t n, void* stream);
  /* d_msg[out_off + r n, out_off + (r + 1) n) <- rank r's d_msg[in_off, in_off + n) */
  int (*all_gather)(void* ctx, int64_t in_off, int64_t n, int64_t out_off, void* stream);
} mw_fit_comm;
int64_t mw_lloyd_fits_msg_len(int64_t rec_total, int F, int world);
int mw_lloyd_fits_sharded(const float* d_X, int64_t S, int F, const float* d_a32, const float* d_b32,
                          const int32_t* d_qexp, const float* h_a32, const float* h_b32,
                          const int32_t* h_qexp, const float* h_xmax, const double* h_mu,
                          const double* h_inv, int n, const int* h_k, const double* h_init,
                          uint8_t* const* d_labels, float* const* d_ub, float* const* d_lb,
                          void* const* d_ws, float* d_par, double* d_out, int max_iter, double tol,
                          int first_kind, int queue_kind, double queue_below, int dense_min,
                          int nobound, double* h_centers, double* h_inertia, int* h_n_iter,
                          int64_t* h_hist, int hist_cap, int* h_hist_len, double* h_timing,
                          const mw_fit_comm* comm, void* stream);

/* ---- empty-cluster relocation support (_k_means_common.pyx:181-226) ---------
 * fp64 distance of every row to centers[labels]; returns the n largest
 * (value desc, index asc) into d_top_idx / d_top_val (n <= 64). */
size_t mw_farthest_ws_bytes(int64_t S);
int mw_farthest(const float* d_X, int64_t S, int F, const float* d_a,
                const float* d_b, const double* d_centers, int k,
                const uint8_t* d_labels, int n, int64_t* d_top_idx,
                double* d_top_val, void* d_ws, void* stream);

/* ---- label + confidence pass (MILWRM.py:237-277, 389-450) -------------------
 * Over n_pix HWC fp32 pixels (C channels, features d_feat[F]):
 * label = argmin_j ||x' - c_j||^2 (x' = x*a + b), conf = (d2 - d1)/d2;
 * mask == 0 → label -1, conf NaN.  Per-block records per label go to d_ws,
 * mw_assign_reduce folds them into d_dom (fp64 [3k]) = [conf hi k | conf lo k
 * | count k]: the per-domain sum of the confidences in exact fixed point,
 * sum of rint(conf * 2^32) = hi * 2^32 + lo, 0 <= lo < 2^32 (value = that * 2^-32; NaN limbs
 * when a confidence of the domain is NaN), and the pixel counts.  Every entry
 * is an integer-valued fp64 below 2^53, so records of several launches (row
 * bands, ranks) add exactly: the domain sums do not depend on how the pixels
 * were split (reference: MILWRM.py:447-449, np.mean per domain). */
size_t mw_assign_ws_bytes(int64_t n_pix, int k);
int mw_assign_conf(const float* d_img, int C, const int32_t* d_feat, int F,
                   const float* d_a, const float* d_b, const float* d_centers,
                   int k, const uint8_t* d_mask, int64_t n_pix,
                   int8_t* d_label, float* d_conf, void* d_ws, void* stream);
/* Fused blur + label/confidence (features = all C channels in order): the
 * same labels and confidences as mw_blur then mw_assign_conf, without the
 * blurred slide in HBM; k <= 16 (k <= 8 for C <= 16).  d_mask must be
 * readable 128 bytes past n_pix.  MW_EUNSUPPORTED (nothing launched) as for
 * mw_blur_sample.  mw_domain_records then writes mw_assign_conf's per-block
 * records from the label/confidence maps (same partition and order), for
 * mw_assign_reduce. */
int mw_blur_assign_conf(const void* d_img, int dtype, int H, int W, int C, const float* d_inv_mean,
                        float pseudoval, const float* h_weights, int radius, const float* d_a,
                        const float* d_b, const float* d_centers, int k, const uint8_t* d_mask,
                        int8_t* d_label, float* d_conf, void* stream);
/* Row-window form (a streamed slide band, as mw_blur_sample_rows): d_img
 * holds slide rows [row_off, row_off + H); rows [r0, r1) are labelled;
 * d_mask, d_label and d_conf are indexed by slide pixel. */
int mw_blur_assign_rows(const void* d_img, int dtype, int H, int W, int C, int64_t row_off, int r0, int r1,
                        const float* d_inv_mean, float pseudoval, const float* h_weights, int radius,
                        const float* d_a, const float* d_b, const float* d_centers, int k,
                        const uint8_t* d_mask, int8_t* d_label, float* d_conf, void* stream);
int mw_domain_records(const int8_t* d_label, const float* d_conf, int64_t n_pix, int C, int k,
                      void* d_ws, void* stream);
int mw_assign_reduce(const void* d_ws, int64_t n_pix, int k, double* d_dom,
                     void* stream);

/* ---- clustering QC statistics ------------------------------------------------
 * Replaces the per-domain loops of estimate_percentage_variance_mxif
 * (MILWRM.py:280-333, dc/dm sums), estimate_mse_mxif (MILWRM.py:453-515) and
 * their ST twins estimate_percentage_variance_st / estimate_mse_st
 * (MILWRM.py:518-554, 601-644; rows as a 1-pixel-wide image).
 * Over n_pix HWC fp32 pixels, x' = x[feat[f]]*a[f] + b[f], y = x' - pivot[f] (fp64).
 * Exact: every term is rounded to the two-level fixed point of its feature,
 * q = rint(v * 2^e) and r = rint((v * 2^e - q) * 2^38) (d_qexp, int32 [3F]: e
 * for (x' - c)^2 | for y | for y^2, chosen by the caller so that |q| <= 2^38),
 * and both levels are summed as integers, so the results do not depend on how
 * the pixels are split over launches (a slide blurred band by band gives the
 * materialised slide's bits) and keep ~2^-76 of the bound.
 * d_out (fp64, M = mw_domain_sse_out_len(k, F) = 4(kF + 2F) + k) =
 * [Q hi limbs | Q lo limbs | R hi limbs | R lo limbs of the NQ = kF + 2F
 * quantities: sum over label == d0+d of (x'_f - c_df)^2 (k x F), sum y_f (F),
 * sum y_f^2 (F, over every pixel)] | pixel count per label (k); with
 * Q = Qhi * 2^32 + Qlo and R likewise, value = (Q + R * 2^-38) * 2^-e.
 * accumulate != 0 adds to d_out (band after
 * band) instead of overwriting it.  Labels outside [d0, d0+k) (other
 * domains; masked / NaN tissue_ID → -1) add to the sums only.  1 <= k <= 20
 * domains per call (more: several calls with d0 = 0, 20, 40, ...), 1 <= F <=
 * 256, at most 2^24 pixels per internal block (n_pix <= ~3.4e10). */
int mw_domain_sse_out_len(int k, int F);
size_t mw_domain_sse_ws_bytes(int64_t n_pix, int k, int F);
int mw_domain_sse(const float* d_img, int C, const int32_t* d_feat, int F, const double* d_a,
                  const double* d_b, const double* d_pivot, const double* d_centers,
                  const int32_t* d_qexp, int k, int d0, const int8_t* d_label, int64_t n_pix,
                  double* d_out, int accumulate, void* d_ws, void* stream);
/* The same over fp64 rows (n_pix x C, row-major): the ST estimators'
 * cluster_data (estimate_percentage_variance_st / estimate_mse_st,
 * MILWRM.py:518-554, 601-644), which the reference holds in float64. */
int mw_domain_sse_f64(const double* d_rows, int C, const int32_t* d_feat, int F, const double* d_a,
                      const double* d_b, const double* d_pivot, const double* d_centers,
                      const int32_t* d_qexp, int k, int d0, const int8_t* d_label, int64_t n_pix,
                      double* d_out, int accumulate, void* d_ws, void* stream);

/* ---- ST feature blur (blur_features_st, ST.py:25-77) --------------------------
 * out[i, f] = mean of X[j, f] over j in (nonzero columns of row i of the CSR
 * spatial graph, in column order) + [i] (a self-loop therefore counts twice,
 * as in the reference), NaN entries skipped (pandas mean); NaN if none.
 * CSR: d_indptr (n+1, int64), d_indices (int32); X, out: n x F fp64 row-major. */
int mw_neighbor_mean(const int64_t* d_indptr, const int32_t* d_indices, int64_t n, const double* d_X,
                     int F, double* d_out, void* stream);

/* ---- synthetic slide generator (benchmark input; SURVEY §8d shape) ----------
 * uint16 HWC + uint8 mask: Voronoi domains (seeds given), per-domain channel
 * profiles, gamma-like multiplicative noise from a counter-based hash. */
int mw_synth_slide(int H, int W, int C, const float* d_seed_yx, int n_seeds,
                   const float* d_profiles, int n_domains, int shape_k,
                   int bg_rows, uint64_t seed, uint16_t* d_img, uint8_t* d_mask,
                   void* stream);
/* Rows [y0, y1) of the same H x W slide into d_img ((y1-y0) x W x C) and, when
 * d_mask != NULL, d_mask ((y1-y0) x W): bit for bit those rows of
 * mw_synth_slide (every value is a hash of its slide pixel index).  The
 * stand-in for reading a slide band from storage in the streamed benchmark. */
int mw_synth_rows(int H, int W, int C, int y0, int y1, const float* d_seed_yx, int n_seeds,
                  const float* d_profiles, int n_domains, int shape_k, int bg_rows, uint64_t seed,
                  uint16_t* d_img, uint8_t* d_mask, void* stream);

/* ---- reference-format label-pass outputs (host) ----------------------------
 * tissue_IDs[i] / confidence_IDs[i] as the reference holds them: float64 H x W
 * with NaN outside the mask (MILWRM.py:275-276, 444-445), from the compact
 * device outputs copied to host memory (int8 labels, -1 = no domain; fp32
 * confidences).  Host loops on `threads` threads (<= 1: the calling thread). */
int mw_host_labels_f64(const int8_t* h_lab, int64_t n, double* h_out, int threads);
int mw_host_f32_to_f64(const float* h_in, int64_t n, double* h_out, int threads);

#ifdef __cplusplus
}
#endif
#endif /* MILWRM_AMD_H */
