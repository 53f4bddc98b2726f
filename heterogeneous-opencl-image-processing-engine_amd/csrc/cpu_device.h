// cpu_device.h — internal: host-thread device and host helpers (see cpu_device.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "filter.h"

namespace mi_blur {

int hardware_threads();
void cpu_blur_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, int R, int y_begin, int y_end,
                   int out_row_shift);
// Rows [y_begin, y_end) with a separable kernel of any radius (the same two passes at runtime taps).
void cpu_blur_rows_sep(const uint8_t *in, uint8_t *out, int W, int H, int C, const SepTaps &k, int y_begin, int y_end,
                       int out_row_shift);
// Rows [y_begin, y_end) of the median of radius R (1..7): a sliding per-channel histogram along each row.
void cpu_median_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, int R, int y_begin, int y_end, int out_row_shift);
// Rows [y_begin, y_end) of the window minimum / maximum / gradient (mi_blur_morph_op) over (2 rx + 1) x (2 ry + 1).
void cpu_morph_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, int op, int rx, int ry, int y_begin, int y_end,
                    int out_row_shift);
// Rows [y_begin, y_end) of the bilateral filter of f (f.bil_r, f.bil_s, f.bil_range): plain integer loops, exact.
// Rows [y_begin, y_end) of the signed convolution of f (f.conv_*): plain integer loops, exact.
void cpu_conv_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int y_begin, int y_end,
                   int out_row_shift);
void cpu_bilateral_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int y_begin, int y_end,
                        int out_row_shift);
// Output rows [Y_begin, Y_end) of the decimating separable filter of f (f.taps, f.down_*): kept rows and columns only.
void cpu_sep_down_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end);
// Output rows [Y_begin, Y_end) of the resize of f (f.resize_*); xtab = resize_xtable(W, f), the x axis of every output column.
void cpu_resize_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end, const ResizeCoord *xtab);
std::vector<ResizeCoord> resize_xtable(int W, const Filter &f);
// Output rows [Y_begin, Y_end) of the area resize of f (f.out_w, f.out_h); xtab = area_xtable(W, f), ytab = area_ytable(H, f):
// area_axis of every output column / row.
void cpu_area_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end, const AreaAxis *xtab, const AreaAxis *ytab);
std::vector<AreaAxis> area_xtable(int W, const Filter &f);
std::vector<AreaAxis> area_ytable(int H, const Filter &f);
// Rows [Y_begin, Y_end) of the colour transform f.color: the output has f.color.co channels.
void cpu_color_rows(const uint8_t *in, uint8_t *out, int W, int C, const Filter &f, int Y_begin, int Y_end);
// Output rows [Y_begin, Y_end) of the affine warp of f (f.warp_*).
void cpu_warp_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end);
// Output rows [Y_begin, Y_end) of the perspective warp of f (f.warp_h).
void cpu_warp_persp_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end);
// Output rows [Y_begin, Y_end) of the remap of f (f.remap_map: host memory).
void cpu_remap_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end);
void cpu_blur_batch(const uint8_t *in, uint8_t *out, int W, int band_rows, int C, const Filter &f, int n_images,
                    int y0, int y1, int n_threads, size_t in_stride = 0, size_t out_stride = 0);
// The box blur of radius R (1|2): the form the host-only sanitizer harness (tests/san_cpu_device.cpp) drives.
inline void cpu_blur_batch(const uint8_t *in, uint8_t *out, int W, int band_rows, int C, int R, int n_images,
                           int y0, int y1, int n_threads, size_t in_stride = 0, size_t out_stride = 0)
{
    cpu_blur_batch(in, out, W, band_rows, C, Filter{FilterKind::BOX, R, {}}, n_images, y0, y1, n_threads, in_stride, out_stride);
}
// The histogram family (include/mi_blur.h, "Histogram, and tone tables made from it") on n_images dense W x H x C images;
// the callers have checked the arguments.  cpu_hist: hist = uint32[n][C][256], overwritten.  cpu_tables: image i through
// tables[i] = uint8[C][256].  cpu_tone: both with tone_tables() (filter.h) between them; work (4-byte aligned,
// n * C * 256 * 5 bytes) receives the histograms, then the tables.
void cpu_hist(const uint8_t *in, uint32_t *hist, int W, int H, int C, int n_images, int n_threads);
void cpu_tables(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const uint8_t *tables, int n_threads);
void cpu_tone(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_tone &t, void *work, int n_threads);
// CLAHE (include/mi_blur.h, "CLAHE"); the callers have checked the arguments.  cpu_clahe_tables: hist =
// uint32[n][TY][TX][C][256] and tables = uint8[n][TY][TX][C][256], both overwritten.  cpu_clahe_apply: every pixel through
// the four tables around it.  cpu_clahe: both; work (4-byte aligned) receives the histograms, then the tables.
void cpu_clahe_tables(const uint8_t *in, uint32_t *hist, uint8_t *tables, int W, int H, int C, int n_images, const mi_blur_clahe &k, int n_threads);
void cpu_clahe_apply(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_clahe &k, const uint8_t *tables, int n_threads);
void cpu_clahe(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_clahe &k, void *work, int n_threads);
// The two-image arithmetic (include/mi_blur.h, "Two-image arithmetic") on n_images dense W x H x C images; the callers
// have checked the arguments (arith_args_ok(), filter.h).  Every byte is arith_byte(); a thread reads a byte's operands
// before it writes the byte, so out may be a, or b where b has the output's extent.
void cpu_arith(const uint8_t *a, const uint8_t *b, const uint8_t *m, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_arith &k, int n_threads);
// The integral images and the box filters made from them (include/mi_blur.h, "Integral images, and box filters") on
// n_images dense W x H x C images; the callers have checked the arguments.  cpu_integral: sum and / or sqsum =
// uint32[n][H][W][C] (either may be null), rows in bands across the threads: the bands' column sums, their prefix over
// the bands of an image, then every band on its own from that carry; false when the carries cannot be allocated.
// cpu_box_from_integral: every output byte is box_byte() of box_window() (filter.h); in is read only by THRESHOLD and only
// at the byte that is written, sqsum only by STDDEV.
bool cpu_integral(const uint8_t *in, uint32_t *sum, uint32_t *sqsum, int W, int H, int C, int n_images, int n_threads);
void cpu_box_from_integral(const uint8_t *in, const uint32_t *sum, const uint32_t *sqsum, uint8_t *out, int W, int H, int C, int n_images,
                           const mi_blur_box &k, int n_threads);
// The distance transform (include/mi_blur.h, "Exact distance transform") on n_images dense W x H x C images; the callers
// have checked the arguments (dist_args_ok(), filter.h).  Exactly one of table (uint32[n][H][W][C]) and out (the byte form
// of k; it may be `in`: the column pass has read the whole input before a row is written) is given.  g, the column
// distances, is allocated here: false when that fails.  Columns in strips across the threads, then rows in bands; every
// value is dist_final() of dist_search(), every byte dist_byte() of it (filter.h).
bool cpu_dist(const uint8_t *in, uint32_t *table, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_dist &k, int n_threads);
// Template matching and the peak search (include/mi_blur.h, "Template matching and peak search"); the callers have checked
// the arguments (match_args_ok(), match_peak_args_ok(), filter.h).  cpu_match: the definition's loops, every window's
// sums made directly, output rows across the threads; a score is match_score().  cpu_match_peak: images across the threads.
void cpu_match(const uint8_t *in, const uint8_t *t, void *out, int W, int H, int C, int n_images, const mi_blur_match &k, int n_threads);
void cpu_match_peak(const void *table, int is_signed, int Wo, int Ho, int n_images, int64_t *peaks, int n_threads);
// planar (CImg storage: all of channel 0, then channel 1, ...) <-> interleaved, n_images frames, a few pool threads
void cpu_repack(const uint8_t *src, uint8_t *dst, int W, int H, int C, int n_images, bool planar_to_interleaved, int n_threads);
void copy_blocks(uint8_t *dst, size_t dst_stride, const uint8_t *src, size_t src_stride, size_t bytes, int n, int n_threads);
void fill_synthetic(uint8_t *host, int W, int H, int C, int first_index, int n_images, int n_threads);
uint64_t fnv1a64(const uint8_t *p, size_t n);

}  // namespace mi_blur
