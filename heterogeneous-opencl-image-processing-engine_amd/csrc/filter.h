// filter.h — internal: the one filter a launch, a context or a CPU run applies, in the form the GPU kernels (the .hip
// files) and the CPU device (cpu_device.cpp) take it, and the size of its output.  Plain C++, no HIP.
#pragma once

#include "../../include/mi_blur.h"

#include <limits.h>

namespace mi_blur {

constexpr int SEP_MAX_R = 16;

// A validated separable kernel (mi_blur_sep_kernel).  Taps CENTRED: wx[SEP_MAX_R + d] = weight of the pixel d columns
// away, 0 beyond the radius (likewise wy for rows), so loops unrolled over d index them with compile-time constants.
struct SepTaps {
    int rx, ry, shift;      // shift = bx + by: the one truncating shift at the end
    unsigned wx[2 * SEP_MAX_R + 1], wy[2 * SEP_MAX_R + 1];
};

enum class FilterKind { BOX, SEP, MEDIAN, MORPH, BILATERAL, CONV, SEP_DOWN, RESIZE };

// BOX: the fixed 3x3 / 5x5 kernel of `radius` 1|2.  SEP: the separable kernel `taps`.  MEDIAN: the median of `radius` 1..7.
// MORPH: the window minimum / maximum / their difference (`morph_op`) over (2 morph_rx + 1) x (2 morph_ry + 1).
// BILATERAL: the bilateral filter of radius `bil_r` with the spatial table `bil_s` (CENTRED in the 17 x 17 frame:
// bil_s[(j + 8) * 17 + (i + 8)] = S[j][i], 0 beyond the radius) and the range table `bil_range`.
// CONV: the signed 2-D convolution (mi_blur_conv) of radii `conv_rx`, `conv_ry` with the taps CENTRED in the 15 x 15 frame:
// conv_k[t][(j + 7) * 15 + (i + 7)] = K[j][i] (t = 0) or K2[j][i] (t = 1, MAG only; zeros otherwise), 0 beyond the radii.
// SEP_DOWN: the separable kernel `taps` on the whole image, of whose result only column down_ox + X * down_sx and row
// down_oy + Y * down_sy are kept (mi_blur_decimation): its output is smaller than its input.
// RESIZE: the fixed-point resize (mi_blur_resize) to resize_w x resize_h in `resize_mode`: the output may be smaller or
// larger than the input, in either axis.
struct Filter {
    FilterKind kind;
    int radius;             // BOX and MEDIAN
    SepTaps taps;           // SEP
    int morph_op = 0, morph_rx = 0, morph_ry = 0;   // MORPH (mi_blur_morph_op, radii 0..16); after taps, so {kind, radius, taps} still initialises a Filter
    int bil_r = 0;          // BILATERAL (radius 1..8)
    uint8_t bil_s[17 * 17] = {}, bil_range[256] = {};
    int conv_rx = 0, conv_ry = 0, conv_mode = 0, conv_shift = 0;   // CONV (radii 0..7, mi_blur_conv_mode, shift 0..16)
    int32_t conv_bias = 0;
    int16_t conv_k[2][15 * 15] = {};
    int down_sx = 1, down_sy = 1, down_ox = 0, down_oy = 0;   // SEP_DOWN (strides 1..4, phases below them); after the older fields, so the initialisers above stay
    int resize_w = 0, resize_h = 0, resize_mode = 0;          // RESIZE (1..MI_BLUR_RESIZE_MAX_DIM each way, mi_blur_resize_mode); last, for the same reason
};

#if defined(__HIP__)
#define MI_BLUR_HD __host__ __device__
#else
#define MI_BLUR_HD
#endif
// One axis of the resize (include/mi_blur.h, "Image resize"): output index X of n_out samples over n_in input samples,
// pixel centres aligned.  BILINEAR: the two input samples a <= b <= a + 1 and the weight f of b in 0..2048.  NEAREST:
// a = b = the input sample whose cell holds the output centre, f = 0.  The GPU kernels, the CPU device and
// mi_blur_resize_coord all come through here.  1 <= n_in, n_out <= MI_BLUR_RESIZE_MAX_DIM keeps everything in 32 bits.
struct ResizeCoord { int a, b, f; };
MI_BLUR_HD inline ResizeCoord resize_axis(int n_in, int n_out, int mode, int X)
{
    const unsigned den = 2u * (unsigned)n_out;
    ResizeCoord r;
    if (mode == MI_BLUR_RESIZE_NEAREST) {
        r.a = r.b = (int)(((unsigned)(2 * X + 1) * (unsigned)n_in) / den);
        r.f = 0;
        return r;
    }
    const int num = (2 * X + 1) * n_in - n_out;       // >= n_in - n_out > -den
    int i0;
    unsigned rem;
    if (num < 0) { i0 = -1; rem = (unsigned)(num + (int)den); }
    else { i0 = (int)((unsigned)num / den); rem = (unsigned)num - (unsigned)i0 * den; }
    r.f = (int)((rem * 2048u + (unsigned)n_out) / den);
    r.a = i0 < 0 ? 0 : i0 > n_in - 1 ? n_in - 1 : i0;
    r.b = i0 + 1 > n_in - 1 ? n_in - 1 : i0 + 1;
    return r;
}
// A resize that is valid for a W x H image of C channels: sizes 1..MI_BLUR_RESIZE_MAX_DIM both sides, a known mode, and
// input and output images inside the per-image byte limits of a launch.
inline bool resize_ok(const mi_blur_resize *r, int W, int H, int C)
{
    return r && r->out_width >= 1 && r->out_height >= 1 && r->out_width <= MI_BLUR_RESIZE_MAX_DIM && r->out_height <= MI_BLUR_RESIZE_MAX_DIM &&
           W >= 1 && H >= 1 && C >= 1 && W <= MI_BLUR_RESIZE_MAX_DIM && H <= MI_BLUR_RESIZE_MAX_DIM &&
           (r->mode == MI_BLUR_RESIZE_NEAREST || r->mode == MI_BLUR_RESIZE_BILINEAR) &&
           (long long)W * C <= INT_MAX / 2 && (long long)W * C * H <= INT_MAX &&
           (long long)r->out_width * C <= INT_MAX / 2 && (long long)r->out_width * C * r->out_height <= INT_MAX;
}

// Output size of a decimation of a W x H image: kept columns / rows (> 0 for a valid decimation, down_ok()).
inline int down_cols(int W, int sx, int ox) { return (W - ox + sx - 1) / sx; }
inline int down_rows(int H, int sy, int oy) { return (H - oy + sy - 1) / sy; }
// A decimation that is valid for a W x H image: strides 1..4, phases below them and inside the image.
inline bool down_ok(const mi_blur_decimation *d, int W, int H)
{
    return d && d->sx >= 1 && d->sx <= MI_BLUR_DECIMATE_MAX && d->sy >= 1 && d->sy <= MI_BLUR_DECIMATE_MAX && d->ox >= 0 &&
           d->ox < d->sx && d->oy >= 0 && d->oy < d->sy && d->ox < W && d->oy < H;
}

// The output geometry of a filter, for everything above the kernels (launch checks, slot sizes, counters, the CPU device).
// whole_image_only: the output image is not the input's size, so the filter takes whole images only: no bands, no halo
// rows, no planar or resident forms (a band's phase or source rows would depend on where it starts).
inline bool whole_image_only(const Filter &f) { return f.kind == FilterKind::SEP_DOWN || f.kind == FilterKind::RESIZE; }
// Width and rows of the output block of one band of band_rows rows x W of which rows [y0, y1) are asked for: those rows
// at the input's width, or the filter's own output image (of the whole band) for a whole_image_only filter.
struct OutShape { int width, rows; };
inline OutShape out_shape(const Filter &f, int W, int band_rows, int y0, int y1)
{
    if (f.kind == FilterKind::SEP_DOWN) return {down_cols(W, f.down_sx, f.down_ox), down_rows(band_rows, f.down_sy, f.down_oy)};
    if (f.kind == FilterKind::RESIZE) return {f.resize_w, f.resize_h};
    return {W, y1 - y0};
}

// The constructors validate: MI_BLUR_OK, or MI_BLUR_ERR_INVALID with *f untouched.
inline int filter_box(int radius, Filter *f)
{
    if (radius != 1 && radius != 2) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::BOX, radius, {}};
    return MI_BLUR_OK;
}

inline int filter_sep(const mi_blur_sep_kernel *k, Filter *f)
{
    if (!k || !f) return MI_BLUR_ERR_INVALID;
    if (k->rx < 0 || k->rx > MI_BLUR_SEP_MAX_RADIUS || k->ry < 0 || k->ry > MI_BLUR_SEP_MAX_RADIUS) return MI_BLUR_ERR_INVALID;
    if (k->bx < 0 || k->bx > 8 || k->by < 0 || k->by > 8) return MI_BLUR_ERR_INVALID;
    SepTaps t{};
    long long sx = 0, sy = 0;
    for (int i = 0; i <= 2 * k->rx; i++) { sx += k->wx[i]; t.wx[SEP_MAX_R - k->rx + i] = k->wx[i]; }
    for (int j = 0; j <= 2 * k->ry; j++) { sy += k->wy[j]; t.wy[SEP_MAX_R - k->ry + j] = k->wy[j]; }
    if (sx != (1LL << k->bx) || sy != (1LL << k->by)) return MI_BLUR_ERR_INVALID;
    t.rx = k->rx; t.ry = k->ry; t.shift = k->bx + k->by;
    *f = Filter{FilterKind::SEP, 0, t};
    return MI_BLUR_OK;
}

// The taps as filter_sep; the strides and phases of *d (the image size is checked where it is known: down_ok()).
inline int filter_sep_down(const mi_blur_sep_kernel *k, const mi_blur_decimation *d, Filter *f)
{
    if (!d || !f || !down_ok(d, MI_BLUR_DECIMATE_MAX, MI_BLUR_DECIMATE_MAX)) return MI_BLUR_ERR_INVALID;
    Filter g;
    if (const int rc = filter_sep(k, &g)) return rc;
    g.kind = FilterKind::SEP_DOWN;
    g.down_sx = d->sx; g.down_sy = d->sy; g.down_ox = d->ox; g.down_oy = d->oy;
    *f = g;
    return MI_BLUR_OK;
}

// The target size and mode of *r (the image size is checked where it is known: resize_ok()).
inline int filter_resize(const mi_blur_resize *r, Filter *f)
{
    if (!f || !resize_ok(r, 1, 1, 1)) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::RESIZE, 0, {}};
    f->resize_w = r->out_width; f->resize_h = r->out_height; f->resize_mode = r->mode;
    return MI_BLUR_OK;
}

inline int filter_median(int radius, Filter *f)
{
    if (radius < 1 || radius > MI_BLUR_MEDIAN_MAX_RADIUS) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::MEDIAN, radius, {}};
    return MI_BLUR_OK;
}

inline int filter_morph(int op, int rx, int ry, Filter *f)
{
    if (op != MI_BLUR_MORPH_ERODE && op != MI_BLUR_MORPH_DILATE && op != MI_BLUR_MORPH_GRADIENT) return MI_BLUR_ERR_INVALID;
    if (rx < 0 || rx > MI_BLUR_MORPH_MAX_RADIUS || ry < 0 || ry > MI_BLUR_MORPH_MAX_RADIUS) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::MORPH, 0, {}};
    f->morph_op = op; f->morph_rx = rx; f->morph_ry = ry;
    return MI_BLUR_OK;
}

inline int filter_bilateral(const mi_blur_bilateral *k, Filter *f)
{
    if (!k || !f) return MI_BLUR_ERR_INVALID;
    const int r = k->radius, n = 2 * r + 1;
    if (r < 1 || r > MI_BLUR_BILATERAL_MAX_RADIUS) return MI_BLUR_ERR_INVALID;
    long long sum = 0;
    for (int q = 0; q < n * n; q++) sum += k->spatial[q];
    if (k->spatial[r * n + r] == 0 || k->range[0] == 0 || sum > 65535) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::BILATERAL, 0, {}};
    f->bil_r = r;
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) f->bil_s[(j - r + 8) * 17 + (i - r + 8)] = k->spatial[j * n + i];
    for (int d = 0; d < 256; d++) f->bil_range[d] = k->range[d];
    return MI_BLUR_OK;
}

inline int filter_conv(const mi_blur_conv *k, Filter *f)
{
    if (!k || !f) return MI_BLUR_ERR_INVALID;
    if (k->mode != MI_BLUR_CONV_SAT && k->mode != MI_BLUR_CONV_ABS && k->mode != MI_BLUR_CONV_MAG) return MI_BLUR_ERR_INVALID;
    if (k->rx < 0 || k->rx > MI_BLUR_CONV_MAX_RADIUS || k->ry < 0 || k->ry > MI_BLUR_CONV_MAX_RADIUS) return MI_BLUR_ERR_INVALID;
    if (k->shift < 0 || k->shift > 16 || k->bias > (1 << 24) || k->bias < -(1 << 24)) return MI_BLUR_ERR_INVALID;
    const int nx = 2 * k->rx + 1, ny = 2 * k->ry + 1, tables = k->mode == MI_BLUR_CONV_MAG ? 2 : 1;
    for (int t = 0; t < tables; t++) {
        const int16_t *src = t ? k->k2 : k->k;
        long long sum = 0;
        for (int q = 0; q < nx * ny; q++) sum += src[q] < 0 ? -(long long)src[q] : src[q];
        if (sum > 65535) return MI_BLUR_ERR_INVALID;
    }
    *f = Filter{FilterKind::CONV, 0, {}};
    f->conv_rx = k->rx; f->conv_ry = k->ry; f->conv_mode = k->mode; f->conv_shift = k->shift; f->conv_bias = k->bias;
    for (int t = 0; t < tables; t++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) f->conv_k[t][(j - k->ry + 7) * 15 + (i - k->rx + 7)] = (t ? k->k2 : k->k)[j * nx + i];
    return MI_BLUR_OK;
}

}  // namespace mi_blur
