// filter.h — internal: the one filter a launch, a context or a CPU run applies, in the form the GPU kernels (the .hip
// files) and the CPU device (cpu_device.cpp) take it, the size of its output, and (last section) the tile geometry the
// tiled kernels and their host-side LDS sizing share.  Plain C++, no HIP: g++ compiles it (tests/san_*.cpp).
#pragma once

#include "../../include/mi_blur.h"

#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace mi_blur {

constexpr int SEP_MAX_R = 16;

// A validated separable kernel (mi_blur_sep_kernel).  Taps CENTRED: wx[SEP_MAX_R + d] = weight of the pixel d columns
// away, 0 beyond the radius (likewise wy for rows), so loops unrolled over d index them with compile-time constants.
struct SepTaps {
    int rx, ry, shift;      // shift = bx + by: the one truncating shift at the end
    unsigned wx[2 * SEP_MAX_R + 1], wy[2 * SEP_MAX_R + 1];
};

enum class FilterKind { BOX, SEP, MEDIAN, MORPH, BILATERAL, CONV, SEP_DOWN, RESIZE, WARP, WARP_PERSP, REMAP, AREA, COLOR };

// BOX: the fixed 3x3 / 5x5 kernel of `radius` 1|2.  SEP: the separable kernel `taps`.  MEDIAN: the median of `radius` 1..7.
// MORPH: the window minimum / maximum / their difference (`morph_op`) over (2 morph_rx + 1) x (2 morph_ry + 1).
// BILATERAL: the bilateral filter of radius `bil_r` with the spatial table `bil_s` (CENTRED in the 17 x 17 frame:
// bil_s[(j + 8) * 17 + (i + 8)] = S[j][i], 0 beyond the radius) and the range table `bil_range`.
// CONV: the signed 2-D convolution (mi_blur_conv) of radii `conv_rx`, `conv_ry` with the taps CENTRED in the 15 x 15 frame:
// conv_k[t][(j + 7) * 15 + (i + 7)] = K[j][i] (t = 0) or K2[j][i] (t = 1, MAG only; zeros otherwise), 0 beyond the radii.
// SEP_DOWN: the separable kernel `taps` on the whole image, of whose result only column down_ox + X * down_sx and row
// down_oy + Y * down_sy are kept (mi_blur_decimation): its output is smaller than its input.
// RESIZE: the fixed-point resize (mi_blur_resize) to out_w x out_h in `sample_mode`: the output may be smaller or
// larger than the input, in either axis.
// WARP: the affine warp (mi_blur_warp) to out_w x out_h: output pixel (X, Y) samples the input at the Q16 position
// warp_m maps it to, in `sample_mode`, with the border rule `warp_border` / `warp_fill`.  Whatever produces positions
// goes through a position function (warp_position() below for warp_m), so another map source slots in beside it:
// WARP_PERSP: the perspective warp (mi_blur_warp_perspective): as WARP, but the position of output pixel (X, Y) is the
// quotient of two linear forms of warp_h (persp_position(), persp_axis() below): the second map source.
// REMAP: the remap (mi_blur_remap): as WARP, but output pixel (X, Y) samples the position entry (Y, X) of the table
// remap_map gives it, 11 fraction bits (remap_axis() below): the third map source.  The table is NOT owned by the Filter:
// device memory for a launch, host memory for the CPU device; whoever builds the Filter keeps it alive.
// AREA: the area resize (mi_blur_area) to out_w x out_h: every output pixel is the box average of the input pixels its
// footprint covers, partly covered ones by their share (area_axis() below), one rounding.  No mode, no border.
// COLOR: the colour transform (mi_blur_color) `color`: pointwise, every output pixel a channel matrix of the input pixel
// at the same place, optionally through a table (color_channel() below).  The image keeps its size; its channel count
// becomes color.co: the one filter whose output has another channel count than its input (out_shape()).
struct ColorSpec {
    int co = 0, shift = 0, lut_on = 0;      // validated: co 1..4, shift 0..16, lut_on 0 | 1
    int32_t m[4][4] = {}, bias[4] = {};     // rows >= co are zero
    uint8_t lut[4][256] = {};               // zero unless lut_on
};
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
    int out_w = 0, out_h = 0, sample_mode = 0;                // RESIZE, WARP and AREA (no mode): the output image (1..MI_BLUR_RESIZE_MAX_DIM each way) and mi_blur_resize_mode; after them, for the same reason
    int warp_border = 0, warp_fill = 0;                       // WARP (mi_blur_warp_border, fill 0..255); last, for the same reason
    int64_t warp_m[6] = {};                                   // WARP: the OUTPUT -> INPUT map, Q16, row-major 2 x 3
    int64_t warp_h[9] = {};                                   // WARP_PERSP: the OUTPUT -> INPUT homography, row-major 3 x 3, free scale; out_w .. warp_fill as WARP
    const int32_t *remap_map = nullptr;                       // REMAP: int32[out_h][out_w][2] = (px, py), MI_BLUR_REMAP_FRAC fraction bits; out_w .. warp_fill as WARP
    int remap_stage_bytes = 0;                                // REMAP: the largest tile footprint the tiled kernel stages in LDS (16..REMAP_STAGE_MAX; the constructor resolves 0)
    ColorSpec color = {};                                     // COLOR; last, for the same reason
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
// A resize to out_w x out_h in `mode` that is valid for a W x H image of C channels: sizes 1..MI_BLUR_RESIZE_MAX_DIM both
// sides, a known mode, and input and output images inside the per-image byte limits of a launch.  (A Filter's fields or the ABI struct's.)
inline bool resize_ok(int out_w, int out_h, int mode, int W, int H, int C)
{
    return out_w >= 1 && out_h >= 1 && out_w <= MI_BLUR_RESIZE_MAX_DIM && out_h <= MI_BLUR_RESIZE_MAX_DIM &&
           W >= 1 && H >= 1 && C >= 1 && W <= MI_BLUR_RESIZE_MAX_DIM && H <= MI_BLUR_RESIZE_MAX_DIM &&
           (mode == MI_BLUR_RESIZE_NEAREST || mode == MI_BLUR_RESIZE_BILINEAR) &&
           (long long)W * C <= INT_MAX / 2 && (long long)W * C * H <= INT_MAX &&
           (long long)out_w * C <= INT_MAX / 2 && (long long)out_w * C * out_h <= INT_MAX;
}
inline bool resize_ok(const mi_blur_resize *r, int W, int H, int C) { return r && resize_ok(r->out_width, r->out_height, r->mode, W, H, C); }

// The blend of four taps a b / c d with the weights fx, fy (0..BLEND_ONE) of the right column and the lower row, one
// rounding: the one every bilinear sample of RESIZE and WARP goes through (the tiled kernels in its v_mad_u32_u24 form,
// lerp24() of kernel_common.h, on the same constants).  fx = fy = 0 (NEAREST) gives tap a back exactly.
constexpr unsigned BLEND_ONE = 2048u, BLEND_SHIFT = 22, BLEND_BIAS = 1u << (BLEND_SHIFT - 1);   // BLEND_ONE^2 = 1 << BLEND_SHIFT
MI_BLUR_HD inline unsigned bilinear_blend(unsigned a, unsigned b, unsigned c, unsigned d, unsigned fx, unsigned fy)
{
    const unsigned top = (BLEND_ONE - fx) * a + fx * b, bot = (BLEND_ONE - fx) * c + fx * d;
    return ((BLEND_ONE - fy) * top + fy * bot + BLEND_BIAS) >> BLEND_SHIFT;
}

// ---- the affine warp (include/mi_blur.h, "Affine warp").  The GPU kernels, the CPU device and mi_blur_warp_coord all
// take their coordinates from warp_position() and warp_axis().
// The Q16 input position of output pixel (X, Y): |m| within the limits of warp_ok() keeps both below 2^47.
struct WarpPos { int64_t sx, sy; };
MI_BLUR_HD inline WarpPos warp_position(const int64_t *m, int X, int Y)
{
    return {m[0] * X + m[1] * Y + m[2], m[3] * X + m[4] * Y + m[5]};
}
// One axis of a position S: the first tap i0 and the weight f (0..2047) of tap i0 + 1.  BILINEAR: the position rounded
// to 11 fraction bits, p = (S + 16) >> 5, i0 = p >> 11, f = p & 2047.  NEAREST: i0 = (S + 32768) >> 16, f = 0.  All shifts
// floor.  n > 0: p is clamped into [-2 * 2048, (n + 1) * 2048] first (NEAREST: i0 into [-2, n + 1]), which changes no
// output byte of an axis of n samples under either border rule (both taps of a position out there lie on the same
// side outside the axis) and lets the callers go on in 32 bits.  n == 0: not clamped (|S| < 2^47, so i0 fits an int).
struct WarpAxis { int i0, f; };
MI_BLUR_HD inline WarpAxis warp_axis(int64_t S, int mode, int n)
{
    int64_t p = mode == MI_BLUR_RESIZE_NEAREST ? (S + 32768) >> 5 : (S + 16) >> 5;    // NEAREST: i0 = p >> 11 all the same
    if (n > 0) {
        const int64_t lo = -2 * 2048, hi = ((int64_t)n + 1) * 2048;
        p = p < lo ? lo : p > hi ? hi : p;
    }
    return {(int)(p >> 11), mode == MI_BLUR_RESIZE_NEAREST ? 0 : (int)(p & 2047)};
}
struct WarpCoord { int x0, y0, fx, fy; };
MI_BLUR_HD inline WarpCoord warp_coord(const int64_t *m, int mode, int W, int H, int X, int Y)
{
    const WarpPos s = warp_position(m, X, Y);
    const WarpAxis ax = warp_axis(s.sx, mode, W), ay = warp_axis(s.sy, mode, H);
    return {ax.i0, ay.i0, ax.f, ay.f};
}
// One output byte from the W x H image whose channel-c bytes start at img (pitch bytes per row, C per pixel), for
// coordinates clamped by warp_axis (n > 0).  Each tap is decided on its own: CLAMP clamps its index, CONSTANT makes it
// `fill` when it lies outside the image.
MI_BLUR_HD inline unsigned warp_sample(const uint8_t *img, size_t pitch, int C, int W, int H, int border, unsigned fill, const WarpCoord &q)
{
    const int xa = q.x0 < 0 ? 0 : q.x0 > W - 1 ? W - 1 : q.x0, xb = q.x0 + 1 < 0 ? 0 : q.x0 + 1 > W - 1 ? W - 1 : q.x0 + 1;
    const int ya = q.y0 < 0 ? 0 : q.y0 > H - 1 ? H - 1 : q.y0, yb = q.y0 + 1 < 0 ? 0 : q.y0 + 1 > H - 1 ? H - 1 : q.y0 + 1;
    const uint8_t *ra = img + (size_t)ya * pitch, *rb = img + (size_t)yb * pitch;
    unsigned a = ra[(size_t)xa * C], b = ra[(size_t)xb * C], c = rb[(size_t)xa * C], d = rb[(size_t)xb * C];
    if (border == MI_BLUR_WARP_CONSTANT) {
        const bool ixa = xa == q.x0, ixb = xb == q.x0 + 1, iya = ya == q.y0, iyb = yb == q.y0 + 1;
        a = ixa && iya ? a : fill; b = ixb && iya ? b : fill; c = ixa && iyb ? c : fill; d = ixb && iyb ? d : fill;
    }
    return bilinear_blend(a, b, c, d, (unsigned)q.fx, (unsigned)q.fy);
}
// The input pixels the taps of output pixels [X0, X1] x [Y0, Y1] (inclusive) can touch: an affine map has its extrema
// at the four corners and warp_axis is monotone in S, so the box of the corners' taps, with the + 1 tap, holds them all.
// CLAMP: the box clamped into the image (clamping is monotone, so clamped taps stay inside it; never empty).  CONSTANT:
// the box intersected with the image (taps outside it are `fill`); empty (x0 > x1 or y0 > y1) when it misses the image.
struct WarpBox { int x0, x1, y0, y1; };
MI_BLUR_HD inline WarpBox warp_footprint(const int64_t *m, int mode, int border, int W, int H, int X0, int X1, int Y0, int Y1)
{
    const WarpPos c0 = warp_position(m, X0, Y0), c1 = warp_position(m, X1, Y0), c2 = warp_position(m, X0, Y1), c3 = warp_position(m, X1, Y1);
    const int64_t sx_lo = c0.sx < c1.sx ? c0.sx : c1.sx, sx_lo2 = c2.sx < c3.sx ? c2.sx : c3.sx;
    const int64_t sx_hi = c0.sx > c1.sx ? c0.sx : c1.sx, sx_hi2 = c2.sx > c3.sx ? c2.sx : c3.sx;
    const int64_t sy_lo = c0.sy < c1.sy ? c0.sy : c1.sy, sy_lo2 = c2.sy < c3.sy ? c2.sy : c3.sy;
    const int64_t sy_hi = c0.sy > c1.sy ? c0.sy : c1.sy, sy_hi2 = c2.sy > c3.sy ? c2.sy : c3.sy;
    WarpBox b;
    b.x0 = warp_axis(sx_lo < sx_lo2 ? sx_lo : sx_lo2, mode, W).i0;
    b.x1 = warp_axis(sx_hi > sx_hi2 ? sx_hi : sx_hi2, mode, W).i0 + 1;
    b.y0 = warp_axis(sy_lo < sy_lo2 ? sy_lo : sy_lo2, mode, H).i0;
    b.y1 = warp_axis(sy_hi > sy_hi2 ? sy_hi : sy_hi2, mode, H).i0 + 1;
    if (border == MI_BLUR_WARP_CONSTANT) {
        b.x0 = b.x0 < 0 ? 0 : b.x0; b.x1 = b.x1 > W - 1 ? W - 1 : b.x1;
        b.y0 = b.y0 < 0 ? 0 : b.y0; b.y1 = b.y1 > H - 1 ? H - 1 : b.y1;
    } else {
        b.x0 = b.x0 < 0 ? 0 : b.x0 > W - 1 ? W - 1 : b.x0; b.x1 = b.x1 < 0 ? 0 : b.x1 > W - 1 ? W - 1 : b.x1;
        b.y0 = b.y0 < 0 ? 0 : b.y0 > H - 1 ? H - 1 : b.y0; b.y1 = b.y1 < 0 ? 0 : b.y1 > H - 1 ? H - 1 : b.y1;
    }
    return b;
}
// A warp that is valid for a W x H image of C channels: the sizes, mode and byte limits of resize_ok(), and what
// warp_map_ok() adds: a known border, fill 0..255, the linear part within 2^26 and the translation within 2^46 (Q16), so
// positions stay below 2^47.
inline bool warp_map_ok(int border, int fill, const int64_t *m)
{
    if ((border != MI_BLUR_WARP_CLAMP && border != MI_BLUR_WARP_CONSTANT) || fill < 0 || fill > 255) return false;
    const int64_t lin = (int64_t)1 << 26, off = (int64_t)1 << 46;
    for (int i = 0; i < 6; i++) {
        const int64_t lim = i % 3 == 2 ? off : lin;
        if (m[i] > lim || m[i] < -lim) return false;
    }
    return true;
}
inline bool warp_ok(const mi_blur_warp *w, int W, int H, int C)
{
    return w && resize_ok(w->out_width, w->out_height, w->mode, W, H, C) && warp_map_ok(w->border, w->fill, w->m);
}

// ---- the perspective warp (include/mi_blur.h, "Perspective warp").  The GPU kernels, the CPU device and
// mi_blur_warp_perspective_coord all take their coordinates from persp_position() and persp_axis(); the taps, the blend
// and the border rules are the affine warp's (warp_sample(), warp_tap()).
// The numerators and the denominator of output pixel (X, Y): |h| within the limits of persp_map_ok() keeps all three below 2^49.
struct PerspPos { int64_t nx, ny, d; };
MI_BLUR_HD inline PerspPos persp_position(const int64_t *h, int X, int Y)
{
    return {h[0] * X + h[1] * Y + h[2], h[3] * X + h[4] * Y + h[5], h[6] * X + h[7] * Y + h[8]};
}
// floor(a / b) for b > 0.
MI_BLUR_HD inline int64_t floor_div(int64_t a, int64_t b)
{
    const int64_t q = a / b, r = a - q * b;
    return r < 0 ? q - 1 : q;
}
// min(max(floor(num / den), lo), hi) for |num| < 2^62, 0 < den < 2^51, |lo|, |hi| < 2^27 and rden = 1.0 / (double)den,
// without a 64-bit division: the double estimate est = num * rden is within 2^-51 of the quotient t in relative terms
// (den is exact in a double, num and the reciprocal are rounded once each, the product once).  est >= hi + 2 means
// t > hi + 1 and est <= lo - 2 means t < lo - 1: the clamp decides alone.  Otherwise |t| < 2^27 + 3, the estimate is off
// by less than 2^-23, floor(est) is floor(t) or one beside it, and the exact remainder (|q * den| <= |num| + den < 2^63)
// says which.  The same bytes on the CPU and the GPU whatever the last bit of either's double division: the remainder decides.
MI_BLUR_HD inline int64_t floor_div_clamped(int64_t num, int64_t den, double rden, int64_t lo, int64_t hi)
{
    const double est = (double)num * rden;
    if (est >= (double)(hi + 2)) return hi;
    if (est <= (double)(lo - 2)) return lo;
    int64_t q = (int64_t)__builtin_floor(est);
    const int64_t r = num - q * den;
    q = r < 0 ? q - 1 : r >= den ? q + 1 : q;
    return q < lo ? lo : q > hi ? hi : q;
}
// One axis of a position N / D (D >= 1): the first tap i0 and the weight f (0..2047) of tap i0 + 1.  BILINEAR: the position
// rounded to 11 fraction bits, p = floor((N * 4096 + D) / (2 D)), i0 = p >> 11, f = p & 2047.  NEAREST:
// i0 = floor((2 N + D) / (2 D)), f = 0.  n > 0: p is clamped into [-2 * 2048, (n + 1) * 2048] (NEAREST: i0 into
// [-2, n + 1]) as warp_axis() does, for the same reason, and rden = 1.0 / (double)(2 D) (one reciprocal serves both
// axes of a pixel).  n == 0: not clamped, the plain 64-bit division, rden unused; i0 can reach 2^50.
struct PerspAxis { int64_t i0; int f; };
MI_BLUR_HD inline PerspAxis persp_axis(int64_t N, int64_t D, double rden, int mode, int n)
{
    const bool nearest = mode == MI_BLUR_RESIZE_NEAREST;
    const int64_t num = nearest ? 2 * N + D : N * 4096 + D, den = 2 * D;
    if (n == 0) {
        const int64_t p = floor_div(num, den);
        return nearest ? PerspAxis{p, 0} : PerspAxis{p >> 11, (int)(p & 2047)};
    }
    if (nearest) return {floor_div_clamped(num, den, rden, -2, (int64_t)n + 1), 0};
    const int64_t p = floor_div_clamped(num, den, rden, -2 * 2048, ((int64_t)n + 1) * 2048);
    return {p >> 11, (int)(p & 2047)};
}
MI_BLUR_HD inline double persp_rden(int64_t D) { return 1.0 / (double)(2 * D); }
// The clamped coordinates of a position (W, H > 0), in the form warp_sample() and warp_tap() take.
MI_BLUR_HD inline WarpCoord persp_coord_at(const PerspPos &s, int mode, int W, int H)
{
    const double rden = persp_rden(s.d);
    const PerspAxis ax = persp_axis(s.nx, s.d, rden, mode, W), ay = persp_axis(s.ny, s.d, rden, mode, H);
    return {(int)ax.i0, (int)ay.i0, ax.f, ay.f};
}
MI_BLUR_HD inline WarpCoord persp_coord(const int64_t *h, int mode, int W, int H, int X, int Y)
{
    return persp_coord_at(persp_position(h, X, Y), mode, W, H);
}
// The input pixels the taps of output pixels [X0, X1] x [Y0, Y1] (inclusive) can touch, as warp_footprint(): the box of
// the four corners' taps with the + 1 tap.  Why the corners still do for a projective map: along any straight segment
// of output pixels on which D > 0 (every segment inside a valid output: D is linear and >= 1 at its corners),
// N / D = (a + b t) / (c + d t) has the derivative (b c - a d) / (c + d t)^2, of one sign, so it is monotone; p is a
// floor of 2048 N / D + 1/2 and the clamp and the shift are monotone too.  A pixel of the rectangle lies on a horizontal
// segment between two pixels of its left and right edges, and those on vertical segments between corners: its x0 is
// between the x0 of two edge pixels, each between those of two corners.  Likewise y0.
MI_BLUR_HD inline WarpBox persp_footprint(const int64_t *h, int mode, int border, int W, int H, int X0, int X1, int Y0, int Y1)
{
    const WarpCoord c0 = persp_coord(h, mode, W, H, X0, Y0), c1 = persp_coord(h, mode, W, H, X1, Y0);
    const WarpCoord c2 = persp_coord(h, mode, W, H, X0, Y1), c3 = persp_coord(h, mode, W, H, X1, Y1);
    const int x_lo = c0.x0 < c1.x0 ? c0.x0 : c1.x0, x_lo2 = c2.x0 < c3.x0 ? c2.x0 : c3.x0;
    const int x_hi = c0.x0 > c1.x0 ? c0.x0 : c1.x0, x_hi2 = c2.x0 > c3.x0 ? c2.x0 : c3.x0;
    const int y_lo = c0.y0 < c1.y0 ? c0.y0 : c1.y0, y_lo2 = c2.y0 < c3.y0 ? c2.y0 : c3.y0;
    const int y_hi = c0.y0 > c1.y0 ? c0.y0 : c1.y0, y_hi2 = c2.y0 > c3.y0 ? c2.y0 : c3.y0;
    WarpBox b;
    b.x0 = x_lo < x_lo2 ? x_lo : x_lo2; b.x1 = (x_hi > x_hi2 ? x_hi : x_hi2) + 1;
    b.y0 = y_lo < y_lo2 ? y_lo : y_lo2; b.y1 = (y_hi > y_hi2 ? y_hi : y_hi2) + 1;
    if (border == MI_BLUR_WARP_CONSTANT) {
        b.x0 = b.x0 < 0 ? 0 : b.x0; b.x1 = b.x1 > W - 1 ? W - 1 : b.x1;
        b.y0 = b.y0 < 0 ? 0 : b.y0; b.y1 = b.y1 > H - 1 ? H - 1 : b.y1;
    } else {
        b.x0 = b.x0 < 0 ? 0 : b.x0 > W - 1 ? W - 1 : b.x0; b.x1 = b.x1 < 0 ? 0 : b.x1 > W - 1 ? W - 1 : b.x1;
        b.y0 = b.y0 < 0 ? 0 : b.y0 > H - 1 ? H - 1 : b.y0; b.y1 = b.y1 < 0 ? 0 : b.y1 > H - 1 ? H - 1 : b.y1;
    }
    return b;
}
// A homography that is valid for an output of out_w x out_h (1..MI_BLUR_RESIZE_MAX_DIM each): a known border, fill
// 0..255, the six coefficients of X and Y within 2^32, the three constants within 2^48, and D >= 1 at the four corner
// pixels of the output, so (D is linear) at every output pixel: no horizon crosses the output.
inline bool persp_map_ok(int border, int fill, const int64_t *h, int out_w, int out_h)
{
    if ((border != MI_BLUR_WARP_CLAMP && border != MI_BLUR_WARP_CONSTANT) || fill < 0 || fill > 255) return false;
    const int64_t lin = (int64_t)1 << 32, off = (int64_t)1 << 48;
    for (int i = 0; i < 9; i++) {
        const int64_t lim = i % 3 == 2 ? off : lin;
        if (h[i] > lim || h[i] < -lim) return false;
    }
    const int xs[2] = {0, out_w - 1}, ys[2] = {0, out_h - 1};
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++)
            if (persp_position(h, xs[i], ys[j]).d < 1) return false;
    return true;
}
inline bool persp_ok(const mi_blur_warp_perspective *w, int W, int H, int C)
{
    return w && resize_ok(w->out_width, w->out_height, w->mode, W, H, C) && persp_map_ok(w->border, w->fill, w->h, w->out_width, w->out_height);
}

// ---- the remap (include/mi_blur.h, "Remap").  The GPU kernels, the CPU device, mi_blur_remap_coord and mi_blur_remap_plan
// all take their coordinates from remap_axis(); the taps, the blend and the border rules are the affine warp's.
// One axis of a map entry pv (11 fraction bits) on an axis of n >= 1 samples: p = pv clamped into [-2 * 2048, (n + 1) * 2048]
// (the clamp of warp_axis(), for the same reason: any int32 is a valid entry, and (n + 1) * 2048 < 2^27), then BILINEAR
// i0 = p >> 11, f = p & 2047; NEAREST i0 = (p + 1024) >> 11, f = 0.
MI_BLUR_HD inline WarpAxis remap_axis(int32_t pv, int mode, int n)
{
    const int32_t lo = -2 * 2048, hi = (n + 1) * 2048;
    const int32_t p = pv < lo ? lo : pv > hi ? hi : pv;
    if (mode == MI_BLUR_RESIZE_NEAREST) return {(p + 1024) >> 11, 0};
    return {p >> 11, p & 2047};
}
MI_BLUR_HD inline WarpCoord remap_coord(int32_t px, int32_t py, int mode, int W, int H)
{
    const WarpAxis ax = remap_axis(px, mode, W), ay = remap_axis(py, mode, H);
    return {ax.i0, ay.i0, ax.f, ay.f};
}
// The input pixels the taps of a set of output pixels can touch, from the extrema of their first taps (x0, y0): the box
// [x_lo, x_hi + 1] x [y_lo, y_hi + 1], finished exactly as warp_footprint() finishes its own: clamped into the image
// (CLAMP; never empty) or intersected with it (CONSTANT; empty when it misses the image).  blur_remap_tiled_kernel
// reduces the extrema over a tile's map entries, mi_blur_remap_plan walks the same tiles on the host: one function.
MI_BLUR_HD inline WarpBox remap_box(int x_lo, int x_hi, int y_lo, int y_hi, int border, int W, int H)
{
    WarpBox b{x_lo, x_hi + 1, y_lo, y_hi + 1};
    if (border == MI_BLUR_WARP_CONSTANT) {
        b.x0 = b.x0 < 0 ? 0 : b.x0; b.x1 = b.x1 > W - 1 ? W - 1 : b.x1;
        b.y0 = b.y0 < 0 ? 0 : b.y0; b.y1 = b.y1 > H - 1 ? H - 1 : b.y1;
    } else {
        b.x0 = b.x0 < 0 ? 0 : b.x0 > W - 1 ? W - 1 : b.x0; b.x1 = b.x1 < 0 ? 0 : b.x1 > W - 1 ? W - 1 : b.x1;
        b.y0 = b.y0 < 0 ? 0 : b.y0 > H - 1 ? H - 1 : b.y0; b.y1 = b.y1 < 0 ? 0 : b.y1 > H - 1 ? H - 1 : b.y1;
    }
    return b;
}
// A remap that is valid for a W x H image of C channels: the sizes, mode and byte limits of resize_ok(), a known border,
// fill 0..255, stage_bytes 0 (the default) or 16..REMAP_STAGE_MAX.  The map's entries are not looked at: every one is valid.
constexpr int REMAP_STAGE_MAX = 65520;
inline bool remap_ok(const mi_blur_remap *r, int W, int H, int C)
{
    return r && resize_ok(r->out_width, r->out_height, r->mode, W, H, C) &&
           (r->border == MI_BLUR_WARP_CLAMP || r->border == MI_BLUR_WARP_CONSTANT) && r->fill >= 0 && r->fill <= 255 &&
           (r->stage_bytes == 0 || (r->stage_bytes >= 16 && r->stage_bytes <= REMAP_STAGE_MAX));
}

// ---- the area resize (include/mi_blur.h, "Area resize").  The GPU kernels, the CPU device and mi_blur_area_coord all take
// their taps from area_axis().
// One axis: output X of n_out samples over n_in input samples, in units where an input pixel is n_out long and an output
// pixel n_in.  Taps i_lo..i_hi; the first weighs w_lo, the last w_hi (0 when i_hi == i_lo: w_lo is then n_in), every tap
// between them n_out.  1 <= n_in, n_out <= MI_BLUR_RESIZE_MAX_DIM keeps everything in 32 bits ((X + 1) * n_in <= 2^30).
struct AreaAxis { int i_lo, i_hi, w_lo, w_hi; };
MI_BLUR_HD inline AreaAxis area_axis(int n_in, int n_out, int X)
{
    const unsigned a = (unsigned)X * (unsigned)n_in, b = a + (unsigned)n_in;
    AreaAxis r;
    r.i_lo = (int)(a / (unsigned)n_out);
    r.i_hi = (int)((b - 1u) / (unsigned)n_out);
    if (r.i_hi == r.i_lo) { r.w_lo = n_in; r.w_hi = 0; }
    else { r.w_lo = (int)((unsigned)(r.i_lo + 1) * (unsigned)n_out - a); r.w_hi = (int)(b - (unsigned)r.i_hi * (unsigned)n_out); }
    return r;
}
MI_BLUR_HD inline unsigned area_weight(const AreaAxis &ax, int n_out, int i) { return (unsigned)(i == ax.i_lo ? ax.w_lo : i == ax.i_hi ? ax.w_hi : n_out); }
// The one rounding: floor((2 S + D) / (2 D)) for the weighted sum S <= 255 D of a W x H image, D = W * H <= 2^30, and
// rden = area_rden(W, H).  floor_div_clamped() gives the same byte whatever the last bit of the double estimate.
MI_BLUR_HD inline double area_rden(int W, int H) { return 1.0 / (double)(2 * ((int64_t)W * H)); }
MI_BLUR_HD inline unsigned area_round(uint64_t S, int64_t D, double rden) { return (unsigned)floor_div_clamped((int64_t)(2 * S) + D, 2 * D, rden, 0, 255); }
// An area resize to out_w x out_h that is valid for a W x H image of C channels: the sizes and byte limits of resize_ok()
// and a reduction of at most MI_BLUR_AREA_MAX_RATIO on either axis (enlargements are valid).
inline bool area_ok(int out_w, int out_h, int W, int H, int C)
{
    return resize_ok(out_w, out_h, MI_BLUR_RESIZE_BILINEAR, W, H, C) && (long long)W <= (long long)MI_BLUR_AREA_MAX_RATIO * out_w &&
           (long long)H <= (long long)MI_BLUR_AREA_MAX_RATIO * out_h;
}
inline bool area_ok(const mi_blur_area *r, int W, int H, int C) { return r && area_ok(r->out_width, r->out_height, W, H, C); }

// ---- the colour transform (include/mi_blur.h, "Colour transform").  The GPU's generic kernel and the CPU device take
// every byte from color_channel(); the tiled kernel does the same sum with its channel counts as template arguments and
// ends in the same color_clamp().
// v = clamp(acc >> shift, 0, 255); the shift is arithmetic, so it floors.
// On the device the empty asm keeps the shift and the clamp apart, as conv_pack() (conv_kernels.hip) does and for its
// reason: left together, hipcc fuses the shift-and-clamp of two neighbouring bytes into v_ashr_pk_u8_i32 and ORs the
// other two bytes of the dword onto its result as if the upper half of that register were zero, which on the MI355X it
// is not: bytes 2 and 3 of every output dword of blur_color_tiled_kernel came out ORed with stale bits.
MI_BLUR_HD inline int color_clamp(int32_t acc, int shift)
{
    int32_t v = acc >> shift;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v < 0 ? 0 : v > 255 ? 255 : v;
}
// One output channel of the input pixel px[0 .. C - 1], C <= 4: m = the channel's row of weights, lut = its table or null.
// |acc| < 2^27 for a valid transform: 32 bits are exact.
MI_BLUR_HD inline uint8_t color_channel(const int32_t *m, int32_t bias, int shift, const uint8_t *lut, int C, const uint8_t *px)
{
    int32_t acc = bias;
    for (int i = 0; i < C; i++) acc += m[i] * (int32_t)px[i];
    const int v = color_clamp(acc, shift);
    return lut ? lut[v] : (uint8_t)v;
}
inline uint8_t color_channel(const ColorSpec &k, int C, const uint8_t *px, int o)
{
    return color_channel(k.m[o], k.bias[o], k.shift, k.lut_on ? k.lut[o] : nullptr, C, px);
}
// A colour transform that is valid whatever the image: the fields' ranges, and per used row sum |m| <= 2^18 over all
// four columns (C is not known yet) and |bias| <= 2^26.  Rows >= out_channels are not read.
constexpr int64_t COLOR_ROW_MAX = (int64_t)1 << 18, COLOR_BIAS_MAX = (int64_t)1 << 26;
inline bool color_ok(const mi_blur_color *k)
{
    if (!k || k->out_channels < 1 || k->out_channels > MI_BLUR_COLOR_MAX_CHANNELS || k->shift < 0 || k->shift > 16 ||
        (k->lut_on != 0 && k->lut_on != 1))
        return false;
    for (int o = 0; o < k->out_channels; o++) {
        int64_t sum = 0;
        for (int i = 0; i < MI_BLUR_COLOR_MAX_CHANNELS; i++) sum += k->m[o][i] < 0 ? -(int64_t)k->m[o][i] : (int64_t)k->m[o][i];
        if (sum > COLOR_ROW_MAX || k->bias[o] > COLOR_BIAS_MAX || k->bias[o] < -COLOR_BIAS_MAX) return false;
    }
    return true;
}
// ... and for a W x H image of C channels: 1..4 channels in, and the per-image byte limits of resize_ok() on the input
// (with C) and on the output (with co).
inline bool color_image_ok(int co, int W, int H, int C)
{
    return C >= 1 && C <= MI_BLUR_COLOR_MAX_CHANNELS && resize_ok(W, H, MI_BLUR_RESIZE_BILINEAR, W, H, C) &&
           resize_ok(W, H, MI_BLUR_RESIZE_BILINEAR, W, H, co);
}

// ---- histogram and tone tables (include/mi_blur.h, "Histogram, and tone tables made from it").  The host export, the
// CPU device and blur_tone_table_kernel all take a table's bytes from tone_entry(), and lo / hi from the two predicates
// below: c(v) is monotone, so lo = the number of v with tone_below_lo() and hi = the number with tone_upto_hi() minus 1,
// which the kernel counts across its threads and tone_table() in a loop.
// An image the family takes: 1..4 channels and the per-image byte limits of resize_ok(), so a count fits 32 bits.
inline bool hist_image_ok(int W, int H, int C)
{
    return C >= 1 && C <= MI_BLUR_COLOR_MAX_CHANNELS && resize_ok(W, H, MI_BLUR_RESIZE_BILINEAR, W, H, C);
}
constexpr int TONE_CLIP_MAX = 32767;
inline bool tone_ok(const mi_blur_tone *t, int C)
{
    if (!t || C < 1 || C > MI_BLUR_COLOR_MAX_CHANNELS) return false;
    if (t->mode != MI_BLUR_TONE_EQUALIZE && t->mode != MI_BLUR_TONE_STRETCH) return false;
    if (t->clip_lo < 0 || t->clip_hi < 0 || t->clip_lo > TONE_CLIP_MAX || t->clip_hi > TONE_CLIP_MAX) return false;
    if (t->mode == MI_BLUR_TONE_EQUALIZE && (t->clip_lo || t->clip_hi)) return false;
    return (t->joint == 0 || t->joint == 1) && t->channel_mask >= 0 && t->channel_mask < (1 << C);
}
// The channels *t transforms, as a mask without the "0 = all" form.
MI_BLUR_HD inline int tone_mask(int channel_mask, int C) { return channel_mask ? channel_mask : (1 << C) - 1; }
// k = floor(N * clip / 65536): N <= 2^33, clip < 2^15.  EQUALIZE: clips of 0, so k = 0 and lo = m, the first level present.
MI_BLUR_HD inline uint64_t tone_clip_count(uint64_t N, int clip) { return (N * (uint64_t)clip) >> 16; }
MI_BLUR_HD inline bool tone_below_lo(uint64_t cv, uint64_t k_lo) { return cv <= k_lo; }                                 // v < lo
MI_BLUR_HD inline bool tone_upto_hi(uint64_t N, uint64_t c_prev, uint64_t k_hi) { return N - c_prev > k_hi; }           // v <= hi
// lut[v], from c(v), N > 0, lo, hi and c(lo) (EQUALIZE: lo = m and c(lo) = h(m); hi is not used).
MI_BLUR_HD inline uint8_t tone_entry(int mode, int v, uint64_t cv, uint64_t N, int lo, int hi, uint64_t c_lo)
{
    if (mode == MI_BLUR_TONE_EQUALIZE) {
        const uint64_t D = N - c_lo;
        if (D == 0) return (uint8_t)v;
        return v < lo ? 0 : (uint8_t)((510u * (cv - c_lo) + D) / (2u * D));
    }
    if (lo == hi) return (uint8_t)v;
    if (v <= lo) return 0;
    if (v >= hi) return 255;
    const unsigned d = (unsigned)(hi - lo);
    return (uint8_t)((510u * (unsigned)(v - lo) + d) / (2u * d));
}
// One table from the cumulative histogram cum[v] = c(v).
inline void tone_table(const mi_blur_tone &t, const uint64_t *cum, uint8_t *lut)
{
    const uint64_t N = cum[MI_BLUR_HIST_BINS - 1];
    if (N == 0) { for (int v = 0; v < MI_BLUR_HIST_BINS; v++) lut[v] = (uint8_t)v; return; }
    const uint64_t k_lo = tone_clip_count(N, t.clip_lo), k_hi = tone_clip_count(N, t.clip_hi);
    int lo = 0, n_hi = 0;
    for (int v = 0; v < MI_BLUR_HIST_BINS; v++) {
        lo += tone_below_lo(cum[v], k_lo);
        n_hi += tone_upto_hi(N, v ? cum[v - 1] : 0, k_hi);
    }
    for (int v = 0; v < MI_BLUR_HIST_BINS; v++) lut[v] = tone_entry(t.mode, v, cum[v], N, lo, n_hi - 1, cum[lo]);
}
// The tables of one image: hist uint32[C][256] -> tables uint8[C][256] (t valid for C: tone_ok()).
inline void tone_tables(const mi_blur_tone &t, const uint32_t *hist, int C, uint8_t *tables)
{
    const int mask = tone_mask(t.channel_mask, C);
    uint64_t cum[MI_BLUR_HIST_BINS];
    uint8_t joint_lut[MI_BLUR_HIST_BINS];
    if (t.joint) {
        uint64_t run = 0;
        for (int v = 0; v < MI_BLUR_HIST_BINS; v++) {
            for (int c = 0; c < C; c++) if ((mask >> c) & 1) run += hist[c * MI_BLUR_HIST_BINS + v];
            cum[v] = run;
        }
        tone_table(t, cum, joint_lut);
    }
    for (int c = 0; c < C; c++) {
        uint8_t *lut = tables + c * MI_BLUR_HIST_BINS;
        if (!((mask >> c) & 1)) { for (int v = 0; v < MI_BLUR_HIST_BINS; v++) lut[v] = (uint8_t)v; continue; }
        if (t.joint) { for (int v = 0; v < MI_BLUR_HIST_BINS; v++) lut[v] = joint_lut[v]; continue; }
        uint64_t run = 0;
        for (int v = 0; v < MI_BLUR_HIST_BINS; v++) { run += hist[c * MI_BLUR_HIST_BINS + v]; cum[v] = run; }
        tone_table(t, cum, lut);
    }
}

// ---- CLAHE (include/mi_blur.h, "CLAHE").  The host exports mi_blur_clahe_coord and mi_blur_clahe_table, the CPU device
// and the four kernels take a tile's edges from clahe_edge(), a bin after clipping from clahe_bin(), a table's byte from
// clahe_entry(), a pixel's tiles and weight on one axis from clahe_axis() and the output byte from bilinear_blend().
inline bool clahe_ok(const mi_blur_clahe *k, int W, int H, int C)
{
    if (!k || C < 1 || C > MI_BLUR_COLOR_MAX_CHANNELS) return false;
    if (k->tiles_x < 1 || k->tiles_y < 1 || k->tiles_x > MI_BLUR_CLAHE_MAX_TILES || k->tiles_y > MI_BLUR_CLAHE_MAX_TILES) return false;
    if (k->tiles_x > W || k->tiles_y > H) return false;
    return k->clip_q8 >= 0 && k->clip_q8 <= 65536 && k->channel_mask >= 0 && k->channel_mask < (1 << C);
}
// b_t = floor(t * S / T): S <= 32768 and t <= T <= 64, so 32 bits hold it.
MI_BLUR_HD inline int clahe_edge(int S, int T, int t) { return (int)((unsigned)t * (unsigned)S / (unsigned)T); }
// m_t = b_t + b_(t+1): the centre of tile t in half-pixels.
MI_BLUR_HD inline int clahe_mid(int S, int T, int t) { return clahe_edge(S, T, t) + clahe_edge(S, T, t + 1); }
// (t0, t1, frac) of pixel x on an axis of S pixels and T <= S tiles.  x lies in tile t = ceil((x + 1) T / S) - 1, and
// with p = 2x + 1: 2 b_t < p < 2 b_(t+1), so m_(t-1) < p < m_(t+1) (no tile is empty) and t0 is t or t - 1.
MI_BLUR_HD inline void clahe_axis(int S, int T, int x, int &t0, int &t1, int &frac)
{
    const int p = 2 * x + 1;
    if (T == 1 || p <= clahe_mid(S, T, 0)) { t0 = t1 = 0; frac = 0; return; }
    if (p >= clahe_mid(S, T, T - 1)) { t0 = t1 = T - 1; frac = 0; return; }
    const int t = (int)((((unsigned)x + 1u) * (unsigned)T - 1u) / (unsigned)S);
    int m0 = clahe_mid(S, T, t);
    t0 = t;
    if (m0 > p) { t0 = t - 1; m0 = clahe_mid(S, T, t0); }
    t1 = t0 + 1;
    frac = (int)((unsigned)(p - m0) * BLEND_ONE / (unsigned)(clahe_mid(S, T, t1) - m0));      // (p - m0) < 2 S <= 2^16
}
// Pixels on an axis fall into T + 1 classes by the tiles they blend: class k = the number of centres m_t <= p, whose
// pixels take the tiles max(k - 1, 0) and min(k, T - 1) (at p == m_0 that is (0, 1) with frac 0 where clahe_axis() says
// (0, 0): the same byte).  Class k is the pixels [clahe_class_lo(k), clahe_class_lo(k + 1)); it may be empty.
MI_BLUR_HD inline int clahe_class_lo(int S, int T, int k) { return k <= 0 ? 0 : k > T ? S : clahe_mid(S, T, k - 1) >> 1; }
// The clip of a tile of A pixels.  clip_q8 == 0 (no clipping) is the clip A: no bin holds more.
MI_BLUR_HD inline uint32_t clahe_clip(uint32_t A, int clip_q8)
{
    if (clip_q8 == 0) return A;
    const uint64_t c = ((uint64_t)(unsigned)clip_q8 * A) >> 16;
    return c < 1 ? 1u : (uint32_t)c;
}
MI_BLUR_HD inline uint32_t clahe_over(uint32_t h, uint32_t clip) { return h > clip ? h - clip : 0u; }
// h'(v): bin v clipped, plus its share of `excess` = the sum of clahe_over() over the bins.
MI_BLUR_HD inline uint32_t clahe_bin(uint32_t h, uint32_t clip, uint32_t excess, int v)
{
    const uint32_t residual = excess % MI_BLUR_HIST_BINS;
    uint32_t r = (h < clip ? h : clip) + excess / MI_BLUR_HIST_BINS;
    if (residual) {
        const uint32_t q = MI_BLUR_HIST_BINS / residual, step = q < 1 ? 1u : q;
        if ((uint32_t)v % step == 0 && (uint32_t)v / step < residual) r++;
    }
    return r;
}
// lut[v] from c(v) and the area: 255 c / A rounded once, half up.
MI_BLUR_HD inline uint8_t clahe_entry(uint64_t cv, uint64_t A)
{
    if (A < (1u << 22)) return (uint8_t)((510u * (uint32_t)cv + (uint32_t)A) / (2u * (uint32_t)A));     // the same value in 32 bits: cv <= A
    return (uint8_t)((510u * cv + A) / (2u * A));
}
// One table from one histogram whose bins sum to A > 0.
inline void clahe_table(const uint32_t *hist, uint32_t A, int clip_q8, uint8_t *lut)
{
    const uint32_t clip = clahe_clip(A, clip_q8);
    uint64_t excess = 0, run = 0;
    for (int v = 0; v < MI_BLUR_HIST_BINS; v++) excess += clahe_over(hist[v], clip);
    for (int v = 0; v < MI_BLUR_HIST_BINS; v++) {
        run += clahe_bin(hist[v], clip, (uint32_t)excess, v);
        lut[v] = clahe_entry(run, A);
    }
}
inline size_t clahe_tables_of(int n_images, const mi_blur_clahe &k, int C) { return (size_t)n_images * (size_t)k.tiles_y * (size_t)k.tiles_x * (size_t)C; }

// ---- two-image arithmetic (include/mi_blur.h, "Two-image arithmetic").  The host export mi_blur_arith_value, the CPU
// device and all three kernels take an output byte from arith_byte(); the tiled kernels call it with a constant op.
constexpr int32_t ARITH_MAX_W = 1 << 16, ARITH_MAX_W_MUL = 1 << 10, ARITH_MAX_BIAS = 1 << 26;
constexpr int ARITH_MAX_SHIFT = 16;
inline bool arith_ok(const mi_blur_arith *k)
{
    if (!k) return false;
    const auto flag = [](int f) { return f == 0 || f == 1; };
    const auto within = [](int32_t v, int32_t lim) { return v >= -lim && v <= lim; };
    if (!flag(k->b_plane) || !flag(k->b_shared) || !flag(k->m_plane) || !flag(k->m_shared)) return false;
    if (k->op != MI_BLUR_ARITH_LERP && (k->m_plane || k->m_shared)) return false;
    switch (k->op) {
    case MI_BLUR_ARITH_LINEAR:
        return within(k->wa, ARITH_MAX_W) && within(k->wb, ARITH_MAX_W) && within(k->bias, ARITH_MAX_BIAS) && k->shift >= 0 && k->shift <= ARITH_MAX_SHIFT;
    case MI_BLUR_ARITH_ABSDIFF:
    case MI_BLUR_ARITH_MUL:
        return within(k->wa, k->op == MI_BLUR_ARITH_MUL ? ARITH_MAX_W_MUL : ARITH_MAX_W) && k->wb == 0 && within(k->bias, ARITH_MAX_BIAS) &&
               k->shift >= 0 && k->shift <= ARITH_MAX_SHIFT;
    case MI_BLUR_ARITH_MIN:
    case MI_BLUR_ARITH_MAX:
    case MI_BLUR_ARITH_LERP:
        return k->wa == 0 && k->wb == 0 && k->bias == 0 && k->shift == 0;
    default:
        return false;
    }
}
// w * v for |w| <= 2^16 and 0 <= v <= 65025.  Both fit a signed 24-bit operand; the sign extension from bit 23 changes
// no valid w and lets the device compiler see that, so it takes v_mad_i32_i24 (v comes from bytes, which it sees itself).
MI_BLUR_HD inline int32_t arith_mul(int32_t w, int32_t v) { return ((int32_t)((uint32_t)w << 8) >> 8) * v; }
// floor((2 t + 255) / 510) for t = a * m + b * (255 - m) <= 65025, as (257 t + 32896) >> 16 (< 2^24 before the shift).
MI_BLUR_HD inline int arith_lerp(int a, int b, int m) { return (arith_mul(257, arith_mul(a, m) + arith_mul(b, 255 - m)) + 32896) >> 16; }
// The output byte of a valid struct's fields for the operand bytes a, b, m.  The shift and the clamp are color_clamp(),
// which keeps them apart on the device.
MI_BLUR_HD inline int arith_byte(int op, int32_t wa, int32_t wb, int32_t bias, int shift, int a, int b, int m)
{
    switch (op) {
    case MI_BLUR_ARITH_LINEAR: return color_clamp(arith_mul(wa, a) + arith_mul(wb, b) + bias, shift);
    case MI_BLUR_ARITH_ABSDIFF: return color_clamp(arith_mul(wa, a > b ? a - b : b - a) + bias, shift);
    case MI_BLUR_ARITH_MIN: return a < b ? a : b;
    case MI_BLUR_ARITH_MAX: return a > b ? a : b;
    case MI_BLUR_ARITH_MUL: return color_clamp(arith_mul(wa, arith_mul(a, b)) + bias, shift);
    default: return arith_lerp(a, b, m);
    }
}
// The flags as the launches see them: a plane of a one-channel image is a full operand, a shared operand of one image
// is its own.
inline mi_blur_arith arith_normalised(const mi_blur_arith &k, int C, int n_images)
{
    mi_blur_arith r = k;
    if (C == 1) r.b_plane = r.m_plane = 0;
    if (n_images <= 1) r.b_shared = r.m_shared = 0;
    return r;
}
// Bytes of one image of an operand and of the whole operand.
inline long long arith_image_bytes(int W, int H, int C, int plane) { return (long long)W * H * (plane ? 1 : C); }
inline long long arith_operand_bytes(int W, int H, int C, int n_images, int plane, int shared) { return arith_image_bytes(W, H, C, plane) * (shared ? 1 : n_images); }
// "Aliasing": the output may be A, and B where B has the output's extent; no other overlap with an operand.
inline bool arith_alias_ok(const uint8_t *a, const uint8_t *b, const uint8_t *m, const uint8_t *out, int W, int H, int C, int n_images, const mi_blur_arith &k)
{
    const mi_blur_arith q = arith_normalised(k, C, n_images);
    const uintptr_t o0 = (uintptr_t)out, ob = (uintptr_t)arith_operand_bytes(W, H, C, n_images, 0, 0);
    const auto apart = [&](const uint8_t *p, long long bytes) { return (uintptr_t)p + (uintptr_t)bytes <= o0 || o0 + ob <= (uintptr_t)p; };
    if (ob == 0) return true;
    if (a != out && !apart(a, (long long)ob)) return false;
    if (!(b == out && !q.b_plane && !q.b_shared) && !apart(b, arith_operand_bytes(W, H, C, n_images, q.b_plane, q.b_shared))) return false;
    return !m || apart(m, arith_operand_bytes(W, H, C, n_images, q.m_plane, q.m_shared));
}
// Every argument of the three entry points but the device: the pointers, the image, the struct and the aliasing.
inline bool arith_args_ok(const uint8_t *a, const uint8_t *b, const uint8_t *m, const uint8_t *out, int W, int H, int C, int n_images, const mi_blur_arith *k)
{
    if (!a || !b || !out || n_images < 0 || !arith_ok(k) || !hist_image_ok(W, H, C)) return false;
    if ((k->op == MI_BLUR_ARITH_LERP) != (m != nullptr)) return false;
    return arith_alias_ok(a, b, m, out, W, H, C, n_images, *k);
}

// ---- integral images and the box filters made from them (include/mi_blur.h, "Integral images, and box filters").  The
// host export mi_blur_box_value, the CPU device and both consumer kernels take a window's sum from box_axis() /
// box_window() and an output byte from box_byte(); the tiled kernel calls box_byte() with a constant op and, in the
// interior, with the sum of its own four reads.
inline bool box_ok(const mi_blur_box *k)
{
    if (!k || k->op < MI_BLUR_BOX_MEAN || k->op > MI_BLUR_BOX_THRESHOLD) return false;
    if (k->rx < 0 || k->rx > MI_BLUR_BOX_MAX_RADIUS || k->ry < 0 || k->ry > MI_BLUR_BOX_MAX_RADIUS) return false;
    if (k->op != MI_BLUR_BOX_THRESHOLD) return k->offset == 0 && k->invert == 0;
    return k->offset >= -255 && k->offset <= 255 && (k->invert == 0 || k->invert == 1);
}
inline int box_tables(const mi_blur_box &k) { return k.op == MI_BLUR_BOX_STDDEV ? 2 : 1; }
// The five terms of one axis at position X (extent N, radius r): the clamped sum is the sum of coef[t] * F(idx[t]).  A
// term that the definition skips (coefficient 0, or a read at -1) has coef 0 and idx 0.
struct BoxAxis { int idx[5]; int coef[5]; };
MI_BLUR_HD inline BoxAxis box_axis(int X, int N, int r)
{
    const int a = X - r > 0 ? X - r : 0, b = X + r < N - 1 ? X + r : N - 1;
    const int e0 = r - X > 0 ? r - X : 0, e1 = X + r - (N - 1) > 0 ? X + r - (N - 1) : 0;
    BoxAxis q;
    q.idx[0] = b; q.coef[0] = 1;
    q.idx[1] = a > 0 ? a - 1 : 0; q.coef[1] = a > 0 ? -1 : 0;
    q.idx[2] = 0; q.coef[2] = e0;
    q.idx[3] = N - 1; q.coef[3] = e1;
    q.idx[4] = N > 1 ? N - 2 : 0; q.coef[4] = N > 1 ? -e1 : 0;
    return q;
}
// Sum (or SumSq) of the window around (X, Y) in channel c of one image's table T = uint32[H][W][C], in uint32.
MI_BLUR_HD inline uint32_t box_window(const uint32_t *T, int W, int H, int C, int X, int Y, int c, int rx, int ry)
{
    const BoxAxis ax = box_axis(X, W, rx), ay = box_axis(Y, H, ry);
    uint32_t s = 0;
    for (int j = 0; j < 5; j++) {
        if (!ay.coef[j]) continue;
        const uint32_t *row = T + (size_t)ay.idx[j] * W * C + c;
        uint32_t t = 0;
        for (int i = 0; i < 5; i++)
            if (ax.coef[i]) t += (uint32_t)ax.coef[i] * row[(size_t)ax.idx[i] * C];
        s += (uint32_t)ay.coef[j] * t;
    }
    return s;
}
// floor(n / d) for n < 2^26 and 2 <= d <= 2^17 with inv = 1.0f / d: the float estimate is within 1 of the quotient
// (n / d <= 2^25 only matters below 2^23: here the quotient is at most 256), the exact remainder corrects it.
MI_BLUR_HD inline uint32_t box_div(uint32_t n, uint32_t d, float inv)
{
    uint32_t q = (uint32_t)((float)n * inv);
    const int32_t r = (int32_t)(n - q * d);
    if (r < 0) q--;
    else if ((uint32_t)r >= d) q++;
    return q;
}
// sqrt(D) / A rounded half up for D < 2^49, as the largest s in 0..128 with s == 0 or (2 s - 1)^2 A^2 <= 4 D: the
// double estimate, then the exact comparison either way ((2 * 128 + 1)^2 * 65025^2 < 2^49).
MI_BLUR_HD inline int box_root(uint64_t D, uint32_t A, double inv_a)
{
    const uint64_t a2 = (uint64_t)A * A, d4 = 4u * D;
    int s = (int)(sqrt((double)D) * inv_a + 0.5);
    s = s < 0 ? 0 : s > 128 ? 128 : s;
    while (s > 0 && (uint64_t)((2 * s - 1) * (2 * s - 1)) * a2 > d4) s--;
    while (s < 128 && (uint64_t)((2 * s + 1) * (2 * s + 1)) * a2 <= d4) s++;
    return s;
}
// What a launch derives from A once.
struct BoxConst { uint32_t A; float inv_2a; double inv_a; };
inline BoxConst box_const(const mi_blur_box &k)
{
    BoxConst q;
    q.A = (uint32_t)((2 * k.rx + 1) * (2 * k.ry + 1));
    q.inv_2a = 1.0f / (float)(2u * q.A);
    q.inv_a = 1.0 / (double)q.A;
    return q;
}
// The output byte of a valid struct's fields for a window's sums and the centre byte a.
MI_BLUR_HD inline int box_byte(int op, int offset, int invert, uint32_t A, float inv_2a, double inv_a, uint32_t sum, uint32_t sqsum, int a)
{
    switch (op) {
    case MI_BLUR_BOX_MEAN: return (int)box_div(2u * sum + A, 2u * A, inv_2a);
    case MI_BLUR_BOX_STDDEV: return box_root((uint64_t)A * sqsum - (uint64_t)sum * sum, A, inv_a);
    default: return ((int32_t)A * (a + offset) > (int32_t)sum) != (invert != 0) ? 255 : 0;
    }
}
// Every argument of the integral's entry points but the work buffer and the device; `align` = 16 on the device, 4 on
// the host.
inline bool integral_args_ok(const void *in, const void *sum, const void *sqsum, int W, int H, int C, int n_images, uintptr_t align)
{
    if (!in || (!sum && !sqsum) || n_images < 0 || !hist_image_ok(W, H, C)) return false;
    return (uintptr_t)sum % align == 0 && (uintptr_t)sqsum % align == 0;
}
// ... and of mi_blur_enqueue_box_from_integral: S always, Q exactly for STDDEV, the images exactly for THRESHOLD.
inline bool box_from_args_ok(const void *in, const void *sum, const void *sqsum, const void *out, int W, int H, int C, int n_images, const mi_blur_box *k)
{
    if (!sum || !out || n_images < 0 || !box_ok(k) || !hist_image_ok(W, H, C)) return false;
    if ((k->op == MI_BLUR_BOX_STDDEV) != (sqsum != nullptr) || (k->op == MI_BLUR_BOX_THRESHOLD) != (in != nullptr)) return false;
    return (uintptr_t)sum % 16 == 0 && (uintptr_t)sqsum % 16 == 0;
}
// ... and of the forms that make their own tables.
inline bool box_args_ok(const void *in, const void *out, int W, int H, int C, int n_images, const mi_blur_box *k)
{
    return in && out && n_images >= 0 && box_ok(k) && hist_image_ok(W, H, C);
}

// ---- distance transform (include/mi_blur.h, "Exact distance transform").  The host export mi_blur_dist_value, the CPU
// device and both row-pass kernels take a candidate from dist_cand(), the value a search starts from and ends with from
// dist_start() / dist_final(), the search itself from dist_search() / dist_search_plain() and a byte from dist_byte().
// g, the column distance, is 16 bits: 0..32767, or DIST_G_NONE, which is never squared or added: every use selects on it.
constexpr uint32_t DIST_G_NONE = 0xFFFFu;
constexpr int DIST_G_MAX = 32767;                   // H <= 32768
// bytes: the struct of a byte call; otherwise of a table call, where byte_op and invert are unused.
inline bool dist_ok(const mi_blur_dist *k, bool bytes)
{
    if (!k || k->metric < MI_BLUR_DIST_L2 || k->metric > MI_BLUR_DIST_LINF) return false;
    if ((k->sites_nonzero != 0 && k->sites_nonzero != 1) || k->limit < 0 || k->limit > MI_BLUR_DIST_MAX_LIMIT) return false;
    if (!bytes || k->byte_op == MI_BLUR_DIST_BYTE) return k->byte_op == MI_BLUR_DIST_BYTE && k->invert == 0;
    return k->byte_op == MI_BLUR_DIST_WITHIN && k->limit >= 1 && (k->invert == 0 || k->invert == 1);
}
// The candidate a site dx columns away offers through its column distance g (dx, g <= 32767, g not the marker): at most
// 2 * 32767^2 < 2^31, in unsigned arithmetic throughout.
template <int METRIC>
MI_BLUR_HD inline uint32_t dist_cand(uint32_t dx, uint32_t g)
{
    if (METRIC == MI_BLUR_DIST_L2) return dx * dx + g * g;
    if (METRIC == MI_BLUR_DIST_L1) return dx + g;
    return dx > g ? dx : g;
}
MI_BLUR_HD inline uint32_t dist_cand(int metric, uint32_t dx, uint32_t g)
{
    return metric == MI_BLUR_DIST_L2 ? dist_cand<MI_BLUR_DIST_L2>(dx, g) : metric == MI_BLUR_DIST_L1 ? dist_cand<MI_BLUR_DIST_L1>(dx, g) : dist_cand<MI_BLUR_DIST_LINF>(dx, g);
}
// The largest T any image gives.
inline uint32_t dist_max(int metric) { return dist_cand(metric, DIST_G_MAX, DIST_G_MAX); }
// A search starts from the first value beyond the limit (limit^2 + 1 <= 32767^2 + 1 fits) and only smaller candidates
// replace it; what is left at the end is T, or NONE if nothing did.
MI_BLUR_HD inline uint32_t dist_start(int metric, int limit) { return limit ? dist_cand(metric, (uint32_t)limit, 0u) + 1u : MI_BLUR_DIST_NONE; }
MI_BLUR_HD inline uint32_t dist_final(uint32_t best, uint32_t start) { return best < start ? best : MI_BLUR_DIST_NONE; }
// What the column pass stores for a column distance d (or the marker): with a limit, anything above it offers nothing.
MI_BLUR_HD inline uint32_t dist_g_cap(uint32_t d, uint32_t cap) { return d > cap ? DIST_G_NONE : d; }
inline uint32_t dist_cap(int limit) { return limit ? (uint32_t)limit : (uint32_t)DIST_G_MAX; }
// T over one row from a PLANE of g: the row's g of one channel, x-major, padded with the marker to nch whole chunks of
// CHUNK columns, and cm[ch] = the minimum of chunk ch.  First the columns nearer than CHUNK, one dx at a time on both
// sides: where sites are dense the search ends there, after a few reads.  That covers x's own chunk; then the other
// chunks outwards, left and right in turn: a side ends when its chunk's nearest dx alone cannot beat `best`, a chunk is
// skipped when its minimum cannot.  At most CHUNK + nch steps.
template <int METRIC, int CHUNK>
MI_BLUR_HD inline uint32_t dist_search(const uint16_t *g, const uint16_t *cm, int nch, int x, uint32_t start)
{
    const int cx = x / CHUNK, wp = nch * CHUNK;
    uint32_t best = start;
    for (int dx = 0; dx < CHUNK; dx++) {
        if (dist_cand<METRIC>((uint32_t)dx, 0u) >= best) return best;
        const uint32_t gl = x - dx >= 0 ? g[x - dx] : DIST_G_NONE, gr = x + dx < wp ? g[x + dx] : DIST_G_NONE;
        const uint32_t gg = gl < gr ? gl : gr;                         // the same dx: the smaller g offers the smaller candidate
        const uint32_t v = gg == DIST_G_NONE ? MI_BLUR_DIST_NONE : dist_cand<METRIC>((uint32_t)dx, gg);
        best = v < best ? v : best;
    }
    for (int k = 1; k < nch; k++) {
        bool open = false;
        for (int side = 0; side < 2; side++) {
            const int ch = side ? cx + k : cx - k;
            if (ch < 0 || ch >= nch) continue;
            const int x0 = ch * CHUNK;
            const uint32_t near = side ? (uint32_t)(x0 - x) : (uint32_t)(x - (x0 + CHUNK - 1));
            if (dist_cand<METRIC>(near, 0u) >= best) continue;
            open = true;
            const uint32_t m = cm[ch];
            if (m == DIST_G_NONE || dist_cand<METRIC>(near, m) >= best) continue;
            const uint16_t *q = g + x0;
#pragma unroll
            for (int j = 0; j < CHUNK; j++) {
                const uint32_t gg = q[j];
                const uint32_t dx = (uint32_t)(x0 + j > x ? x0 + j - x : x - (x0 + j));
                const uint32_t v = gg == DIST_G_NONE ? MI_BLUR_DIST_NONE : dist_cand<METRIC>(dx, gg);
                best = v < best ? v : best;
            }
        }
        if (!open) break;
    }
    return best;
}
// The same from g as it lies in memory (entry x of the row and channel at g[x * stride]), without minima: dx outwards,
// both sides in step, until dx alone cannot beat `best` or both sides have left the row.  At most W steps.
template <int METRIC>
MI_BLUR_HD inline uint32_t dist_search_plain(const uint16_t *g, int stride, int W, int x, uint32_t start)
{
    uint32_t best = start;
    for (int dx = 0; dx < W; dx++) {
        const int xl = x - dx, xr = x + dx;
        if (dist_cand<METRIC>((uint32_t)dx, 0u) >= best || (xl < 0 && xr >= W)) break;
        if (xl >= 0) {
            const uint32_t gg = g[(size_t)xl * stride];
            const uint32_t v = gg == DIST_G_NONE ? MI_BLUR_DIST_NONE : dist_cand<METRIC>((uint32_t)dx, gg);
            best = v < best ? v : best;
        }
        if (dx && xr < W) {
            const uint32_t gg = g[(size_t)xr * stride];
            const uint32_t v = gg == DIST_G_NONE ? MI_BLUR_DIST_NONE : dist_cand<METRIC>((uint32_t)dx, gg);
            best = v < best ? v : best;
        }
    }
    return best;
}
// sqrt(T) rounded half up, capped at 255: the largest s with s == 0 or (2 s - 1)^2 <= 4 T.  509^2 <= 4 T from T = 64771
// on; below that T is exact as a float and its root is within 2^-15 of the float root, so the estimate is the answer or
// one off it, and one exact comparison either way settles it (no loop: the kernels take four roots a thread).
MI_BLUR_HD inline int dist_root(uint32_t T)
{
    if (T >= 64771u) return 255;
    int s = (int)(sqrtf((float)T) + 0.5f);
    s -= s > 0 && (uint32_t)((2 * s - 1) * (2 * s - 1)) > 4u * T;
    s += (uint32_t)((2 * s + 1) * (2 * s + 1)) <= 4u * T;
    return s;
}
// The byte of a valid byte struct's fields for the table value T.
MI_BLUR_HD inline int dist_byte(int metric, int byte_op, int invert, uint32_t T)
{
    if (byte_op == MI_BLUR_DIST_WITHIN) return (T != MI_BLUR_DIST_NONE) != (invert != 0) ? 255 : 0;
    if (T == MI_BLUR_DIST_NONE) return 255;
    if (metric == MI_BLUR_DIST_L2) return dist_root(T);
    return T > 255u ? 255 : (int)T;
}
// Every argument of the family's entry points but the work buffer and the device; `align` of the table = 16 on the
// device, 4 on the host.  The byte form may be written over the input; no other overlap of the two.
inline bool dist_args_ok(const uint8_t *in, const void *out, int W, int H, int C, int n_images, const mi_blur_dist *k, bool bytes, uintptr_t align)
{
    if (!in || !out || n_images < 0 || !dist_ok(k, bytes) || !hist_image_ok(W, H, C)) return false;
    if (!bytes) return (uintptr_t)out % align == 0;
    const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out, size = (uintptr_t)W * H * C * (uintptr_t)n_images;
    return i0 == o0 || i0 + size <= o0 || o0 + size <= i0;
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
// whole_image_only: the output image is not the input's size or channel count, so the filter takes whole images only: no
// bands, no halo rows, no planar or resident forms (a band's phase or source rows would depend on where it starts, and a
// band of another channel count has no place in those forms).
inline bool whole_image_only(const Filter &f)
{
    return f.kind == FilterKind::SEP_DOWN || f.kind == FilterKind::RESIZE || f.kind == FilterKind::WARP || f.kind == FilterKind::WARP_PERSP ||
           f.kind == FilterKind::REMAP || f.kind == FilterKind::AREA || f.kind == FilterKind::COLOR;
}
// Width, rows and channels of the output block of one band of band_rows rows x W x C of which rows [y0, y1) are asked
// for: those rows at the input's width, or the filter's own output image (of the whole band) for a whole_image_only
// filter.  The channels are the input's for every filter but COLOR, whose output has its own count.
struct OutShape { int width, rows, channels; };
inline OutShape out_shape(const Filter &f, int W, int band_rows, int C, int y0, int y1)
{
    if (f.kind == FilterKind::SEP_DOWN) return {down_cols(W, f.down_sx, f.down_ox), down_rows(band_rows, f.down_sy, f.down_oy), C};
    if (f.kind == FilterKind::RESIZE || f.kind == FilterKind::WARP || f.kind == FilterKind::WARP_PERSP || f.kind == FilterKind::REMAP || f.kind == FilterKind::AREA) return {f.out_w, f.out_h, C};
    if (f.kind == FilterKind::COLOR) return {W, band_rows, f.color.co};
    return {W, y1 - y0, C};
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
    f->out_w = r->out_width; f->out_h = r->out_height; f->sample_mode = r->mode;
    return MI_BLUR_OK;
}

// The target size, mode, border and map of *w (the image size is checked where it is known: warp_ok()).
inline int filter_warp(const mi_blur_warp *w, Filter *f)
{
    if (!f || !warp_ok(w, 1, 1, 1)) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::WARP, 0, {}};
    f->out_w = w->out_width; f->out_h = w->out_height; f->sample_mode = w->mode; f->warp_border = w->border; f->warp_fill = w->fill;
    for (int i = 0; i < 6; i++) f->warp_m[i] = w->m[i];
    return MI_BLUR_OK;
}

// The target size, mode, border and homography of *w (the image size is checked where it is known: persp_ok()).
inline int filter_warp_persp(const mi_blur_warp_perspective *w, Filter *f)
{
    if (!f || !persp_ok(w, 1, 1, 1)) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::WARP_PERSP, 0, {}};
    f->out_w = w->out_width; f->out_h = w->out_height; f->sample_mode = w->mode; f->warp_border = w->border; f->warp_fill = w->fill;
    for (int i = 0; i < 9; i++) f->warp_h[i] = w->h[i];
    return MI_BLUR_OK;
}

// The target size, mode, border and staging limit of *r and the table `map` (not copied; the image size is checked where
// it is known: remap_ok()).
inline int filter_remap(const mi_blur_remap *r, const int32_t *map, Filter *f)
{
    if (!f || !map || !remap_ok(r, 1, 1, 1)) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::REMAP, 0, {}};
    f->out_w = r->out_width; f->out_h = r->out_height; f->sample_mode = r->mode; f->warp_border = r->border; f->warp_fill = r->fill;
    f->remap_map = map; f->remap_stage_bytes = r->stage_bytes ? r->stage_bytes : REMAP_STAGE_MAX;
    return MI_BLUR_OK;
}

// The target size of *r (the image size, and with it the ratio, is checked where it is known: area_ok()).
inline int filter_area(const mi_blur_area *r, Filter *f)
{
    if (!f || !area_ok(r, 1, 1, 1)) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::AREA, 0, {}};
    f->out_w = r->out_width; f->out_h = r->out_height;
    return MI_BLUR_OK;
}

// *k, copied: rows beyond out_channels as zeros, the tables only when lut_on (what the image must satisfy is checked
// where it is known: color_image_ok()).
inline int filter_color(const mi_blur_color *k, Filter *f)
{
    if (!f || !color_ok(k)) return MI_BLUR_ERR_INVALID;
    *f = Filter{FilterKind::COLOR, 0, {}};
    ColorSpec &c = f->color;
    c.co = k->out_channels; c.shift = k->shift; c.lut_on = k->lut_on;
    for (int o = 0; o < c.co; o++) {
        for (int i = 0; i < 4; i++) c.m[o][i] = k->m[o][i];
        c.bias[o] = k->bias[o];
        if (c.lut_on) for (int v = 0; v < 256; v++) c.lut[o][v] = k->lut[o][v];
    }
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

// ---- Tile geometry of the tiled kernels, and the LDS arithmetic of the two that stage a footprint they compute
// (blur_resize_tiled_kernel, blur_warp_tiled_kernel).  The kernels index their LDS with these functions and the host sizes
// it with the same ones, walking the tiles of a launch, so the two agree by construction; tests/san_tile_bounds.cpp
// walks them again on the CPU under sanitizers and checks every position against the size.
constexpr int TILE_TH = 32;         // rows per tile
constexpr int TILE_NCOLS = 32;      // at most this many 16-byte chunk columns per tile

// Rows of cpr chunks x `rows` rows cut into tiles: strips of whole units of `unit` chunks, at most max_units of them,
// all strips but the last equally wide; TILE_TH rows.  kernel_common.h: fill_tiles() hands it to the kernels, whose
// tile_coords() gives block L the tile tile_at(g, rows, L % nstrips, L / nstrips % ntiles_y).
struct TileGrid { int cpr, nstrips, ncols, ntiles_y; };
inline TileGrid tile_grid(int cpr, int rows, int unit = 1, int max_units = TILE_NCOLS)
{
    const int units = cpr / unit, nstrips = (units + max_units - 1) / max_units;
    return {cpr, nstrips, unit * ((units + nstrips - 1) / nstrips), (rows + TILE_TH - 1) / TILE_TH};
}
struct Tile { int ty0, rows_out, x0c, nc; };      // first row and rows, first chunk column and chunk columns
inline Tile tile_at(const TileGrid &g, int rows, int strip, int ty)
{
    const int ty0 = ty * TILE_TH, x0c = strip * g.ncols;
    return {ty0, rows - ty0 < TILE_TH ? rows - ty0 : TILE_TH, x0c, g.cpr - x0c < g.ncols ? g.cpr - x0c : g.ncols};
}
// The pixels of C bytes that begin in chunks [x0c, x0c + nc) (all of the pixels of a strip that starts and ends on
// one), and the 16-byte chunks that hold pixels x0..x1.  A tile stages rows r.lo..r.hi of chunks sc.lo..sc.hi of the
// input, row after row: slot (row - r.lo) * sc.n() + (chunk - sc.lo).
struct Span { int lo, hi; MI_BLUR_HD int n() const { return hi - lo + 1; } };
MI_BLUR_HD inline Span tile_pixels(int x0c, int nc, int C) { return {(x0c * 16) / C, ((x0c + nc) * 16 - 1) / C}; }
MI_BLUR_HD inline Span chunk_span(int x0, int x1, int C) { return {(x0 * C) >> 4, (x1 * C + C - 1) >> 4}; }

// ---- blur_resize_tiled_kernel.  LDS: the x table (one dword per output byte of a tile row), the y table (one per output
// row), the staged box, then RS_GROUP V rows of one dword per staged byte of a row.  a and b of resize_axis are clamped
// already, so the box lies inside the image.
constexpr int RS_GROUP = 8;                         // output rows per pass
constexpr int RS_XTAB = TILE_NCOLS * 16 * 4;        // bytes of the x table
constexpr int RS_YTAB = TILE_TH * 4;                // bytes of the y table
MI_BLUR_HD inline Span resize_stage_rows(int H, int Ho, int ty0, int rows_out)
{
    return {resize_axis(H, Ho, MI_BLUR_RESIZE_BILINEAR, ty0).a, resize_axis(H, Ho, MI_BLUR_RESIZE_BILINEAR, ty0 + rows_out - 1).b};
}
MI_BLUR_HD inline Span resize_stage_chunks(int W, int Wo, int C, int x0c, int nc)
{
    const Span px = tile_pixels(x0c, nc, C);
    return chunk_span(resize_axis(W, Wo, MI_BLUR_RESIZE_BILINEAR, px.lo).a, resize_axis(W, Wo, MI_BLUR_RESIZE_BILINEAR, px.hi).b, C);
}
// x table entry of channel c of an output pixel with the coordinate rc: the V dword position of input byte (a, c) |
// that of (b, c) << 10 | f << 20, the position of staged byte q being plane (q >> 2) & 3, chunk q >> 4, byte q & 3 (a V
// row is 4 planes of nsc x 4 dwords).  y table entry of an output row: the staged rows a - r0 | b - r0 << 8 | f << 16.
// Positions below 1024 (nsc <= 64) and rows below 256 are what the fields hold: resize_tiles_fit().
MI_BLUR_HD inline uint32_t resize_v_pos(int q, int nsc) { return (uint32_t)(((q >> 2) & 3) * nsc * 4 + (q >> 4) * 4 + (q & 3)); }
MI_BLUR_HD inline uint32_t resize_x_entry(const ResizeCoord &rc, int C, int c, int sc0, int nsc)
{
    return resize_v_pos(rc.a * C + c - sc0 * 16, nsc) | (resize_v_pos(rc.b * C + c - sc0 * 16, nsc) << 10) | ((uint32_t)rc.f << 20);
}
MI_BLUR_HD inline uint32_t resize_x_pos_a(uint32_t e) { return e & 1023u; }
MI_BLUR_HD inline uint32_t resize_x_pos_b(uint32_t e) { return (e >> 10) & 1023u; }
MI_BLUR_HD inline uint32_t resize_x_f(uint32_t e) { return e >> 20; }
MI_BLUR_HD inline uint32_t resize_y_entry(const ResizeCoord &rc, int r0) { return (uint32_t)(rc.a - r0) | ((uint32_t)(rc.b - r0) << 8) | ((uint32_t)rc.f << 16); }
MI_BLUR_HD inline uint32_t resize_y_row_a(uint32_t e) { return e & 0xffu; }
MI_BLUR_HD inline uint32_t resize_y_row_b(uint32_t e) { return (e >> 8) & 0xffu; }
MI_BLUR_HD inline uint32_t resize_y_f(uint32_t e) { return e >> 16; }
// The largest box of a launch, per axis (rows depend on the tile row only, chunks on the strip), whether the table fields
// hold it (an enlargement stays far inside: at most 34 rows x 35 chunks; else the generic kernel), and the LDS it takes.
struct ResizeTiles { int max_nsc, max_nsr; };
inline ResizeTiles resize_tiles(const TileGrid &g, int W, int H, int Wo, int Ho, int C)
{
    ResizeTiles t{1, 1};
    for (int s = 0; s < g.nstrips; s++) {
        const Tile tl = tile_at(g, Ho, s, 0);
        const Span sc = resize_stage_chunks(W, Wo, C, tl.x0c, tl.nc);
        if (sc.n() > t.max_nsc) t.max_nsc = sc.n();
    }
    for (int ty = 0; ty < g.ntiles_y; ty++) {
        const Tile tl = tile_at(g, Ho, 0, ty);
        const Span r = resize_stage_rows(H, Ho, tl.ty0, tl.rows_out);
        if (r.n() > t.max_nsr) t.max_nsr = r.n();
    }
    return t;
}
inline bool resize_tiles_fit(const ResizeTiles &t) { return t.max_nsc <= 64 && t.max_nsr <= 255; }
inline int resize_v_off(const ResizeTiles &t) { return RS_XTAB + RS_YTAB + t.max_nsr * t.max_nsc * 16; }       // LDS byte offset of the V rows
inline size_t resize_lds_bytes(const ResizeTiles &t) { return (size_t)resize_v_off(t) + (size_t)RS_GROUP * t.max_nsc * 64u; }

// ---- blur_warp_tiled_kernel.  LDS: the staged box alone, then WARP_LDS_SLACK bytes.  A tile is at most WARP_TILE_PX
// output pixels wide, in strips of whole units: the smallest run of chunks that starts and ends on a pixel.
constexpr int WARP_TILE_PX = 64;
constexpr int warp_unit(int C) { return C == 3 ? 3 : 1; }
constexpr int warp_max_cols(int C) { return WARP_TILE_PX * C / 16; }
inline TileGrid warp_grid(int cpr, int Ho, int C) { return tile_grid(cpr, Ho, warp_unit(C), warp_max_cols(C) / warp_unit(C)); }
// The input pixels a tile's taps can touch (warp_footprint() of its pixels) and whether they miss the image (CONSTANT
// only: the tile is `fill`).  The box lies inside the image; rows b.y0..b.y1 of chunk_span(b.x0, b.x1, C) are staged.
MI_BLUR_HD inline WarpBox warp_tile_box(const int64_t *m, int border, int W, int H, int C, int ty0, int rows_out, int x0c, int nc)
{
    const Span px = tile_pixels(x0c, nc, C);
    return warp_footprint(m, MI_BLUR_RESIZE_BILINEAR, border, W, H, px.lo, px.hi, ty0, ty0 + rows_out - 1);
}
MI_BLUR_HD inline bool warp_box_empty(const WarpBox &b) { return b.x0 > b.x1 || b.y0 > b.y1; }
// The taps of a position whose first tap is pixel (x0, y0), clamped into the box b: under CLAMP that is the clamp into
// the image, under CONSTANT a tap the clamp moves lies outside the image and the kernel replaces it.  off_a, off_b: the
// LDS byte offsets of pixel xa on rows ya and yb; the tap at xb is the pixel behind it, or the same pixel (`one`) where
// the clamp met the edge of the box.  The kernel reads warp_read_bytes(C) bytes from the 4-byte aligned address at or
// below each offset: at most 11 bytes past the start of a pixel inside the box, which WARP_LDS_SLACK keeps inside the LDS.
struct WarpTap { int off_a, off_b; bool one; };
MI_BLUR_HD inline int clamp_int(int v, int lo, int hi) { const int u = v > lo ? v : lo; return u < hi ? u : hi; }   // min(max(v, lo), hi)
MI_BLUR_HD inline WarpTap warp_tap(const WarpBox &b, const Span &sc, int C, int x0, int y0)
{
    const int xa = clamp_int(x0, b.x0, b.x1), xb = clamp_int(x0 + 1, b.x0, b.x1);
    const int ya = clamp_int(y0, b.y0, b.y1), yb = clamp_int(y0 + 1, b.y0, b.y1);
    const int rowb = sc.n() * 16, col0 = sc.lo * 16;               // bytes of a staged row; image byte column of staged byte 0
    return {(ya - b.y0) * rowb - col0 + xa * C, (yb - b.y0) * rowb - col0 + xa * C, xb == xa};
}
constexpr int warp_read_bytes(int C) { return C == 3 ? 12 : 8; }
constexpr long long WARP_LDS_SLACK = 16;            // LDS behind the staged box that the tap reads may touch
constexpr long long WARP_LDS_MAX = 65536 - WARP_LDS_SLACK;   // largest box: with the slack, the dynamic LDS a launch may ask for without raising the limit
// LDS bytes of the largest box of a launch (the walk stops at the first one over WARP_LDS_MAX: the launch is not admitted).
inline long long warp_tiles_max_bytes(const TileGrid &g, const int64_t *m, int border, int W, int H, int Ho, int C)
{
    long long max_bytes = 0;
    for (int ty = 0; ty < g.ntiles_y && max_bytes <= WARP_LDS_MAX; ty++)
        for (int s = 0; s < g.nstrips; s++) {
            const Tile tl = tile_at(g, Ho, s, ty);
            const WarpBox b = warp_tile_box(m, border, W, H, C, tl.ty0, tl.rows_out, tl.x0c, tl.nc);
            if (warp_box_empty(b)) continue;
            const long long bytes = (long long)(b.y1 - b.y0 + 1) * chunk_span(b.x0, b.x1, C).n() * 16;
            max_bytes = bytes > max_bytes ? bytes : max_bytes;
        }
    return max_bytes;
}

// ---- blur_warp_persp_tiled_kernel: the tiles, the LDS layout, warp_tap() and the slack of blur_warp_tiled_kernel; the box
// of a tile comes from persp_footprint(), so boxes differ from tile to tile and the walk takes the largest.
MI_BLUR_HD inline WarpBox persp_tile_box(const int64_t *h, int border, int W, int H, int C, int ty0, int rows_out, int x0c, int nc)
{
    const Span px = tile_pixels(x0c, nc, C);
    return persp_footprint(h, MI_BLUR_RESIZE_BILINEAR, border, W, H, px.lo, px.hi, ty0, ty0 + rows_out - 1);
}
inline long long persp_tiles_max_bytes(const TileGrid &g, const int64_t *h, int border, int W, int H, int Ho, int C)
{
    long long max_bytes = 0;
    for (int ty = 0; ty < g.ntiles_y && max_bytes <= WARP_LDS_MAX; ty++)
        for (int s = 0; s < g.nstrips; s++) {
            const Tile tl = tile_at(g, Ho, s, ty);
            const WarpBox b = persp_tile_box(h, border, W, H, C, tl.ty0, tl.rows_out, tl.x0c, tl.nc);
            if (warp_box_empty(b)) continue;
            const long long bytes = (long long)(b.y1 - b.y0 + 1) * chunk_span(b.x0, b.x1, C).n() * 16;
            max_bytes = bytes > max_bytes ? bytes : max_bytes;
        }
    return max_bytes;
}

// ---- blur_remap_tiled_kernel: the tiles, warp_tap() and the slack of blur_warp_tiled_kernel.  The map lives in device
// memory, so the workgroup finds its box itself (remap_tile_box() is what its reduction computes) and decides per tile:
// empty (CONSTANT, `fill`), staged (the box takes at most stage_bytes of LDS) or direct (taps from global memory).
// LDS: REMAP_RED_BYTES of reduction words (4 waves x 4 extrema), then the staged box, then WARP_LDS_SLACK.
constexpr int REMAP_RED_BYTES = 64;
inline size_t remap_lds_bytes(int stage_bytes) { return (size_t)REMAP_RED_BYTES + (size_t)stage_bytes + (size_t)WARP_LDS_SLACK; }
// Whether the shape is the tiled kernel's (pointers and strides assumed aligned): BILINEAR, 1-4 channels, rows of whole chunks both sides.
inline bool remap_shape_tiled(int W, int C, int Wo, int mode)
{
    return mode == MI_BLUR_RESIZE_BILINEAR && C >= 1 && C <= 4 && (long long)W * C % 16 == 0 && (long long)Wo * C % 16 == 0;
}
// The box of the tile of output rows ty0 .. ty0 + rows_out - 1 x chunk columns x0c .. x0c + nc - 1, from the host's copy of the map.
inline WarpBox remap_tile_box(const int32_t *map, int border, int W, int H, int Wo, int C, int ty0, int rows_out, int x0c, int nc)
{
    const Span px = tile_pixels(x0c, nc, C);
    int x_lo = INT_MAX, x_hi = INT_MIN, y_lo = INT_MAX, y_hi = INT_MIN;
    for (int Y = ty0; Y < ty0 + rows_out; Y++)
        for (int X = px.lo; X <= px.hi; X++) {
            const int32_t *e = map + ((size_t)Y * (size_t)Wo + (size_t)X) * 2;
            const WarpCoord q = remap_coord(e[0], e[1], MI_BLUR_RESIZE_BILINEAR, W, H);
            x_lo = q.x0 < x_lo ? q.x0 : x_lo; x_hi = q.x0 > x_hi ? q.x0 : x_hi;
            y_lo = q.y0 < y_lo ? q.y0 : y_lo; y_hi = q.y0 > y_hi ? q.y0 : y_hi;
        }
    return remap_box(x_lo, x_hi, y_lo, y_hi, border, W, H);
}
inline long long remap_box_bytes(const WarpBox &b, int C) { return (long long)(b.y1 - b.y0 + 1) * chunk_span(b.x0, b.x1, C).n() * 16; }
// The walk of mi_blur_remap_plan over the tiles of one output image (remap_shape_tiled() holds).
inline void remap_walk(const int32_t *map, int W, int H, int C, int Wo, int Ho, int border, int stage_bytes, mi_blur_remap_tiles *t)
{
    const TileGrid g = warp_grid(Wo * C / 16, Ho, C);
    for (int ty = 0; ty < g.ntiles_y; ty++)
        for (int s = 0; s < g.nstrips; s++) {
            const Tile tl = tile_at(g, Ho, s, ty);
            const WarpBox b = remap_tile_box(map, border, W, H, Wo, C, tl.ty0, tl.rows_out, tl.x0c, tl.nc);
            t->tiles++;
            if (warp_box_empty(b)) { t->empty++; continue; }
            const long long bytes = remap_box_bytes(b, C);
            t->max_box_bytes = bytes > t->max_box_bytes ? bytes : t->max_box_bytes;
            if (bytes <= stage_bytes) { t->staged++; t->max_staged_bytes = bytes > t->max_staged_bytes ? bytes : t->max_staged_bytes; }
            else t->direct++;
        }
}

// ---- blur_area_tiled_kernel.  A tile is AREA_TH output rows x a strip of output chunks (whole units, warp_unit()).  Its
// 256 threads are 256 / span row groups of `span` (64 | 128 | 256) threads: a group owns AREA_TH / (256 / span)
// consecutive output rows, thread `col` of it the input chunk column sc.lo + col of the strip's input span sc.  LDS: the x
// table (two dwords per output byte of a tile row), then one V row per group: one dword per input byte of the span, the
// dword of byte q at area_v_pos(q).  Nothing of the input is staged.
constexpr int AREA_TH = 4;                          // output rows per tile
constexpr int AREA_THREADS = 256;
constexpr int AREA_MAX_SPAN = 256;                  // input chunks under a strip: one per thread of the widest group
constexpr int AREA_WAVE_SPAN = 64;                  // what strips are cut for: one input chunk per lane of one wave
// The input chunks under output chunks [x0c, x0c + nc): the first tap of their first pixel to the last tap of their last.
MI_BLUR_HD inline Span area_stage_chunks(int W, int Wo, int C, int x0c, int nc)
{
    const Span px = tile_pixels(x0c, nc, C);
    return chunk_span(area_axis(W, Wo, px.lo).i_lo, area_axis(W, Wo, px.hi).i_hi, C);
}
// V dword of input byte q of the span: one spare dword every eight, so that the horizontal pass's reads (lanes four
// output bytes = 4 * ratio input bytes apart) and the vertical pass's writes (lanes 16 bytes apart) spread over the banks.
MI_BLUR_HD inline uint32_t area_v_pos(int q) { return (uint32_t)(q + (q >> 3)); }
MI_BLUR_HD inline int area_v_row(int nsc) { return nsc * 18; }      // dwords of a V row of nsc chunks: area_v_pos(16 nsc - 1) + 1 <= 18 nsc
// x table entry of channel c of output pixel X: the span byte of its first tap | taps << 16, then w_lo | w_hi << 16.
MI_BLUR_HD inline uint32_t area_x_entry0(const AreaAxis &ax, int C, int c, int sc0) { return (uint32_t)(ax.i_lo * C + c - sc0 * 16) | ((uint32_t)(ax.i_hi - ax.i_lo + 1) << 16); }
MI_BLUR_HD inline uint32_t area_x_entry1(const AreaAxis &ax) { return (uint32_t)ax.w_lo | ((uint32_t)ax.w_hi << 16); }
// The tiles of a launch (Wo <= W, rows of whole chunks both sides): strips as wide as keep every strip's input span within
// AREA_WAVE_SPAN chunks, at least one unit, and narrower still while the horizontal pass of a 64-thread group (one output
// dword per thread and step) would take a last step less than half full: a strip of 18 chunks is two steps for 72
// dwords, one of 15 is one.  max_nsc is the largest span of the launch (the walk below), span the group size that holds
// it.  One unit at the ratio cap spans at most 194 chunks (C = 3: 16 pixels, 1025 input pixels), so
// max_nsc <= AREA_MAX_SPAN for every valid launch; area_tiles_fit() is the guard all the same.
struct AreaTiles { TileGrid g; int max_nsc, span; };
inline int area_max_span(const TileGrid &g, int W, int Wo, int C)
{
    int m = 1;
    for (int s = 0; s < g.nstrips; s++) {
        const int x0c = s * g.ncols, nc = g.cpr - x0c < g.ncols ? g.cpr - x0c : g.ncols;
        const int n = area_stage_chunks(W, Wo, C, x0c, nc).n();
        m = n > m ? n : m;
    }
    return m;
}
inline AreaTiles area_tiles(int W, int Wo, int Ho, int C)
{
    const int cpr = (int)((long long)Wo * C / 16), unit = warp_unit(C), units = cpr / unit;
    long long m = (long long)(AREA_WAVE_SPAN - 3) * Wo / ((long long)W * unit);
    m = m < 1 ? 1 : m > units ? units : m;
    AreaTiles t;
    for (;; m--) {
        t.g = tile_grid(cpr, Ho, unit, (int)m);
        t.g.ntiles_y = (Ho + AREA_TH - 1) / AREA_TH;
        t.max_nsc = area_max_span(t.g, W, Wo, C);
        const int dwords = t.g.ncols * 4, last_step = (dwords - 1) % AREA_WAVE_SPAN + 1;
        if (m == 1 || (t.max_nsc <= AREA_WAVE_SPAN && (dwords <= AREA_WAVE_SPAN || 2 * last_step >= AREA_WAVE_SPAN))) break;
    }
    t.span = t.max_nsc <= 64 ? 64 : t.max_nsc <= 128 ? 128 : 256;
    return t;
}
inline bool area_tiles_fit(const AreaTiles &t) { return t.max_nsc <= AREA_MAX_SPAN; }
inline int area_xtab_bytes(const AreaTiles &t) { return t.g.ncols * 16 * 8; }
inline size_t area_lds_bytes(const AreaTiles &t) { return (size_t)area_xtab_bytes(t) + (size_t)(AREA_THREADS / t.span) * (size_t)area_v_row(t.max_nsc) * 4u; }

// ---- blur_color_tiled_kernel.  A pointwise filter on dense images does not care about rows: per image it works on the
// flat run of W * H pixels.  A group is 16 pixels: exactly C input chunks and co output chunks of 16 bytes.  One thread
// owns one group, one workgroup a run of COLOR_RUN consecutive groups of one image (the last run of an image may be short).
constexpr int COLOR_GROUP = 16;                     // pixels per group
constexpr int COLOR_RUN = 256;                      // groups per workgroup = its threads
inline bool color_flat_ok(int W, int H) { return (long long)W * H % COLOR_GROUP == 0; }
inline int color_runs(int W, int H) { return (int)(((long long)W * H / COLOR_GROUP + COLOR_RUN - 1) / COLOR_RUN); }

// ---- blur_hist_tiled_kernel and blur_tables_tiled_kernel: the flat rule and the groups of the colour kernel, but a
// workgroup of HIST_THREADS threads owns a run of HIST_RUN consecutive groups of one image and loops over it, thread t
// taking groups t, t + HIST_THREADS, ... of the run: the flush of the histogram kernel's bins and the load of the tables
// kernel's tables are paid once per run.
constexpr int HIST_THREADS = 512;
constexpr int HIST_RUN = 512;                       // groups per workgroup
inline int hist_runs(int W, int H) { return (int)(((long long)W * H / COLOR_GROUP + HIST_RUN - 1) / HIST_RUN); }
// The histogram kernel alone gives an image at most HIST_IMAGE_BLOCKS workgroups (one per CU): workgroup b of a larger
// image takes runs b, b + HIST_IMAGE_BLOCKS, ... and flushes once.  Every flush lands on the image's one C KiB of
// counters, and that row takes about one flush per 16 ns whoever sends it (profiles/r19_hist.md).
constexpr int HIST_IMAGE_BLOCKS = 256;
inline int hist_blocks(int W, int H) { const int r = hist_runs(W, H); return r < HIST_IMAGE_BLOCKS ? r : HIST_IMAGE_BLOCKS; }

// ---- the CLAHE kernels.  Both tiled kernels take rows of whole groups of COLOR_GROUP pixels (W a multiple of 16) and
// 16-byte aligned images, so a group is C chunks of 16 bytes and never straddles a row; tile edges fall anywhere.
// blur_clahe_tables_tiled_kernel and its generic form: one workgroup of CLAHE_THREADS threads (= bins) per (image, tile);
// the generic form has at most CLAHE_GENERIC_BLOCKS workgroups, which stride over the tiles.
// blur_clahe_apply_tiled_kernel: a workgroup owns up to CLAHE_ROWS rows of one row class (clahe_class_lo()) and a span of
// CLAHE_SPAN pixels; it stages the tables of both tile rows for the tile columns from t0 of the span's first pixel to t1
// of its last.  The launch is tiled when the widest such run of columns, times 2 * C * 256 bytes, fits
// CLAHE_LDS_TABLE_BYTES.
constexpr int CLAHE_THREADS = 256;
constexpr int CLAHE_GENERIC_BLOCKS = 256 * 64;
constexpr int CLAHE_SPAN = 256;                     // pixels: 16 groups
constexpr int CLAHE_ROWS = 32;
constexpr int CLAHE_LDS_TABLE_BYTES = 32768;
constexpr int CLAHE_LDS_TABLE = MI_BLUR_HIST_BINS + 4;      // a staged table's stride: one bank on from its neighbour
static_assert(CLAHE_THREADS == MI_BLUR_HIST_BINS && CLAHE_SPAN == CLAHE_THREADS, "thread v is bin v, and column v of a span");
inline bool clahe_tiled_ok(int W) { return W % COLOR_GROUP == 0; }
inline int clahe_spans(int W) { return (W + CLAHE_SPAN - 1) / CLAHE_SPAN; }
// The most tile columns one span needs.
inline int clahe_span_cols(int W, int TX)
{
    int most = 1;
    for (int s = 0; s < clahe_spans(W); s++) {
        const int xa = s * CLAHE_SPAN, xb = (xa + CLAHE_SPAN < W ? xa + CLAHE_SPAN : W) - 1;
        int a0, a1, b0, b1, f;
        clahe_axis(W, TX, xa, a0, a1, f);
        clahe_axis(W, TX, xb, b0, b1, f);
        most = b1 - a0 + 1 > most ? b1 - a0 + 1 : most;
    }
    return most;
}
inline size_t clahe_table_lds(int W, int TX, int C) { return (size_t)clahe_span_cols(W, TX) * 2u * (size_t)C * MI_BLUR_HIST_BINS; }
// LDS bytes of the staged tables with their padding, to 16 bytes (the entries behind them are read 16 bytes at a time).
MI_BLUR_HD inline size_t clahe_apply_lds_tables(int max_cols, int C) { return ((size_t)2 * max_cols * C * CLAHE_LDS_TABLE + 15) & ~(size_t)15; }
inline bool clahe_apply_tiled_ok(int W, int TX, int C) { return clahe_tiled_ok(W) && clahe_table_lds(W, TX, C) <= (size_t)CLAHE_LDS_TABLE_BYTES; }
// Slices of up to CLAHE_ROWS rows of all row classes of an image.
inline int clahe_slices(int H, int TY)
{
    int n = 0;
    for (int k = 0; k <= TY; k++) n += (clahe_class_lo(H, TY, k + 1) - clahe_class_lo(H, TY, k) + CLAHE_ROWS - 1) / CLAHE_ROWS;
    return n;
}

// ---- blur_arith_flat_kernel: the flat rule one step flatter.  With every operand at the image's channel count the
// operation is bytewise, so an image is the run of its W * H * C bytes cut into chunks of ARITH_CHUNK bytes and the
// channel count does not enter: W * H * C a multiple of ARITH_CHUNK, 16-byte aligned pointers.  A thread owns one chunk,
// a workgroup of ARITH_THREADS threads a run of ARITH_RUN consecutive chunks of one image.
// blur_arith_plane_kernel (a one-channel operand on an image of 2..4 channels): the colour kernel's rule and units, one
// thread per group of COLOR_GROUP pixels, a workgroup per run of ARITH_PLANE_RUN groups.
constexpr int ARITH_CHUNK = 16;
constexpr int ARITH_THREADS = 256;
constexpr int ARITH_RUN = 256;                      // chunks per workgroup = its threads
constexpr int ARITH_PLANE_RUN = 256;                // groups per workgroup = its threads
inline bool arith_flat_ok(int W, int H, int C) { return (long long)W * H * C % ARITH_CHUNK == 0; }
inline long long arith_flat_runs(int W, int H, int C) { return ((long long)W * H * C / ARITH_CHUNK + ARITH_RUN - 1) / ARITH_RUN; }
inline long long arith_plane_runs(int W, int H) { return ((long long)W * H / COLOR_GROUP + ARITH_PLANE_RUN - 1) / ARITH_PLANE_RUN; }

// ---- blur_integral_tiled_kernel: one workgroup per (image, band of rows) spans the whole row, a thread owns
// INTEGRAL_PIXELS pixels, so the widest image it takes is INTEGRAL_PIXELS * INTEGRAL_MAX_THREADS pixels; its workgroup
// has the fewest whole waves that cover the row.  A band is INTEGRAL_BAND rows ("integral_band" replaces it in A/B
// runs): the bands kernel leaves one row of W * C column sums per band and table in the work buffer.
constexpr int INTEGRAL_PIXELS = 16;
constexpr int INTEGRAL_MAX_THREADS = 512;
constexpr int INTEGRAL_MAX_W = 8192;
constexpr int INTEGRAL_BAND = 16;
static_assert(INTEGRAL_MAX_W == INTEGRAL_PIXELS * INTEGRAL_MAX_THREADS, "the tiled cap is what one workgroup spans");
inline bool integral_tiled_ok(int W) { return W % INTEGRAL_PIXELS == 0 && W <= INTEGRAL_MAX_W; }
inline int integral_threads(int W) { return (W / INTEGRAL_PIXELS + 63) / 64 * 64; }
inline int integral_bands(int H, int band) { return (H + band - 1) / band; }
inline size_t integral_work_bytes(int W, int H, int C, int n_images, int tables, int band)
{
    return (size_t)n_images * (size_t)integral_bands(H, band) * (size_t)tables * (size_t)W * (size_t)C * sizeof(uint32_t);
}
// Dwords of one table.
inline size_t integral_words(int W, int H, int C, int n_images) { return (size_t)n_images * (size_t)H * (size_t)W * (size_t)C; }
// blur_box_tiled_kernel: rows of whole 16-byte chunks, a thread per chunk, BOX_THREADS chunks of one row per workgroup.
constexpr int BOX_THREADS = 256;
inline bool box_tiled_ok(int W, int C) { return (long long)W * C % 16 == 0; }

// ---- the distance transform's kernels.  The column pass works in bands of DIST_BAND rows ("dist_band" replaces it in
// A/B runs) and leaves, next to g, two rows of W * C row numbers per band.  blur_dist_tiled_kernel: a workgroup of
// DIST_THREADS threads owns dist_rows() whole rows (about DIST_TILE_ELEMS elements, at most DIST_MAX_ROWS rows), rows of
// whole 16-byte chunks of g (W * C a multiple of 8) of at most DIST_MAX_ROW elements: a row's planes, padded to whole
// search chunks of 2^DIST_CHUNK_LOG2 columns ("dist_chunk_log2": 3..5), and their minima then fit 64 KiB of LDS.
constexpr int DIST_BAND = 32;
constexpr int DIST_THREADS = 256;
constexpr int DIST_TILE_ELEMS = 4096;
constexpr int DIST_MAX_ROWS = 8;
constexpr int DIST_MAX_ROW = 24576;
constexpr int DIST_CHUNK_LOG2 = 4;
inline bool dist_tiled_ok(int W, int C) { return (long long)W * C % 8 == 0 && (long long)W * C <= DIST_MAX_ROW; }
inline int dist_rows(int W, int C) { const int r = DIST_TILE_ELEMS / (W * C); return r < 1 ? 1 : r > DIST_MAX_ROWS ? DIST_MAX_ROWS : r; }
inline int dist_chunks(int W, int chunk) { return (W + chunk - 1) / chunk; }
// LDS of one workgroup: the planes (uint16 [rows][C][nch * chunk]) and the minima (uint16 [rows][C][nch]), to 16 bytes.
inline size_t dist_lds_bytes(int W, int C, int rows, int chunk)
{
    const size_t nch = (size_t)dist_chunks(W, chunk);
    return ((size_t)rows * C * nch * (chunk + 1) * sizeof(uint16_t) + 15) & ~(size_t)15;
}
// C * nch <= W * C / chunk + C: the smallest chunk is the largest case (55 368 bytes; 52 360 at 16).
static_assert((DIST_MAX_ROW / 8 + 4) * (8 + 1) * 2 <= 65536, "one row of DIST_MAX_ROW elements fits 64 KiB at every chunk size");
inline int dist_bands(int H, int band) { return (H + band - 1) / band; }
inline size_t dist_g_bytes(int W, int H, int C, int n_images) { return ((size_t)n_images * (size_t)H * (size_t)W * (size_t)C * sizeof(uint16_t) + 15) & ~(size_t)15; }
inline size_t dist_work_bytes(int W, int H, int C, int n_images, int band)
{
    return dist_g_bytes(W, H, C, n_images) + (size_t)n_images * (size_t)dist_bands(H, band) * 2u * (size_t)W * (size_t)C * sizeof(uint16_t);
}

// ---- template matching and peak search (include/mi_blur.h, "Template matching and peak search").  The host export
// mi_blur_match_value, the CPU device and blur_match_score_kernel take a score from match_score(); the raw sums are
// plain loops wherever they are made.
inline bool match_ok(const mi_blur_match *k, int W, int H, int C)
{
    if (!k || k->method < MI_BLUR_MATCH_SQDIFF || k->method > MI_BLUR_MATCH_ZNCC || (k->t_shared != 0 && k->t_shared != 1)) return false;
    if (k->tw < 1 || k->th < 1 || k->tw > MI_BLUR_MATCH_MAX_SIDE || k->th > MI_BLUR_MATCH_MAX_SIDE || k->tw > W || k->th > H) return false;
    return (long long)k->tw * k->th * C <= MI_BLUR_MATCH_MAX_AREA;
}
inline bool match_is_score(int method) { return method == MI_BLUR_MATCH_NCC || method == MI_BLUR_MATCH_ZNCC; }
// The arguments of the three match exports: out = 32-bit words, `align` bytes aligned, and neither input.
inline bool match_args_ok(const void *in, const void *t, const void *out, int W, int H, int C, int n_images, const mi_blur_match *k, uintptr_t align)
{
    if (!in || !t || !out || out == in || out == t || n_images < 0 || !hist_image_ok(W, H, C) || !match_ok(k, W, H, C)) return false;
    return (uintptr_t)out % align == 0;
}
// ... and of the peak search: peaks = int64[n][6].
inline bool match_peak_args_ok(const void *table, int is_signed, int Wo, int Ho, int n_images, const void *peaks, uintptr_t table_align, uintptr_t peaks_align)
{
    if (!table || !peaks || table == peaks || n_images < 0 || (is_signed != 0 && is_signed != 1)) return false;
    if (Wo < 1 || Ho < 1 || (long long)Wo * Ho > INT_MAX) return false;
    return (uintptr_t)table % table_align == 0 && (uintptr_t)peaks % peaks_align == 0;
}
// The score of consistent sums (the caller's business): sign(N) k, k the largest integer in 0..16384 that is 0 or has
// (2k - 1)^2 D <= 2^30 N^2.  A double-precision estimate, then the exact comparison in 128 bits moves it as far as it
// must (the estimate is within one of k; the loops do not rely on that).
MI_BLUR_HD inline int32_t match_score(int method, uint32_t A, uint32_t sum_at, uint32_t sum_a, uint32_t sum_aa, uint32_t sum_t, uint32_t sum_tt)
{
    typedef unsigned __int128 u128;
    int64_t N;
    uint64_t Da, Dt;
    if (method == MI_BLUR_MATCH_NCC) {
        N = (int64_t)sum_at; Da = sum_aa; Dt = sum_tt;
    } else {
        N = (int64_t)((uint64_t)A * sum_at) - (int64_t)((uint64_t)sum_a * sum_t);
        Da = (uint64_t)A * sum_aa - (uint64_t)sum_a * sum_a;
        Dt = (uint64_t)A * sum_tt - (uint64_t)sum_t * sum_t;
    }
    if (Da == 0 || Dt == 0 || N == 0) return 0;
    const uint64_t n = (uint64_t)(N < 0 ? -N : N);
    const u128 D = (u128)Da * Dt, rhs = ((u128)n * n) << 30;
    const double est = 16384.0 * (double)n / (sqrt((double)Da) * sqrt((double)Dt));
    int k = est >= 16384.0 ? MI_BLUR_MATCH_ONE : (int)(est + 0.5);
    const auto holds = [&](int kk) { const u128 o = (u128)(uint64_t)(2 * kk - 1); return o * o * D <= rhs; };
    while (k > 0 && !holds(k)) k--;
    while (k < MI_BLUR_MATCH_ONE && holds(k + 1)) k++;
    return N < 0 ? -k : k;
}
// blur_match_tiled_kernel: a workgroup of MATCH_THREADS = MATCH_TX lanes x MATCH_THREADS / 64 waves owns MATCH_TX x
// MATCH_TY outputs, MATCH_R output rows a thread; it stages the input rows of as many template rows as MATCH_LDS_BYTES
// hold at a time.  Rows of whole 16-byte chunks; the template rows zero-padded to MATCH_ROW_PAD bytes.
constexpr int MATCH_THREADS = 256, MATCH_TX = 64, MATCH_R = 4, MATCH_TY = MATCH_THREADS / 64 * MATCH_R;
constexpr int MATCH_ROW_PAD = 16, MATCH_LDS_BYTES = 48 * 1024, MATCH_LDS_SLACK = 64;
inline bool match_tiled_ok(int W, int C) { return (long long)W * C % 16 == 0; }
inline size_t match_round16(size_t b) { return (b + 15) & ~(size_t)15; }
inline int match_templates(const mi_blur_match &k, int n_images) { return k.t_shared ? 1 : n_images; }
inline size_t match_row_pad(const mi_blur_match &k, int C) { return ((size_t)k.tw * C + MATCH_ROW_PAD - 1) / MATCH_ROW_PAD * MATCH_ROW_PAD; }
// The work buffer: sums[templates][4] (sum_t, sum_tt, 0, 0), the padded templates, then for a score the CCORR table, S, Q
// and the integral's own work.
inline size_t match_sums_bytes(const mi_blur_match &k, int n_images) { return (size_t)match_templates(k, n_images) * 16u; }
inline size_t match_pad_bytes(const mi_blur_match &k, int C, int n_images) { return (size_t)match_templates(k, n_images) * k.th * match_row_pad(k, C); }
inline size_t match_table_bytes(const mi_blur_match &k, int W, int H, int n_images)
{
    return match_round16((size_t)n_images * (size_t)(H - k.th + 1) * (size_t)(W - k.tw + 1) * sizeof(uint32_t));
}
constexpr int MATCH_PEAK_THREADS = 256;

}  // namespace mi_blur
