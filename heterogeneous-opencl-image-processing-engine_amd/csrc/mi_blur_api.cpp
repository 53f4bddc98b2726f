// mi_blur_api.cpp — implementation of the C ABI declared in include/mi_blur.h.
//
// Each block names the reference OpenCL plumbing it replaces (paths relative to the
// reference tree).  No torch, no OpenCL; HIP runtime only (the multi-GPU exports: comm_api.cpp; the families outside Filter: table_api.cpp).
#include "api_internal.h"
#include "blur_launch.h"
#include "cpu_device.h"

#include <sched.h>
#include <time.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <deque>
#include <functional>
#include <condition_variable>
#include <thread>
#include <vector>

using namespace mi_blur;

// Runtime default, applied when the library is loaded and only if the user has not set it: keep kernel
// arguments in host memory (HIP_FORCE_DEV_KERNARG=0).  With the runtime's gfx9 default (a device-memory
// kernarg pool written over PCIe) a stream of argument-carrying launches issues at ~3.3 us per launch on this
// platform, with host kernargs at ~1.6 us (tools/ubench/dispatch_floor.hip); the batch-35 stream is bounded by
// that rate, not by the kernel (+30 % images/s measured).  The flag is read when the HIP
// runtime initialises, so it takes effect if this library (or the Python package, which sets it too) is
// loaded before the process's first HIP call.
__attribute__((constructor)) static void mi_blur_runtime_defaults() { setenv("HIP_FORCE_DEV_KERNARG", "0", 0); }

// ----------------------------------------------------------------------------------
// status / discovery   (replaces cl_error strings + heterogeneous_blur.c:142-184)
// ----------------------------------------------------------------------------------
extern "C" const char *mi_blur_strerror(int status)
{
    static thread_local char buf[160];
    switch (status) {
    case MI_BLUR_OK: return "success";
    case MI_BLUR_ERR_INVALID: return "invalid argument";
    case MI_BLUR_ERR_NO_DEVICE: return "no usable HIP device";
    case MI_BLUR_ERR_NOMEM: return "out of memory";
    case MI_BLUR_ERR_STATE: return "call not valid in this state";
    case MI_BLUR_ERR_UNSUPPORTED: return "not supported in this build/environment";
    }
    if (status <= MI_BLUR_ERR_RCCL_BASE && status > MI_BLUR_ERR_RCCL_BASE - 100) {
        snprintf(buf, sizeof buf, "RCCL error %d", MI_BLUR_ERR_RCCL_BASE - status);
        return buf;
    }
    if (status <= MI_BLUR_ERR_HIP_BASE) {
        const hipError_t e = (hipError_t)(MI_BLUR_ERR_HIP_BASE - status);
        snprintf(buf, sizeof buf, "HIP error %d: %s", (int)e, hipGetErrorString(e));
        return buf;
    }
    snprintf(buf, sizeof buf, "unknown status %d", status);
    return buf;
}

extern "C" int mi_blur_version(void) { return MI_BLUR_VERSION; }

extern "C" const char *mi_blur_last_kernel(void) { return last_kernel(); }

extern "C" int mi_blur_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

extern "C" int mi_blur_set_option(const char *key, int value)
{
    if (!key) return MI_BLUR_ERR_INVALID;
    Tunables t = tunables();      // copy, edit, publish: launches in other threads see the old set or the new one
    const Knob *k = std::find_if(std::begin(KNOBS), std::end(KNOBS), [&](const Knob &r) { return !strcmp(r.key, key); });
    if (k == std::end(KNOBS) || !knob_set(*k, t, value)) return MI_BLUR_ERR_INVALID;
    set_tunables(t);
    return MI_BLUR_OK;
}

// ----------------------------------------------------------------------------------
// kernel level   (clSetKernelArg x5 + clEnqueueNDRangeKernel)
// ----------------------------------------------------------------------------------
// What an export checks itself, before it asks for a device; launch() checks everything (again) behind the device check.
// Each family's exports were written from their neighbours', so the levels differ, and a caller without a GPU sees
// which one an export has: an argument error below its level reads MI_BLUR_ERR_INVALID, one above it
// MI_BLUR_ERR_NO_DEVICE.  Inherited and observable (tests/test_entry_statuses_host.py), so kept as it is.  Each level
// adds to the one before it, the last two both to ARGS.
enum class PreCheck {
    NOTHING,    // box
    FILTER,     // sep: the constructor's status
    ARGS,       // median, morph, bilateral, conv: + pointers, dimensions, image count
    ARGS_ROWS,  // conv_band: + the row range
    ARGS_SIZE,  // sep_down, resize, warp, warp_perspective, remap, area, color: + the image within INT_MAX bytes
};

// Every mi_blur_enqueue* export: one launch of f on device memory.  built: the status of f's constructor.
static int enqueue_filter(int built, const Filter &f, PreCheck level, const uint8_t *d_in, uint8_t *d_out, int width,
                          int band_rows, int channels, int n_images, int y0, int y1, int variant, void *stream,
                          const uint8_t *halo_top = nullptr, const uint8_t *halo_bottom = nullptr)
{
    if (level >= PreCheck::FILTER && built) return built;
    if (level >= PreCheck::ARGS && (!d_in || !d_out || d_in == d_out || width <= 0 || band_rows <= 0 || channels <= 0 || n_images < 0))
        return MI_BLUR_ERR_INVALID;
    if (level == PreCheck::ARGS_ROWS && (y0 < 0 || y1 > band_rows || y0 >= y1)) return MI_BLUR_ERR_INVALID;
    if (level == PreCheck::ARGS_SIZE && (long long)width * channels * band_rows > INT_MAX) return MI_BLUR_ERR_INVALID;
    if (mi_blur_device_count() <= 0) return MI_BLUR_ERR_NO_DEVICE;
    LaunchDesc d{};
    d.filter = &f;
    d.in = d_in; d.out = d_out; d.width = width; d.band_rows = band_rows; d.channels = channels;
    d.n_images = n_images; d.y0 = y0; d.y1 = y1; d.variant = variant; d.stream = (hipStream_t)stream;
    d.halo_top = halo_top; d.halo_bottom = halo_bottom;
    return launch(d);
}

// The three filters whose validity depends on the image they are applied to: the constructor, then down_ok / resize_ok /
// warp_ok against it.  The enqueue and cpu_run exports and the context setters all build them here.
static int sep_down_for(const mi_blur_sep_kernel *k, const mi_blur_decimation *d, int W, int H, Filter *f)
{
    const int rc = filter_sep_down(k, d, f);
    return rc ? rc : down_ok(d, W, H) ? MI_BLUR_OK : MI_BLUR_ERR_INVALID;
}
static int resize_for(const mi_blur_resize *r, int W, int H, int C, Filter *f)
{
    const int rc = filter_resize(r, f);
    return rc ? rc : resize_ok(r, W, H, C) ? MI_BLUR_OK : MI_BLUR_ERR_INVALID;
}
static int area_for(const mi_blur_area *r, int W, int H, int C, Filter *f)
{
    const int rc = filter_area(r, f);
    return rc ? rc : area_ok(r, W, H, C) ? MI_BLUR_OK : MI_BLUR_ERR_INVALID;
}
static int color_for(const mi_blur_color *k, int W, int H, int C, Filter *f)
{
    const int rc = filter_color(k, f);
    return rc ? rc : color_image_ok(k->out_channels, W, H, C) ? MI_BLUR_OK : MI_BLUR_ERR_INVALID;
}

static int warp_for(const mi_blur_warp *w, int W, int H, int C, Filter *f)
{
    const int rc = filter_warp(w, f);
    return rc ? rc : warp_ok(w, W, H, C) ? MI_BLUR_OK : MI_BLUR_ERR_INVALID;
}

// The box radius is not checked here: launch() rejects a bad one, after the device check.
static Filter box_unchecked(int radius) { return Filter{FilterKind::BOX, radius, {}}; }

extern "C" int mi_blur_enqueue_ex(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                                  int radius, int n_images, int out_row_begin, int out_row_end, int variant,
                                  void *stream)
{
    return enqueue_filter(MI_BLUR_OK, box_unchecked(radius), PreCheck::NOTHING, d_in, d_out, width, band_rows, channels, n_images,
                          out_row_begin, out_row_end, variant, stream);
}

extern "C" int mi_blur_enqueue(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels,
                               int radius, int n_images, void *stream)
{
    return mi_blur_enqueue_ex(d_in, d_out, width, height, channels, radius, n_images, 0, height,
                              MI_BLUR_VARIANT_AUTO, stream);
}

extern "C" int mi_blur_enqueue_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                                    int radius, int out_row_begin, int out_row_end, void *stream)
{
    return mi_blur_enqueue_ex(d_in, d_out, width, band_rows, channels, radius, 1, out_row_begin, out_row_end,
                              MI_BLUR_VARIANT_AUTO, stream);
}

// Band whose halo rows are read in place from the neighbouring shards (peer memory): exchange and blur in one launch.
extern "C" int mi_blur_enqueue_band_peer(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                                         int radius, int out_row_begin, int out_row_end, const uint8_t *top_src,
                                         const uint8_t *bottom_src, void *stream)
{
    return enqueue_filter(MI_BLUR_OK, box_unchecked(radius), PreCheck::NOTHING, d_in, d_out, width, band_rows, channels, 1,
                          out_row_begin, out_row_end, MI_BLUR_VARIANT_AUTO, stream, top_src, bottom_src);
}

// ----------------------------------------------------------------------------------
// separable kernels of any radius up to 16 (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_gauss_taps(double sigma, int radius, int bits, uint16_t *taps, int *radius_out)
{
    if (!taps || !(sigma > 0.0) || radius < 0 || radius > MI_BLUR_SEP_MAX_RADIUS || bits < 0 || bits > 8) return MI_BLUR_ERR_INVALID;
    const int r = radius ? radius : (int)std::min(16.0, std::max(1.0, std::ceil(3.0 * sigma)));
    double w[2 * MI_BLUR_SEP_MAX_RADIUS + 1], sum = 0.0;
    for (int i = -r; i <= r; i++) { w[i + r] = std::exp(-(double)i * i / (2.0 * sigma * sigma)); sum += w[i + r]; }
    long long t[2 * MI_BLUR_SEP_MAX_RADIUS + 1], tsum = 0;
    const double scale = (double)(1 << bits);
    for (int i = 0; i <= 2 * r; i++) { t[i] = (long long)std::floor(w[i] * scale / sum + 0.5); tsum += t[i]; }
    t[r] += (1LL << bits) - tsum;                       // the centre absorbs the rounding
    if (t[r] <= 0) return MI_BLUR_ERR_INVALID;
    int re = r;                                         // drop outer pairs that rounded to 0
    while (re > 0 && t[r - re] == 0 && t[r + re] == 0) re--;
    for (int i = 0; i <= 2 * re; i++) taps[i] = (uint16_t)t[r - re + i];
    if (radius_out) *radius_out = re;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_sep_kernel_gauss(double sigma_x, double sigma_y, int radius, int bits, mi_blur_sep_kernel *k)
{
    if (!k) return MI_BLUR_ERR_INVALID;
    if (sigma_y <= 0.0) sigma_y = sigma_x;
    mi_blur_sep_kernel g{};
    int rc = mi_blur_gauss_taps(sigma_x, radius, bits, g.wx, &g.rx);
    if (rc) return rc;
    rc = mi_blur_gauss_taps(sigma_y, radius, bits, g.wy, &g.ry);
    if (rc) return rc;
    g.bx = g.by = bits;
    *k = g;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_sep_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                                        int out_row_begin, int out_row_end, const mi_blur_sep_kernel *k, void *stream)
{
    Filter f;
    return enqueue_filter(filter_sep(k, &f), f, PreCheck::FILTER, d_in, d_out, width, band_rows, channels, 1, out_row_begin,
                          out_row_end, MI_BLUR_VARIANT_AUTO, stream);
}

extern "C" int mi_blur_enqueue_sep(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                   const mi_blur_sep_kernel *k, void *stream)
{
    Filter f;
    return enqueue_filter(filter_sep(k, &f), f, PreCheck::FILTER, d_in, d_out, width, height, channels, n_images, 0, height,
                          MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// decimating separable filter: only the kept rows and columns are computed (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_decimated_size(int width, int height, const mi_blur_decimation *d, int *out_width, int *out_height)
{
    if (!out_width || !out_height || width <= 0 || height <= 0 || !down_ok(d, width, height)) return MI_BLUR_ERR_INVALID;
    *out_width = down_cols(width, d->sx, d->ox);
    *out_height = down_rows(height, d->sy, d->oy);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_sep_down_preset(int preset, mi_blur_sep_kernel *k, mi_blur_decimation *d)
{
    if (!k || !d || preset < MI_BLUR_DOWN_PYR || preset > MI_BLUR_DOWN_AREA4) return MI_BLUR_ERR_INVALID;
    static const uint16_t PYR[5] = {1, 4, 6, 4, 1}, AREA2[3] = {0, 1, 1}, AREA4[7] = {0, 0, 0, 1, 1, 1, 1};
    const uint16_t *taps = preset == MI_BLUR_DOWN_PYR ? PYR : preset == MI_BLUR_DOWN_AREA2 ? AREA2 : AREA4;
    const int r = preset == MI_BLUR_DOWN_PYR ? 2 : preset == MI_BLUR_DOWN_AREA2 ? 1 : 3;
    const int bits = preset == MI_BLUR_DOWN_PYR ? 4 : preset == MI_BLUR_DOWN_AREA2 ? 1 : 2;
    const int stride = preset == MI_BLUR_DOWN_AREA4 ? 4 : 2;
    mi_blur_sep_kernel g{};
    g.rx = g.ry = r; g.bx = g.by = bits;
    for (int i = 0; i <= 2 * r; i++) g.wx[i] = g.wy[i] = taps[i];
    *k = g;
    *d = mi_blur_decimation{stride, stride, 0, 0};
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_sep_down(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                        const mi_blur_sep_kernel *k, const mi_blur_decimation *d, void *stream)
{
    Filter f;
    return enqueue_filter(sep_down_for(k, d, width, height, &f), f, PreCheck::ARGS_SIZE, d_in, d_out, width, height, channels,
                          n_images, 0, height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// image resize: fixed-point bilinear and nearest, any output size (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_resize_coord(int n_in, int n_out, int mode, int X, int *i0, int *i1, int *frac)
{
    if (!i0 || !i1 || !frac || n_in < 1 || n_out < 1 || n_in > MI_BLUR_RESIZE_MAX_DIM || n_out > MI_BLUR_RESIZE_MAX_DIM ||
        (mode != MI_BLUR_RESIZE_NEAREST && mode != MI_BLUR_RESIZE_BILINEAR) || X < 0 || X >= n_out)
        return MI_BLUR_ERR_INVALID;
    const ResizeCoord r = resize_axis(n_in, n_out, mode, X);
    *i0 = r.a; *i1 = r.b; *frac = r.f;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_resize(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                      const mi_blur_resize *r, void *stream)
{
    Filter f;
    return enqueue_filter(resize_for(r, width, height, channels, &f), f, PreCheck::ARGS_SIZE, d_in, d_out, width, height,
                          channels, n_images, 0, height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// area resize: exact box average, any output size, reductions up to 64x (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_area_coord(int n_in, int n_out, int X, int *i_lo, int *i_hi, int *w_lo, int *w_hi)
{
    if (!i_lo || !i_hi || !w_lo || !w_hi || n_in < 1 || n_out < 1 || n_in > MI_BLUR_RESIZE_MAX_DIM || n_out > MI_BLUR_RESIZE_MAX_DIM ||
        X < 0 || X >= n_out)
        return MI_BLUR_ERR_INVALID;
    const AreaAxis a = area_axis(n_in, n_out, X);
    *i_lo = a.i_lo; *i_hi = a.i_hi; *w_lo = a.w_lo; *w_hi = a.w_hi;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_area(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                    const mi_blur_area *r, void *stream)
{
    Filter f;
    return enqueue_filter(area_for(r, width, height, channels, &f), f, PreCheck::ARGS_SIZE, d_in, d_out, width, height,
                          channels, n_images, 0, height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// colour transform: exact channel matrix + table, 1-4 channels in and out (no reference analogue)
// ----------------------------------------------------------------------------------
namespace {
// q(x) = floor(x * 65536 + 0.5) of the JFIF constants (include/mi_blur.h, the table of presets).
constexpr int32_t CQ = 65536, CR = 32768;
constexpr int32_t LUMA[3] = {19595, 38470, 7471};

void color_rows(mi_blur_color *k, int co, int shift) { *k = mi_blur_color{}; k->out_channels = co; k->shift = shift; }
void color_permute(mi_blur_color *k, int co, const int *src)
{
    color_rows(k, co, 0);
    for (int o = 0; o < co; o++) if (src[o] >= 0) k->m[o][src[o]] = 1;
}
}  // namespace

extern "C" int mi_blur_color_preset(int preset, mi_blur_color *k)
{
    if (!k) return MI_BLUR_ERR_INVALID;
    switch (preset) {
    case MI_BLUR_COLOR_RGB2GRAY:
    case MI_BLUR_COLOR_BGR2GRAY:
        color_rows(k, 1, 16);
        for (int i = 0; i < 3; i++) k->m[0][i] = LUMA[preset == MI_BLUR_COLOR_RGB2GRAY ? i : 2 - i];
        k->bias[0] = CR;
        return MI_BLUR_OK;
    case MI_BLUR_COLOR_GRAY2RGB: { const int s[3] = {0, 0, 0}; color_permute(k, 3, s); return MI_BLUR_OK; }
    case MI_BLUR_COLOR_RGB2BGR: { const int s[3] = {2, 1, 0}; color_permute(k, 3, s); return MI_BLUR_OK; }
    case MI_BLUR_COLOR_RGBA2BGRA: { const int s[4] = {2, 1, 0, 3}; color_permute(k, 4, s); return MI_BLUR_OK; }
    case MI_BLUR_COLOR_RGBA2RGB: { const int s[3] = {0, 1, 2}; color_permute(k, 3, s); return MI_BLUR_OK; }
    case MI_BLUR_COLOR_RGB2RGBA: { const int s[4] = {0, 1, 2, -1}; color_permute(k, 4, s); k->bias[3] = 255; return MI_BLUR_OK; }
    case MI_BLUR_COLOR_RGB2YCBCR: {
        color_rows(k, 3, 16);
        const int32_t cb[3] = {-11058, -21710, 32768}, cr[3] = {32768, -27439, -5329};
        for (int i = 0; i < 3; i++) { k->m[0][i] = LUMA[i]; k->m[1][i] = cb[i]; k->m[2][i] = cr[i]; }
        k->bias[0] = CR; k->bias[1] = k->bias[2] = 128 * CQ + CR;
        return MI_BLUR_OK;
    }
    case MI_BLUR_COLOR_YCBCR2RGB: {
        color_rows(k, 3, 16);
        const int32_t r[3] = {CQ, 0, 91881}, g[3] = {CQ, -22553, -46802}, b[3] = {CQ, 116130, 0};
        for (int i = 0; i < 3; i++) { k->m[0][i] = r[i]; k->m[1][i] = g[i]; k->m[2][i] = b[i]; }
        k->bias[0] = CR - 128 * 91881; k->bias[1] = CR + 128 * (22553 + 46802); k->bias[2] = CR - 128 * 116130;
        return MI_BLUR_OK;
    }
    }
    return MI_BLUR_ERR_INVALID;
}

extern "C" int mi_blur_color_identity(int channels, mi_blur_color *k)
{
    if (!k || channels < 1 || channels > MI_BLUR_COLOR_MAX_CHANNELS) return MI_BLUR_ERR_INVALID;
    const int s[4] = {0, 1, 2, 3};
    color_permute(k, channels, s);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_color_lut_gamma(double gamma, uint8_t lut[256])
{
    if (!lut || !std::isfinite(gamma) || !(gamma > 0.0)) return MI_BLUR_ERR_INVALID;
    for (int v = 0; v < 256; v++) lut[v] = (uint8_t)std::floor(255.0 * std::pow((double)v / 255.0, gamma) + 0.5);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_color_lut_threshold(int t, int lo, int hi, uint8_t lut[256])
{
    if (!lut || t < -1 || t > 255 || lo < 0 || lo > 255 || hi < 0 || hi > 255) return MI_BLUR_ERR_INVALID;
    for (int v = 0; v < 256; v++) lut[v] = (uint8_t)(v > t ? hi : lo);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_color(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                     const mi_blur_color *k, void *stream)
{
    Filter f;
    return enqueue_filter(color_for(k, width, height, channels, &f), f, PreCheck::ARGS_SIZE, d_in, d_out, width, height,
                          channels, n_images, 0, height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// affine warp: fixed-point rotate, scale, shear, translate (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_warp_coord(const mi_blur_warp *w, int X, int Y, int *x0, int *y0, int *fx, int *fy)
{
    if (!w || !x0 || !y0 || !fx || !fy || X < 0 || Y < 0 || X >= MI_BLUR_RESIZE_MAX_DIM || Y >= MI_BLUR_RESIZE_MAX_DIM) return MI_BLUR_ERR_INVALID;
    mi_blur_warp probe = *w;                            // only the mode and the matrix count here
    probe.out_width = probe.out_height = 1; probe.border = MI_BLUR_WARP_CLAMP; probe.fill = 0;
    if (!warp_ok(&probe, 1, 1, 1)) return MI_BLUR_ERR_INVALID;
    const WarpPos s = warp_position(w->m, X, Y);
    const WarpAxis ax = warp_axis(s.sx, w->mode, 0), ay = warp_axis(s.sy, w->mode, 0);
    *x0 = ax.i0; *y0 = ay.i0; *fx = ax.f; *fy = ay.f;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_warp_rotation(double cx, double cy, double angle_deg, double scale, double fwd[6])
{
    if (!fwd || !std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(angle_deg) || !std::isfinite(scale)) return MI_BLUR_ERR_INVALID;
    const double rad = angle_deg * 3.14159265358979323846 / 180.0, a = scale * std::cos(rad), b = scale * std::sin(rad);
    fwd[0] = a; fwd[1] = b; fwd[2] = (1.0 - a) * cx - b * cy;
    fwd[3] = -b; fwd[4] = a; fwd[5] = b * cx + (1.0 - a) * cy;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_warp_set_matrix(mi_blur_warp *w, const double m[6], int inverse)
{
    if (!w || !m) return MI_BLUR_ERR_INVALID;
    double v[6];
    for (int i = 0; i < 6; i++) { if (!std::isfinite(m[i])) return MI_BLUR_ERR_INVALID; v[i] = m[i]; }
    if (!inverse) {
        const double det = m[0] * m[4] - m[1] * m[3];
        if (det == 0.0 || !std::isfinite(1.0 / det)) return MI_BLUR_ERR_INVALID;
        v[0] = m[4] / det; v[1] = -m[1] / det; v[3] = -m[3] / det; v[4] = m[0] / det;
        v[2] = -(v[0] * m[2] + v[1] * m[5]); v[5] = -(v[3] * m[2] + v[4] * m[5]);
    }
    int64_t q[6];
    for (int i = 0; i < 6; i++) {
        const double lim = i % 3 == 2 ? 70368744177664.0 : 67108864.0;      // 2^46, 2^26
        const double r = std::floor(v[i] * 65536.0 + 0.5);
        if (!(r >= -lim && r <= lim)) return MI_BLUR_ERR_INVALID;           // NaN fails both
        q[i] = (int64_t)r;
    }
    for (int i = 0; i < 6; i++) w->m[i] = q[i];
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_warp(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                    const mi_blur_warp *w, void *stream)
{
    Filter f;
    return enqueue_filter(warp_for(w, width, height, channels, &f), f, PreCheck::ARGS_SIZE, d_in, d_out, width, height,
                          channels, n_images, 0, height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// perspective warp: fixed-point homography (no reference analogue)
// ----------------------------------------------------------------------------------
static int warp_persp_for(const mi_blur_warp_perspective *w, int W, int H, int C, Filter *f)
{
    const int rc = filter_warp_persp(w, f);
    return rc ? rc : persp_ok(w, W, H, C) ? MI_BLUR_OK : MI_BLUR_ERR_INVALID;
}

extern "C" int mi_blur_warp_perspective_coord(const mi_blur_warp_perspective *w, int X, int Y, int64_t *x0, int64_t *y0, int *fx, int *fy)
{
    if (!w || !x0 || !y0 || !fx || !fy || X < 0 || Y < 0 || X >= MI_BLUR_RESIZE_MAX_DIM || Y >= MI_BLUR_RESIZE_MAX_DIM) return MI_BLUR_ERR_INVALID;
    if (w->mode != MI_BLUR_RESIZE_NEAREST && w->mode != MI_BLUR_RESIZE_BILINEAR) return MI_BLUR_ERR_INVALID;
    if (!persp_map_ok(MI_BLUR_WARP_CLAMP, 0, w->h, 1, 1)) return MI_BLUR_ERR_INVALID;     // the limits, and h8 >= 1
    const PerspPos s = persp_position(w->h, X, Y);
    if (s.d < 1) return MI_BLUR_ERR_INVALID;
    const PerspAxis ax = persp_axis(s.nx, s.d, 0.0, w->mode, 0), ay = persp_axis(s.ny, s.d, 0.0, w->mode, 0);
    *x0 = ax.i0; *y0 = ay.i0; *fx = ax.f; *fy = ay.f;
    return MI_BLUR_OK;
}

// The 8 x 8 system of getPerspectiveTransform, by elimination with partial pivoting.
extern "C" int mi_blur_warp_perspective_quad(const double src[8], const double dst[8], double H[9])
{
    if (!src || !dst || !H) return MI_BLUR_ERR_INVALID;
    double scale = 0.0;
    for (int i = 0; i < 8; i++) {
        if (!std::isfinite(src[i]) || !std::isfinite(dst[i])) return MI_BLUR_ERR_INVALID;
        scale = std::max(scale, std::max(std::fabs(src[i]), std::fabs(dst[i])));
    }
    for (const double *p : {src, dst})                  // three collinear points: twice the triangle's area is 0
        for (int skip = 0; skip < 4; skip++) {
            const int a = skip == 0 ? 1 : 0, b = skip <= 1 ? 2 : 1, c = skip <= 2 ? 3 : 2;
            const double cross = (p[2 * b] - p[2 * a]) * (p[2 * c + 1] - p[2 * a + 1]) - (p[2 * b + 1] - p[2 * a + 1]) * (p[2 * c] - p[2 * a]);
            if (!(std::fabs(cross) > 1e-12 * scale * scale)) return MI_BLUR_ERR_INVALID;
        }
    double A[8][9];
    for (int i = 0; i < 4; i++) {
        const double x = src[2 * i], y = src[2 * i + 1], u = dst[2 * i], v = dst[2 * i + 1];
        const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, u}, r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
        std::copy(r0, r0 + 9, A[2 * i]);
        std::copy(r1, r1 + 9, A[2 * i + 1]);
    }
    for (int col = 0; col < 8; col++) {
        int piv = col;
        for (int r = col + 1; r < 8; r++)
            if (std::fabs(A[r][col]) > std::fabs(A[piv][col])) piv = r;
        if (A[piv][col] == 0.0) return MI_BLUR_ERR_INVALID;
        if (piv != col) std::swap_ranges(A[piv], A[piv] + 9, A[col]);
        for (int r = 0; r < 8; r++) {
            if (r == col) continue;
            const double f = A[r][col] / A[col][col];
            for (int k = col; k < 9; k++) A[r][k] -= f * A[col][k];
        }
    }
    double out[9];
    for (int i = 0; i < 8; i++) {
        out[i] = A[i][8] / A[i][i];
        if (!std::isfinite(out[i])) return MI_BLUR_ERR_INVALID;
    }
    out[8] = 1.0;
    std::copy(out, out + 9, H);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_warp_perspective_set_matrix(mi_blur_warp_perspective *w, const double H[9], int inverse)
{
    if (!w || !H) return MI_BLUR_ERR_INVALID;
    double v[9];
    for (int i = 0; i < 9; i++) { if (!std::isfinite(H[i])) return MI_BLUR_ERR_INVALID; v[i] = H[i]; }
    if (!inverse) {                                     // the adjugate; the determinant only scales it, and the division by v[8] below takes any scale out
        const double det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
        if (det == 0.0 || !std::isfinite(det)) return MI_BLUR_ERR_INVALID;
        v[0] = H[4] * H[8] - H[5] * H[7]; v[1] = H[2] * H[7] - H[1] * H[8]; v[2] = H[1] * H[5] - H[2] * H[4];
        v[3] = H[5] * H[6] - H[3] * H[8]; v[4] = H[0] * H[8] - H[2] * H[6]; v[5] = H[2] * H[3] - H[0] * H[5];
        v[6] = H[3] * H[7] - H[4] * H[6]; v[7] = H[1] * H[6] - H[0] * H[7]; v[8] = H[0] * H[4] - H[1] * H[3];
    }
    const double v8 = v[8];
    if (v8 == 0.0 || !std::isfinite(v8)) return MI_BLUR_ERR_INVALID;
    for (int i = 0; i < 9; i++) { v[i] /= v8; if (!std::isfinite(v[i])) return MI_BLUR_ERR_INVALID; }
    int k = 30;
    for (; k >= 0; k--) {
        bool fits = true;
        for (int i = 0; i < 9; i++) fits = fits && std::fabs(v[i]) * std::ldexp(1.0, k) <= (i % 3 == 2 ? 281474976710655.0 : 4294967295.0);   // 2^48 - 1, 2^32 - 1
        if (fits) break;
    }
    if (k < 0) return MI_BLUR_ERR_INVALID;
    mi_blur_warp_perspective q = *w;
    for (int i = 0; i < 9; i++) q.h[i] = (int64_t)std::floor(std::ldexp(v[i], k) + 0.5);
    if (q.out_width < 1 || q.out_height < 1 || q.out_width > MI_BLUR_RESIZE_MAX_DIM || q.out_height > MI_BLUR_RESIZE_MAX_DIM ||
        !persp_map_ok(MI_BLUR_WARP_CLAMP, 0, q.h, q.out_width, q.out_height))
        return MI_BLUR_ERR_INVALID;
    for (int i = 0; i < 9; i++) w->h[i] = q.h[i];
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_warp_perspective(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                                const mi_blur_warp_perspective *w, void *stream)
{
    Filter f;
    return enqueue_filter(warp_persp_for(w, width, height, channels, &f), f, PreCheck::ARGS_SIZE, d_in, d_out, width, height,
                          channels, n_images, 0, height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// remap: fixed-point sampling through a per-pixel map (no reference analogue)
// ----------------------------------------------------------------------------------
// map: device memory for a launch, host memory for the CPU device; the Filter points at it, it is not copied here.
static int remap_for(const mi_blur_remap *r, const int32_t *map, int W, int H, int C, Filter *f)
{
    const int rc = filter_remap(r, map, f);
    return rc ? rc : remap_ok(r, W, H, C) && (uintptr_t)map % 4 == 0 ? MI_BLUR_OK : MI_BLUR_ERR_INVALID;
}

extern "C" int mi_blur_remap_coord(const mi_blur_remap *r, int W, int H, int32_t px, int32_t py, int *x0, int *y0, int *fx, int *fy)
{
    if (!r || !x0 || !y0 || !fx || !fy || W < 1 || H < 1 || W > MI_BLUR_RESIZE_MAX_DIM || H > MI_BLUR_RESIZE_MAX_DIM) return MI_BLUR_ERR_INVALID;
    if (r->mode != MI_BLUR_RESIZE_NEAREST && r->mode != MI_BLUR_RESIZE_BILINEAR) return MI_BLUR_ERR_INVALID;
    const WarpCoord q = remap_coord(px, py, r->mode, W, H);
    *x0 = q.x0; *y0 = q.y0; *fx = q.fx; *fy = q.fy;
    return MI_BLUR_OK;
}

// q(v) = floor(v * 2048 + 0.5) clamped into [-2^30, 2^30]; v finite.
static int32_t remap_quantise(double v)
{
    const double q = std::floor(v * 2048.0 + 0.5), lim = 1073741824.0;
    return (int32_t)(q < -lim ? -lim : q > lim ? lim : q);
}

extern "C" int mi_blur_remap_from_float(const float *map_x, const float *map_y, size_t n, int32_t *map)
{
    if (!map_x || !map_y || !map) return MI_BLUR_ERR_INVALID;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(map_x[i]) || !std::isfinite(map_y[i])) return MI_BLUR_ERR_INVALID;
    for (size_t i = 0; i < n; i++) { map[2 * i] = remap_quantise((double)map_x[i]); map[2 * i + 1] = remap_quantise((double)map_y[i]); }
    return MI_BLUR_OK;
}

extern "C" int mi_blur_remap_undistort(const double K[4], const double dist[5], const double new_K[4], int out_width, int out_height, int32_t *map)
{
#pragma clang fp contract(off)      // every product and sum rounded on its own: a restatement in any language can match it
    if (!K || !dist || !map || out_width < 1 || out_height < 1 || out_width > MI_BLUR_RESIZE_MAX_DIM || out_height > MI_BLUR_RESIZE_MAX_DIM)
        return MI_BLUR_ERR_INVALID;
    const double *N = new_K ? new_K : K;
    for (int i = 0; i < 4; i++) if (!std::isfinite(K[i]) || !std::isfinite(N[i])) return MI_BLUR_ERR_INVALID;
    for (int i = 0; i < 5; i++) if (!std::isfinite(dist[i])) return MI_BLUR_ERR_INVALID;
    if (N[0] == 0.0 || N[1] == 0.0) return MI_BLUR_ERR_INVALID;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    for (int Y = 0; Y < out_height; Y++)
        for (int X = 0; X < out_width; X++) {
            const double x = ((double)X - N[2]) / N[0], y = ((double)Y - N[3]) / N[1];
            const double r2 = x * x + y * y;
            const double rad = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
            const double xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
            const double yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
            const double u = fx * xd + cx, v = fy * yd + cy;
            if (!std::isfinite(u) || !std::isfinite(v)) return MI_BLUR_ERR_INVALID;
            int32_t *e = map + ((size_t)Y * (size_t)out_width + (size_t)X) * 2;
            e[0] = remap_quantise(u); e[1] = remap_quantise(v);
        }
    return MI_BLUR_OK;
}

extern "C" int mi_blur_remap_plan(const int32_t *host_map, int width, int height, int channels, const mi_blur_remap *r, mi_blur_remap_tiles *tiles)
{
    Filter f;
    if (!tiles || remap_for(r, host_map, width, height, channels, &f)) return MI_BLUR_ERR_INVALID;
    *tiles = mi_blur_remap_tiles{};
    if (!remap_shape_tiled(width, channels, f.out_w, f.sample_mode)) return MI_BLUR_OK;
    tiles->tiled = 1;
    remap_walk(host_map, width, height, channels, f.out_w, f.out_h, f.warp_border, f.remap_stage_bytes, tiles);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_remap(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                     const mi_blur_remap *r, const int32_t *d_map, void *stream)
{
    Filter f;
    const int built = (const void *)d_map == (const void *)d_out ? MI_BLUR_ERR_INVALID : remap_for(r, d_map, width, height, channels, &f);
    return enqueue_filter(built, f, PreCheck::ARGS_SIZE, d_in, d_out, width, height, channels, n_images, 0, height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// median blur, radius 1..7 (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_enqueue_median_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                                           int radius, int out_row_begin, int out_row_end, void *stream)
{
    Filter f;
    return enqueue_filter(filter_median(radius, &f), f, PreCheck::ARGS, d_in, d_out, width, band_rows, channels, 1,
                          out_row_begin, out_row_end, MI_BLUR_VARIANT_AUTO, stream);
}

extern "C" int mi_blur_enqueue_median(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int radius,
                                      int n_images, void *stream)
{
    Filter f;
    return enqueue_filter(filter_median(radius, &f), f, PreCheck::ARGS, d_in, d_out, width, height, channels, n_images, 0,
                          height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// erode / dilate / morphological gradient, radii 0..16 per axis (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_enqueue_morph_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels, int op,
                                          int rx, int ry, int out_row_begin, int out_row_end, void *stream)
{
    Filter f;
    return enqueue_filter(filter_morph(op, rx, ry, &f), f, PreCheck::ARGS, d_in, d_out, width, band_rows, channels, 1,
                          out_row_begin, out_row_end, MI_BLUR_VARIANT_AUTO, stream);
}

extern "C" int mi_blur_enqueue_morph(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int op, int rx,
                                     int ry, int n_images, void *stream)
{
    Filter f;
    return enqueue_filter(filter_morph(op, rx, ry, &f), f, PreCheck::ARGS, d_in, d_out, width, height, channels, n_images, 0,
                          height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// bilateral filter, radius 1..8, integer tables (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_bilateral_gauss(double sigma_space, double sigma_range, int radius, mi_blur_bilateral *k)
{
    if (!k || !(sigma_range > 0.0) || radius < 1 || radius > MI_BLUR_BILATERAL_MAX_RADIUS) return MI_BLUR_ERR_INVALID;
    if (!(sigma_space > 0.0)) sigma_space = radius / 2.0;
    mi_blur_bilateral g{};
    g.radius = radius;
    const int n = 2 * radius + 1;
    for (int j = -radius; j <= radius; j++)
        for (int i = -radius; i <= radius; i++)
            g.spatial[(j + radius) * n + (i + radius)] =
                (uint8_t)std::floor(128.0 * std::exp(-(double)(i * i + j * j) / (2.0 * sigma_space * sigma_space)) + 0.5);
    for (int d = 0; d < 256; d++) g.range[d] = (uint8_t)std::floor(255.0 * std::exp(-(double)d * d / (2.0 * sigma_range * sigma_range)) + 0.5);
    *k = g;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_bilateral_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                                              int out_row_begin, int out_row_end, const mi_blur_bilateral *k, void *stream)
{
    Filter f;
    return enqueue_filter(filter_bilateral(k, &f), f, PreCheck::ARGS, d_in, d_out, width, band_rows, channels, 1,
                          out_row_begin, out_row_end, MI_BLUR_VARIANT_AUTO, stream);
}

extern "C" int mi_blur_enqueue_bilateral(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                         const mi_blur_bilateral *k, void *stream)
{
    Filter f;
    return enqueue_filter(filter_bilateral(k, &f), f, PreCheck::ARGS, d_in, d_out, width, height, channels, n_images, 0,
                          height, MI_BLUR_VARIANT_AUTO, stream);
}

// ----------------------------------------------------------------------------------
// 2-D convolution with signed integer taps, radii 0..7 per axis (no reference analogue)
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_conv_preset(int preset, mi_blur_conv *k)
{
    static const int16_t SOBEL[9] = {-1, 0, 1, -2, 0, 2, -1, 0, 1}, SCHARR[9] = {-3, 0, 3, -10, 0, 10, -3, 0, 3};
    static const int16_t LAP4[9] = {0, 1, 0, 1, -4, 1, 0, 1, 0}, LAP8[9] = {1, 1, 1, 1, -8, 1, 1, 1, 1};
    static const int16_t SHARPEN[9] = {0, -1, 0, -1, 5, -1, 0, -1, 0}, EMBOSS[9] = {-2, -1, 0, -1, 1, 1, 0, 1, 2};
    if (!k || preset < MI_BLUR_CONV_SOBEL_X || preset > MI_BLUR_CONV_EMBOSS) return MI_BLUR_ERR_INVALID;
    mi_blur_conv g{};
    g.rx = g.ry = 1;
    g.mode = MI_BLUR_CONV_ABS;
    const int16_t *x = nullptr, *y = nullptr;           // x: taken as is; y: taken transposed
    switch (preset) {
    case MI_BLUR_CONV_SOBEL_X: x = SOBEL; break;
    case MI_BLUR_CONV_SOBEL_Y: y = SOBEL; break;
    case MI_BLUR_CONV_SOBEL_MAG: x = y = SOBEL; g.mode = MI_BLUR_CONV_MAG; break;
    case MI_BLUR_CONV_SCHARR_X: x = SCHARR; break;
    case MI_BLUR_CONV_SCHARR_Y: y = SCHARR; break;
    case MI_BLUR_CONV_SCHARR_MAG: x = y = SCHARR; g.mode = MI_BLUR_CONV_MAG; break;
    case MI_BLUR_CONV_LAPLACIAN4: x = LAP4; break;
    case MI_BLUR_CONV_LAPLACIAN8: x = LAP8; break;
    case MI_BLUR_CONV_SHARPEN: x = SHARPEN; g.mode = MI_BLUR_CONV_SAT; break;
    default: x = EMBOSS; g.mode = MI_BLUR_CONV_SAT; g.bias = 128; break;
    }
    int16_t *ydst = x ? g.k2 : g.k;                     // the y table is the second one only beside an x table
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) {
            if (x) g.k[j * 3 + i] = x[j * 3 + i];
            if (y) ydst[j * 3 + i] = y[i * 3 + j];
        }
    *k = g;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_conv_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                                         int out_row_begin, int out_row_end, const mi_blur_conv *k, void *stream)
{
    Filter f;
    return enqueue_filter(filter_conv(k, &f), f, PreCheck::ARGS_ROWS, d_in, d_out, width, band_rows, channels, 1,
                          out_row_begin, out_row_end, MI_BLUR_VARIANT_AUTO, stream);
}

extern "C" int mi_blur_enqueue_conv(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                    const mi_blur_conv *k, void *stream)
{
    Filter f;
    return enqueue_filter(filter_conv(k, &f), f, PreCheck::ARGS, d_in, d_out, width, height, channels, n_images, 0, height,
                          MI_BLUR_VARIANT_AUTO, stream);
}

// Frame layout on the device (replaces the host loops heterogeneous_blur.c:125-134 and split_image_blur.c:40-56).
extern "C" int mi_blur_planar_to_interleaved(const uint8_t *d_planar, uint8_t *d_interleaved, int width, int height,
                                             int channels, int n_images, void *stream)
{
    if (mi_blur_device_count() <= 0) return MI_BLUR_ERR_NO_DEVICE;
    return launch_planar_to_interleaved(d_planar, d_interleaved, width, height, channels, n_images, (hipStream_t)stream);
}

extern "C" int mi_blur_interleaved_to_planar(const uint8_t *d_interleaved, uint8_t *d_planar, int width, int height,
                                             int channels, int n_images, void *stream)
{
    if (mi_blur_device_count() <= 0) return MI_BLUR_ERR_NO_DEVICE;
    return launch_interleaved_to_planar(d_interleaved, d_planar, width, height, channels, n_images, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------
// queue level
// ----------------------------------------------------------------------------------
namespace {

static int staging_threads_env()
{
    const char *e = getenv("MI_BLUR_STAGING_THREADS");
    const int n = e ? atoi(e) : 0;
    return n >= 1 && n <= 64 ? n : 8;
}
// pageable caller memory <-> pinned staging: one thread moves ~10 GB/s, the link wants ~45 GB/s each way (8 threads: 220 k
// img/s at batch 35 and 500; 4: 145-180 k; MI_BLUR_STAGING_THREADS overrides)
static const int STAGING_COPY_THREADS = staging_threads_env();

struct Slot {
    hipStream_t stream = nullptr;
    uint8_t *h_in = nullptr, *h_out = nullptr;   // pinned staging (used when the caller's memory is pageable)
    uint8_t *d_in = nullptr, *d_out = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // H2D begin/end, D2H begin/end
    hipEvent_t ks = nullptr, ke = nullptr;                     // kernel dispatch start/stop
    bool busy = false;
    uint8_t *user_out = nullptr;
    size_t out_bytes = 0, out_band = 0, out_stride = 0;   // pending read-back: out_n bands of out_band bytes
    int out_n = 0;
    bool out_staged = false;
    bool zero_copy = false;                               // in flight on the context's zero-copy stream
    bool zc_plain = false;                                // ... as a plain launch without events (experiment)
    hipStream_t zc_stream = nullptr;
    bool zc_server = false;                               // ... as batch zc_index of the context's batch server
    unsigned zc_index = 0;
};

struct TimedLaunch { hipEvent_t s, e; };

// Host side of the zero-copy batch server (blur_launch.h): the descriptor ring in pinned memory, the device-side
// hand-off words, the stream the servers queue on, and what has been published / launched so far.
struct ZcServer {
    ZcHostCtl *ctl = nullptr, *ctl_dev = nullptr;          // pinned host memory and its device address
    ZcDevCtl *dev = nullptr;
    hipStream_t stream = nullptr;
    ZcGeometry geo{};
    unsigned head = 0, launched = 0, tile_base = 0;
    unsigned n_workers = 96, budget = 256, idle_ticks = 30000;
    unsigned long long covered = 0;                      // kernel bucket: the union of [t_begin, t_end] so far reaches this tick
    unsigned long long *trace = nullptr;                 // diagnostics ("zero_copy_trace"): device buffer of per-worker phase stamps
    int fixed_share = 0;                                 // A/B: "zero_copy_tickets" 0
};

// The CPU device's queue: submits run one after another on ONE long-lived thread per context (each of them spreads over the
// worker pool inside cpu_blur_batch) — a thread per submit cost ~60 us, most of a small batch's time.
struct CpuJob {
    std::function<void()> work;
    double ms = 0.0;
    bool done = false;
};
struct CpuWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    std::deque<CpuJob *> q;
    bool stop = false;
    void loop()
    {
        for (;;) {
            CpuJob *j = nullptr;
            {
                std::unique_lock<std::mutex> lk(m);
                cv_work.wait(lk, [&] { return stop || !q.empty(); });
                if (q.empty()) return;                   // stop, nothing left
                j = q.front(); q.pop_front();
            }
            const auto t0 = std::chrono::steady_clock::now();
            j->work();
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            { std::lock_guard<std::mutex> lk(m); j->ms = ms; j->done = true; }
            cv_done.notify_all();
        }
    }
    void push(CpuJob *j)
    {
        { std::lock_guard<std::mutex> lk(m); q.push_back(j); }
        if (!th.joinable()) th = std::thread([this] { loop(); });
        cv_work.notify_one();
    }
    void wait(CpuJob *j)
    {
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return j->done; });
    }
    ~CpuWorker()
    {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv_work.notify_all();
        if (th.joinable()) th.join();
    }
};

}  // namespace

struct mi_blur_ctx {
    int device = 0, W = 0, H = 0, C = 0, max_batch = 0, n_threads = 0;
    Filter filter{};                                             // every submit applies it: mi_blur_create's radius, or what a mi_blur_ctx_set_* put in its place
    size_t image_bytes = 0;
    std::vector<Slot> slots;
    int next_slot = 0;
    mi_blur_timing tm{};
    // resident pool
    uint8_t *pool_in = nullptr, *pool_out = nullptr;
    int pool_images = 0;
    long long cursor = 0;
    int rr = 0;
    std::vector<TimedLaunch> ev_pool;
    size_t ev_used = 0;
    uint64_t timed_launches = 0, timed_bytes_alg = 0;   // resident launches that carried timestamp events
    uint64_t zero_copy_launches = 0;
    // Zero-copy launches of one context may overlap (several streams).  Their kernel bucket is the time during which at
    // least ONE of them was executing — the union of the dispatch intervals, measured against a reference event recorded
    // before the first of them since the last sync — not the sum of overlapping durations.
    hipEvent_t zc_ref = nullptr;
    bool zc_ref_valid = false;
    double zc_covered_ms = 0.0;                                  // the union so far reaches this far past zc_ref
    // fused stream: per-batch completion counters (device) and flags (pinned host memory)
    unsigned *fused_count = nullptr, *fused_host = nullptr;    // device counters; pinned host copy for polling
    int fused_cap = 0, fused_batches = 0;
    unsigned fused_tpb = 0, fused_wpb = 0, fused_blocks = 0;     // geometry of the latest fused pass
    unsigned fused_k = 8;                                        // ... and how many counters each of its batches uses (8 .. 256)
    int fused_n = 0, fused_batch = 0;                            // its (n_images, batch): same again = counters keep counting up
    unsigned fused_passes = 0;                                   // passes accumulated in the counters since they were zeroed
    hipStream_t fused_poll = nullptr;
    unsigned long long *fused_word = nullptr, *fused_word_dev = nullptr;   // watcher's progress word: pinned host memory + its device address
    unsigned fused_watch_seq = 0;                                // sequence number of the latest watched pass (0 = none)
    bool fused_watched = false;                                  // the latest pass has a watcher
    bool fused_watch_busy = false;                               // a watcher was launched and its stream not waited for since
    // overlap of consecutive fused passes ("fused_overlap"): they alternate between slot 0's stream and this one, each behind a
    // one-wave gate kernel that ends when its predecessor raises the gate word (device memory, behind the counters).  The
    // watcher of a watched pass runs here too.
    hipStream_t fused_second = nullptr;
    hipEvent_t fused_ev = nullptr;                               // orders the slot streams behind what fused_second holds
    unsigned fused_seq = 0;                                      // number of the latest fused pass; only ever grows
    bool fused_gated = false;                                    // that pass raises the gate word to fused_seq
    bool fused_on_second = false;                                // ... and was issued to fused_second
    bool fused_second_busy = false;                              // fused_second got a pass since the slot streams last waited for it
    ZcServer *zc = nullptr;                                      // batch server, made on the first submit that can use it
    std::vector<float> place_ms;                                 // resident pool: per-launch ms of each candidate placement tried
    int place_kept = 0;
    // CPU device
    std::vector<CpuJob *> cpu_jobs;
    CpuWorker *cpu_worker = nullptr;
    bool submitted = false;                                      // the mi_blur_ctx_set_* work only before this
    // the context's copy of a remap's map (mi_blur_ctx_set_remap; filter.remap_map points at it): device memory on a GPU
    // context, the vector on the CPU device.  ctx_drop_map() frees it: when another setter replaces the remap, and in mi_blur_destroy
    int32_t *remap_dev = nullptr;
    std::vector<int32_t> remap_host;
    bool is_cpu() const { return device == MI_BLUR_DEVICE_CPU; }
};

// Frees the context's copy of a remap's map, if it has one.  Only before the first submit or in mi_blur_destroy (after the
// streams and the CPU worker have been waited for), so nothing in flight reads it.
static void ctx_drop_map(mi_blur_ctx *c)
{
    if (c->remap_dev) { (void)hipSetDevice(c->device); (void)hipFree(c->remap_dev); c->remap_dev = nullptr; }
    std::vector<int32_t>().swap(c->remap_host);
}

static bool is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// The device-side address of pinned (hipHostMalloc'd or registered) host memory, nullptr for anything else.
static uint8_t *pinned_device_ptr(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return a.type == hipMemoryTypeHost ? (uint8_t *)a.devicePointer : nullptr;
}

extern "C" void *mi_blur_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (mi_blur_device_count() > 0) {
        // portable + mapped: visible to every GPU's contexts (A1 hands one batch buffer to G devices, each of which
        // may work on its share in place)
        if (hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess) return p;
        (void)hipGetLastError();
        return nullptr;
    }
    return malloc(bytes);   // CPU-only operation: ordinary memory
}

extern "C" int mi_blur_host_register(void *p, size_t bytes)
{
    if (!p || bytes == 0) return MI_BLUR_ERR_INVALID;
    if (mi_blur_device_count() <= 0) return MI_BLUR_OK;
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped));
    return MI_BLUR_OK;
}

extern "C" int mi_blur_host_unregister(void *p)
{
    if (!p) return MI_BLUR_ERR_INVALID;
    if (mi_blur_device_count() <= 0) return MI_BLUR_OK;
    HIP_TRY(hipHostUnregister(p));
    return MI_BLUR_OK;
}

extern "C" void mi_blur_host_free(void *p)
{
    if (!p) return;
    if (mi_blur_device_count() > 0 && is_pinned(p)) { (void)hipHostFree(p); return; }
    free(p);
}

// ----------------------------------------------------------------------------------
// NUMA placement of per-GPU host work.  The reference drives both of its devices from one
// host thread on a one-socket desktop (heterogeneous_blur.c:482-539); an 8-GPU MI355X node has two sockets with four
// GPUs each, and a feeder thread, a batch-building memcpy or a pinned buffer on the other socket puts every byte of
// the stream on the inter-socket link first.  No libnuma: the GPU's PCI bus id -> sysfs local_cpulist -> sched_setaffinity.
// ----------------------------------------------------------------------------------
static bool affinity_disabled()
{
    const char *e = getenv("MI_BLUR_NO_AFFINITY");
    return e && atoi(e) != 0;
}

// "0-63,128-191" -> cpu_set_t; false when the text holds no CPU
static bool parse_cpulist(const char *text, cpu_set_t *set)
{
    CPU_ZERO(set);
    bool any = false;
    for (const char *p = text; *p;) {
        char *end = nullptr;
        long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        if (*end == '-') { p = end + 1; b = strtol(p, &end, 10); if (end == p) break; }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++) if (c >= 0) { CPU_SET((int)c, set); any = true; }
        p = end;
        while (*p == ',' || *p == ' ' || *p == '\n') p++;
    }
    return any;
}

static int device_sysfs(int device, const char *leaf, char *buf, size_t n)
{
    if (!buf || n == 0) return MI_BLUR_ERR_INVALID;
    buf[0] = 0;
    const int ndev = mi_blur_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev) return MI_BLUR_ERR_NO_DEVICE;
    char bdf[64] = {0};
    HIP_TRY(hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device));
    for (char *q = bdf; *q; q++) if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');     // sysfs spells it in lower case
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/%s", bdf, leaf);
    FILE *f = fopen(path, "r");
    if (!f) return MI_BLUR_ERR_UNSUPPORTED;
    const bool ok = fgets(buf, (int)n, f) != nullptr;
    fclose(f);
    if (!ok) { buf[0] = 0; return MI_BLUR_ERR_UNSUPPORTED; }
    for (size_t i = strlen(buf); i > 0 && (buf[i - 1] == '\n' || buf[i - 1] == ' '); i--) buf[i - 1] = 0;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_device_cpulist(int device, char *buf, size_t n, int *numa_node)
{
    if (numa_node) {
        char nb[32];
        *numa_node = device_sysfs(device, "numa_node", nb, sizeof nb) == MI_BLUR_OK ? atoi(nb) : -1;
    }
    return device_sysfs(device, "local_cpulist", buf, n);
}

extern "C" int mi_blur_bind_thread_to_device(int device)
{
    if (affinity_disabled()) return 0;
    char list[512];
    if (device_sysfs(device, "local_cpulist", list, sizeof list) != MI_BLUR_OK) return 0;
    cpu_set_t local, allowed, both;
    if (!parse_cpulist(list, &local)) return 0;
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return 0;
    CPU_AND(&both, &local, &allowed);
    const int n = CPU_COUNT(&both);
    if (n == 0) return 0;                                        // a cpuset that excludes the GPU's socket: leave the thread alone
    if (sched_setaffinity(0, sizeof both, &both) != 0) return 0;
    return n;
}

extern "C" void *mi_blur_host_alloc_on(int device, size_t bytes)
{
    if (mi_blur_device_count() <= 0) return malloc(bytes);
    int prev = 0;
    (void)hipGetDevice(&prev);
    cpu_set_t saved;
    const bool have_saved = sched_getaffinity(0, sizeof saved, &saved) == 0;
    // pin + map with the GPU current and from one of its socket's CPUs: the runtime takes the pages from the host pool
    // nearest the current device, and whatever it leaves to first touch is touched from there as well
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    const int bound = mi_blur_bind_thread_to_device(device);
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
    if (bound > 0 && have_saved) (void)sched_setaffinity(0, sizeof saved, &saved);
    (void)hipSetDevice(prev);
    return p;
}

static void free_slot(Slot &s)
{
    if (s.h_in) (void)hipHostFree(s.h_in);
    if (s.h_out) (void)hipHostFree(s.h_out);
    if (s.d_in) (void)hipFree(s.d_in);
    if (s.d_out) (void)hipFree(s.d_out);
    for (auto &e : s.ev) if (e) (void)hipEventDestroy(e);
    if (s.ks) (void)hipEventDestroy(s.ks);
    if (s.ke) (void)hipEventDestroy(s.ke);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = Slot{};
}

// Context + queue + buffers: heterogeneous_blur.c:194-212 (contexts, profiling queues),
// :341-354 (one in + one out buffer per device).  Here: n_slots streams, each with a
// max_batch-image device buffer pair, so one launch covers a whole batch.
extern "C" int mi_blur_create(mi_blur_ctx **out_ctx, int device, int width, int height, int channels, int radius,
                              int max_batch, int n_slots, int n_threads)
{
    if (!out_ctx) return MI_BLUR_ERR_INVALID;
    *out_ctx = nullptr;
    if (width <= 0 || height <= 0 || channels <= 0 || max_batch <= 0 || n_slots <= 0) return MI_BLUR_ERR_INVALID;
    Filter box;
    if (filter_box(radius, &box)) return MI_BLUR_ERR_INVALID;
    if ((long long)width * channels * height > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    mi_blur_ctx *c = new (std::nothrow) mi_blur_ctx;
    if (!c) return MI_BLUR_ERR_NOMEM;
    c->device = device; c->W = width; c->H = height; c->C = channels; c->filter = box;
    c->max_batch = max_batch;
    // 0 = automatic: all cores up to 16.  Waking hundreds of workers for a ~1 ms batch costs more than it returns
    // (256-thread host, 256x256x3, batch 35: 8.5 k img/s with 256 workers, 235 k with 16, 190 k with 32); ask explicitly for more.
    c->n_threads = n_threads > 0 ? n_threads : std::min(hardware_threads(), 16);
    c->image_bytes = (size_t)width * height * channels;
    if (device == MI_BLUR_DEVICE_CPU) { *out_ctx = c; return MI_BLUR_OK; }

    const int ndev = mi_blur_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev) { delete c; return MI_BLUR_ERR_NO_DEVICE; }
    int rc = MI_BLUR_OK;
    auto fail = [&](hipError_t e) { (void)hipGetLastError(); rc = MI_BLUR_ERR_HIP_BASE - (int)e; return true; };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { fail(e); delete c; return rc; }
    c->slots.resize(n_slots);
    for (auto &s : c->slots) {
        if ((e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess && fail(e)) break;
        // the slot's pinned staging pair and device pair (max_batch images each) are made by the first submit that needs them
        // (slot_staging / slot_device): a context whose submits are all in place — pinned caller buffers, the recommended
        // form — never allocates them (a batch of 5000 320x240 frames on 4 slots: 18 GB and ~4 s of set-up otherwise)
        for (auto &ev : s.ev) if ((e = hipEventCreate(&ev)) != hipSuccess && fail(e)) break;
        if (rc) break;
        if ((e = hipEventCreate(&s.ks)) != hipSuccess && fail(e)) break;
        if ((e = hipEventCreate(&s.ke)) != hipSuccess && fail(e)) break;
    }
    // the fused stream's second stream comes right after the slots': HIP hands hardware queues to streams in creation order
    if (!rc && (e = hipStreamCreateWithFlags(&c->fused_second, hipStreamNonBlocking)) != hipSuccess) fail(e);
    if (!rc && (e = hipEventCreateWithFlags(&c->fused_ev, hipEventDisableTiming)) != hipSuccess) fail(e);
    if (rc) { mi_blur_destroy(c); return rc; }
    *out_ctx = c;
    return MI_BLUR_OK;
}

// Bytes of the output block of one band of the context's filter (out_shape(), filter.h).
static size_t out_band_bytes(const mi_blur_ctx *c, int band_rows, int y0, int y1)
{
    const OutShape o = out_shape(c->filter, c->W, band_rows, c->C, y0, y1);
    return (size_t)o.width * (size_t)o.channels * (size_t)o.rows;
}
// Bytes of a slot's output buffers per image: a resize, or a colour transform to more channels, may write more than it reads.  The filter is known by the time a
// slot's buffers are made (setters work only before the first submit); every other context: image_bytes, as before.
static size_t slot_out_image_bytes(const mi_blur_ctx *c) { return std::max(c->image_bytes, out_band_bytes(c, c->H, 0, c->H)); }

// Lazily made slot buffers (see mi_blur_create).  HIP's allocation calls are synchronous with respect to the device only
// where they must be; the slot's streams carry nothing that touches these buffers before they exist.
static int slot_staging(mi_blur_ctx *c, Slot &s, bool in, bool out)
{
    const size_t bytes = c->image_bytes * (size_t)c->max_batch, out_bytes = slot_out_image_bytes(c) * (size_t)c->max_batch;
    if (in && !s.h_in) HIP_TRY(hipHostMalloc((void **)&s.h_in, bytes, hipHostMallocDefault));
    if (out && !s.h_out) HIP_TRY(hipHostMalloc((void **)&s.h_out, out_bytes, hipHostMallocDefault));
    return MI_BLUR_OK;
}
static int slot_device(mi_blur_ctx *c, Slot &s)
{
    const size_t bytes = c->image_bytes * (size_t)c->max_batch, out_bytes = slot_out_image_bytes(c) * (size_t)c->max_batch;
    if (!s.d_in) HIP_TRY(hipMalloc((void **)&s.d_in, bytes));
    if (!s.d_out) HIP_TRY(hipMalloc((void **)&s.d_out, out_bytes));
    return MI_BLUR_OK;
}

static int finish_slot(mi_blur_ctx *c, Slot &s)
{
    if (!s.busy) return MI_BLUR_OK;
    float ms = 0.f;
    if (s.zero_copy && s.zc_server) {                            // batch zc_index of the batch server: wait for its done word
        ZcServer &z = *c->zc;
        const unsigned slot = s.zc_index % ZC_RING, want = s.zc_index + 1u;
        const auto t0 = std::chrono::steady_clock::now();
        // Waiting is a feeder's normal state (a batch takes ~160 us of link time): spin for ~20 us — a batch that is nearly
        // done should be noticed at once — then sleep in short steps so that the core is free for the threads that build
        // the next batch; every few ms ask the stream whether the device is still alive.
        const bool spin_only = tunables().zero_copy_spin != 0;
        for (unsigned spins = 0; __atomic_load_n(&z.ctl->done[slot], __ATOMIC_ACQUIRE) != want; spins++) {
            if (spins < 2048) { __builtin_ia32_pause(); continue; }
            if (__atomic_load_n(&z.ctl->error, __ATOMIC_ACQUIRE)) return MI_BLUR_ERR_STATE;   // a server gave up on a wait (see blur_server_kernel)
            if (spin_only) std::this_thread::yield();
            else { struct timespec ts = {0, 20000}; nanosleep(&ts, nullptr); }
            if ((spins & 63u) == 0) {                            // a faulted device never writes the word: ask the stream now and then
                const hipError_t q = hipStreamQuery(z.stream);
                if (q != hipSuccess && q != hipErrorNotReady) { (void)hipGetLastError(); return MI_BLUR_ERR_HIP_BASE - (int)q; }
                (void)hipGetLastError();
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) return MI_BLUR_ERR_STATE;
            }
        }
        const unsigned long long b = __atomic_load_n(&z.ctl->t_begin[slot], __ATOMIC_RELAXED), e = __atomic_load_n(&z.ctl->t_end[slot], __ATOMIC_RELAXED);
        if (e >= b) {                                            // kernel bucket = union of the batches' [begin, end] (100 MHz device clock)
            const unsigned long long from = std::max(b, z.covered);
            if (e > from) c->tm.kernel_ms += (double)(e - from) / 1e5;
            z.covered = std::max(z.covered, e);
        }
        if (s.out_staged)                                        // the server wrote the slot's staging: scatter to the caller's memory
            copy_blocks(s.user_out, s.out_stride, s.h_out, s.out_band, s.out_band, s.out_n, STAGING_COPY_THREADS);
        s.zero_copy = false; s.zc_server = false; s.busy = false;
        return MI_BLUR_OK;
    }
    if (s.zero_copy) {                                           // launched on one of the context's zero-copy streams
        if (s.zc_plain) {                                        // experiment: no events on the dispatch
            HIP_TRY(hipStreamSynchronize(s.zc_stream));
            s.zero_copy = false; s.busy = false; s.zc_plain = false;
            return MI_BLUR_OK;
        }
        HIP_TRY(hipEventSynchronize(s.ke));
        float a = 0.f, b = 0.f;
        if (c->zc_ref_valid && hipEventElapsedTime(&a, c->zc_ref, s.ks) == hipSuccess && hipEventElapsedTime(&b, c->zc_ref, s.ke) == hipSuccess && b >= a) {
            const double from = std::max((double)a, c->zc_covered_ms);
            if ((double)b > from) c->tm.kernel_ms += (double)b - from;
            c->zc_covered_ms = std::max(c->zc_covered_ms, (double)b);
        } else if (hipEventElapsedTime(&ms, s.ks, s.ke) == hipSuccess) {
            c->tm.kernel_ms += ms;
        }
        (void)hipGetLastError();
        s.zero_copy = false;
        s.busy = false;
        return MI_BLUR_OK;
    }
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (s.out_staged)
        copy_blocks(s.user_out, s.out_stride, s.h_out, s.out_band, s.out_band, s.out_n, STAGING_COPY_THREADS);
    if (hipEventElapsedTime(&ms, s.ev[0], s.ev[1]) == hipSuccess) c->tm.h2d_ms += ms;
    if (hipEventElapsedTime(&ms, s.ks, s.ke) == hipSuccess) c->tm.kernel_ms += ms;
    if (hipEventElapsedTime(&ms, s.ev[2], s.ev[3]) == hipSuccess) c->tm.d2h_ms += ms;
    (void)hipGetLastError();
    s.busy = false;
    return MI_BLUR_OK;
}

static int harvest_resident(mi_blur_ctx *c)
{
    for (size_t i = 0; i < c->ev_used; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[i].s, c->ev_pool[i].e) == hipSuccess) c->tm.kernel_ms += ms;
    }
    (void)hipGetLastError();
    c->ev_used = 0;
    return MI_BLUR_OK;
}

// clFinish + clGetEventProfilingInfo harvest (heterogeneous_blur.c:538-579).
extern "C" int mi_blur_sync(mi_blur_ctx *c, mi_blur_timing *timing)
{
    if (!c) return MI_BLUR_ERR_INVALID;
    if (c->is_cpu()) {
        for (CpuJob *j : c->cpu_jobs) {
            c->cpu_worker->wait(j);
            c->tm.kernel_ms += j->ms;
            delete j;
        }
        c->cpu_jobs.clear();
    } else {
        HIP_TRY(hipSetDevice(c->device));
        for (auto &s : c->slots) {
            int rc = finish_slot(c, s);
            if (rc) return rc;
        }
        for (auto &s : c->slots) HIP_TRY(hipStreamSynchronize(s.stream));
        if (c->fused_second) HIP_TRY(hipStreamSynchronize(c->fused_second));      // every other fused pass runs there
        c->fused_second_busy = false; c->fused_gated = false;        // drained: the next pass has nothing to overlap with, no gate kernel
        // (a watched fused pass: its watcher, on the second stream, ends with the pass; after a sync the count it published is final)
        c->fused_watch_busy = false;
        harvest_resident(c);
        c->zc_ref_valid = false;                                 // everything drained: the next zero-copy launch starts a new window
    }
    if (timing) *timing = c->tm;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_get_timing(mi_blur_ctx *c, mi_blur_timing *timing)
{
    if (!c || !timing) return MI_BLUR_ERR_INVALID;
    *timing = c->tm;
    return MI_BLUR_OK;
}

extern "C" uint64_t mi_blur_zero_copy_launches(mi_blur_ctx *c) { return c ? c->zero_copy_launches : 0; }

extern "C" void mi_blur_reset_timing(mi_blur_ctx *c)
{
    if (!c) return;
    c->tm = mi_blur_timing{};
    c->timed_launches = 0; c->timed_bytes_alg = 0;
}

// For resident runs that time only every n-th launch: how many launches (and how many
// algorithmic bytes) the accumulated kernel_ms covers.  Submit paths time every launch.
extern "C" void mi_blur_timed_coverage(mi_blur_ctx *c, uint64_t *launches, uint64_t *bytes_alg)
{
    if (launches) *launches = c ? c->timed_launches : 0;
    if (bytes_alg) *bytes_alg = c ? c->timed_bytes_alg : 0;
}

// Cleanup: heterogeneous_blur.c:727-744.
extern "C" void mi_blur_destroy(mi_blur_ctx *c)
{
    if (!c) return;
    for (CpuJob *j : c->cpu_jobs) { c->cpu_worker->wait(j); delete j; }
    delete c->cpu_worker;
    if (!c->is_cpu()) {
        (void)hipSetDevice(c->device);
        for (auto &s : c->slots) { if (s.stream) (void)hipStreamSynchronize(s.stream); }
        if (c->fused_second) (void)hipStreamSynchronize(c->fused_second);
        if (c->zc) {                                             // tell the servers to leave, wait for them, release
            ZcServer &z = *c->zc;
            if (z.ctl) __atomic_store_n(&z.ctl->quit, 1u, __ATOMIC_RELEASE);
            if (getenv("MI_BLUR_DEBUG_SERVER"))
                fprintf(stderr, "[mi_blur] destroy: server state head %u launched %u servers_done %u tail %u; stream query %d\n", z.head, z.launched,
                        z.ctl ? z.ctl->servers_done : 0u, z.ctl ? z.ctl->tail : 0u, z.stream ? (int)hipStreamQuery(z.stream) : -1);
            if (z.stream) { (void)hipStreamSynchronize(z.stream); (void)hipStreamDestroy(z.stream); }
            if (getenv("MI_BLUR_DEBUG_SERVER")) fprintf(stderr, "[mi_blur] destroy: servers gone\n");
            if (z.dev) (void)hipFree(z.dev);
            if (z.trace) (void)hipFree(z.trace);
            if (z.ctl) (void)hipHostFree(z.ctl);
            delete c->zc;
            c->zc = nullptr;
        }
        for (auto &s : c->slots) free_slot(s);
        for (auto &t : c->ev_pool) { (void)hipEventDestroy(t.s); (void)hipEventDestroy(t.e); }
        if (c->zc_ref) (void)hipEventDestroy(c->zc_ref);
        if (c->fused_count) (void)hipFree(c->fused_count);
        if (c->fused_host) (void)hipHostFree(c->fused_host);
        if (c->fused_poll) { (void)hipStreamSynchronize(c->fused_poll); (void)hipStreamDestroy(c->fused_poll); }
        if (c->fused_word) (void)hipHostFree(c->fused_word);
        if (c->fused_second) (void)hipStreamDestroy(c->fused_second);
        if (c->fused_ev) (void)hipEventDestroy(c->fused_ev);
        if (c->pool_in) (void)hipFree(c->pool_in);
        if (c->pool_out) (void)hipFree(c->pool_out);
        ctx_drop_map(c);
        (void)hipGetLastError();
    }
    delete c;
}

// Hand one zero-copy batch to the context's batch server.  MI_BLUR_ERR_UNSUPPORTED = "not this path" (another tile shape
// than the running server's): the caller launches the batch the classic way.
static int zc_server_submit(mi_blur_ctx *c, Slot &s, const LaunchDesc &d, const Tunables &tun)
{
    if (c->filter.kind != FilterKind::BOX) return MI_BLUR_ERR_UNSUPPORTED;   // the server's tiles are the radius-1|2 kernel's: one launch per batch
    if (c->slots.size() > ZC_RING) return MI_BLUR_ERR_UNSUPPORTED;
    if (!c->zc) {
        ZcServer *z = new (std::nothrow) ZcServer;
        if (!z) return MI_BLUR_ERR_NOMEM;
        // The server stream is non-blocking, i.e. NOT ordered behind the NULL stream, and hipMemset of device memory may
        // return before the fill has run: the zero-fills go on the server stream itself, in front of the first server.
        hipError_t e = hipHostMalloc((void **)&z->ctl, sizeof(ZcHostCtl), hipHostMallocDefault);
        if (e == hipSuccess) { memset(z->ctl, 0, sizeof(ZcHostCtl)); e = hipHostGetDevicePointer((void **)&z->ctl_dev, z->ctl, 0); }
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&z->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc((void **)&z->dev, sizeof(ZcDevCtl));
        if (e == hipSuccess) e = hipMemsetAsync(z->dev, 0, sizeof(ZcDevCtl), z->stream);
        if (e == hipSuccess && tun.zero_copy_trace) {
            const size_t tb = (size_t)ZC_TRACE_BATCHES * (size_t)tun.zero_copy_workers * 5u * sizeof(unsigned long long);
            e = hipMalloc((void **)&z->trace, tb);
            if (e == hipSuccess) e = hipMemsetAsync(z->trace, 0, tb, z->stream);
        }
        if (e == hipSuccess && tun.zero_copy_debug_base > 0) {
            // test hook: start just short of the 2^32 wrap of the batch and tile numbers.  Every word that holds a number is set
            // to what a server that had really served that many batches would have left behind.
            const unsigned B = 0u - (unsigned)tun.zero_copy_debug_base, T = 0u - 7u * (unsigned)tun.zero_copy_debug_base;
            ZcDevCtl init{};
            init.next[0] = B; init.gnext[0] = T; init.avail = B; init.ticket = T;
            e = hipMemcpyAsync(z->dev, &init, offsetof(ZcDevCtl, tiles_done), hipMemcpyHostToDevice, z->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(z->stream);      // `init` is on this stack
            z->ctl->tail = B;
            for (unsigned i = 0; i < ZC_RING; i++) z->ctl->done[i] = B - ((B - i - 1u) % ZC_RING);   // (last batch before B in slot i) + 1
            z->head = B; z->tile_base = T;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(z->stream);          // once per context: the fills are done before anything is launched
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (z->stream) (void)hipStreamDestroy(z->stream);
            if (z->dev) (void)hipFree(z->dev);
            if (z->trace) (void)hipFree(z->trace);
            if (z->ctl) (void)hipHostFree(z->ctl);
            delete z;
            return MI_BLUR_ERR_HIP_BASE - (int)e;
        }
        z->fixed_share = tun.zero_copy_tickets ? 0 : 1;
        z->n_workers = (unsigned)tun.zero_copy_workers;
        z->budget = (unsigned)tun.zero_copy_budget;
        z->idle_ticks = (unsigned)tun.zero_copy_idle_us * 100u;      // 100 MHz device clock
        c->zc = z;
    }
    ZcServer &z = *c->zc;
    ZcBatch b{};
    unsigned n_tiles = 0;
    int rc = zc_fill_batch(d, &z.geo, &b, &n_tiles);
    if (rc) return rc;
    // A worker scans the descriptors from the batch of its last ticket to the batch of its next one, and the ticket counter
    // can be n_workers tiles beyond the newest published batch: with batches of very few tiles that span, plus the batches
    // the host may publish meanwhile, must stay inside the ring.  (Such batches gain nothing from the server anyway.)
    if (n_tiles == 0 || z.n_workers / n_tiles + 2u * (unsigned)c->slots.size() + 2u > ZC_RING) return MI_BLUR_ERR_UNSUPPORTED;
    b.tile_first = z.tile_base;                                          // tiles are numbered through the batches
    b.n_tiles = n_tiles;
    z.tile_base += n_tiles;
    const unsigned k = z.head;
    memcpy(&z.ctl->batch[k % ZC_RING], &b, sizeof b);
    __atomic_store_n(&z.ctl->tail, k + 1u, __ATOMIC_RELEASE);           // the frames and the descriptor are written: publish
    z.head = k + 1u;
    // Keep TWO servers that have not said they stopped: the running one may be deciding to leave (idle, budget) just as
    // this batch is published; the one queued behind it on the same stream then takes it.
    const unsigned stopped = __atomic_load_n(&z.ctl->servers_done, __ATOMIC_ACQUIRE);
    while (z.launched - stopped < 2u) {
        rc = zc_launch_server(z.geo, z.ctl_dev, z.dev, z.launched, z.n_workers, z.budget, z.idle_ticks, z.stream, z.trace, z.fixed_share);
        if (rc) return rc;
        z.launched++;
    }
    s.zc_server = true; s.zc_index = k;
    return MI_BLUR_OK;
}

// The launch of the context's filter over n_images bands of band_rows rows (output rows [y0, y1) of each): dense strides,
// AUTO variant, no stream and no events yet.  Every launch a context makes starts here.
static LaunchDesc ctx_launch(const mi_blur_ctx *c, const uint8_t *in, uint8_t *out, int band_rows, int n_images, int y0, int y1)
{
    LaunchDesc d{};
    d.filter = &c->filter;
    d.in = in; d.out = out; d.width = c->W; d.band_rows = band_rows; d.channels = c->C;
    d.n_images = n_images; d.y0 = y0; d.y1 = y1; d.variant = MI_BLUR_VARIANT_AUTO;
    return d;
}

// What one submit adds to the context's counters.  h2d / d2h: the bytes that cross the host link (none on the CPU device).
static void count_submit(mi_blur_ctx *c, int n_images, size_t out_bytes, size_t h2d, size_t d2h, bool zero_copy)
{
    c->tm.bytes_h2d += h2d; c->tm.bytes_d2h += d2h;
    // a filter that reads whole images and writes images of another size: input + output; every other filter 2 * output
    c->tm.bytes_alg += whole_image_only(c->filter) ? (uint64_t)c->image_bytes * (uint64_t)n_images + out_bytes : 2ull * out_bytes;
    c->tm.images += (uint64_t)n_images;
    c->tm.launches += 1;
    if (zero_copy) c->zero_copy_launches += 1;
}

// A submit on the CPU device: `work` runs on the context's worker thread, after the submits before it.
static int cpu_enqueue(mi_blur_ctx *c, std::function<void()> work)
{
    CpuJob *j = new (std::nothrow) CpuJob;
    if (!j) return MI_BLUR_ERR_NOMEM;
    if (!c->cpu_worker) { c->cpu_worker = new (std::nothrow) CpuWorker; if (!c->cpu_worker) { delete j; return MI_BLUR_ERR_NOMEM; } }
    j->work = std::move(work);
    c->cpu_worker->push(j);
    c->cpu_jobs.push_back(j);
    return MI_BLUR_OK;
}

namespace {
// One submit of caller memory: n_images bands of band_rows rows, in_stride bytes apart from `in`; output rows [y0, y1) of
// each, out_stride bytes apart from `out`.  band_in / band_out: the bytes of one band / one output block.
struct HostBatch {
    const uint8_t *in;
    uint8_t *out;
    int band_rows, n_images, y0, y1;
    size_t band_in, band_out, in_stride, out_stride;
    size_t in_bytes() const { return band_in * (size_t)n_images; }
    size_t out_bytes() const { return band_out * (size_t)n_images; }
};
}  // namespace

// Hand the batch of d (pinned memory the kernel works on in place) to the batch server.  MI_BLUR_ERR_UNSUPPORTED: not
// taken, the caller launches it another way.
static int submit_to_server(mi_blur_ctx *c, Slot &s, const HostBatch &b, const LaunchDesc &d, const Tunables &tun)
{
    const int rc = zc_server_submit(c, s, d, tun);
    if (rc == MI_BLUR_ERR_UNSUPPORTED) s.zc_server = false;
    if (rc) return rc;
    s.zero_copy = true; s.busy = true;
    count_submit(c, b.n_images, b.out_bytes(), b.in_bytes(), b.out_bytes(), true);
    return MI_BLUR_OK;
}

// Both caller buffers pinned (zin / zout: their device addresses): the kernel reads and writes them in place over PCIe.
// On this platform one kernel moving both directions sustains ~70 GB/s (35 each way) while the copy engines give ~55 GB/s
// one way at a time and collapse to ~28 GB/s total when H2D and D2H overlap (profiles/r01_zero_copy.txt): +33-40 %
// images/s end to end.  Each zero-copy launch keeps only "zero_copy_blocks" workgroups resident (they loop over the
// tiles) and consecutive launches alternate over up to "zero_copy_streams" of the context's streams, so that reads
// of one tile and writes of another keep both directions of the link busy (profiles/r02_e2e.txt).
static int submit_in_place(mi_blur_ctx *c, Slot &s, const HostBatch &b, const uint8_t *zin, uint8_t *zout, const Tunables &tun)
{
    s.out_staged = false; s.user_out = b.out; s.out_bytes = b.out_bytes(); s.out_band = b.band_out; s.out_stride = b.out_stride;
    s.out_n = b.n_images;
    // consecutive zero-copy launches alternate over the first zn streams of the context
    const int zn = std::max(1, std::min(tun.zero_copy_streams, (int)c->slots.size()));
    const hipStream_t zs = c->slots[(c->zero_copy_launches % (uint64_t)zn)].stream;
    // one dispatch packet, nothing else: the kernel's own stop event doubles as the completion event (every
    // extra hipEventRecord is a barrier packet between two kernels)
    LaunchDesc d = ctx_launch(c, zin, zout, b.band_rows, b.n_images, b.y0, b.y1);
    d.in_stride = (long long)b.in_stride; d.out_stride = (long long)b.out_stride;
    // small batches stay with one launch each: the server's hand-off (descriptor over the link, poller, completion
    // word, the host's wait) costs ~26 us per batch against ~8 us for a launch — below ~1.3 MB each way the launch
    // wins, by up to 3x for a single 256x256 frame (profiles/r03_e2e_shape_sweep.txt)
    if (tun.zero_copy_server && b.out_bytes() >= (size_t)tun.zero_copy_server_min_kb * 1024u) {
        const int rc = submit_to_server(c, s, b, d, tun);
        if (rc != MI_BLUR_ERR_UNSUPPORTED) return rc;
    }
    const bool with_events = tun.zero_copy_events != 0;
    d.stream = zs;
    if (with_events) { d.start = s.ks; d.stop = s.ke; }
    s.zc_plain = !with_events; s.zc_stream = zs;
    d.max_blocks = tun.zero_copy_blocks;
    // once per sync window, in front of its first launch (and again every ~10 s of a window that never syncs,
    // so the float milliseconds since the reference keep their resolution)
    if (with_events && (!c->zc_ref_valid || c->zc_covered_ms > 10e3)) {
        if (!c->zc_ref) HIP_TRY(hipEventCreate(&c->zc_ref));
        HIP_TRY(hipEventRecord(c->zc_ref, zs));
        c->zc_ref_valid = true; c->zc_covered_ms = 0.0;
    }
    const int rc = launch(d);
    if (rc) return rc;
    s.zero_copy = true;                            // only now: a failed launch leaves the slot idle and staged
    s.busy = true;
    count_submit(c, b.n_images, b.out_bytes(), b.in_bytes(), b.out_bytes(), true);
    return MI_BLUR_OK;
}

// Pageable caller memory (the reference's malloc'd batch buffers, kept as they are): the staging buffers ARE pinned, so
// the batch server takes the batch from them in place — staging in -> blur -> staging out as one kernel stream over the
// link — instead of a DMA copy each way around a launch (copies in both directions at once collapse to ~28 GB/s in
// total on this platform, profiles/r01_pcie_probe.txt).  What stays is the host's own gather / scatter between the
// caller's memory and the staging.  src / src_stride: where the batch's input now is.  MI_BLUR_ERR_UNSUPPORTED: not taken.
// (any batch size: for small batches too the server on the staging beats two DMA copies around a launch — a single
// 256x256 frame per submit: 78 k against 36 k img/s)
static int submit_staged_server(mi_blur_ctx *c, Slot &s, const HostBatch &b, const uint8_t *src, size_t src_stride,
                                const Tunables &tun)
{
    const uint8_t *zin = pinned_device_ptr(src);
    uint8_t *zout = pinned_device_ptr(s.out_staged ? s.h_out : b.out);
    if (!zin || !zout) return MI_BLUR_ERR_UNSUPPORTED;
    LaunchDesc d = ctx_launch(c, zin, zout, b.band_rows, b.n_images, b.y0, b.y1);
    d.in_stride = (long long)src_stride; d.out_stride = (long long)(s.out_staged ? b.band_out : b.out_stride);
    return submit_to_server(c, s, b, d, tun);
}

// DMA copy in, launch on the slot's device buffers, DMA copy out, all on the slot's stream.  A strided batch (src_stride
// or out_stride not dense) takes a 2-D copy that gathers / scatters the bands.
static int submit_dma(mi_blur_ctx *c, Slot &s, const HostBatch &b, const uint8_t *src, size_t src_stride)
{
    int rc = slot_device(c, s);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s.ev[0], s.stream));
    if (src_stride == b.band_in)
        HIP_TRY(hipMemcpyAsync(s.d_in, src, b.in_bytes(), hipMemcpyHostToDevice, s.stream));
    else
        HIP_TRY(hipMemcpy2DAsync(s.d_in, b.band_in, src, src_stride, b.band_in, (size_t)b.n_images, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipEventRecord(s.ev[1], s.stream));
    LaunchDesc d = ctx_launch(c, s.d_in, s.d_out, b.band_rows, b.n_images, b.y0, b.y1);
    d.stream = s.stream; d.start = s.ks; d.stop = s.ke;
    d.concurrent = (int)c->slots.size();
    rc = launch(d);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s.ev[2], s.stream));
    if (s.out_staged || b.out_stride == b.band_out)
        HIP_TRY(hipMemcpyAsync(s.out_staged ? s.h_out : b.out, s.d_out, b.out_bytes(), hipMemcpyDeviceToHost, s.stream));
    else
        HIP_TRY(hipMemcpy2DAsync(b.out, b.out_stride, s.d_out, b.band_out, b.band_out, (size_t)b.n_images, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipEventRecord(s.ev[3], s.stream));
    s.busy = true;
    count_submit(c, b.n_images, b.out_bytes(), b.in_bytes(), b.out_bytes(), false);
    return MI_BLUR_OK;
}

// One batch through a slot: Write -> NDRange -> Read (heterogeneous_blur.c:520-533), but one
// launch (and one DMA each way) for the whole batch instead of one triple per image.
// in_stride/out_stride: bytes between consecutive images' first band row / first output row in
// HOST memory (a strided batch = Approach 2's "same rows of every image": a 2-D DMA gathers
// the bands into one contiguous device batch).
static int submit_common(mi_blur_ctx *c, const uint8_t *host_in, uint8_t *host_out, int band_rows, int n_images,
                         int y0, int y1, size_t in_stride, size_t out_stride)
{
    const size_t pitch = (size_t)c->W * c->C;
    const size_t band_in = pitch * band_rows;
    const size_t band_out = out_band_bytes(c, band_rows, y0, y1);
    const HostBatch b{host_in, host_out, band_rows, n_images, y0, y1, band_in, band_out,
                      in_stride ? in_stride : band_in, out_stride ? out_stride : band_out};
    c->submitted = true;
    if (c->is_cpu()) {
        const int W = c->W, C = c->C, nt = c->n_threads;
        const int rc = cpu_enqueue(c, [=, f = c->filter]() {
            cpu_blur_batch(b.in, b.out, W, band_rows, C, f, n_images, y0, y1, nt, b.in_stride, b.out_stride);
        });
        if (rc) return rc;
        count_submit(c, n_images, b.out_bytes(), 0, 0, false);
        return MI_BLUR_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    Slot &s = c->slots[c->next_slot];
    c->next_slot = (c->next_slot + 1) % (int)c->slots.size();
    int rc = finish_slot(c, s);
    if (rc) return rc;
    const Tunables tun = tunables();    // ONE copy of the knobs for this submit
    if (tun.zero_copy) {
        const uint8_t *zin = pinned_device_ptr(host_in);
        uint8_t *zout = pinned_device_ptr(host_out);
        const bool dense = b.in_stride == band_in && b.out_stride == band_out;
        if (zin && zout && (dense || (tiled_eligible(zin, zout, c->W, c->C) && b.in_stride % 16 == 0 && b.out_stride % 16 == 0)))
            return submit_in_place(c, s, b, zin, zout, tun);
    }
    const bool in_pinned = is_pinned(host_in);
    s.zero_copy = false;
    s.out_staged = !is_pinned(host_out);
    s.user_out = host_out; s.out_bytes = b.out_bytes(); s.out_band = band_out; s.out_stride = b.out_stride; s.out_n = n_images;
    const uint8_t *src = host_in;
    size_t src_stride = b.in_stride;
    rc = slot_staging(c, s, !in_pinned, s.out_staged);
    if (rc) return rc;
    if (!in_pinned) {                       // pageable caller memory: gather into the slot's pinned staging
        copy_blocks(s.h_in, band_in, host_in, b.in_stride, band_in, n_images, STAGING_COPY_THREADS);
        src = s.h_in; src_stride = band_in;
    }
    if (tun.zero_copy && tun.zero_copy_server && tun.staged_server) {
        rc = submit_staged_server(c, s, b, src, src_stride, tun);
        if (rc != MI_BLUR_ERR_UNSUPPORTED) return rc;
    }
    return submit_dma(c, s, b, src, src_stride);
}

extern "C" int mi_blur_submit(mi_blur_ctx *c, const uint8_t *host_in, uint8_t *host_out, int n_images)
{
    if (!c || !host_in || !host_out || host_in == host_out) return MI_BLUR_ERR_INVALID;
    if (n_images < 0 || n_images > c->max_batch) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    return submit_common(c, host_in, host_out, c->H, n_images, 0, c->H, 0, 0);
}

extern "C" int mi_blur_submit_band(mi_blur_ctx *c, const uint8_t *host_in, uint8_t *host_out, int band_rows,
                                   int halo_top, int halo_bottom)
{
    if (!c || !host_in || !host_out || host_in == host_out) return MI_BLUR_ERR_INVALID;
    if (whole_image_only(c->filter)) return MI_BLUR_ERR_UNSUPPORTED;   // no band forms: a band's phase depends on where it starts
    if (band_rows <= 0 || band_rows > c->H || halo_top < 0 || halo_bottom < 0) return MI_BLUR_ERR_INVALID;
    if (halo_top + halo_bottom >= band_rows) return MI_BLUR_ERR_INVALID;
    return submit_common(c, host_in, host_out, band_rows, 1, halo_top, band_rows - halo_bottom, 0, 0);
}

extern "C" int mi_blur_submit_bands(mi_blur_ctx *c, const uint8_t *host_in, uint8_t *host_out, int n_images,
                                    size_t host_image_stride, int band_rows, int halo_top, int halo_bottom)
{
    if (!c || !host_in || !host_out || host_in == host_out) return MI_BLUR_ERR_INVALID;
    if (whole_image_only(c->filter)) return MI_BLUR_ERR_UNSUPPORTED;
    if (n_images < 0 || n_images > c->max_batch) return MI_BLUR_ERR_INVALID;
    if (band_rows <= 0 || band_rows > c->H || halo_top < 0 || halo_bottom < 0) return MI_BLUR_ERR_INVALID;
    if (halo_top + halo_bottom >= band_rows) return MI_BLUR_ERR_INVALID;
    if (host_image_stride < (size_t)c->W * c->C * band_rows) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    return submit_common(c, host_in, host_out, band_rows, n_images, halo_top, band_rows - halo_bottom,
                         host_image_stride, host_image_stride);
}

// Frames as the reference's loader hands them over: PLANAR (CImg storage).  The reference interleaves every frame on one
// host core before the stream is built (heterogeneous_blur.c:125-134) and de-interleaves on the way out to save one
// (split_image_blur.c:40-56); here both repacks are GPU kernels inside the submit.  The repack-in kernel reads the
// pinned planar frames straight over PCIe (it IS the upload: its duration is the h2d bucket) and writes the
// interleaved batch into HBM; the blur runs HBM -> HBM; the way out is either a D2H copy of the interleaved batch or the
// repack-out kernel writing planar frames straight into pinned host memory.  The slot's two device buffers are enough:
// d_in is free again once the blur has read it, so the planar result is built there.
extern "C" int mi_blur_submit_planar(mi_blur_ctx *c, const uint8_t *host_planar_in, uint8_t *host_out, int n_images, int planar_out)
{
    if (!c || !host_planar_in || !host_out || host_planar_in == host_out) return MI_BLUR_ERR_INVALID;
    if (whole_image_only(c->filter)) return MI_BLUR_ERR_UNSUPPORTED;
    if (n_images < 0 || n_images > c->max_batch) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const size_t bytes = c->image_bytes * (size_t)n_images;
    c->submitted = true;
    if (c->is_cpu()) {
        // the scratch frames are allocated here, not in the job, so that running out of memory is a status
        uint8_t *a = new (std::nothrow) uint8_t[bytes], *b = planar_out ? new (std::nothrow) uint8_t[bytes] : nullptr;
        const int W = c->W, H = c->H, C = c->C, nt = c->n_threads;
        int rc = !a || (planar_out && !b) ? MI_BLUR_ERR_NOMEM : MI_BLUR_OK;
        if (!rc)
            rc = cpu_enqueue(c, [=, f = c->filter]() {
                cpu_repack(host_planar_in, a, W, H, C, n_images, true, nt);
                cpu_blur_batch(a, planar_out ? b : host_out, W, H, C, f, n_images, 0, H, nt);
                if (planar_out) cpu_repack(b, host_out, W, H, C, n_images, false, nt);
                delete[] a;
                delete[] b;
            });
        if (rc) { delete[] a; delete[] b; return rc; }
        count_submit(c, n_images, bytes, 0, 0, false);
        return MI_BLUR_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    Slot &s = c->slots[c->next_slot];
    c->next_slot = (c->next_slot + 1) % (int)c->slots.size();
    int rc = finish_slot(c, s);
    if (rc) return rc;
    s.zero_copy = false;
    // source the repack-in kernel can read: the caller's frames if they are pinned, the slot's pinned staging otherwise
    const uint8_t *src = pinned_device_ptr(host_planar_in);
    rc = slot_device(c, s);
    if (!rc) rc = slot_staging(c, s, !src, !pinned_device_ptr(host_out));
    if (rc) return rc;
    if (!src) {
        copy_blocks(s.h_in, bytes, host_planar_in, bytes, bytes, 1, STAGING_COPY_THREADS);
        src = pinned_device_ptr(s.h_in);
        if (!src) return MI_BLUR_ERR_STATE;
    }
    uint8_t *dst_pinned = pinned_device_ptr(host_out);
    s.out_staged = !dst_pinned;
    s.user_out = host_out; s.out_bytes = bytes; s.out_band = bytes; s.out_stride = bytes; s.out_n = 1;
    HIP_TRY(hipEventRecord(s.ev[0], s.stream));
    rc = launch_planar_to_interleaved(src, s.d_in, c->W, c->H, c->C, n_images, s.stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s.ev[1], s.stream));
    LaunchDesc d = ctx_launch(c, s.d_in, s.d_out, c->H, n_images, 0, c->H);
    d.stream = s.stream; d.start = s.ks; d.stop = s.ke;
    d.concurrent = (int)c->slots.size();
    rc = launch(d);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s.ev[2], s.stream));
    if (planar_out) {
        uint8_t *dst = dst_pinned ? dst_pinned : pinned_device_ptr(s.h_out);
        if (!dst) return MI_BLUR_ERR_STATE;
        rc = launch_interleaved_to_planar(s.d_out, dst, c->W, c->H, c->C, n_images, s.stream);
        if (rc) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(s.out_staged ? s.h_out : host_out, s.d_out, bytes, hipMemcpyDeviceToHost, s.stream));
    }
    HIP_TRY(hipEventRecord(s.ev[3], s.stream));
    s.busy = true;
    count_submit(c, n_images, bytes, bytes, bytes, false);
    return MI_BLUR_OK;
}

// Every mi_blur_ctx_set_*: the filter that build(&f) makes in place of the context's, for every submit from now on (before the
// first one only; the whole_image_only ones for mi_blur_submit only).  null_arg: a required pointer argument is null,
// which set_kernel, set_sep_down, set_resize, set_area, set_color, set_warp and set_warp_perspective answer before they look at the state; the other setters leave a null
// table to the constructor, behind the state.
template <typename B>
static int ctx_set_filter(mi_blur_ctx *c, bool null_arg, B &&build)
{
    if (!c || null_arg) return MI_BLUR_ERR_INVALID;
    if (c->submitted) return MI_BLUR_ERR_STATE;
    Filter f;
    if (const int rc = build(&f)) return rc;
    c->filter = f;
    ctx_drop_map(c);                                    // the remap it replaced, if any, owned a map
    return MI_BLUR_OK;
}

extern "C" int mi_blur_ctx_set_kernel(mi_blur_ctx *c, const mi_blur_sep_kernel *k)
{
    return ctx_set_filter(c, !k, [&](Filter *f) { return filter_sep(k, f); });
}

extern "C" int mi_blur_ctx_set_sep_down(mi_blur_ctx *c, const mi_blur_sep_kernel *k, const mi_blur_decimation *d)
{
    return ctx_set_filter(c, !k || !d, [&](Filter *f) { return sep_down_for(k, d, c->W, c->H, f); });
}

extern "C" int mi_blur_ctx_set_resize(mi_blur_ctx *c, const mi_blur_resize *r)
{
    return ctx_set_filter(c, !r, [&](Filter *f) { return resize_for(r, c->W, c->H, c->C, f); });
}

extern "C" int mi_blur_ctx_set_area(mi_blur_ctx *c, const mi_blur_area *r)
{
    return ctx_set_filter(c, !r, [&](Filter *f) { return area_for(r, c->W, c->H, c->C, f); });
}

extern "C" int mi_blur_ctx_set_color(mi_blur_ctx *c, const mi_blur_color *k)
{
    return ctx_set_filter(c, !k, [&](Filter *f) { return color_for(k, c->W, c->H, c->C, f); });
}

extern "C" int mi_blur_ctx_set_warp(mi_blur_ctx *c, const mi_blur_warp *w)
{
    return ctx_set_filter(c, !w, [&](Filter *f) { return warp_for(w, c->W, c->H, c->C, f); });
}

extern "C" int mi_blur_ctx_set_warp_perspective(mi_blur_ctx *c, const mi_blur_warp_perspective *w)
{
    return ctx_set_filter(c, !w, [&](Filter *f) { return warp_persp_for(w, c->W, c->H, c->C, f); });
}

// The copy of the map is made first, so a failure leaves the old filter and the old map in place.
extern "C" int mi_blur_ctx_set_remap(mi_blur_ctx *c, const mi_blur_remap *r, const int32_t *host_map)
{
    if (!c || !r || !host_map) return MI_BLUR_ERR_INVALID;
    if (c->submitted) return MI_BLUR_ERR_STATE;
    Filter f;
    if (const int rc = remap_for(r, host_map, c->W, c->H, c->C, &f)) return rc;
    const size_t n = (size_t)f.out_w * (size_t)f.out_h * 2;
    if (c->is_cpu()) {
        std::vector<int32_t> copy;
        try { copy.assign(host_map, host_map + n); } catch (...) { return MI_BLUR_ERR_NOMEM; }
        ctx_drop_map(c);
        c->remap_host.swap(copy);
        f.remap_map = c->remap_host.data();
    } else {
        HIP_TRY(hipSetDevice(c->device));
        int32_t *dev = nullptr;
        HIP_TRY(hipMalloc((void **)&dev, n * sizeof(int32_t)));
        const hipError_t e = hipMemcpy(dev, host_map, n * sizeof(int32_t), hipMemcpyHostToDevice);     // synchronous: host_map is free again on return
        if (e != hipSuccess) { (void)hipFree(dev); (void)hipGetLastError(); return MI_BLUR_ERR_HIP_BASE - (int)e; }
        ctx_drop_map(c);
        c->remap_dev = dev;
        f.remap_map = dev;
    }
    c->filter = f;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_ctx_set_median(mi_blur_ctx *c, int radius)
{
    return ctx_set_filter(c, false, [&](Filter *f) { return filter_median(radius, f); });
}

extern "C" int mi_blur_ctx_set_morph(mi_blur_ctx *c, int op, int rx, int ry)
{
    return ctx_set_filter(c, false, [&](Filter *f) { return filter_morph(op, rx, ry, f); });
}

extern "C" int mi_blur_ctx_set_bilateral(mi_blur_ctx *c, const mi_blur_bilateral *k)
{
    return ctx_set_filter(c, false, [&](Filter *f) { return filter_bilateral(k, f); });
}

extern "C" int mi_blur_ctx_set_conv(mi_blur_ctx *c, const mi_blur_conv *k)
{
    return ctx_set_filter(c, false, [&](Filter *f) { return filter_conv(k, f); });
}

// Wait for the OLDEST submit still in flight (its output is then in caller memory), so a host
// that rotates n_slots batch buffers can refill the oldest one while the newer ones run.
extern "C" int mi_blur_wait_oldest(mi_blur_ctx *c)
{
    if (!c) return MI_BLUR_ERR_INVALID;
    if (c->is_cpu()) {
        if (c->cpu_jobs.empty()) return MI_BLUR_OK;
        CpuJob *j = c->cpu_jobs.front();
        c->cpu_worker->wait(j);
        c->tm.kernel_ms += j->ms;
        delete j;
        c->cpu_jobs.erase(c->cpu_jobs.begin());
        return MI_BLUR_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int n = (int)c->slots.size();
    for (int i = 0; i < n; i++) {
        Slot &s = c->slots[(c->next_slot + i) % n];
        if (s.busy) return finish_slot(c, s);
    }
    return MI_BLUR_OK;
}

// ----------------------------------------------------------------------------------
// device-resident stream
// ----------------------------------------------------------------------------------
// Where a pool lands in HBM moves the big launches between two levels ~6 % apart (1080p 5x5: 138 <-> 148 us; the 3x3
// stream: 322 <-> 345 us): same request counts on every channel, but 1.5x the read DRAM-credit stalls on the slow
// placements (profiles/r03_placement_channels.txt).  Nothing in the address says which it will be, and hipMalloc offers no
// handle on it — but a placement keeps its level for as long as it lives, so the pool is CHOSEN: "resident_place_trials"
// candidate inputs and as many candidate outputs are allocated side by side, every (input, output) pair is timed on the
// launch the pool is for (the context's kernel over the whole pool, after a clock ramp), the fastest pair is kept and the
// other buffers are freed.
static int place_pool(mi_blur_ctx *c, size_t bytes, int pool_images, int trials)
{
    // `trials` input and `trials` output candidates; EVERY (input, output) pair is timed — the level belongs to the pair, and
    // n + n buffers give n x n pairs to choose from for the price of n.
    std::vector<uint8_t *> in((size_t)trials, nullptr), out((size_t)trials, nullptr);
    int n_ok = 0;
    for (int i = 0; i < trials; i++) {
        if (hipMalloc((void **)&in[i], bytes) != hipSuccess || hipMalloc((void **)&out[i], bytes) != hipSuccess) {
            (void)hipGetLastError();
            if (in[i]) { (void)hipFree(in[i]); in[i] = nullptr; }
            break;                                              // memory is short: choose among what there is
        }
        n_ok++;
    }
    if (n_ok == 0) return MI_BLUR_ERR_HIP_BASE - (int)hipErrorOutOfMemory;
    c->place_ms.clear();
    int keep_in = 0, keep_out = 0;
    if (n_ok > 1) {
        hipStream_t st = c->slots[0].stream;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        std::vector<float> best((size_t)n_ok * n_ok, 1e30f);
        if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            auto pass = [&](int i, int j) {
                LaunchDesc d = ctx_launch(c, in[i], out[j], c->H, pool_images, 0, c->H);
                d.stream = st;
                return launch(d);
            };
            int rc = MI_BLUR_OK;
            const auto t0 = std::chrono::steady_clock::now();      // ~50 ms of launches first: the clocks ramp (r02_clock_ramp.txt)
            while (rc == MI_BLUR_OK && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(50)) {
                for (int r = 0; r < 4 && rc == MI_BLUR_OK; r++) rc = pass(0, 0);
                if (hipStreamSynchronize(st) != hipSuccess) rc = MI_BLUR_ERR_STATE;
            }
            for (int round = 0; round < 2 && rc == MI_BLUR_OK; round++)
                for (int i = 0; i < n_ok && rc == MI_BLUR_OK; i++)
                    for (int j = 0; j < n_ok && rc == MI_BLUR_OK; j++) {
                        rc = pass(i, j);                            // one untimed launch: this pair's lines and TLB entries
                        (void)hipEventRecord(e0, st);
                        for (int r = 0; r < 2 && rc == MI_BLUR_OK; r++) rc = pass(i, j);
                        (void)hipEventRecord(e1, st);
                        float ms = 0.f;
                        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0.f)
                            best[(size_t)i * n_ok + j] = std::min(best[(size_t)i * n_ok + j], ms / 2.0f);
                    }
            (void)hipGetLastError();
            for (int i = 0; i < n_ok; i++)
                for (int j = 0; j < n_ok; j++) {
                    c->place_ms.push_back(best[(size_t)i * n_ok + j]);
                    if (best[(size_t)i * n_ok + j] < best[(size_t)keep_in * n_ok + keep_out]) { keep_in = i; keep_out = j; }
                }
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    c->pool_in = in[keep_in]; c->pool_out = out[keep_out];
    c->place_kept = keep_in * n_ok + keep_out;
    for (int i = 0; i < trials; i++) {
        if (i != keep_in && in[i]) (void)hipFree(in[i]);
        if (i != keep_out && out[i]) (void)hipFree(out[i]);
    }
    return MI_BLUR_OK;
}

extern "C" int mi_blur_resident_alloc(mi_blur_ctx *c, int pool_images)
{
    if (!c || pool_images <= 0) return MI_BLUR_ERR_INVALID;
    if (c->is_cpu()) return MI_BLUR_ERR_STATE;
    HIP_TRY(hipSetDevice(c->device));
    if (c->pool_in) { (void)hipFree(c->pool_in); c->pool_in = nullptr; }
    if (c->pool_out) { (void)hipFree(c->pool_out); c->pool_out = nullptr; }
    c->pool_images = 0; c->cursor = 0;
    const size_t bytes = c->image_bytes * (size_t)pool_images;
    // placement only matters to launches that stream hundreds of MB; candidates are only tried while they are cheap to hold
    const int trials = tunables().resident_place_trials;
    if (trials > 1 && bytes >= ((size_t)128 << 20) && bytes <= ((size_t)8 << 30)) {
        int rc = place_pool(c, bytes, pool_images, std::min(trials, 8));
        if (rc) return rc;
    } else {
        c->place_ms.clear(); c->place_kept = 0;
        HIP_TRY(hipMalloc((void **)&c->pool_in, bytes));
        HIP_TRY(hipMalloc((void **)&c->pool_out, bytes));
    }
    c->pool_images = pool_images;
    return MI_BLUR_OK;
}

// What mi_blur_resident_alloc measured when it chose the pool: the per-launch time (ms) of each candidate placement, and
// which one it kept.  n = 0: no trial was run (small pool, "resident_place_trials" <= 1).
extern "C" int mi_blur_resident_placement(mi_blur_ctx *c, float *ms, int max_n, int *kept)
{
    if (!c) return MI_BLUR_ERR_INVALID;
    const int n = (int)std::min<size_t>(c->place_ms.size(), (size_t)std::max(max_n, 0));
    for (int i = 0; i < n && ms; i++) ms[i] = c->place_ms[i];
    if (kept) *kept = c->place_kept;
    return n;
}

extern "C" int mi_blur_resident_upload(mi_blur_ctx *c, int pool_index, const uint8_t *host_in, int n_images)
{
    if (!c || !host_in || !c->pool_in) return MI_BLUR_ERR_STATE;
    if (pool_index < 0 || n_images < 0 || pool_index + n_images > c->pool_images) return MI_BLUR_ERR_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(c->pool_in + (size_t)pool_index * c->image_bytes, host_in, c->image_bytes * (size_t)n_images,
                      hipMemcpyHostToDevice));
    return MI_BLUR_OK;
}

extern "C" int mi_blur_resident_download(mi_blur_ctx *c, int pool_index, uint8_t *host_out, int n_images)
{
    if (!c || !host_out || !c->pool_out) return MI_BLUR_ERR_STATE;
    if (pool_index < 0 || n_images < 0 || pool_index + n_images > c->pool_images) return MI_BLUR_ERR_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, c->pool_out + (size_t)pool_index * c->image_bytes, c->image_bytes * (size_t)n_images,
                      hipMemcpyDeviceToHost));
    return MI_BLUR_OK;
}

extern "C" int mi_blur_resident_fill_synthetic(mi_blur_ctx *c, int first_index)
{
    if (!c || !c->pool_in) return MI_BLUR_ERR_STATE;
    const int chunk = std::max(1, (int)std::min<size_t>((size_t)c->pool_images, ((size_t)256 << 20) / c->image_bytes));
    std::vector<uint8_t> host;
    try { host.resize(c->image_bytes * (size_t)chunk); } catch (...) { return MI_BLUR_ERR_NOMEM; }
    for (int i = 0; i < c->pool_images; i += chunk) {
        const int n = std::min(chunk, c->pool_images - i);
        fill_synthetic(host.data(), c->W, c->H, c->C, first_index + i, n, c->n_threads);
        int rc = mi_blur_resident_upload(c, i, host.data(), n);
        if (rc) return rc;
    }
    return MI_BLUR_OK;
}

extern "C" void *mi_blur_resident_in(mi_blur_ctx *c) { return c ? c->pool_in : nullptr; }
extern "C" void *mi_blur_resident_out(mi_blur_ctx *c) { return c ? c->pool_out : nullptr; }

// What follows on the slot streams comes after the fused passes that went to the second stream (an event; no host wait).
static int fused_join(mi_blur_ctx *c)
{
    if (!c->fused_second_busy) return MI_BLUR_OK;
    HIP_TRY(hipEventRecord(c->fused_ev, c->fused_second));
    for (auto &s : c->slots) HIP_TRY(hipStreamWaitEvent(s.stream, c->fused_ev, 0));
    c->fused_second_busy = false;
    return MI_BLUR_OK;
}

// One pass of the stream over the resident pool: the batch loop of
// heterogeneous_blur.c:418-427 with the transfers gone (data already in HBM).
extern "C" int mi_blur_resident_run(mi_blur_ctx *c, int n_images, int batch, int timed_every)
{
    if (!c || n_images < 0 || batch <= 0) return MI_BLUR_ERR_INVALID;
    if (c->filter.kind != FilterKind::BOX) return MI_BLUR_ERR_UNSUPPORTED;
    if (c->is_cpu() || !c->pool_in) return MI_BLUR_ERR_STATE;
    if (batch > c->pool_images) return MI_BLUR_ERR_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    { int rc = fused_join(c); if (rc) return rc; }
    int launch_idx = 0;
    for (int done = 0; done < n_images; done += batch, launch_idx++) {
        const int b = std::min(batch, n_images - done);
        const bool timed = timed_every > 0 && launch_idx % timed_every == 0;
        if (c->cursor + b > c->pool_images) c->cursor = 0;
        Slot &s = c->slots[c->rr];
        c->rr = (c->rr + 1) % (int)c->slots.size();
        LaunchDesc d = ctx_launch(c, c->pool_in + (size_t)c->cursor * c->image_bytes, c->pool_out + (size_t)c->cursor * c->image_bytes,
                                  c->H, b, 0, c->H);
        d.stream = s.stream;
        d.concurrent = (int)c->slots.size();
        if (timed) {
            if (c->ev_used == c->ev_pool.size()) {
                TimedLaunch t{};
                HIP_TRY(hipEventCreate(&t.s));
                HIP_TRY(hipEventCreate(&t.e));
                c->ev_pool.push_back(t);
            }
            d.start = c->ev_pool[c->ev_used].s; d.stop = c->ev_pool[c->ev_used].e;
            c->ev_used++;
        }
        int rc = launch(d);
        if (rc) return rc;
        c->cursor += b;
        c->tm.launches += 1;
        if (timed) { c->timed_launches += 1; c->timed_bytes_alg += 2ull * c->image_bytes * (uint64_t)b; }
    }
    c->tm.images += (uint64_t)n_images;
    c->tm.bytes_alg += 2ull * c->image_bytes * (uint64_t)n_images;
    return MI_BLUR_OK;
}

// The same pass as ONE dispatch (blur_fused_kernel): the GPU walks the batches in order and raises a host-visible
// flag per finished batch, so the batch stays the unit of completion without being the unit of dispatch.
// Words of the per-batch completion counters for a pool of `cap` images: 8 per batch at the smallest batch (one image), plus room
// for a few batches of thousands of tiles to spread over up to 256 words each (two 8192x8192 frames are two batches of 3200 tiles)
static size_t fused_words(int cap) { return 8 * (size_t)cap + 16384; }
// Behind the counters: the ticket word of a pass's dynamic tail in two banks (passes alternate, so two passes in flight never
// share one; each is zero between passes) and the overlap gate word, 128 bytes apart.
constexpr size_t FUSED_TAIL_BANK = 32, FUSED_GATE_WORD = 64, FUSED_EXTRA_WORDS = 96;

extern "C" int mi_blur_resident_run_fused(mi_blur_ctx *c, int n_images, int batch, int timed)
{
    if (!c || n_images <= 0 || batch <= 0) return MI_BLUR_ERR_INVALID;
    if (c->filter.kind != FilterKind::BOX) return MI_BLUR_ERR_UNSUPPORTED;
    if (c->is_cpu() || !c->pool_in) return MI_BLUR_ERR_STATE;
    if (n_images > c->pool_images) return MI_BLUR_ERR_INVALID;           // one contiguous run of the pool
    HIP_TRY(hipSetDevice(c->device));
    const int nb = (n_images + batch - 1) / batch;
    if (nb > c->fused_cap) {
        // the previous pass may still be writing its flags
        for (auto &s : c->slots) HIP_TRY(hipStreamSynchronize(s.stream));
        if (c->fused_second) HIP_TRY(hipStreamSynchronize(c->fused_second));
        c->fused_second_busy = false; c->fused_gated = false;
        if (c->fused_count) { (void)hipFree(c->fused_count); c->fused_count = nullptr; }
        if (c->fused_host) { (void)hipHostFree(c->fused_host); c->fused_host = nullptr; }
        c->fused_cap = 0;
        const int cap = std::max(nb, c->pool_images);      // enough for any batch size on this pool: never reallocated
        HIP_TRY(hipMalloc((void **)&c->fused_count, sizeof(unsigned) * (fused_words(cap) + FUSED_EXTRA_WORDS)));
        HIP_TRY(hipMemset(c->fused_count + fused_words(cap), 0, sizeof(unsigned) * FUSED_EXTRA_WORDS));
        // the gate word starts at the number of the latest pass (all of them are over), never below: it only ever grows
        HIP_TRY(hipMemcpy(c->fused_count + fused_words(cap) + FUSED_GATE_WORD, &c->fused_seq, sizeof(unsigned), hipMemcpyHostToDevice));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipHostMalloc((void **)&c->fused_host, sizeof(unsigned) * fused_words(cap), hipHostMallocDefault));
        c->fused_cap = cap;
        c->fused_passes = 0;
    }
    if (!c->fused_poll) {
        HIP_TRY(hipStreamCreateWithFlags(&c->fused_poll, hipStreamNonBlocking));
        // the first device-to-host copy of this size class sets up the copy engine's queue (~8 ms): pay it here, not
        // in the first poll
        HIP_TRY(hipMemcpyAsync(c->fused_host, c->fused_count, sizeof(unsigned) * fused_words(c->fused_cap), hipMemcpyDeviceToHost, c->fused_poll));
        HIP_TRY(hipStreamSynchronize(c->fused_poll));
    }
    if (c->cursor + n_images > c->pool_images) c->cursor = 0;
    Slot &s = c->slots[0];
    LaunchDesc d = ctx_launch(c, c->pool_in + (size_t)c->cursor * c->image_bytes, c->pool_out + (size_t)c->cursor * c->image_bytes,
                              c->H, n_images, 0, c->H);
    d.variant = MI_BLUR_VARIANT_TILED; d.stream = s.stream;
    // The launch geometry (blocks per batch) depends on the tuning knobs as well as on the shape: take ONE copy of the
    // knobs, ask for the geometry first, launch with the same copy.
    const Tunables tun = tunables();
    unsigned tpb = 0, wpb = 0, blocks = 0, kcnt = 8, ntail = 0;
    unsigned *const extra = c->fused_count + fused_words(c->fused_cap);
    const unsigned seq = c->fused_seq + 1u;
    FusedDesc f{c->fused_count, batch, &tpb, &wpb, &blocks, &tun, true, extra + (tun.fused_overlap > 0 ? (seq & 1u) * FUSED_TAIL_BANK : 0), (long long)fused_words(c->fused_cap), &kcnt,
                &ntail, nullptr, seq};
    int rc = launch_fused(d, f);
    if (rc) return rc;
    const bool same = n_images == c->fused_n && batch == c->fused_batch && tpb == c->fused_tpb && wpb == c->fused_wpb && kcnt == c->fused_k &&
                      blocks == c->fused_blocks && c->fused_passes > 0 && c->fused_passes < (1u << 20);
    // "fused_overlap": a pass with a dynamic tail on whole-chunk rows, unwatched, raises the gate word when it enters its tail.  The
    // pass after it — if it is of the same kind and its counters count on — goes to the OTHER stream behind a gate kernel and starts
    // there.  The gate is a hint: the gate kernel always ends, and nothing but the moment pass p+1 starts depends on it.  Every other
    // pass stays on slot 0's stream, ordered by an event behind what the second stream still holds.
    const bool raises = tun.fused_overlap > 0 && ntail > 0 && !(timed & 2) && tiled_eligible(d.in, d.out, c->W, c->C);
    const bool overlap = raises && same && c->fused_gated;
    if (overlap) {
        d.stream = c->fused_on_second ? s.stream : c->fused_second;
        rc = launch_fused_gate(extra + FUSED_GATE_WORD, c->fused_seq, d.stream);
        if (rc) return rc;
    } else {
        rc = fused_join(c);          // (also in front of the zeroing fill below: the pass on the other stream still counts)
        if (rc) return rc;
    }
    if (raises) f.gate = extra + FUSED_GATE_WORD;
    // Repeated passes of the same shape AND geometry do not zero the counters (that would be one more dispatch per
    // pass): every pass adds the same amounts, so batch b of pass p is complete when its counters sum to p x (its blocks).
    if (same) {
        c->fused_passes += 1;
    } else {
        // the counters are about to be zeroed: a watcher of an earlier pass must have seen that pass's last counts first
        // (it ends with its pass, but walks the batches one by one and may still be on its way when unwatched passes have
        // followed; zeros under it would leave it waiting for its hard limit)
        if (c->fused_watch_busy) { HIP_TRY(hipStreamSynchronize(c->fused_second)); c->fused_watch_busy = false; }
        HIP_TRY(hipMemsetAsync(c->fused_count, 0, sizeof(unsigned) * (size_t)kcnt * (size_t)nb, s.stream));
        c->fused_n = n_images; c->fused_batch = batch; c->fused_passes = 1;
        c->fused_tpb = tpb; c->fused_wpb = wpb; c->fused_blocks = blocks; c->fused_k = kcnt;
    }
    c->fused_batches = nb;
    c->fused_watched = false;
    if (timed & 2) {
        // a watcher wave keeps (pass, leading batches complete) in pinned host memory for this pass.  Counters that were just
        // zeroed must BE zero before it looks at them: it runs on its own stream, so wait for the fill.
        if (c->fused_passes == 1) HIP_TRY(hipStreamSynchronize(s.stream));
        if (!c->fused_word) {
            HIP_TRY(hipHostMalloc((void **)&c->fused_word, sizeof(unsigned long long), hipHostMallocDefault));
            *c->fused_word = 0;
            HIP_TRY(hipHostGetDevicePointer((void **)&c->fused_word_dev, c->fused_word, 0));
        }
    }
    if (timed & 1) {
        if (c->ev_used == c->ev_pool.size()) {
            TimedLaunch t{};
            HIP_TRY(hipEventCreate(&t.s));
            HIP_TRY(hipEventCreate(&t.e));
            c->ev_pool.push_back(t);
        }
        d.start = c->ev_pool[c->ev_used].s; d.stop = c->ev_pool[c->ev_used].e;
        c->ev_used++;
    }
    f.geometry_only = false;
    rc = launch_fused(d, f);
    if (rc) { c->fused_passes = 0; c->fused_batches = 0; c->fused_gated = false; return rc; }     // nothing ran: zero the counters next time
    c->fused_seq = seq;
    c->fused_gated = raises;
    c->fused_on_second = d.stream == c->fused_second;
    if (c->fused_on_second) c->fused_second_busy = true;
    c->cursor += n_images;
    c->tm.launches += 1;
    c->tm.images += (uint64_t)n_images;
    c->tm.bytes_alg += 2ull * c->image_bytes * (uint64_t)n_images;
    if (timed & 1) { c->timed_launches += 1; c->timed_bytes_alg += 2ull * c->image_bytes * (uint64_t)n_images; }
    if (timed & 2) {
        // The watcher runs on the second stream (a watched pass never does; peeks on fused_poll must not queue behind it), so a
        // context has as many streams as it had before the second one carried passes: streams beyond the hardware queues share
        // one, and a queue runs its dispatches in order.  For the same reason it is queued AFTER its pass: in front of it on a
        // shared queue it would hold the pass back until its own hard limit.
        c->fused_watch_seq += 1;
        rc = launch_fused_watch(c->fused_count, (unsigned)nb, tpb, blocks, wpb * c->fused_passes, c->fused_word_dev, c->fused_watch_seq, c->fused_second, c->fused_k);
        if (rc) return rc;
        c->fused_watched = true;
        c->fused_watch_busy = true;
        c->fused_second_busy = true;
    }
    return MI_BLUR_OK;
}

// Non-blocking: how many LEADING batches of the latest fused pass are complete (their outputs are in the pool); >= 0.
// A NEGATIVE value is a mi_blur_status: the counters could not be read (a failed copy, a faulted device), which a
// polling caller must treat as the end of the poll, not as "none done yet".
extern "C" int mi_blur_resident_batches_done(mi_blur_ctx *c)
{
    if (!c) return MI_BLUR_ERR_INVALID;
    if (c->is_cpu()) return MI_BLUR_ERR_STATE;
    if (!c->fused_count || !c->fused_batches) return 0;       // no fused pass issued (or the last one failed to launch)
    if (c->fused_watched) {                                   // a watcher wave keeps the answer in host memory: no copy, no HIP call
        const unsigned long long w = __atomic_load_n(c->fused_word, __ATOMIC_ACQUIRE);
        return (unsigned)(w >> 32) == c->fused_watch_seq ? (int)(unsigned)(w & 0xffffffffu) : 0;
    }
    // read the counters on a stream of their own (the pass may still be running on the compute stream)
    HIP_TRY(hipSetDevice(c->device));
    const unsigned K = c->fused_k;
    HIP_TRY(hipMemcpyAsync(c->fused_host, c->fused_count, sizeof(unsigned) * (size_t)K * (size_t)c->fused_batches, hipMemcpyDeviceToHost, c->fused_poll));
    HIP_TRY(hipStreamSynchronize(c->fused_poll));
    int n = 0;
    for (; n < c->fused_batches; n++) {
        const unsigned first = (unsigned)n * c->fused_tpb;
        const unsigned blocks = std::min(c->fused_tpb, c->fused_blocks - first);
        unsigned sum = 0;
        for (unsigned k = 0; k < K; k++) sum += c->fused_host[(size_t)K * n + k];
        if (sum != blocks * c->fused_wpb * c->fused_passes) break;
    }
    return n;
}

// Read outputs of batches that mi_blur_resident_batches_done has reported, WITHOUT waiting for the dispatch that is
// still producing the later ones: a copy on the poll stream, which is ordered behind nothing on the compute streams.
extern "C" int mi_blur_resident_peek(mi_blur_ctx *c, int pool_index, uint8_t *host_out, int n_images)
{
    if (!c || !host_out || !c->pool_out || !c->fused_poll) return MI_BLUR_ERR_STATE;
    if (pool_index < 0 || n_images < 0 || pool_index + n_images > c->pool_images) return MI_BLUR_ERR_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(host_out, c->pool_out + (size_t)pool_index * c->image_bytes, c->image_bytes * (size_t)n_images,
                           hipMemcpyDeviceToHost, c->fused_poll));
    HIP_TRY(hipStreamSynchronize(c->fused_poll));
    return MI_BLUR_OK;
}

// ----------------------------------------------------------------------------------
// CPU device kernel + helpers
// ----------------------------------------------------------------------------------
// Every mi_blur_cpu_run* export.  built: the status of f's constructor.  Every failure here is MI_BLUR_ERR_INVALID, so the
// order of the checks does not show.  Every filter but the box blur refuses images of more than INT_MAX bytes, as before.
// cpu_blur_batch takes the size of the output from f.
static int cpu_run_filter(int built, const Filter &f, const uint8_t *in, uint8_t *out, int width, int height, int channels,
                          int n_images, int n_threads)
{
    if (built || !in || !out || in == out || width <= 0 || height <= 0 || channels <= 0 || n_images < 0)
        return MI_BLUR_ERR_INVALID;
    if (f.kind != FilterKind::BOX && (long long)width * channels * height > INT_MAX) return MI_BLUR_ERR_INVALID;
    cpu_blur_batch(in, out, width, height, channels, f, n_images, 0, height, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_cpu_run(const uint8_t *in, uint8_t *out, int width, int height, int channels, int radius,
                               int n_images, int n_threads)
{
    Filter f;
    return cpu_run_filter(filter_box(radius, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_sep(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                   const mi_blur_sep_kernel *k, int n_threads)
{
    Filter f;
    return cpu_run_filter(filter_sep(k, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_sep_down(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                        const mi_blur_sep_kernel *k, const mi_blur_decimation *d, int n_threads)
{
    Filter f;
    return cpu_run_filter(sep_down_for(k, d, width, height, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_resize(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                      const mi_blur_resize *r, int n_threads)
{
    Filter f;
    return cpu_run_filter(resize_for(r, width, height, channels, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_area(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                    const mi_blur_area *r, int n_threads)
{
    Filter f;
    return cpu_run_filter(area_for(r, width, height, channels, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_color(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                     const mi_blur_color *k, int n_threads)
{
    Filter f;
    return cpu_run_filter(color_for(k, width, height, channels, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_warp(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                    const mi_blur_warp *w, int n_threads)
{
    Filter f;
    return cpu_run_filter(warp_for(w, width, height, channels, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_warp_perspective(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                                const mi_blur_warp_perspective *w, int n_threads)
{
    Filter f;
    return cpu_run_filter(warp_persp_for(w, width, height, channels, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_remap(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                     const mi_blur_remap *r, const int32_t *host_map, int n_threads)
{
    Filter f;
    const int built = (const void *)host_map == (const void *)out ? MI_BLUR_ERR_INVALID : remap_for(r, host_map, width, height, channels, &f);
    return cpu_run_filter(built, f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_median(const uint8_t *in, uint8_t *out, int width, int height, int channels, int radius,
                                      int n_images, int n_threads)
{
    Filter f;
    return cpu_run_filter(filter_median(radius, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_morph(const uint8_t *in, uint8_t *out, int width, int height, int channels, int op, int rx, int ry,
                                     int n_images, int n_threads)
{
    Filter f;
    return cpu_run_filter(filter_morph(op, rx, ry, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_bilateral(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                         const mi_blur_bilateral *k, int n_threads)
{
    Filter f;
    return cpu_run_filter(filter_bilateral(k, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" int mi_blur_cpu_run_conv(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                    const mi_blur_conv *k, int n_threads)
{
    Filter f;
    return cpu_run_filter(filter_conv(k, &f), f, in, out, width, height, channels, n_images, n_threads);
}

extern "C" void mi_blur_fill_synthetic(uint8_t *host, int width, int height, int channels, int first_index,
                                       int n_images, int n_threads)
{
    if (host && width > 0 && height > 0 && channels > 0)
        fill_synthetic(host, width, height, channels, first_index, n_images, n_threads);
}

// Diagnostics (see mi_blur.h): fold the per-workgroup times of the tiled kernel per XCD, and optionally re-arm the slots.
extern "C" int mi_blur_debug_xcd_times(uint64_t end_ticks[8], uint64_t begin_ticks[8], int rearm)
{
    unsigned long long *d = debug_xcd_buffer();
    if (!d) return MI_BLUR_ERR_NOMEM;
    const size_t n = debug_xcd_slots();
    std::vector<unsigned long long> h;
    try { h.resize(2 * n); } catch (...) { return MI_BLUR_ERR_NOMEM; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h.data(), d, 16 * n, hipMemcpyDeviceToHost));
    uint64_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8];
    for (int i = 0; i < 8; i++) b[i] = ~0ull;
    for (size_t i = 0; i < n; i++) {
        if (!h[2 * i]) continue;                                  // workgroup slot not written since the last re-arm
        const int x = (int)(h[2 * i] & 7u);
        e[x] = std::max<uint64_t>(e[x], h[2 * i] >> 4);
        b[x] = std::min<uint64_t>(b[x], h[2 * i + 1]);
    }
    for (int i = 0; i < 8; i++) { if (end_ticks) end_ticks[i] = e[i]; if (begin_ticks) begin_ticks[i] = b[i]; }
    if (rearm) HIP_TRY(hipMemset(d, 0, 16 * n));
    return MI_BLUR_OK;
}

// Diagnostics (see mi_blur.h): the raw stamps of slots [first_slot, first_slot + n_slots).
extern "C" int mi_blur_debug_xcd_raw(uint64_t *out, size_t first_slot, size_t n_slots)
{
    unsigned long long *d = debug_xcd_buffer();
    if (!d) return MI_BLUR_ERR_NOMEM;
    if (!out || first_slot > debug_xcd_slots() || n_slots > debug_xcd_slots() - first_slot) return MI_BLUR_ERR_INVALID;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d + 2 * first_slot, 16 * n_slots, hipMemcpyDeviceToHost));
    return MI_BLUR_OK;
}

// Diagnostics (see mi_blur.h): the batch server's per-worker phase stamps of the most recent batches.
extern "C" int mi_blur_debug_zc_trace(mi_blur_ctx *c, uint64_t *out, int max_batches, int *n_workers, unsigned *batches_published)
{
    if (!c || !out || max_batches <= 0) return MI_BLUR_ERR_INVALID;
    if (c->is_cpu() || !c->zc || !c->zc->trace) return MI_BLUR_ERR_STATE;
    ZcServer &z = *c->zc;
    HIP_TRY(hipSetDevice(c->device));
    const int nb = std::min<int>(max_batches, (int)ZC_TRACE_BATCHES);
    std::vector<unsigned long long> all;
    try { all.resize((size_t)ZC_TRACE_BATCHES * z.n_workers * 5u); } catch (...) { return MI_BLUR_ERR_NOMEM; }
    HIP_TRY(hipMemcpy(all.data(), z.trace, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));   // (waits for idle servers to leave)
    // the context's first nb batches (the trace covers batches 0 .. ZC_TRACE_BATCHES-1 of a context)
    const int have = (int)std::min<unsigned>(z.head, (unsigned)nb);
    memcpy(out, all.data(), (size_t)have * z.n_workers * 5u * sizeof(unsigned long long));
    const int nb_out = have;
    if (n_workers) *n_workers = (int)z.n_workers;
    if (batches_published) *batches_published = z.head;
    return nb_out;
}

extern "C" uint64_t mi_blur_fnv1a64(const uint8_t *host, size_t n) { return fnv1a64(host, n); }

// heterogeneous_blur.c:449-458 — evaluated in float exactly as there.
extern "C" void mi_blur_a1_partition(int mode, int batch_count, float gpu_ratio, int *n_cpu, int *n_gpu)
{
    int nc, ng;
    if (mode == 0) { ng = (int)(batch_count * gpu_ratio); nc = batch_count - ng; }
    else if (mode == 1) { nc = batch_count; ng = 0; }
    else { nc = 0; ng = batch_count; }
    if (n_cpu) *n_cpu = nc;
    if (n_gpu) *n_gpu = ng;
}

extern "C" void mi_blur_shard_range(long long n_units, int g, int G, long long *begin, long long *end)
{
    if (G <= 0) G = 1;
    if (begin) *begin = n_units * g / G;
    if (end) *end = n_units * (g + 1) / G;
}

// split_image_blur.c:144-166.
extern "C" void mi_blur_a2_split(int height, float gpu_ratio, int halo, mi_blur_a2_geometry *g)
{
    if (!g) return;
    int split_row = (int)(height * (1.0f - gpu_ratio));
    if (split_row < halo) split_row = halo;
    if (split_row > height - halo) split_row = height - halo;
    g->split_row = split_row;
    g->cpu_input_rows = split_row + halo;
    g->cpu_output_rows = split_row;
    g->gpu_input_rows = (height - split_row) + halo;
    g->gpu_output_rows = height - split_row;
}

extern "C" void mi_blur_band_of(int height, int radius, int g, int G, mi_blur_band *b)
{
    if (!b) return;
    if (G <= 0) G = 1;
    b->row_begin = (int)((long long)height * g / G);
    b->row_end = (int)((long long)height * (g + 1) / G);
    b->halo_top = std::min(radius, b->row_begin);
    b->halo_bottom = std::min(radius, height - b->row_end);
}
