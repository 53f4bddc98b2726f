// color_kernels.hip — gfx950 kernels of the colour transform (mi_blur_enqueue_color, include/mi_blur.h): per pixel a
// channel matrix, a bias, one arithmetic shift, a clamp to a byte and optionally a table, 1-4 channels in and 1-4 out.
// The sum and the clamp are color_channel() / color_clamp() (filter.h), which the CPU device uses too.
//
// Tiled kernel (blur_color_tiled_kernel<C, CO, LUT>): W * H a multiple of 16, 16-byte aligned buffers and strides.  The
// rule is FLAT: a pointwise filter on dense images does not care about rows, so rows need not be whole chunks; an image
// is the run of its W * H pixels, cut into groups of COLOR_GROUP = 16 pixels: exactly C input chunks and CO output
// chunks of 16 bytes.  One thread owns one group: C loads of 16 bytes (a lane stride of 16 C bytes: no single
// instruction is contiguous across the wave, but every fetched line is used whole by the C loads of the lanes on it),
// 16 x CO sums of v_mad_i32_i24 with the weights in scalar registers, CO stores of 16 bytes.  No barrier on the way.
// One workgroup = a run of COLOR_RUN consecutive groups of one image; blockIdx -> (image, run) in the XCD-contiguous
// order of fill_tiles() for grids of 16 workgroups and more.  C and CO are template arguments, so the de-interleave and
// the re-interleave are compile-time byte picks; LUT is one too, so the forms without a table carry none: with it the
// CO x 256 table travels in the kernel arguments and goes to LDS once per workgroup.  No scratch.  32 instantiations.
//
// Generic kernel (blur_color_generic_kernel): one output pixel per thread, grid-strided, any shape and alignment.
#include "kernel_common.h"

#include <string.h>

namespace mi_blur {

namespace {

struct ColorMatrix {
    int32_t m[4][4], bias[4];
    int shift;
};
// The tables as dwords, lut[o][v] = byte v & 3 of w[o * 64 + v / 4]; one dword that nobody reads where there is none.
template <int LUT>
struct ColorTable { uint32_t w[LUT ? 4 * 64 : 1]; };

struct ColorTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per input image / output image
    unsigned groups, runs;            // groups of 16 pixels and runs of COLOR_RUN groups per image
    unsigned nblocks;
    int xcd;
    ColorMatrix k;
};

template <int C, int CO, int LUT>
__global__ __launch_bounds__(COLOR_RUN) void blur_color_tiled_kernel(const ColorTiledParams p, const ColorTable<LUT> tab)
{
    __shared__ uint32_t lut_w[LUT ? CO * 64 : 1];
    const int t = threadIdx.x;
    if constexpr (LUT) {
        if (t < CO * 64) lut_w[t] = tab.w[t];
        __syncthreads();
    }
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lut_w);
    // blockIdx -> (image, run): runs fastest, then images
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const unsigned img = L / p.runs, run = L - img * p.runs;
    const unsigned g = run * COLOR_RUN + (unsigned)t;
    if (g >= p.groups) return;                                  // the last run of an image may be short
    const uint4 *src = reinterpret_cast<const uint4 *>(p.in + (long long)img * p.in_stride + (size_t)g * (16u * C));
    uint4 *dst = reinterpret_cast<uint4 *>(p.out + (long long)img * p.out_stride + (size_t)g * (16u * CO));

    uint32_t w[4 * C], r[4 * CO];
#pragma unroll
    for (int j = 0; j < C; j++) {
        const uint4 v = src[j];
        w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < 4 * CO; q++) r[q] = 0;
#pragma unroll
    for (int px = 0; px < COLOR_GROUP; px++) {
        int v[C];
#pragma unroll
        for (int i = 0; i < C; i++) v[i] = (int)window_byte(w, px * C + i);
#pragma unroll
        for (int o = 0; o < CO; o++) {
            int32_t acc = p.k.bias[o];
#pragma unroll
            for (int i = 0; i < C; i++) acc = __mul24(p.k.m[o][i], v[i]) + acc;   // |weight| <= 2^18, a byte: exact in 24 bits
            uint32_t b = (uint32_t)color_clamp(acc, p.k.shift);
            if constexpr (LUT) b = lut[o * 256 + (int)b];
            r[(px * CO + o) >> 2] |= b << (8 * ((px * CO + o) & 3));
        }
    }
#pragma unroll
    for (int j = 0; j < CO; j++) dst[j] = make_uint4(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]);
}

struct ColorGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per input image / output image
    long long pixels, total;          // pixels per image, pixels of the launch
    int channels, co, lut_on;
    ColorMatrix k;
};

__global__ __launch_bounds__(256) void blur_color_generic_kernel(const ColorGenericParams p, const ColorTable<1> tab)
{
    __shared__ uint32_t lut_w[4 * 64];
    if (p.lut_on) {
        lut_w[threadIdx.x] = tab.w[threadIdx.x];
        __syncthreads();
    }
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lut_w);
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const long long img = idx / p.pixels, px = idx - img * p.pixels;
        const uint8_t *src = p.in + img * p.in_stride + px * p.channels;
        uint8_t *dst = p.out + img * p.out_stride + px * p.co;
        uint8_t v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = i < p.channels ? src[i] : 0;
#pragma unroll
        for (int o = 0; o < 4; o++)
            if (o < p.co) dst[o] = color_channel(p.k.m[o], p.k.bias[o], p.k.shift, p.lut_on ? lut + o * 256 : nullptr, p.channels, v);
    }
}

void fill_matrix(ColorMatrix &k, const ColorSpec &c)
{
    memcpy(k.m, c.m, sizeof k.m);
    memcpy(k.bias, c.bias, sizeof k.bias);
    k.shift = c.shift;
}

// The flat rule: groups of 16 pixels, 16-byte aligned buffers and strides (dense strides then are).
bool color_tile_aligned(const LaunchDesc &d)
{
    return color_flat_ok(d.width, d.band_rows) && (uintptr_t)d.in % 16 == 0 && (uintptr_t)d.out % 16 == 0 && d.in_stride % 16 == 0 &&
           d.out_stride % 16 == 0;
}

template <int LUT>
int launch_color_tiled(const LaunchDesc &d)
{
    const ColorSpec &c = d.filter->color;
    ColorTiledParams p{};
    p.in = d.in; p.out = d.out;
    p.in_stride = d.in_stride ? d.in_stride : dense_in(d);
    p.out_stride = d.out_stride ? d.out_stride : dense_out(d);
    p.groups = (unsigned)((long long)d.width * d.band_rows / COLOR_GROUP);
    p.runs = (unsigned)color_runs(d.width, d.band_rows);
    if (const int st = fill_flat(p, d.n_images, p.runs)) return st;
    fill_matrix(p.k, c);
    ColorTable<LUT> tab{};
    if constexpr (LUT != 0) memcpy(tab.w, c.lut, sizeof c.lut);
    set_last_kernel("blur_color_tiled_kernel");
    const dim3 grid(p.nblocks);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto CC) {
        return dispatch<1, 2, 3, 4>(c.co, [&](auto CO) {
            return do_launch(blur_color_tiled_kernel<CC, CO, LUT>, grid, dim3(COLOR_RUN), 0, d, p, tab);
        });
    });
}

int launch_color_generic(const LaunchDesc &d)
{
    const ColorSpec &c = d.filter->color;
    set_last_kernel("blur_color_generic_kernel");
    ColorGenericParams p{};
    p.in = d.in; p.out = d.out;
    p.in_stride = d.in_stride ? d.in_stride : dense_in(d);
    p.out_stride = d.out_stride ? d.out_stride : dense_out(d);
    p.pixels = (long long)d.width * d.band_rows;
    p.total = p.pixels * d.n_images;
    p.channels = d.channels; p.co = c.co; p.lut_on = c.lut_on;
    fill_matrix(p.k, c);
    ColorTable<1> tab{};
    memcpy(tab.w, c.lut, sizeof c.lut);
    return do_launch(blur_color_generic_kernel, byte_grid(p.total), dim3(256), 0, d, p, tab);
}

}  // namespace

// Only whole images (launch_checks()); out_stride is measured against the image with the output's channels (dense_out()).
int launch_color(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::COLOR, [&](const Filter &f) {
        const ColorSpec &c = f.color;
        return c.co >= 1 && c.co <= 4 && c.shift >= 0 && c.shift <= 16 && (c.lut_on == 0 || c.lut_on == 1) &&
               color_image_ok(c.co, d.width, d.band_rows, d.channels);
    });
    if (st != LAUNCH_GO) return st;
    if (color_tile_aligned(d)) return d.filter->color.lut_on ? launch_color_tiled<1>(d) : launch_color_tiled<0>(d);
    return launch_color_generic(d);
}

}  // namespace mi_blur
