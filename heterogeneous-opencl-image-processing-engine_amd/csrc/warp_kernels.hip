// warp_kernels.hip — gfx950 kernels of the affine warp (mi_blur_enqueue_warp, include/mi_blur.h): exact fixed-point
// bilinear and nearest under a Q16 output -> input matrix, CLAMP or CONSTANT border, any output size.  Every coordinate
// comes from warp_position() / warp_axis() (filter.h), the functions the CPU device and mi_blur_warp_coord use too.
//
// Tiled kernel (blur_warp_tiled_kernel<C>): BILINEAR, 1-4 channels, input and output rows of whole 16-byte chunks,
// 16-byte aligned buffers and strides, largest footprint at most WARP_LDS_MAX bytes.  One workgroup = one tile of TILE_TH
// OUTPUT rows x nc (<= 4 * C: 64 pixels) OUTPUT chunk columns: the shared fill_tiles / tile_coords (kernel_common.h, no halo) on
// the OUTPUT image, in strips of warp_grid() (filter.h).  A rotated tile costs its bounding box, so the tile is close to
// square in pixels (resize's 32-chunk strip would stage 3-8 times as much).  The box a tile stages and where a tap lies in
// it comes from filter.h ("Tile geometry"), as does the host's sizing; the staging is the shared stage_box, the blend lerp24:
//   * the tile's source footprint — warp_footprint() (filter.h): the box of the taps of its four corner pixels with the
//     + 1 tap, clamped into the image (CLAMP) or intersected with it (CONSTANT) — widened to whole 16-byte chunks, is
//     staged in LDS with 16-byte loads.  It lies inside the image, so staging clamps nothing;
//   * a work item is one output row x a run of whole pixels, so which byte of which pixel goes where is known at compile
//     time, and a 64 x 32 pixel tile has at least 256 items, one per thread: one 16-byte chunk for 2 and 4 channels (8 and 4
//     pixels); half a chunk for 1 channel (8 pixels, one 8-byte store); for 3 channels, where only every third chunk starts
//     on a pixel, half a group of 3 chunks: 8 pixels = 24 bytes, stored as 16 + 8 or 8 + 16 bytes (a strip is a whole
//     number of groups).  Sx, Sy once per item in 64 bits, then + m[0], + m[3] per pixel; the two taps of a row are neighbours
//     (or one pixel, at the edge of the box), so each row is one 8-byte LDS read at a run-time, 4-byte aligned address
//     (ds_read2_b32; a third dword for 3 channels) and a 64-bit shift, two reads per pixel whatever C; taps outside the image are replaced by `fill`
//     under CONSTANT; v_mad_u32_u24 blends, one rounding shift;
//   * a tile whose footprint misses the image (CONSTANT only) writes `fill`.
//   The host sizes the LDS from the exact largest footprint of the launch (warp_tiles_max_bytes(), filter.h: it walks the
//   tiles of one image with the kernel's own warp_tile_box), so no bound on the footprint is assumed.  4 instantiations, no scratch.
//
// Generic kernel (blur_warp_generic_kernel): one output byte per thread, any shape, map, mode, border and alignment.
//
// The perspective warp (mi_blur_enqueue_warp_perspective) has the same two kernels on its own position source: at the end of this file.
#include "kernel_common.h"

#include <algorithm>    // std::equal, std::copy

namespace mi_blur {

namespace {

struct WarpTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per input image / output image
    long long m[6];
    int W, H, Wo, Ho;
    int pitch, opitch;                // bytes per input row / output row
    int cpr;                          // OUTPUT 16-byte chunks per row
    int ncols, nstrips, ntiles_y;
    unsigned nblocks;
    int xcd;
    int border;
    unsigned fill;                    // the fill byte in all four bytes
};

// warp_taps<C>, the read of the two taps of a staged row, is in kernel_common.h: blur_remap_tiled_kernel shares it.
template <int C>
__global__ __launch_bounds__(TILE_THREADS) void blur_warp_tiled_kernel(const WarpTiledParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int U = warp_unit(C), NPIX = C == 1 || C == 3 ? 8 : 16 / C, NITEM = U * 16 / (NPIX * C);   // pixels of a work item; items per group of U chunks
    const int t = threadIdx.x;
    const TileCoords tc = tile_coords<0>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, 0, p.Ho, 0);
    const int ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc;
    const int64_t m[6] = {p.m[0], p.m[1], p.m[2], p.m[3], p.m[4], p.m[5]};

    // footprint (uniform): input pixels b.x0..b.x1 x b.y0..b.y1, staged as rows b.y0..b.y1 of chunks sc.lo..sc.hi
    const int px0 = tile_pixels(x0c, nc, C).lo;
    const WarpBox b = warp_tile_box(m, p.border, p.W, p.H, C, ty0, rows_out, x0c, nc);
    const int nu = nc / U * NITEM, nitems = rows_out * nu;
    uint8_t *out_img = p.out + (long long)tc.img * p.out_stride;

    if (warp_box_empty(b)) {                            // CONSTANT, every tap outside the image: the blend of four fills is fill
        u32x4 v;
        v.x = v.y = v.z = v.w = p.fill;
        for (int i = t; i < rows_out * nc; i += TILE_THREADS) {
            const int row = i / nc, cc = i - row * nc;
            *reinterpret_cast<u32x4 *>(out_img + ((unsigned)(ty0 + row) * (unsigned)p.opitch + (unsigned)(x0c + cc) * 16u)) = v;
        }
        return;
    }
    const Span sc = chunk_span(b.x0, b.x1, C);
    stage_box(lds, p.in + (long long)tc.img * p.in_stride + ((unsigned)b.y0 * (unsigned)p.pitch + (unsigned)sc.lo * 16u), p.pitch, b.y1 - b.y0 + 1, sc.n(), t);
    __syncthreads();

    const bool constant = p.border == MI_BLUR_WARP_CONSTANT;
    const uint32_t fillp = p.fill;
    for (int i = t; i < nitems; i += TILE_THREADS) {
        const int row = i / nu, u = i - row * nu;
        const int Y = ty0 + row, X = px0 + u * NPIX;    // px0 is exact: a strip starts on a group of U chunks
        WarpPos s = warp_position(m, X, Y);
        uint32_t o[NPIX * C / 4];
#pragma unroll
        for (int q = 0; q < NPIX * C / 4; q++) o[q] = 0;
#pragma unroll
        for (int k = 0; k < NPIX; k++) {
            const WarpAxis ax = warp_axis(s.sx, MI_BLUR_RESIZE_BILINEAR, p.W), ay = warp_axis(s.sy, MI_BLUR_RESIZE_BILINEAR, p.H);
            // the taps, clamped into the staged box (warp_tap, filter.h): a tap the clamp moved out of the image is replaced
            // below under CONSTANT.  xb is xa + 1, or xa where the clamp met the edge of the box: both taps of a row come
            // from one read at xa
            const WarpTap wt = warp_tap(b, sc, C, ax.i0, ay.i0);
            uint32_t ta, tb, tc2, td;
            warp_taps<C>(lds, wt.off_a, ta, tb);
            warp_taps<C>(lds, wt.off_b, tc2, td);
            if (wt.one) { tb = ta; td = tc2; }
            if (constant) {
                const bool ixa = (unsigned)ax.i0 < (unsigned)p.W, ixb = (unsigned)(ax.i0 + 1) < (unsigned)p.W;
                const bool iya = (unsigned)ay.i0 < (unsigned)p.H, iyb = (unsigned)(ay.i0 + 1) < (unsigned)p.H;
                ta = ixa && iya ? ta : fillp; tb = ixb && iya ? tb : fillp;
                tc2 = ixa && iyb ? tc2 : fillp; td = ixb && iyb ? td : fillp;
            }
            const uint32_t fx = (uint32_t)ax.f, fy = (uint32_t)ay.f;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const uint32_t top = lerp24((ta >> (8 * c)) & 0xffu, (tb >> (8 * c)) & 0xffu, fx);
                const uint32_t bot = lerp24((tc2 >> (8 * c)) & 0xffu, (td >> (8 * c)) & 0xffu, fx);
                const uint32_t v = lerp24_round(top, bot, fy);    // top, bot < 2^20
                const int e = k * C + c;                // byte of the item: a constant
                o[e >> 2] |= v << (8 * (e & 3));
            }
            s.sx += m[0]; s.sy += m[3];
        }
        uint8_t *dst = out_img + ((unsigned)Y * (unsigned)p.opitch + (unsigned)x0c * 16u + (unsigned)u * (unsigned)(NPIX * C));
        if constexpr (C == 3) {
            // 24 bytes: the first half of a group of 3 chunks stores 16 + 8 bytes, the second 8 + 16, all naturally aligned
            const bool second = u & 1;
            u32x4 v;
            u32x2 h;
            v.x = second ? o[2] : o[0]; v.y = second ? o[3] : o[1]; v.z = second ? o[4] : o[2]; v.w = second ? o[5] : o[3];
            h.x = second ? o[0] : o[4]; h.y = second ? o[1] : o[5];
            *reinterpret_cast<u32x4 *>(dst + (second ? 8 : 0)) = v;
            *reinterpret_cast<u32x2 *>(dst + (second ? 0 : 16)) = h;
        } else if constexpr (C == 1) {
            u32x2 h;
            h.x = o[0]; h.y = o[1];
            *reinterpret_cast<u32x2 *>(dst) = h;
        } else {
            u32x4 v;
            v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
            *reinterpret_cast<u32x4 *>(dst) = v;
        }
    }
}

struct WarpGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per image (Ho * opitch)
    long long m[6];
    int W, H, channels, pitch, opitch, mode, border;
    unsigned fill;
};

__global__ __launch_bounds__(256) void blur_warp_generic_kernel(const WarpGenericParams p)
{
    const int64_t m[6] = {p.m[0], p.m[1], p.m[2], p.m[3], p.m[4], p.m[5]};
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.opitch, p.channels, 0, p.in, p.in_stride);   // q.y, q.x: the OUTPUT pixel
        const WarpCoord wc = warp_coord(m, p.mode, p.W, p.H, q.x, q.y);
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)warp_sample(q.src + q.c, (size_t)p.pitch, p.channels, p.W, p.H, p.border, p.fill, wc);
    }
}

// tile_aligned (kernel_common.h) with output rows of whole chunks too, BILINEAR.
bool warp_tile_aligned(const LaunchDesc &d) { return tile_aligned(d) && out_pitch(d) % 16 == 0 && d.filter->sample_mode == MI_BLUR_RESIZE_BILINEAR; }

// LDS bytes of the largest footprint of a launch whose OUTPUT image is cut into the tiles g (warp_tiles_max_bytes(),
// filter.h).  A stream of launches repeats one geometry, so each thread keeps the last answer.
long long warp_tiles(const LaunchDesc &d, const TileGrid &g)
{
    const Filter &f = *d.filter;
    const int64_t *m = f.warp_m, key[12] = {d.width, d.band_rows, d.channels, f.out_w, f.out_h, f.warp_border, m[0], m[1], m[2], m[3], m[4], m[5]};
    thread_local int64_t last_key[12];
    thread_local long long last = -1;
    if (last >= 0 && std::equal(key, key + 12, last_key)) return last;
    std::copy(key, key + 12, last_key);
    return last = warp_tiles_max_bytes(g, f.warp_m, f.warp_border, d.width, d.band_rows, f.out_h, d.channels);
}

// g: the tiles of the OUTPUT image; max_bytes: its largest footprint, at most WARP_LDS_MAX.
int launch_warp_tiled(const LaunchDesc &d, const TileGrid &g, long long max_bytes)
{
    const Filter &f = *d.filter;
    WarpTiledParams p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid, g)) return st;
    set_last_kernel("blur_warp_tiled_kernel");
    std::copy(f.warp_m, f.warp_m + 6, p.m);
    p.W = d.width; p.Wo = f.out_w; p.Ho = f.out_h; p.border = f.warp_border; p.fill = (unsigned)f.warp_fill * 0x01010101u;
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto CC) { return do_launch(blur_warp_tiled_kernel<CC>, grid, dim3(TILE_THREADS), (size_t)(max_bytes + WARP_LDS_SLACK), d, p); });
}

int launch_warp_generic(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    set_last_kernel("blur_warp_generic_kernel");
    WarpGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    std::copy(f.warp_m, f.warp_m + 6, p.m);
    p.W = d.width; p.mode = f.sample_mode; p.border = f.warp_border; p.fill = (unsigned)f.warp_fill;
    return do_launch(blur_warp_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

// Only whole images (launch_checks()); out_stride is measured against the WARPED image (dense_out()).
int launch_warp(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::WARP, [&](const Filter &f) {
        return resize_ok(f.out_w, f.out_h, f.sample_mode, d.width, d.band_rows, d.channels) && warp_map_ok(f.warp_border, f.warp_fill, f.warp_m);
    });
    if (st != LAUNCH_GO) return st;
    if (warp_tile_aligned(d)) {
        const TileGrid g = warp_grid(out_pitch(d) / 16, d.filter->out_h, d.channels);
        const long long max_bytes = warp_tiles(d, g);
        if (max_bytes <= WARP_LDS_MAX) return launch_warp_tiled(d, g, max_bytes);
    }
    return launch_warp_generic(d);
}

// ----------------------------------------------------------------------------------
// The perspective warp (mi_blur_enqueue_warp_perspective): the two kernels above with the second map source of filter.h,
// persp_position() / persp_axis().  blur_warp_persp_tiled_kernel<C> keeps the tiles, the staging, the tap reads, the
// blend and the stores of blur_warp_tiled_kernel; a work item computes Nx, Ny, D once in 64 bits, adds h[0], h[3], h[6]
// per pixel, and divides twice per pixel: one double reciprocal of 2 D, two double products, and the exact 64-bit
// remainder that corrects each estimate (floor_div_clamped(), filter.h), so no 64-bit integer division is expanded.
// The box of a tile is persp_tile_box(): boxes differ from tile to tile, the host's walk (persp_tiles_max_bytes()) sizes
// the LDS for the largest.  No scratch.
// ----------------------------------------------------------------------------------
namespace {

struct WarpPerspTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per input image / output image
    long long h[9];
    int W, H, Wo, Ho;
    int pitch, opitch;                // bytes per input row / output row
    int cpr;                          // OUTPUT 16-byte chunks per row
    int ncols, nstrips, ntiles_y;
    unsigned nblocks;
    int xcd;
    int border;
    unsigned fill;                    // the fill byte in all four bytes
};

template <int C>
__global__ __launch_bounds__(TILE_THREADS) void blur_warp_persp_tiled_kernel(const WarpPerspTiledParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int U = warp_unit(C), NPIX = C == 1 || C == 3 ? 8 : 16 / C, NITEM = U * 16 / (NPIX * C);   // as blur_warp_tiled_kernel
    const int t = threadIdx.x;
    const TileCoords tc = tile_coords<0>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, 0, p.Ho, 0);
    const int ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc;
    const int64_t h[9] = {p.h[0], p.h[1], p.h[2], p.h[3], p.h[4], p.h[5], p.h[6], p.h[7], p.h[8]};

    const int px0 = tile_pixels(x0c, nc, C).lo;
    const WarpBox b = persp_tile_box(h, p.border, p.W, p.H, C, ty0, rows_out, x0c, nc);
    const int nu = nc / U * NITEM, nitems = rows_out * nu;
    uint8_t *out_img = p.out + (long long)tc.img * p.out_stride;

    if (warp_box_empty(b)) {                            // CONSTANT, every tap outside the image
        u32x4 v;
        v.x = v.y = v.z = v.w = p.fill;
        for (int i = t; i < rows_out * nc; i += TILE_THREADS) {
            const int row = i / nc, cc = i - row * nc;
            *reinterpret_cast<u32x4 *>(out_img + ((unsigned)(ty0 + row) * (unsigned)p.opitch + (unsigned)(x0c + cc) * 16u)) = v;
        }
        return;
    }
    const Span sc = chunk_span(b.x0, b.x1, C);
    stage_box(lds, p.in + (long long)tc.img * p.in_stride + ((unsigned)b.y0 * (unsigned)p.pitch + (unsigned)sc.lo * 16u), p.pitch, b.y1 - b.y0 + 1, sc.n(), t);
    __syncthreads();

    const bool constant = p.border == MI_BLUR_WARP_CONSTANT;
    const uint32_t fillp = p.fill;
    for (int i = t; i < nitems; i += TILE_THREADS) {
        const int row = i / nu, u = i - row * nu;
        const int Y = ty0 + row, X = px0 + u * NPIX;
        PerspPos s = persp_position(h, X, Y);           // every pixel of the item lies in the output: s.d >= 1 throughout
        uint32_t o[NPIX * C / 4];
#pragma unroll
        for (int q = 0; q < NPIX * C / 4; q++) o[q] = 0;
#pragma unroll
        for (int k = 0; k < NPIX; k++) {
            const WarpCoord wc = persp_coord_at(s, MI_BLUR_RESIZE_BILINEAR, p.W, p.H);
            const WarpTap wt = warp_tap(b, sc, C, wc.x0, wc.y0);
            uint32_t ta, tb, tc2, td;
            warp_taps<C>(lds, wt.off_a, ta, tb);
            warp_taps<C>(lds, wt.off_b, tc2, td);
            if (wt.one) { tb = ta; td = tc2; }
            if (constant) {
                const bool ixa = (unsigned)wc.x0 < (unsigned)p.W, ixb = (unsigned)(wc.x0 + 1) < (unsigned)p.W;
                const bool iya = (unsigned)wc.y0 < (unsigned)p.H, iyb = (unsigned)(wc.y0 + 1) < (unsigned)p.H;
                ta = ixa && iya ? ta : fillp; tb = ixb && iya ? tb : fillp;
                tc2 = ixa && iyb ? tc2 : fillp; td = ixb && iyb ? td : fillp;
            }
            const uint32_t fx = (uint32_t)wc.fx, fy = (uint32_t)wc.fy;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const uint32_t top = lerp24((ta >> (8 * c)) & 0xffu, (tb >> (8 * c)) & 0xffu, fx);
                const uint32_t bot = lerp24((tc2 >> (8 * c)) & 0xffu, (td >> (8 * c)) & 0xffu, fx);
                const uint32_t v = lerp24_round(top, bot, fy);
                const int e = k * C + c;
                o[e >> 2] |= v << (8 * (e & 3));
            }
            s.nx += h[0]; s.ny += h[3]; s.d += h[6];
        }
        uint8_t *dst = out_img + ((unsigned)Y * (unsigned)p.opitch + (unsigned)x0c * 16u + (unsigned)u * (unsigned)(NPIX * C));
        if constexpr (C == 3) {
            const bool second = u & 1;                  // 24 bytes as 16 + 8 or 8 + 16, as blur_warp_tiled_kernel
            u32x4 v;
            u32x2 hh;
            v.x = second ? o[2] : o[0]; v.y = second ? o[3] : o[1]; v.z = second ? o[4] : o[2]; v.w = second ? o[5] : o[3];
            hh.x = second ? o[0] : o[4]; hh.y = second ? o[1] : o[5];
            *reinterpret_cast<u32x4 *>(dst + (second ? 8 : 0)) = v;
            *reinterpret_cast<u32x2 *>(dst + (second ? 0 : 16)) = hh;
        } else if constexpr (C == 1) {
            u32x2 hh;
            hh.x = o[0]; hh.y = o[1];
            *reinterpret_cast<u32x2 *>(dst) = hh;
        } else {
            u32x4 v;
            v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
            *reinterpret_cast<u32x4 *>(dst) = v;
        }
    }
}

struct WarpPerspGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per image (Ho * opitch)
    long long h[9];
    int W, H, channels, pitch, opitch, mode, border;
    unsigned fill;
};

__global__ __launch_bounds__(256) void blur_warp_persp_generic_kernel(const WarpPerspGenericParams p)
{
    const int64_t h[9] = {p.h[0], p.h[1], p.h[2], p.h[3], p.h[4], p.h[5], p.h[6], p.h[7], p.h[8]};
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.opitch, p.channels, 0, p.in, p.in_stride);   // q.y, q.x: the OUTPUT pixel
        const WarpCoord wc = persp_coord(h, p.mode, p.W, p.H, q.x, q.y);
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)warp_sample(q.src + q.c, (size_t)p.pitch, p.channels, p.W, p.H, p.border, p.fill, wc);
    }
}

// warp_tiles() for the perspective warp: the key holds the nine entries.
long long warp_persp_tiles(const LaunchDesc &d, const TileGrid &g)
{
    const Filter &f = *d.filter;
    const int64_t *h = f.warp_h, key[15] = {d.width, d.band_rows, d.channels, f.out_w, f.out_h, f.warp_border, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8]};
    thread_local int64_t last_key[15];
    thread_local long long last = -1;
    if (last >= 0 && std::equal(key, key + 15, last_key)) return last;
    std::copy(key, key + 15, last_key);
    return last = persp_tiles_max_bytes(g, f.warp_h, f.warp_border, d.width, d.band_rows, f.out_h, d.channels);
}

int launch_warp_persp_tiled(const LaunchDesc &d, const TileGrid &g, long long max_bytes)
{
    const Filter &f = *d.filter;
    WarpPerspTiledParams p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid, g)) return st;
    set_last_kernel("blur_warp_persp_tiled_kernel");
    std::copy(f.warp_h, f.warp_h + 9, p.h);
    p.W = d.width; p.Wo = f.out_w; p.Ho = f.out_h; p.border = f.warp_border; p.fill = (unsigned)f.warp_fill * 0x01010101u;
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto CC) { return do_launch(blur_warp_persp_tiled_kernel<CC>, grid, dim3(TILE_THREADS), (size_t)(max_bytes + WARP_LDS_SLACK), d, p); });
}

int launch_warp_persp_generic(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    set_last_kernel("blur_warp_persp_generic_kernel");
    WarpPerspGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    std::copy(f.warp_h, f.warp_h + 9, p.h);
    p.W = d.width; p.mode = f.sample_mode; p.border = f.warp_border; p.fill = (unsigned)f.warp_fill;
    return do_launch(blur_warp_persp_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

int launch_warp_persp(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::WARP_PERSP, [&](const Filter &f) {
        return resize_ok(f.out_w, f.out_h, f.sample_mode, d.width, d.band_rows, d.channels) && persp_map_ok(f.warp_border, f.warp_fill, f.warp_h, f.out_w, f.out_h);
    });
    if (st != LAUNCH_GO) return st;
    if (warp_tile_aligned(d)) {
        const TileGrid g = warp_grid(out_pitch(d) / 16, d.filter->out_h, d.channels);
        const long long max_bytes = warp_persp_tiles(d, g);
        if (max_bytes <= WARP_LDS_MAX) return launch_warp_persp_tiled(d, g, max_bytes);
    }
    return launch_warp_persp_generic(d);
}

}  // namespace mi_blur
