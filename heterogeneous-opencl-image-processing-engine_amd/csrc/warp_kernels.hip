// warp_kernels.hip — gfx950 kernels of the affine warp (mi_blur_enqueue_warp, include/mi_blur.h): exact fixed-point
// bilinear and nearest under a Q16 output -> input matrix, CLAMP or CONSTANT border, any output size.  Every coordinate
// comes from warp_position() / warp_axis() (filter.h), the functions the CPU device and mi_blur_warp_coord use too.
//
// Tiled kernel (blur_warp_tiled_kernel<C>): BILINEAR, 1-4 channels, input and output rows of whole 16-byte chunks,
// 16-byte aligned buffers and strides, largest footprint at most WARP_LDS_MAX bytes.  One workgroup = one tile of TILE_TH
// OUTPUT rows x nc (<= 4 * C: 64 pixels) OUTPUT chunk columns, laid out by tile_coords (kernel_common.h, no halo).  A rotated
// tile costs its bounding box, so the tile is close to square in pixels (resize's 32-chunk strip would stage 3-8 times as much):
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
//   The host sizes the LDS from the exact largest footprint of the launch (it walks the tiles of one image with
//   warp_footprint), so no bound on the footprint is assumed.  4 instantiations, no scratch.
//
// Generic kernel (blur_warp_generic_kernel): one output byte per thread, any shape, map, mode, border and alignment.
#include "kernel_common.h"

#include <algorithm>

namespace mi_blur {

namespace {

constexpr long long WARP_LDS_SLACK = 16;            // LDS behind the staged footprint that the 8-byte tap reads may touch
constexpr long long WARP_LDS_MAX = 65536 - WARP_LDS_SLACK;   // largest footprint: with the slack, the dynamic LDS a launch may ask for without raising the limit
constexpr int WARP_TILE_PX = 64;                    // output pixels across a tile (at most)

// Chunks of the smallest run of chunks that starts and ends on a pixel (a strip is a whole number of them), and of the widest tile.
constexpr int warp_unit(int C) { return C == 3 ? 3 : 1; }
constexpr int warp_max_cols(int C) { return WARP_TILE_PX * C / 16; }

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

// Pixels xa and xa + 1 of a staged row, pixel xa starting at byte offset `off` of the footprint: a (and b) = their C
// bytes, lowest channel lowest.  Two dword reads at the 4-byte aligned address below `off` (one ds_read2_b32) and a 64-bit
// shift; 3 channels can straddle a third dword (bytes 3 .. 8 of the two).  The reads reach at most 11 bytes past the start
// of pixel xa, which WARP_LDS_SLACK keeps inside the launch's LDS.
template <int C>
__device__ __forceinline__ void warp_taps(const uint8_t *lds, int off, uint32_t &a, uint32_t &b)
{
    constexpr uint32_t PIX = C == 4 ? 0xffffffffu : (1u << (8 * (C & 3))) - 1u;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(lds + (off & ~3));
    const int sh = 8 * (off & 3);
    const uint64_t v = (((uint64_t)q[1] << 32) | q[0]) >> sh;
    a = (uint32_t)v & PIX;
    if constexpr (C == 3) {
        const uint64_t v2 = (((uint64_t)q[2] << 32) | q[1]) >> sh;      // the bytes from off + 4 on; pixel b starts at off + 3
        b = (((uint32_t)v >> 24) | ((uint32_t)v2 << 8)) & PIX;
    } else {
        b = (uint32_t)(v >> (8 * C)) & PIX;
    }
}

template <int C>
__global__ __launch_bounds__(TILE_THREADS) void blur_warp_tiled_kernel(const WarpTiledParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int U = warp_unit(C), NPIX = C == 1 || C == 3 ? 8 : 16 / C, NITEM = U * 16 / (NPIX * C);   // pixels of a work item; items per group of U chunks
    const int t = threadIdx.x;
    const TileCoords tc = tile_coords<0>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, 0, p.Ho, 0);
    const int ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc;
    const int64_t m[6] = {p.m[0], p.m[1], p.m[2], p.m[3], p.m[4], p.m[5]};

    // footprint (uniform): input pixels bx0..bx1 x by0..by1, staged as rows by0..by1 of chunks sc0..sc1
    const int px0 = (x0c * 16) / C, px1 = ((x0c + nc) * 16 - 1) / C;
    const WarpBox b = warp_footprint(m, MI_BLUR_RESIZE_BILINEAR, p.border, p.W, p.H, px0, px1, ty0, ty0 + rows_out - 1);
    const int nu = nc / U * NITEM, nitems = rows_out * nu;
    uint8_t *out_img = p.out + (long long)tc.img * p.out_stride;

    if (b.x0 > b.x1 || b.y0 > b.y1) {                   // CONSTANT, every tap outside the image: the blend of four fills is fill
        u32x4 v;
        v.x = v.y = v.z = v.w = p.fill;
        for (int i = t; i < rows_out * nc; i += TILE_THREADS) {
            const int row = i / nc, cc = i - row * nc;
            *reinterpret_cast<u32x4 *>(out_img + ((unsigned)(ty0 + row) * (unsigned)p.opitch + (unsigned)(x0c + cc) * 16u)) = v;
        }
        return;
    }
    const int sc0 = (b.x0 * C) >> 4, sc1 = (b.x1 * C + C - 1) >> 4;
    const int nsr = b.y1 - b.y0 + 1, nsc = sc1 - sc0 + 1;
    {
        const uint8_t *src = p.in + (long long)tc.img * p.in_stride + ((unsigned)b.y0 * (unsigned)p.pitch + (unsigned)sc0 * 16u);
        const int nslots = nsr * nsc;
#pragma unroll 2
        for (int s = t; s < nslots; s += TILE_THREADS) {
            const int row = s / nsc, cc = s - row * nsc;
            const uint4 v = *reinterpret_cast<const uint4 *>(src + ((unsigned)row * (unsigned)p.pitch + (unsigned)cc * 16u));
            *reinterpret_cast<uint4 *>(lds + (size_t)s * 16u) = v;
        }
    }
    __syncthreads();

    const int rowb = nsc * 16, col0 = sc0 * 16;         // bytes of a staged row; image byte column of staged byte 0
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
            // the taps, clamped into the staged box: under CLAMP that is the clamp into the image, under CONSTANT a tap
            // the clamp moves lies outside the image and is replaced below
            const int xa = min(max(ax.i0, b.x0), b.x1), xb = min(max(ax.i0 + 1, b.x0), b.x1);
            const int ya = min(max(ay.i0, b.y0), b.y1), yb = min(max(ay.i0 + 1, b.y0), b.y1);
            const int oa = (ya - b.y0) * rowb - col0, ob = (yb - b.y0) * rowb - col0;   // + x * C: inside the staged rows
            // xb is xa + 1, or xa where the clamp met the edge of the box: both taps of a row come from one read at xa
            uint32_t ta, tb, tc2, td;
            warp_taps<C>(lds, oa + xa * C, ta, tb);
            warp_taps<C>(lds, ob + xa * C, tc2, td);
            if (xb == xa) { tb = ta; td = tc2; }
            if (constant) {
                const bool ixa = (unsigned)ax.i0 < (unsigned)p.W, ixb = (unsigned)(ax.i0 + 1) < (unsigned)p.W;
                const bool iya = (unsigned)ay.i0 < (unsigned)p.H, iyb = (unsigned)(ay.i0 + 1) < (unsigned)p.H;
                ta = ixa && iya ? ta : fillp; tb = ixb && iya ? tb : fillp;
                tc2 = ixa && iyb ? tc2 : fillp; td = ixb && iyb ? td : fillp;
            }
            const uint32_t fx = (uint32_t)ax.f, gx = 2048u - fx, fy = (uint32_t)ay.f, gy = 2048u - fy;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const uint32_t top = __umul24((ta >> (8 * c)) & 0xffu, gx) + __umul24((tb >> (8 * c)) & 0xffu, fx);
                const uint32_t bot = __umul24((tc2 >> (8 * c)) & 0xffu, gx) + __umul24((td >> (8 * c)) & 0xffu, fx);
                const uint32_t v = (__umul24(top, gy) + __umul24(bot, fy) + (1u << 21)) >> 22;   // top, bot < 2^20
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

// Bytes of one row of the warped image.
long long warp_opitch(const LaunchDesc &d) { return (long long)d.filter->warp_w * d.channels; }

// BILINEAR, 1-4 channels, input and output rows of whole 16-byte chunks, 16-byte aligned buffers and strides.
bool warp_tile_aligned(const LaunchDesc &d)
{
    return d.filter->warp_mode == MI_BLUR_RESIZE_BILINEAR && d.channels <= 4 && (long long)d.width * d.channels % 16 == 0 &&
           warp_opitch(d) % 16 == 0 && (uintptr_t)d.in % 16 == 0 && (uintptr_t)d.out % 16 == 0 && d.in_stride % 16 == 0 && d.out_stride % 16 == 0;
}

// The tile decomposition of a launch and the LDS bytes of its largest footprint, exactly as the kernel computes them:
// the host walks the tiles of one image with warp_footprint (and stops at the first one over WARP_LDS_MAX).  A stream of
// launches repeats one geometry, so each thread keeps the last answer.
struct WarpTiles { int cpr, nstrips, ncols, ntiles_y; long long max_bytes; };
struct WarpTilesKey {
    int W, H, C, Wo, Ho, border;
    int64_t m[6];
    bool operator==(const WarpTilesKey &o) const
    {
        return W == o.W && H == o.H && C == o.C && Wo == o.Wo && Ho == o.Ho && border == o.border && std::equal(m, m + 6, o.m);
    }
};
WarpTiles warp_tiles(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    const int C = d.channels, W = d.width, H = d.band_rows, Wo = f.warp_w, Ho = f.warp_h, U = warp_unit(C);
    WarpTilesKey key{W, H, C, Wo, Ho, f.warp_border, {}};
    std::copy(f.warp_m, f.warp_m + 6, key.m);
    thread_local WarpTilesKey last_key{};
    thread_local WarpTiles last{};
    if (last.cpr && key == last_key) return last;
    WarpTiles t{};
    t.cpr = (int)(warp_opitch(d) / 16);
    const int units = t.cpr / U, max_units = warp_max_cols(C) / U;
    t.nstrips = (units + max_units - 1) / max_units;
    t.ncols = U * ((units + t.nstrips - 1) / t.nstrips);
    t.ntiles_y = (Ho + TILE_TH - 1) / TILE_TH;
    for (int ty = 0; ty < t.ntiles_y && t.max_bytes <= WARP_LDS_MAX; ty++) {
        const int ty0 = ty * TILE_TH, rows = std::min(TILE_TH, Ho - ty0);
        for (int s = 0; s < t.nstrips; s++) {
            const int x0c = s * t.ncols, nc = std::min(t.ncols, t.cpr - x0c);
            if (nc <= 0) continue;
            const int px0 = (x0c * 16) / C, px1 = ((x0c + nc) * 16 - 1) / C;
            const WarpBox b = warp_footprint(f.warp_m, MI_BLUR_RESIZE_BILINEAR, f.warp_border, W, H, px0, px1, ty0, ty0 + rows - 1);
            if (b.x0 > b.x1 || b.y0 > b.y1) continue;
            const long long nsc = ((b.x1 * C + C - 1) >> 4) - ((b.x0 * C) >> 4) + 1, nsr = b.y1 - b.y0 + 1;
            t.max_bytes = std::max(t.max_bytes, nsr * nsc * 16);
        }
    }
    last_key = key; last = t;
    return t;
}

int launch_warp_tiled(const LaunchDesc &d, const WarpTiles &t)
{
    const Filter &f = *d.filter;
    const int C = d.channels;
    WarpTiledParams p{};
    p.in = d.in; p.out = d.out;
    p.W = d.width; p.H = d.band_rows; p.Wo = f.warp_w; p.Ho = f.warp_h;
    p.pitch = d.width * C; p.opitch = (int)warp_opitch(d);
    p.in_stride = d.in_stride ? d.in_stride : dense_in(d);
    p.out_stride = d.out_stride ? d.out_stride : dense_out(d);
    for (int i = 0; i < 6; i++) p.m[i] = f.warp_m[i];
    p.border = f.warp_border; p.fill = (unsigned)f.warp_fill * 0x01010101u;
    p.cpr = t.cpr; p.nstrips = t.nstrips; p.ncols = t.ncols; p.ntiles_y = t.ntiles_y;
    const long long nblocks = (long long)d.n_images * p.ntiles_y * p.nstrips;
    if (nblocks > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    set_last_kernel("blur_warp_tiled_kernel");
    p.nblocks = (unsigned)nblocks;
    p.xcd = nblocks >= 16 ? 1 : 0;
    const dim3 grid((unsigned)nblocks), block(TILE_THREADS);
    return dispatch<1, 2, 3, 4>(C, [&](auto CC) { return do_launch(blur_warp_tiled_kernel<CC>, grid, block, (size_t)(t.max_bytes + WARP_LDS_SLACK), d, p); });
}

int launch_warp_generic(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    set_last_kernel("blur_warp_generic_kernel");
    WarpGenericParams p{};
    p.in = d.in; p.out = d.out;
    p.W = d.width; p.H = d.band_rows; p.channels = d.channels;
    p.pitch = d.width * d.channels; p.opitch = (int)warp_opitch(d); p.mode = f.warp_mode; p.border = f.warp_border; p.fill = (unsigned)f.warp_fill;
    for (int i = 0; i < 6; i++) p.m[i] = f.warp_m[i];
    p.in_stride = d.in_stride ? d.in_stride : dense_in(d);
    p.block = dense_out(d);
    p.out_stride = d.out_stride ? d.out_stride : p.block;
    p.total = p.block * d.n_images;
    return do_launch(blur_warp_generic_kernel, byte_grid(p.total), dim3(256), 0, d, p);
}

}  // namespace

// Only whole images (launch_checks()); out_stride is measured against the WARPED image (dense_out()).
int launch_warp(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::WARP, [&](const Filter &f) {
        mi_blur_warp w{f.warp_w, f.warp_h, f.warp_mode, f.warp_border, f.warp_fill, {}};
        for (int i = 0; i < 6; i++) w.m[i] = f.warp_m[i];
        return warp_ok(&w, d.width, d.band_rows, d.channels);
    });
    if (st != LAUNCH_GO) return st;
    if (warp_tile_aligned(d)) {
        const WarpTiles t = warp_tiles(d);
        if (t.max_bytes <= WARP_LDS_MAX) return launch_warp_tiled(d, t);
    }
    return launch_warp_generic(d);
}

}  // namespace mi_blur
