// resize_kernels.hip — gfx950 kernels of the image resize (mi_blur_enqueue_resize, include/mi_blur.h): exact fixed-point
// bilinear and nearest at any output size.  Every coordinate comes from resize_axis() (filter.h), the one function the
// CPU device and mi_blur_resize_coord use too.
//
// Tiled kernel (blur_resize_tiled_kernel<C>): BILINEAR, 1-4 channels, Wo >= W and Ho >= H, input and output rows of
// whole 16-byte chunks, 16-byte aligned buffers and strides.  One workgroup = one tile of TILE_TH OUTPUT rows x nc
// (<= TILE_NCOLS) OUTPUT chunk columns, laid out by tile_coords (kernel_common.h, unchanged, no halo):
//   * the first threads compute the tile's tables with the exact integer division of resize_axis: one dword per output
//     BYTE of a tile row (the V positions of its two input bytes and fx), one per output row (the two staged rows and
//     fy).  No device-side table, no allocation;
//   * the tile's input footprint — rows ya(first row) .. yb(last row), at most TILE_TH + 2 of them for an enlargement,
//     and the aligned chunks that hold pixels xa(first pixel) .. xb(last pixel) — is staged in LDS.  a and b are already
//     clamped, so the footprint lies inside the image and staging clamps nothing;
//   * the output rows are taken in groups of RS_GROUP.  Vertical blend first, once per staged input byte and output
//     row: V = (2048 - fy) * in[ya] + fy * in[yb] < 2^20, kept as one dword per byte, the four dwords of byte quad j of
//     every chunk side by side (V row = 4 planes of nsc x 16 bytes), so a wave's 16-byte writes are contiguous;
//   * horizontal pass: one output chunk per thread, its 16 table entries held in registers across the groups.  Per output
//     byte two ds_read_b32 at run-time addresses, two v_mad_u32_u24, one rounding shift; one 16-byte store per chunk.
//   The host sizes the LDS from the exact largest footprint of the launch (it walks the strips and tile rows with
//   resize_axis), so no bound on the footprint is assumed.  4 instantiations.
//
// Generic kernel (blur_resize_generic_kernel): one output byte per thread, any shape, ratio, mode and alignment.
#include "kernel_common.h"

#include <algorithm>

namespace mi_blur {

namespace {

constexpr int RS_GROUP = 8;                         // output rows per pass of the tiled kernel
constexpr int RS_XTAB = TILE_NCOLS * 16 * 4;        // bytes of the x table: one dword per output byte of a tile row
constexpr int RS_YTAB = TILE_TH * 4;                // bytes of the y table
constexpr int RS_BIAS = 1 << 21, RS_SHIFT = 22, RS_ONE = 2048;

struct ResizeTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per input image / output image
    int W, H, Wo, Ho;
    int pitch, opitch;                // bytes per input row / output row
    int cpr;                          // OUTPUT 16-byte chunks per row
    int ncols, nstrips, ntiles_y;
    unsigned nblocks;
    int xcd;
    int v_off;                        // LDS byte offset of the V rows (after the tables and the staged footprint)
};

template <int C>
__global__ __launch_bounds__(TILE_THREADS) void blur_resize_tiled_kernel(const ResizeTiledParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint32_t *xtab = reinterpret_cast<uint32_t *>(lds);
    uint32_t *ytab = reinterpret_cast<uint32_t *>(lds + RS_XTAB);
    uint8_t *stage = lds + RS_XTAB + RS_YTAB;
    uint32_t *vbuf = reinterpret_cast<uint32_t *>(lds + p.v_off);
    const int t = threadIdx.x;
    const TileCoords tc = tile_coords<0>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, 0, p.Ho, 0);
    const int ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc;

    // footprint: staged rows r0..r1 and staged chunks sc0..sc1 of the input image (uniform)
    const int r0 = resize_axis(p.H, p.Ho, MI_BLUR_RESIZE_BILINEAR, ty0).a;
    const int r1 = resize_axis(p.H, p.Ho, MI_BLUR_RESIZE_BILINEAR, ty0 + rows_out - 1).b;
    const int px0 = (x0c * 16) / C, px1 = ((x0c + nc) * 16 - 1) / C;
    const int sc0 = (resize_axis(p.W, p.Wo, MI_BLUR_RESIZE_BILINEAR, px0).a * C) >> 4;
    const int sc1 = (resize_axis(p.W, p.Wo, MI_BLUR_RESIZE_BILINEAR, px1).b * C + C - 1) >> 4;
    const int nsr = r1 - r0 + 1, nsc = sc1 - sc0 + 1;

    // ---- tables.  x entry of output byte ob: V dword position of in byte (xa, c) | that of (xb, c) << 10 | fx << 20,
    // the position of staged byte q being plane (q >> 2) & 3, chunk q >> 4, byte q & 3.  y entry: ya - r0 | yb - r0 << 8 | fy << 16
    for (int ob = t; ob < nc * 16; ob += TILE_THREADS) {
        const int gb = x0c * 16 + ob, X = gb / C, c = gb - X * C;
        const ResizeCoord rc = resize_axis(p.W, p.Wo, MI_BLUR_RESIZE_BILINEAR, X);
        const int qa = rc.a * C + c - sc0 * 16, qb = rc.b * C + c - sc0 * 16;
        const uint32_t pa = (uint32_t)(((qa >> 2) & 3) * nsc * 4 + (qa >> 4) * 4 + (qa & 3));
        const uint32_t pb = (uint32_t)(((qb >> 2) & 3) * nsc * 4 + (qb >> 4) * 4 + (qb & 3));
        xtab[ob] = pa | (pb << 10) | ((uint32_t)rc.f << 20);
    }
    if (t < rows_out) {
        const ResizeCoord rc = resize_axis(p.H, p.Ho, MI_BLUR_RESIZE_BILINEAR, ty0 + t);
        ytab[t] = (uint32_t)(rc.a - r0) | ((uint32_t)(rc.b - r0) << 8) | ((uint32_t)rc.f << 16);
    }
    // ---- stage the footprint: nsr rows x nsc chunks, all inside the image
    {
        const uint8_t *src = p.in + (long long)tc.img * p.in_stride + ((unsigned)r0 * (unsigned)p.pitch + (unsigned)sc0 * 16u);
        const int nslots = nsr * nsc;
#pragma unroll 2
        for (int s = t; s < nslots; s += TILE_THREADS) {
            const int row = s / nsc, cc = s - row * nsc;
            const uint4 v = *reinterpret_cast<const uint4 *>(src + ((unsigned)row * (unsigned)p.pitch + (unsigned)cc * 16u));
            *reinterpret_cast<uint4 *>(stage + (size_t)s * 16u) = v;
        }
    }
    __syncthreads();

    // this thread's output chunk in every group: row hk of the group, chunk column hcc; its 16 table entries
    const int hk = t / nc, hcc = t - hk * nc;
    const bool hact = hk < RS_GROUP;
    uint32_t tx[16];
    {
        const uint4 *xp = reinterpret_cast<const uint4 *>(xtab + (hact ? hcc : 0) * 16);
#pragma unroll
        for (int q = 0; q < 4; q++) { const uint4 e = xp[q]; tx[4 * q] = e.x; tx[4 * q + 1] = e.y; tx[4 * q + 2] = e.z; tx[4 * q + 3] = e.w; }
    }
    const int vrow = nsc * 16;                          // dwords of one V row
    uint8_t *out_img = p.out + (long long)tc.img * p.out_stride;

    for (int g0 = 0; g0 < rows_out; g0 += RS_GROUP) {
        const int ng = min(RS_GROUP, rows_out - g0);
        // ---- vertical blend: item = (row k of the group, staged chunk sc)
        for (int i = t; i < ng * nsc; i += TILE_THREADS) {
            const int k = i / nsc, sc = i - k * nsc;
            const uint32_t ye = ytab[g0 + k];
            const uint32_t fy = ye >> 16, gy = RS_ONE - fy;
            const uint4 A = *reinterpret_cast<const uint4 *>(stage + ((size_t)(ye & 0xffu) * nsc + sc) * 16u);
            const uint4 B = *reinterpret_cast<const uint4 *>(stage + ((size_t)((ye >> 8) & 0xffu) * nsc + sc) * 16u);
            const uint32_t a[4] = {A.x, A.y, A.z, A.w}, b[4] = {B.x, B.y, B.z, B.w};
            uint32_t *vp = vbuf + (size_t)k * vrow + sc * 4;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint4 v;
                v.x = __umul24(a[j] & 0xffu, gy) + __umul24(b[j] & 0xffu, fy);
                v.y = __umul24((a[j] >> 8) & 0xffu, gy) + __umul24((b[j] >> 8) & 0xffu, fy);
                v.z = __umul24((a[j] >> 16) & 0xffu, gy) + __umul24((b[j] >> 16) & 0xffu, fy);
                v.w = __umul24(a[j] >> 24, gy) + __umul24(b[j] >> 24, fy);
                *reinterpret_cast<uint4 *>(vp + j * nsc * 4) = v;
            }
        }
        __syncthreads();
        // ---- horizontal pass: V < 2^20 and fx <= 2^11, so both products are v_mad_u32_u24 and the sum < 2^32
        if (hact && hk < ng) {
            const uint32_t *vr = vbuf + (size_t)hk * vrow;
            uint32_t o[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t w = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const uint32_t x = tx[4 * q + e], fx = x >> 20;
                    const uint32_t s = __umul24(vr[x & 1023u], RS_ONE - fx) + __umul24(vr[(x >> 10) & 1023u], fx);
                    w |= ((s + RS_BIAS) >> RS_SHIFT) << (8 * e);
                }
                o[q] = w;
            }
            u32x4 v;
            v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
            *reinterpret_cast<u32x4 *>(out_img + ((unsigned)(ty0 + g0 + hk) * (unsigned)p.opitch + (unsigned)(x0c + hcc) * 16u)) = v;
        }
        __syncthreads();                                // the next group's blends overwrite the V rows
    }
}

struct ResizeGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per image (Ho * opitch)
    int W, H, Wo, Ho, channels, pitch, opitch, mode;
};

__global__ __launch_bounds__(256) void blur_resize_generic_kernel(const ResizeGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.opitch, p.channels, 0, p.in, p.in_stride);   // q.y, q.x: the OUTPUT pixel
        const ResizeCoord cx = resize_axis(p.W, p.Wo, p.mode, q.x), cy = resize_axis(p.H, p.Ho, p.mode, q.y);
        const uint8_t *ra = q.src + (size_t)cy.a * (size_t)p.pitch + q.c, *rb = q.src + (size_t)cy.b * (size_t)p.pitch + q.c;
        const size_t xa = (size_t)cx.a * (size_t)p.channels, xb = (size_t)cx.b * (size_t)p.channels;
        const unsigned fx = (unsigned)cx.f, fy = (unsigned)cy.f;
        const unsigned top = (RS_ONE - fx) * ra[xa] + fx * ra[xb], bot = (RS_ONE - fx) * rb[xa] + fx * rb[xb];
        const unsigned s = (RS_ONE - fy) * top + fy * bot;      // NEAREST: fx = fy = 0, a = b, s = in << 22
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)((s + RS_BIAS) >> RS_SHIFT);
    }
}

// Bytes of one row of the resized image.
long long resize_opitch(const LaunchDesc &d) { return (long long)d.filter->resize_w * d.channels; }

// BILINEAR, 1-4 channels, no reduction on either axis, input and output rows of whole 16-byte chunks, 16-byte aligned
// buffers and strides.
bool resize_tile_aligned(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    return f.resize_mode == MI_BLUR_RESIZE_BILINEAR && d.channels <= 4 && f.resize_w >= d.width && f.resize_h >= d.band_rows &&
           (long long)d.width * d.channels % 16 == 0 && resize_opitch(d) % 16 == 0 && (uintptr_t)d.in % 16 == 0 && (uintptr_t)d.out % 16 == 0 &&
           d.in_stride % 16 == 0 && d.out_stride % 16 == 0;
}

// The tile decomposition of a launch and its largest input footprint (rows, 16-byte chunks), exactly as the kernel
// computes them: the host walks the strips and the tile rows with resize_axis.
struct ResizeTiles { int cpr, nstrips, ncols, ntiles_y, max_nsc, max_nsr; };
ResizeTiles resize_tiles(const LaunchDesc &d)
{
    const int C = d.channels, W = d.width, H = d.band_rows, Wo = d.filter->resize_w, Ho = d.filter->resize_h;
    ResizeTiles t{};
    t.cpr = (int)(resize_opitch(d) / 16);
    t.nstrips = (t.cpr + TILE_NCOLS - 1) / TILE_NCOLS;
    t.ncols = (t.cpr + t.nstrips - 1) / t.nstrips;
    t.ntiles_y = (Ho + TILE_TH - 1) / TILE_TH;
    t.max_nsc = t.max_nsr = 1;
    for (int s = 0; s < t.nstrips; s++) {
        const int x0c = s * t.ncols, nc = std::min(t.ncols, t.cpr - x0c);
        if (nc <= 0) continue;
        const int px0 = (x0c * 16) / C, px1 = ((x0c + nc) * 16 - 1) / C;
        const int sc0 = (resize_axis(W, Wo, MI_BLUR_RESIZE_BILINEAR, px0).a * C) >> 4;
        const int sc1 = (resize_axis(W, Wo, MI_BLUR_RESIZE_BILINEAR, px1).b * C + C - 1) >> 4;
        t.max_nsc = std::max(t.max_nsc, sc1 - sc0 + 1);
    }
    for (int ty = 0; ty < t.ntiles_y; ty++) {
        const int ty0 = ty * TILE_TH, rows = std::min(TILE_TH, Ho - ty0);
        const int r0 = resize_axis(H, Ho, MI_BLUR_RESIZE_BILINEAR, ty0).a, r1 = resize_axis(H, Ho, MI_BLUR_RESIZE_BILINEAR, ty0 + rows - 1).b;
        t.max_nsr = std::max(t.max_nsr, r1 - r0 + 1);
    }
    return t;
}
// What the kernel's table entries can hold: V positions below 1024 (64 chunks), staged rows below 256.  An enlargement
// stays far inside (at most 34 rows x 35 chunks); a launch that does not fit goes to the generic kernel.
bool resize_tiles_fit(const ResizeTiles &t) { return t.max_nsc <= 64 && t.max_nsr <= 255; }

int launch_resize_tiled(const LaunchDesc &d, const ResizeTiles &t)
{
    const int C = d.channels;
    ResizeTiledParams p{};
    p.in = d.in; p.out = d.out;
    p.W = d.width; p.H = d.band_rows; p.Wo = d.filter->resize_w; p.Ho = d.filter->resize_h;
    p.pitch = d.width * C; p.opitch = (int)resize_opitch(d);
    p.in_stride = d.in_stride ? d.in_stride : dense_in(d);
    p.out_stride = d.out_stride ? d.out_stride : dense_out(d);
    p.cpr = t.cpr; p.nstrips = t.nstrips; p.ncols = t.ncols; p.ntiles_y = t.ntiles_y;
    const long long nblocks = (long long)d.n_images * p.ntiles_y * p.nstrips;
    if (nblocks > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    set_last_kernel("blur_resize_tiled_kernel");
    p.nblocks = (unsigned)nblocks;
    p.xcd = nblocks >= 16 ? 1 : 0;
    p.v_off = RS_XTAB + RS_YTAB + t.max_nsr * t.max_nsc * 16;
    const size_t lds = (size_t)p.v_off + (size_t)RS_GROUP * t.max_nsc * 64u;
    const dim3 grid((unsigned)nblocks), block(TILE_THREADS);
    return dispatch<1, 2, 3, 4>(C, [&](auto CC) { return do_launch(blur_resize_tiled_kernel<CC>, grid, block, lds, d, p); });
}

int launch_resize_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_resize_generic_kernel");
    ResizeGenericParams p{};
    p.in = d.in; p.out = d.out;
    p.W = d.width; p.H = d.band_rows; p.Wo = d.filter->resize_w; p.Ho = d.filter->resize_h; p.channels = d.channels;
    p.pitch = d.width * d.channels; p.opitch = (int)resize_opitch(d); p.mode = d.filter->resize_mode;
    p.in_stride = d.in_stride ? d.in_stride : dense_in(d);
    p.block = dense_out(d);
    p.out_stride = d.out_stride ? d.out_stride : p.block;
    p.total = p.block * d.n_images;
    return do_launch(blur_resize_generic_kernel, byte_grid(p.total), dim3(256), 0, d, p);
}

}  // namespace

// Only whole images (launch_checks()); out_stride is measured against the RESIZED image (dense_out()).
int launch_resize(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::RESIZE, [&](const Filter &f) {
        const mi_blur_resize r{f.resize_w, f.resize_h, f.resize_mode};
        return resize_ok(&r, d.width, d.band_rows, d.channels);
    });
    if (st != LAUNCH_GO) return st;
    if (resize_tile_aligned(d)) {
        const ResizeTiles t = resize_tiles(d);
        if (resize_tiles_fit(t)) return launch_resize_tiled(d, t);
    }
    return launch_resize_generic(d);
}

}  // namespace mi_blur
