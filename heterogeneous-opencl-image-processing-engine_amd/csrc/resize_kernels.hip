// resize_kernels.hip — gfx950 kernels of the image resize (mi_blur_enqueue_resize, include/mi_blur.h): exact fixed-point
// bilinear and nearest at any output size.  Every coordinate comes from resize_axis() (filter.h), the one function the
// CPU device and mi_blur_resize_coord use too.
//
// Tiled kernel (blur_resize_tiled_kernel<C>): BILINEAR, 1-4 channels, Wo >= W and Ho >= H, input and output rows of
// whole 16-byte chunks, 16-byte aligned buffers and strides.  One workgroup = one tile of TILE_TH OUTPUT rows x nc
// (<= TILE_NCOLS) OUTPUT chunk columns: the shared fill_tiles / tile_coords (kernel_common.h, no halo) on the OUTPUT image.
// What a tile stages and where a tap lies in LDS comes from filter.h ("Tile geometry"), as does the host's sizing; the
// staging is the shared stage_box, the blend the shared lerp24:
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
//   The host sizes the LDS from the exact largest footprint of the launch (resize_tiles(), filter.h: it walks the strips
//   and tile rows with the kernel's own functions), so no bound on the footprint is assumed.  4 instantiations.
//
// Generic kernel (blur_resize_generic_kernel): one output byte per thread, any shape, ratio, mode and alignment.
#include "kernel_common.h"

namespace mi_blur {

namespace {

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
    const Span sr = resize_stage_rows(p.H, p.Ho, ty0, rows_out), sc = resize_stage_chunks(p.W, p.Wo, C, x0c, nc);
    const int r0 = sr.lo, sc0 = sc.lo, nsr = sr.n(), nsc = sc.n();

    // ---- tables (resize_x_entry, resize_y_entry: filter.h): one x entry per output byte of a tile row, one y entry per row
    for (int ob = t; ob < nc * 16; ob += TILE_THREADS) {
        const int gb = x0c * 16 + ob, X = gb / C, c = gb - X * C;
        xtab[ob] = resize_x_entry(resize_axis(p.W, p.Wo, MI_BLUR_RESIZE_BILINEAR, X), C, c, sc0, nsc);
    }
    if (t < rows_out) ytab[t] = resize_y_entry(resize_axis(p.H, p.Ho, MI_BLUR_RESIZE_BILINEAR, ty0 + t), r0);
    // ---- stage the footprint: nsr rows x nsc chunks, all inside the image
    stage_box(stage, p.in + (long long)tc.img * p.in_stride + ((unsigned)r0 * (unsigned)p.pitch + (unsigned)sc0 * 16u), p.pitch, nsr, nsc, t);
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
            const uint32_t fy = resize_y_f(ye);
            const uint4 A = *reinterpret_cast<const uint4 *>(stage + ((size_t)resize_y_row_a(ye) * nsc + sc) * 16u);
            const uint4 B = *reinterpret_cast<const uint4 *>(stage + ((size_t)resize_y_row_b(ye) * nsc + sc) * 16u);
            const uint32_t a[4] = {A.x, A.y, A.z, A.w}, b[4] = {B.x, B.y, B.z, B.w};
            uint32_t *vp = vbuf + (size_t)k * vrow + sc * 4;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint4 v;
                v.x = lerp24(a[j] & 0xffu, b[j] & 0xffu, fy);
                v.y = lerp24((a[j] >> 8) & 0xffu, (b[j] >> 8) & 0xffu, fy);
                v.z = lerp24((a[j] >> 16) & 0xffu, (b[j] >> 16) & 0xffu, fy);
                v.w = lerp24(a[j] >> 24, b[j] >> 24, fy);
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
                    const uint32_t x = tx[4 * q + e];
                    w |= lerp24_round(vr[resize_x_pos_a(x)], vr[resize_x_pos_b(x)], resize_x_f(x)) << (8 * e);
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
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)bilinear_blend(ra[xa], ra[xb], rb[xa], rb[xb], (unsigned)cx.f, (unsigned)cy.f);   // NEAREST: fx = fy = 0, a = b
    }
}

// tile_aligned (kernel_common.h) with output rows of whole chunks too, BILINEAR, no reduction on either axis.
bool resize_tile_aligned(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    return tile_aligned(d) && out_pitch(d) % 16 == 0 && f.sample_mode == MI_BLUR_RESIZE_BILINEAR && f.out_w >= d.width && f.out_h >= d.band_rows;
}

// g: the tiles of the OUTPUT image; t: its largest footprint (resize_tiles(), filter.h), which fits.
int launch_resize_tiled(const LaunchDesc &d, const TileGrid &g, const ResizeTiles &t)
{
    ResizeTiledParams p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid, g)) return st;
    set_last_kernel("blur_resize_tiled_kernel");
    p.W = d.width; p.Wo = d.filter->out_w; p.Ho = d.filter->out_h;
    p.v_off = resize_v_off(t);
    const size_t lds = resize_lds_bytes(t);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto CC) { return do_launch(blur_resize_tiled_kernel<CC>, grid, dim3(TILE_THREADS), lds, d, p); });
}

int launch_resize_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_resize_generic_kernel");
    ResizeGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    p.W = d.width; p.Wo = d.filter->out_w; p.Ho = d.filter->out_h; p.mode = d.filter->sample_mode;
    return do_launch(blur_resize_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

// Only whole images (launch_checks()); out_stride is measured against the RESIZED image (dense_out()).
int launch_resize(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::RESIZE, [&](const Filter &f) { return resize_ok(f.out_w, f.out_h, f.sample_mode, d.width, d.band_rows, d.channels); });
    if (st != LAUNCH_GO) return st;
    if (resize_tile_aligned(d)) {
        const Filter &f = *d.filter;
        const TileGrid g = tile_grid(out_pitch(d) / 16, f.out_h);
        const ResizeTiles t = resize_tiles(g, d.width, d.band_rows, f.out_w, f.out_h, d.channels);
        if (resize_tiles_fit(t)) return launch_resize_tiled(d, g, t);
    }
    return launch_resize_generic(d);
}

}  // namespace mi_blur
