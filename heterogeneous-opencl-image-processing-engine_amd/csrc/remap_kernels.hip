// remap_kernels.hip — gfx950 kernels of the remap (mi_blur_enqueue_remap, include/mi_blur.h): exact fixed-point bilinear and
// nearest sampling through a table that gives every output pixel its own input position (int32 pairs, 11 fraction bits),
// CLAMP or CONSTANT border, any output size.  Every coordinate comes from remap_axis() (filter.h), the function the CPU
// device, mi_blur_remap_coord and mi_blur_remap_plan use too; the taps, the blend and the borders are the affine warp's.
//
// Tiled kernel (blur_remap_tiled_kernel<C>): BILINEAR, 1-4 channels, input and output rows of whole 16-byte chunks,
// 16-byte aligned buffers, strides and map.  Tiles and work items are blur_warp_tiled_kernel's (warp_grid(), filter.h: 32
// OUTPUT rows x 64 pixels; an item is one row x NPIX whole pixels).  The host cannot know a tile's source footprint: the
// map is in device memory.  So the workgroup finds it:
//   1. every thread loads the map entries of its item (two items for 4 channels) with 16-byte loads and KEEPS them in
//      registers (at most 16 dwords; the form that shipped: the compiler's resource report shows no scratch), computes
//      x0, y0 of each and reduces their minima and maxima: over its pixels, across the wave (wave64, six xor-shuffles per
//      value), across the four waves through 16 LDS words and one barrier;
//   2. remap_box() (filter.h) turns the four extrema into the box, exactly as warp_footprint() finishes its own;
//   3. uniformly per tile: an empty box (CONSTANT, every tap outside) stores `fill`; a box of at most stage_bytes is staged
//      with stage_box and sampled from LDS as the warp kernel samples (warp_tap, two 8-byte LDS reads per pixel, lerp24);
//      a larger one is sampled straight from global memory with warp_sample().  The item's vector stores in every branch.
//   Why every 16-byte map load is aligned: entry (Y, X) lies (Y * Wo + X) * 8 bytes into the map.  An item starts at
//   X = px0 + u * NPIX, px0 = x0c * 16 / C with x0c a multiple of warp_unit(C): a multiple of 16 (C = 1, 3), 8 (C = 2) or
//   4 (C = 4) pixels, and NPIX is 8, 8, 8, 4: X is a multiple of 4, X * 8 of 32.  Rows of whole chunks make Wo a multiple
//   of 16, 8, 16, 4 pixels, so Y * Wo * 8 is a multiple of 32 too.  With a 16-byte aligned map every run starts on 32 bytes.
//   LDS: REMAP_RED_BYTES of reduction words, stage_bytes of box, WARP_LDS_SLACK (remap_lds_bytes(), filter.h).  No scratch.
//
// Generic kernel (blur_remap_generic_kernel): one output byte per thread, any shape, mode, border and alignment (the map
// 4-byte aligned, as int32 is).
#include "kernel_common.h"

namespace mi_blur {

namespace {

struct RemapTiledParams {
    const uint8_t *in;
    uint8_t *out;
    const int32_t *map;
    long long in_stride, out_stride;  // bytes per input image / output image
    int W, H, Wo, Ho;
    int pitch, opitch;                // bytes per input row / output row
    int cpr;                          // OUTPUT 16-byte chunks per row
    int ncols, nstrips, ntiles_y;
    unsigned nblocks;
    int xcd;
    int border;
    unsigned fill;                    // the fill byte in all four bytes
    int stage_bytes;
};

// The stores of one item: NPIX * C bytes at dst, as blur_warp_tiled_kernel stores them (24 bytes of 3 channels as
// 16 + 8 or 8 + 16, all naturally aligned).
template <int C, int N>
__device__ __forceinline__ void remap_store(uint8_t *dst, const uint32_t (&o)[N], int u)
{
    if constexpr (C == 3) {
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

template <int C>
__global__ __launch_bounds__(TILE_THREADS) void blur_remap_tiled_kernel(const RemapTiledParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int U = warp_unit(C), NPIX = C == 1 || C == 3 ? 8 : 16 / C, NITEM = U * 16 / (NPIX * C);   // as blur_warp_tiled_kernel
    constexpr int ITEMS = C == 4 ? 2 : 1;               // items per thread: a tile has at most 32 rows x 64 / NPIX items
    constexpr int NO = NPIX * C / 4;                    // output dwords of an item
    const int t = threadIdx.x;
    const TileCoords tc = tile_coords<0>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, 0, p.Ho, 0);
    const int ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc;
    const int px0 = tile_pixels(x0c, nc, C).lo;
    const int nu = nc / U * NITEM, nitems = rows_out * nu;   // <= ITEMS * TILE_THREADS
    uint8_t *out_img = p.out + (long long)tc.img * p.out_stride;

    // 1. the map entries of this thread's items, and the extrema of their first taps
    int32_t mp[ITEMS][NPIX * 2];
    int x_lo = INT_MAX, x_hi = INT_MIN, y_lo = INT_MAX, y_hi = INT_MIN;
#pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        const int i = t + j * TILE_THREADS;
#pragma unroll
        for (int e = 0; e < NPIX * 2; e++) mp[j][e] = 0;
        if (i < nitems) {
            const int row = i / nu, u = i - row * nu;
            const long long entry = (long long)(ty0 + row) * p.Wo + (px0 + u * NPIX);
            const u32x4 *src = reinterpret_cast<const u32x4 *>(p.map + entry * 2);      // 32-byte aligned: see the head of this file
#pragma unroll
            for (int v = 0; v < NPIX / 2; v++) {
                const u32x4 e4 = src[v];
                mp[j][4 * v] = (int32_t)e4.x; mp[j][4 * v + 1] = (int32_t)e4.y; mp[j][4 * v + 2] = (int32_t)e4.z; mp[j][4 * v + 3] = (int32_t)e4.w;
            }
#pragma unroll
            for (int k = 0; k < NPIX; k++) {
                const WarpCoord q = remap_coord(mp[j][2 * k], mp[j][2 * k + 1], MI_BLUR_RESIZE_BILINEAR, p.W, p.H);
                x_lo = min(x_lo, q.x0); x_hi = max(x_hi, q.x0); y_lo = min(y_lo, q.y0); y_hi = max(y_hi, q.y0);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        x_lo = min(x_lo, __shfl_xor(x_lo, off)); x_hi = max(x_hi, __shfl_xor(x_hi, off));
        y_lo = min(y_lo, __shfl_xor(y_lo, off)); y_hi = max(y_hi, __shfl_xor(y_hi, off));
    }
    int *red = reinterpret_cast<int *>(lds);            // REMAP_RED_BYTES: [wave][x_lo, x_hi, y_lo, y_hi]
    if ((t & 63) == 0) {
        int *r = red + (t >> 6) * 4;
        r[0] = x_lo; r[1] = x_hi; r[2] = y_lo; r[3] = y_hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TILE_THREADS / 64; w++) {
        x_lo = min(x_lo, red[w * 4]); x_hi = max(x_hi, red[w * 4 + 1]); y_lo = min(y_lo, red[w * 4 + 2]); y_hi = max(y_hi, red[w * 4 + 3]);
    }

    // 2. the box (uniform: every thread holds the same extrema now).  The tile has at least one item, so they are set.
    const WarpBox b = remap_box(x_lo, x_hi, y_lo, y_hi, p.border, p.W, p.H);

    // 3. empty, staged or direct
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
    const uint8_t *in_img = p.in + (long long)tc.img * p.in_stride;
    const bool constant = p.border == MI_BLUR_WARP_CONSTANT;
    const bool staged = (long long)(b.y1 - b.y0 + 1) * sc.n() * 16 <= (long long)p.stage_bytes;
    const uint8_t *box = lds + REMAP_RED_BYTES;         // the staged box: behind the reduction words, which are read above
    if (staged) {
        stage_box(lds + REMAP_RED_BYTES, in_img + ((unsigned)b.y0 * (unsigned)p.pitch + (unsigned)sc.lo * 16u), p.pitch, b.y1 - b.y0 + 1, sc.n(), t);
        __syncthreads();
    }
    const uint32_t fillp = p.fill;
#pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        const int i = t + j * TILE_THREADS;
        if (i >= nitems) break;
        const int row = i / nu, u = i - row * nu;
        uint32_t o[NO];
#pragma unroll
        for (int q = 0; q < NO; q++) o[q] = 0;
#pragma unroll
        for (int k = 0; k < NPIX; k++) {
            const WarpCoord wc = remap_coord(mp[j][2 * k], mp[j][2 * k + 1], MI_BLUR_RESIZE_BILINEAR, p.W, p.H);
            if (staged) {
                // the warp kernel's sampling: the taps clamped into the staged box, both taps of a row from one read at xa
                const WarpTap wt = warp_tap(b, sc, C, wc.x0, wc.y0);
                uint32_t ta, tb, tc2, td;
                warp_taps<C>(box, wt.off_a, ta, tb);
                warp_taps<C>(box, wt.off_b, tc2, td);
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
                    const int e = k * C + c;            // byte of the item: a constant
                    o[e >> 2] |= v << (8 * (e & 3));
                }
            } else {
                // the box is too large for the LDS: the four taps of every byte straight from global memory, warp_sample() itself
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const uint32_t v = warp_sample(in_img + c, (size_t)p.pitch, C, p.W, p.H, p.border, fillp & 0xffu, wc);
                    const int e = k * C + c;
                    o[e >> 2] |= v << (8 * (e & 3));
                }
            }
        }
        remap_store<C>(out_img + ((unsigned)(ty0 + row) * (unsigned)p.opitch + (unsigned)x0c * 16u + (unsigned)u * (unsigned)(NPIX * C)), o, u);
    }
}

struct RemapGenericParams {
    const uint8_t *in;
    uint8_t *out;
    const int32_t *map;
    long long in_stride, out_stride, block, total;   // block = output bytes per image (Ho * opitch)
    int W, H, Wo, channels, pitch, opitch, mode, border;
    unsigned fill;
};

__global__ __launch_bounds__(256) void blur_remap_generic_kernel(const RemapGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.opitch, p.channels, 0, p.in, p.in_stride);   // q.y, q.x: the OUTPUT pixel
        const int32_t *e = p.map + ((long long)q.y * p.Wo + q.x) * 2;
        const WarpCoord wc = remap_coord(e[0], e[1], p.mode, p.W, p.H);
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)warp_sample(q.src + q.c, (size_t)p.pitch, p.channels, p.W, p.H, p.border, p.fill, wc);
    }
}

// The warp's rule (tile_aligned() with output rows of whole chunks too, BILINEAR) plus a 16-byte aligned map.
bool remap_tile_aligned(const LaunchDesc &d)
{
    return tile_aligned(d) && out_pitch(d) % 16 == 0 && d.filter->sample_mode == MI_BLUR_RESIZE_BILINEAR && (uintptr_t)d.filter->remap_map % 16 == 0;
}

int launch_remap_tiled(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    RemapTiledParams p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid, warp_grid(out_pitch(d) / 16, f.out_h, d.channels))) return st;
    set_last_kernel("blur_remap_tiled_kernel");
    p.map = f.remap_map; p.W = d.width; p.Wo = f.out_w; p.Ho = f.out_h; p.border = f.warp_border; p.fill = (unsigned)f.warp_fill * 0x01010101u;
    p.stage_bytes = f.remap_stage_bytes;
    const size_t lds = remap_lds_bytes(f.remap_stage_bytes);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto CC) {
        // the default stage_bytes asks for 64 bytes more than 64 KiB of dynamic LDS: tell the runtime the kernel may (a CU has 160 KiB)
        if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void *>(blur_remap_tiled_kernel<CC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            (void)hipGetLastError();                    // the launch itself reports what the runtime refuses
        return do_launch(blur_remap_tiled_kernel<CC>, grid, dim3(TILE_THREADS), lds, d, p);
    });
}

int launch_remap_generic(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    set_last_kernel("blur_remap_generic_kernel");
    RemapGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    p.map = f.remap_map; p.W = d.width; p.Wo = f.out_w; p.mode = f.sample_mode; p.border = f.warp_border; p.fill = (unsigned)f.warp_fill;
    return do_launch(blur_remap_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

// Only whole images (launch_checks()); out_stride is measured against the REMAPPED image (dense_out()).  The map: not null,
// not the output, 4-byte aligned.
int launch_remap(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::REMAP, [&](const Filter &f) {
        return resize_ok(f.out_w, f.out_h, f.sample_mode, d.width, d.band_rows, d.channels) &&
               (f.warp_border == MI_BLUR_WARP_CLAMP || f.warp_border == MI_BLUR_WARP_CONSTANT) && f.warp_fill >= 0 && f.warp_fill <= 255 &&
               f.remap_stage_bytes >= 16 && f.remap_stage_bytes <= REMAP_STAGE_MAX && f.remap_map &&
               (const void *)f.remap_map != (const void *)d.out && (uintptr_t)f.remap_map % 4 == 0;
    });
    if (st != LAUNCH_GO) return st;
    return remap_tile_aligned(d) ? launch_remap_tiled(d) : launch_remap_generic(d);
}

}  // namespace mi_blur
