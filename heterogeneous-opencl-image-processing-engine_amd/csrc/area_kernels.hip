// area_kernels.hip — gfx950 kernels of the area resize (mi_blur_enqueue_area, include/mi_blur.h): the exact box average
// at any output size, reductions up to MI_BLUR_AREA_MAX_RATIO per axis.  Every tap and weight comes from area_axis() and
// the one rounding from area_round() (filter.h), the functions the CPU device and mi_blur_area_coord use too.
//
// Tiled kernel (blur_area_tiled_kernel<C>): 1-4 channels, Wo <= W and Ho <= H, input and output rows of whole 16-byte
// chunks, 16-byte aligned buffers and strides.  A reduction costs what reading its input costs, so nothing is staged and
// every input byte is loaded once, as one lane's 16 bytes of a coalesced row read.  One workgroup = one tile of AREA_TH
// OUTPUT rows x a strip of OUTPUT chunks (whole pixel units, warp_unit()); the host cuts the strips so that the input
// chunks under one (the span, area_stage_chunks()) number at most AREA_WAVE_SPAN where a unit allows it, and never more
// than AREA_MAX_SPAN, and so that the last 64-dword step of a strip's output row is at least half full (area_tiles()).
// The 256 threads are 256 / span row groups of span = 64 | 128 | 256 threads; a group owns
// consecutive output rows, its thread `col` input chunk column col of the span.  Geometry and LDS positions: filter.h
// ("blur_area_tiled_kernel"), which sizes the LDS on the host from the same functions.
//   * the first threads compute the strip's x table with the exact integer divisions of area_axis: per output byte of a
//     tile row the span byte of its first tap, the number of taps and the two partial weights;
//   * vertical pass, per output row of a group: the input rows i_lo..i_hi top to bottom, up to four loads in flight, each
//     byte times the row's weight (w_lo, Ho or w_hi: v_mad_u32_u24) into 16 dword sums in registers (<= 255 H < 2^23).  A
//     boundary row that feeds two output rows of the group is kept in registers, not loaded again;
//   * hand-over: the sums go to the group's V row in LDS, one dword per input byte;
//   * horizontal pass: one output dword per thread and step.  Per byte the first and last tap weighted, the taps between
//     them (stride C dwords in LDS) summed and multiplied once by Wo, in 64 bits; area_round(); one dword store, a wave's
//     stores contiguous.
//   No scratch, no run-time register indexing.  4 instantiations.
//
// Generic kernel (blur_area_generic_kernel): one output byte per thread, any shape, ratio and alignment, enlargements
// included: the loop over the taps of area_axis on both axes, the statement of the definition.
#include "kernel_common.h"

namespace mi_blur {

namespace {

struct AreaTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per input image / output image
    int W, H, Wo, Ho;
    int pitch, opitch;                // bytes per input row / output row
    int cpr;                          // OUTPUT 16-byte chunks per row
    int ncols, nstrips, ntiles_y;
    unsigned nblocks;
    int xcd;
    int span_log2;                    // threads of a row group: 64 | 128 | 256, as a shift
    int xtab_bytes, vrow;             // LDS: bytes of the x table, dwords of one group's V row
    double rden;                      // area_rden(W, H)
};

// sum[4 * q + e] += w * byte e of dword q of v, for w < 2^24.
__device__ __forceinline__ void area_accumulate(uint32_t (&sum)[16], const uint4 &v, uint32_t w)
{
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        sum[4 * q] += __umul24(d[q] & 0xffu, w);
        sum[4 * q + 1] += __umul24((d[q] >> 8) & 0xffu, w);
        sum[4 * q + 2] += __umul24((d[q] >> 16) & 0xffu, w);
        sum[4 * q + 3] += __umul24(d[q] >> 24, w);
    }
}

template <int C>
__global__ __launch_bounds__(AREA_THREADS) void blur_area_tiled_kernel(const AreaTiledParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint32_t *xtab = reinterpret_cast<uint32_t *>(lds);
    uint32_t *vbuf = reinterpret_cast<uint32_t *>(lds + p.xtab_bytes);
    const int t = threadIdx.x;
    // blockIdx -> tile: strips fastest, then tile rows, then images (fill_tiles(), kernel_common.h, with AREA_TH rows)
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const int strip = (int)(L % (unsigned)p.nstrips);
    const unsigned t2 = L / (unsigned)p.nstrips;
    const int ty0 = (int)(t2 % (unsigned)p.ntiles_y) * AREA_TH, img = (int)(t2 / (unsigned)p.ntiles_y);
    const int rows_out = min(AREA_TH, p.Ho - ty0);
    const int x0c = strip * p.ncols, nc = min(p.ncols, p.cpr - x0c);
    const Span sc = area_stage_chunks(p.W, p.Wo, C, x0c, nc);       // the strip's input chunks (uniform)
    const int sc0 = sc.lo, nsc = sc.n();

    // row groups
    const int span = 1 << p.span_log2, g = t >> p.span_log2, col = t & (span - 1);
    const int rows_per_group = AREA_TH >> (8 - p.span_log2);        // AREA_TH / (256 / span)
    uint32_t *vrow = vbuf + (size_t)g * p.vrow;

    // ---- x table: two dwords per output byte of a tile row
    for (int ob = t; ob < nc * 16; ob += AREA_THREADS) {
        const int gb = x0c * 16 + ob, X = gb / C, c = gb - X * C;
        const AreaAxis ax = area_axis(p.W, p.Wo, X);
        xtab[2 * ob] = area_x_entry0(ax, C, c, sc0);
        xtab[2 * ob + 1] = area_x_entry1(ax);
    }

    const uint8_t *in_col = p.in + (long long)img * p.in_stride + (unsigned)(sc0 + (col < nsc ? col : 0)) * 16u;
    uint8_t *out_img = p.out + (long long)img * p.out_stride;
    const int64_t D = (int64_t)p.W * p.H;
    uint4 kept = make_uint4(0, 0, 0, 0);
    int kept_row = -1;

    for (int k = 0; k < rows_per_group; k++) {
        const int Y = ty0 + g * rows_per_group + k;
        const bool active = Y < ty0 + rows_out;                     // uniform over the group
        if (active && col < nsc) {
            // ---- vertical pass: the weighted sum of input rows i_lo..i_hi of this thread's chunk column
            const AreaAxis ay = area_axis(p.H, p.Ho, Y);
            uint32_t sum[16];
#pragma unroll
            for (int e = 0; e < 16; e++) sum[e] = 0;
            int j = ay.i_lo;
            if (j == kept_row) { area_accumulate(sum, kept, area_weight(ay, p.Ho, j)); j++; }
            auto row = [&](int r) { return *reinterpret_cast<const uint4 *>(in_col + (unsigned)r * (unsigned)p.pitch); };
            for (; j + 3 <= ay.i_hi; j += 4) {
                const uint4 a = row(j), b = row(j + 1), c = row(j + 2), d = row(j + 3);
                area_accumulate(sum, a, area_weight(ay, p.Ho, j));
                area_accumulate(sum, b, area_weight(ay, p.Ho, j + 1));
                area_accumulate(sum, c, area_weight(ay, p.Ho, j + 2));
                area_accumulate(sum, d, area_weight(ay, p.Ho, j + 3));
                kept = d;
            }
            if (j + 1 <= ay.i_hi) {
                const uint4 a = row(j), b = row(j + 1);
                area_accumulate(sum, a, area_weight(ay, p.Ho, j));
                area_accumulate(sum, b, area_weight(ay, p.Ho, j + 1));
                kept = b;
                j += 2;
            }
            if (j <= ay.i_hi) {
                const uint4 a = row(j);
                area_accumulate(sum, a, area_weight(ay, p.Ho, j));
                kept = a;
            }
            kept_row = ay.i_hi;                                     // `kept` holds it: loaded above, or the row kept before (i_hi == i_lo)
            // ---- hand-over: one dword per input byte of the span
#pragma unroll
            for (int e = 0; e < 16; e++) vrow[area_v_pos(col * 16 + e)] = sum[e];
        }
        __syncthreads();
        if (active) {
            // ---- horizontal pass: one output dword per thread and step
            for (int od = col; od < nc * 4; od += span) {
                const uint4 e01 = *reinterpret_cast<const uint4 *>(xtab + od * 8), e23 = *reinterpret_cast<const uint4 *>(xtab + od * 8 + 4);
                const uint32_t ent[8] = {e01.x, e01.y, e01.z, e01.w, e23.x, e23.y, e23.z, e23.w};
                uint32_t word = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int q0 = (int)(ent[2 * e] & 0xffffu), n = (int)(ent[2 * e] >> 16);
                    const uint32_t w_lo = ent[2 * e + 1] & 0xffffu, w_hi = ent[2 * e + 1] >> 16;
                    uint64_t S = (uint64_t)w_lo * vrow[area_v_pos(q0)];
                    uint32_t mid = 0;                               // at most 63 taps of less than 2^23
                    for (int i = 1; i < n - 1; i++) mid += vrow[area_v_pos(q0 + i * C)];
                    S += (uint64_t)(uint32_t)p.Wo * mid;
                    if (n > 1) S += (uint64_t)w_hi * vrow[area_v_pos(q0 + (n - 1) * C)];
                    word |= area_round(S, D, p.rden) << (8 * e);
                }
                *reinterpret_cast<uint32_t *>(out_img + ((unsigned)Y * (unsigned)p.opitch + (unsigned)x0c * 16u + (unsigned)od * 4u)) = word;
            }
        }
        __syncthreads();                                            // the next row's sums overwrite the V rows
    }
}

struct AreaGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per image (Ho * opitch)
    int W, H, Wo, Ho, channels, pitch, opitch;
    double rden;
};

__global__ __launch_bounds__(256) void blur_area_generic_kernel(const AreaGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    const int64_t D = (int64_t)p.W * p.H;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.opitch, p.channels, 0, p.in, p.in_stride);   // q.y, q.x: the OUTPUT pixel
        const AreaAxis ax = area_axis(p.W, p.Wo, q.x), ay = area_axis(p.H, p.Ho, q.y);
        uint64_t S = 0;
        for (int j = ay.i_lo; j <= ay.i_hi; j++) {
            const uint8_t *r = q.src + (size_t)j * (size_t)p.pitch + q.c;
            uint32_t h = 0;                                         // at most 255 W < 2^23
            for (int i = ax.i_lo; i <= ax.i_hi; i++) h += area_weight(ax, p.Wo, i) * r[(size_t)i * (size_t)p.channels];
            S += (uint64_t)area_weight(ay, p.Ho, j) * h;
        }
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)area_round(S, D, p.rden);
    }
}

// tile_aligned (kernel_common.h) with output rows of whole chunks too and no enlargement on either axis.
bool area_tile_aligned(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    return tile_aligned(d) && out_pitch(d) % 16 == 0 && f.out_w <= d.width && f.out_h <= d.band_rows;
}

int launch_area_tiled(const LaunchDesc &d, const AreaTiles &t)
{
    AreaTiledParams p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid, t.g)) return st;
    set_last_kernel("blur_area_tiled_kernel");
    p.W = d.width; p.Wo = d.filter->out_w; p.Ho = d.filter->out_h;
    p.span_log2 = t.span == 64 ? 6 : t.span == 128 ? 7 : 8;
    p.xtab_bytes = area_xtab_bytes(t);
    p.vrow = area_v_row(t.max_nsc);
    p.rden = area_rden(d.width, d.band_rows);
    const size_t lds = area_lds_bytes(t);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto CC) { return do_launch(blur_area_tiled_kernel<CC>, grid, dim3(AREA_THREADS), lds, d, p); });
}

int launch_area_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_area_generic_kernel");
    AreaGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    p.W = d.width; p.Wo = d.filter->out_w; p.Ho = d.filter->out_h;
    p.rden = area_rden(d.width, d.band_rows);
    return do_launch(blur_area_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

// Only whole images (launch_checks()); out_stride is measured against the RESIZED image (dense_out()).
int launch_area(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::AREA, [&](const Filter &f) { return area_ok(f.out_w, f.out_h, d.width, d.band_rows, d.channels); });
    if (st != LAUNCH_GO) return st;
    if (area_tile_aligned(d)) {
        const AreaTiles t = area_tiles(d.width, d.filter->out_w, d.filter->out_h, d.channels);
        if (area_tiles_fit(t)) return launch_area_tiled(d, t);
    }
    return launch_area_generic(d);
}

}  // namespace mi_blur
