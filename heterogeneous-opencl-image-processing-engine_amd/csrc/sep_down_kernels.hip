// sep_down_kernels.hip — gfx950 kernels of the decimating separable filter (mi_blur_enqueue_sep_down, include/mi_blur.h):
//   out[Y][X][c] = F(in)[oy + Y*sy][ox + X*sx][c],   F = the separable filter of sep_kernels.hip on the whole image
// and only the kept outputs are computed.  A one-axis sum is <= 255 * 256 = 65280 (16 bits) and the full sum < 2^24, so
// both pass orders give the same bits.
//
// Tiled kernel (blur_sep_down_tiled_kernel<C, RB>): sx = sy = 2 (either phase on either axis), 1-4 channels, input rows of
// whole 32-byte pairs of chunks (so output rows are whole 16-byte chunks), 16-byte aligned buffers and strides.  One
// workgroup = one tile of TILE_TH INPUT rows x ncols (<= 32, even; 6, 12, 18 or 24 for C = 3) input chunk columns, which
// holds TILE_TH / 2 kept rows x ncols / 2 output chunks:
//   * stage (TILE_TH + 2 ry) rows x (ncols + 2 HC) chunks in LDS with the shared stager (stage_tile, kernel_common.h),
//     tile rows counted in input coordinates, x-clamp included; the host cuts the INPUT image into these tiles with the
//     shared fill_tiles, in strips of whole groups;
//   * VERTICAL PASS FIRST, over the kept rows only and all staged columns: it is the pass that can work in packed
//     16-bit fields (v_pk_mad_u16, two MACs per lane-op, as in blur_sep_tiled_kernel) on whole chunks exactly as they lie
//     in LDS, and skipping rows costs it nothing, so it halves.  Horizontal first would have to gather bytes 2 pixels
//     apart out of the interleaved chunks for every staged row before it could multiply anything.  Each thread takes
//     one chunk column and DOWN_RPG kept rows.  The 16-bit sums replace the staged bytes in LDS, one u16 per input byte
//     in byte order, one pad dword after every 64 bytes of sums;
//   * horizontal pass at the kept columns only, one output chunk per lane.  Output chunks come in GROUPS of G (G = 1;
//     G = 3 for C = 3, where the pixel pattern repeats every 48 output bytes): 16 G / C output pixels that come from the
//     2 G input chunks below them.  A wave-iteration takes 64 groups and the same chunk u of each (u is scalar: three
//     unrolled bodies for C = 3, each wave running one), so 16 kept rows x 4 groups fill a wave three times over and
//     three of the four waves work side by side.  Output byte (X, c) of the group reads the sum at input byte
//     (2 X + D) * C + c for every tap D: relative to the group a compile-time position for every (C, output byte, D), so
//     the gather is one ds_read_u16 at an immediate offset and one v_mad_u32_u24 per tap and byte — no address
//     arithmetic, no runtime-indexed registers.  The phase ox does not enter the kernel: the host hands it the taps
//     shifted by ox (wx[D] = weight of input pixel 2 X + D, D in [ox - rx, ox + rx]).  Lanes are consecutive groups:
//     64 G bytes of sums apart, which the pad dwords turn into 17 G dwords, odd, so a wave's reads hit distinct banks;
//   * one shift, one 16-byte store per output chunk.
//   Taps are kernel arguments, rx and ry runtime bounds; RB in {4, 8, 16} sizes the halo and the unrolled tap loop.
//   4 channels x 3 buckets = 12 instantiations.
//
// Generic kernel (blur_sep_down_generic_kernel): one output byte per thread, any shape, any strides, runtime taps.
#include "kernel_common.h"

#include <algorithm>
#include <utility>

namespace mi_blur {

namespace {

constexpr int DOWN_RPG = 4;                        // kept rows per thread in the vertical pass
constexpr int DOWN_TH = TILE_TH / 2;               // kept rows per tile at most

constexpr int down_halo_chunks(int C, int RB) { return (RB * C + 15) / 16; }
constexpr int down_group(int C) { return C == 3 ? 3 : 1; }    // output chunks per thread of the horizontal pass
// Byte offset in a row of sums of the sum of the input byte at tile byte q: 2 bytes each, a pad dword every 64 bytes.
constexpr int down_sum_at(int q) { return 2 * q + ((2 * q) >> 6) * 4; }
// Bytes of one row of sums for ncw staged chunk columns.
__host__ __device__ constexpr int down_sum_row(int ncw) { return ncw * 32 + (ncw / 2 + 1) * 4; }

struct SepDownTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per input image / output image
    int pitch, cpr;                   // input: bytes per row, 16-byte chunks per row
    int H, y0, y1;                    // input rows; y0 = 0, y1 = H
    int ncols, nstrips, ntiles_y;
    int rx, ry, shift;
    unsigned nblocks;
    int xcd;
    int opitch, oy;                   // output bytes per row; kept rows are oy + 2 Y
    int dlo, dhi;                     // horizontal taps D in [dlo, dhi] = [ox - rx, ox + rx]
    unsigned wx[2 * SEP_MAX_R + 2];   // wx[SEP_MAX_R + D] = weight of input pixel 2 X + D for output pixel X
    unsigned wy2[2 * SEP_MAX_R + 1];  // centred vertical taps, the weight in both 16-bit halves
};

// One tap of the horizontal pass: adds w * (sum at input pixel 2 X + D) to the 16 bytes of output chunk U of the group.
template <int C, int HC, int U, int D>
__device__ __forceinline__ void down_htap(const uint8_t *grp, const unsigned *wx, int dlo, int dhi, uint32_t (&acc)[16])
{
    if (D < dlo || D > dhi) return;                     // uniform
    const uint32_t w = wx[SEP_MAX_R + D];
#pragma unroll
    for (int bb = 0; bb < 16; bb++) {
        const int b = 16 * U + bb, X = b / C, c = b - X * C;   // constants after unrolling
        const int q = HC * 16 + (2 * X + D) * C + c;    // tile byte relative to the group's first staged chunk column - HC
        const uint32_t s = *reinterpret_cast<const uint16_t *>(grp + down_sum_at(q));
        acc[bb] += __umul24(s, w);                      // s <= 65280, w <= 256: v_mad_u32_u24
    }
}
template <int C, int HC, int RB, int U, int... Ds>
__device__ __forceinline__ void down_hpass(std::integer_sequence<int, Ds...>, const uint8_t *grp, const unsigned *wx, int dlo, int dhi,
                                           uint32_t (&acc)[16])
{
    (down_htap<C, HC, U, Ds - RB>(grp, wx, dlo, dhi, acc), ...);
}
// Output chunk U of the group whose sums start at grp: every tap, one shift, one 16-byte store at op + 16 U.
template <int C, int HC, int RB, int U>
__device__ __forceinline__ void down_chunk(const uint8_t *grp, const unsigned *wx, int dlo, int dhi, int shift, uint8_t *op)
{
    uint32_t a[16];
#pragma unroll
    for (int b = 0; b < 16; b++) a[b] = 0u;
    down_hpass<C, HC, RB, U>(std::make_integer_sequence<int, 2 * RB + 2>{}, grp, wx, dlo, dhi, a);
    u32x4 v;
    v.x = (a[0] >> shift) | ((a[1] >> shift) << 8) | ((a[2] >> shift) << 16) | ((a[3] >> shift) << 24);
    v.y = (a[4] >> shift) | ((a[5] >> shift) << 8) | ((a[6] >> shift) << 16) | ((a[7] >> shift) << 24);
    v.z = (a[8] >> shift) | ((a[9] >> shift) << 8) | ((a[10] >> shift) << 16) | ((a[11] >> shift) << 24);
    v.w = (a[12] >> shift) | ((a[13] >> shift) << 8) | ((a[14] >> shift) << 16) | ((a[15] >> shift) << 24);
    *reinterpret_cast<u32x4 *>(op + 16 * U) = v;
}

template <int C, int RB>
__global__ __launch_bounds__(TILE_THREADS) void blur_sep_down_tiled_kernel(const SepDownTiledParams p)
{
    constexpr int HC = down_halo_chunks(C, RB);
    constexpr int G = down_group(C);
    static_assert(HC * 16 - RB * C >= 0, "left halo too small");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x;
    const int ry = p.ry;
    const TileCoords tc = tile_coords<HC>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, p.y0, p.y1, ry);
    const int img = tc.img, ty0 = tc.ty0, x0c = tc.x0c, nc = tc.nc, ncw = tc.ncw;
    stage_tile<C, HC>(lds, p.in + (long long)img * p.in_stride, p.cpr, p.H, p.pitch, tc, ry, t);

    // kept rows of the tile: input rows ty0 + oy + 2 k (ty0 is a multiple of TILE_TH, which is even), k < nk
    const int oy = p.oy;
    const int nk = tc.rows_out > oy ? (tc.rows_out - oy + 1) >> 1 : 0;

    // ---- vertical pass: thread = (chunk column vcc, group g of DOWN_RPG kept rows); staged row oy + 2 k + j feeds kept row k with tap j
    const int ngrp = (nk + DOWN_RPG - 1) / DOWN_RPG;
    const bool vact = t < ncw * ngrp;
    const int g = t / ncw, vcc = t - g * ncw;
    uint32_t acc[DOWN_RPG][8];
#pragma unroll
    for (int m = 0; m < DOWN_RPG; m++)
#pragma unroll
        for (int k = 0; k < 8; k++) acc[m][k] = 0u;
    if (vact) {
        const uint8_t *lp = lds + ((size_t)(oy + 2 * DOWN_RPG * g) * ncw + vcc) * 16u;
        // the staged rows under the group's kept rows, cut at the last staged row of a short tile (what lies beyond feeds unstored outputs only)
        const int span = min(2 * (DOWN_RPG - 1) + 1 + 2 * ry, tc.nrows - (oy + 2 * DOWN_RPG * g));
        for (int e = 0; e < span; e++) {
            const uint4 x = *reinterpret_cast<const uint4 *>(lp + (size_t)e * ncw * 16u);
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
            uint32_t f[8];
#pragma unroll
            for (int k = 0; k < 4; k++) { f[k] = xs[k] & 0x00ff00ffu; f[4 + k] = (xs[k] >> 8) & 0x00ff00ffu; }
#pragma unroll
            for (int m = 0; m < DOWN_RPG; m++) {
                const int j = e - 2 * m;                // tap index 0..2ry of this staged row for kept row DOWN_RPG g + m (uniform)
                if (j >= 0 && j <= 2 * ry) {
                    const u16x2 w = pk16(p.wy2[SEP_MAX_R - ry + j]);
#pragma unroll
                    for (int k = 0; k < 8; k++) acc[m][k] = pk32(pk16(f[k]) * w + pk16(acc[m][k]));
                }
            }
        }
    }
    __syncthreads();                                    // every staged byte read: the sums take the tile's place
    const int rowb = down_sum_row(ncw);
    if (vact) {
#pragma unroll
        for (int m = 0; m < DOWN_RPG; m++) {
            const int k = DOWN_RPG * g + m;
            if (k < nk) {
                // fields (bytes 4i, 4i+2) / (4i+1, 4i+3) -> byte order: (4i, 4i+1), (4i+2, 4i+3)
                uint32_t *vp = reinterpret_cast<uint32_t *>(lds + (size_t)k * rowb + vcc * 32 + (vcc >> 1) * 4);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    vp[2 * i] = __builtin_amdgcn_perm(acc[m][4 + i], acc[m][i], 0x05040100u);
                    vp[2 * i + 1] = __builtin_amdgcn_perm(acc[m][4 + i], acc[m][i], 0x07060302u);
                }
            }
        }
    }
    __syncthreads();

    // ---- horizontal pass: lane = one output chunk; 32-bit sums, one shift.  A wave-iteration ("slot") takes 64 groups of
    // one kept-row-major run and ONE chunk u of each, so the pattern is uniform in the wave and lanes are whole groups apart
    const int ng = nc / (2 * G), nitems = nk * ng, runs = (nitems + 63) >> 6;
    const int shift = p.shift, dlo = p.dlo, dhi = p.dhi;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    uint8_t *out_img = p.out + (long long)img * p.out_stride;
    for (int s = wave; s < G * runs; s += TILE_THREADS / 64) {
        const int run = s / G, u = s - run * G;         // scalar
        const int i = run * 64 + lane;
        if (i >= nitems) continue;
        const int k = i / ng, gi = i - k * ng;
        const uint8_t *grp = lds + (size_t)k * rowb + gi * (68 * G);    // 2 G chunks of sums and their G pad dwords per group
        uint8_t *op = out_img + (size_t)((ty0 >> 1) + k) * (size_t)p.opitch + (size_t)((x0c >> 1) + gi * G) * 16u;
        if constexpr (G == 1) {
            down_chunk<C, HC, RB, 0>(grp, p.wx, dlo, dhi, shift, op);
        } else {
            if (u == 0) down_chunk<C, HC, RB, 0>(grp, p.wx, dlo, dhi, shift, op);
            else if (u == 1) down_chunk<C, HC, RB, 1>(grp, p.wx, dlo, dhi, shift, op);
            else down_chunk<C, HC, RB, 2>(grp, p.wx, dlo, dhi, shift, op);
        }
    }
}

struct SepDownGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per image (Ho * opitch)
    int width, channels, pitch, opitch, H;
    int sx, sy, ox, oy;
    int rx, ry, shift;
    unsigned wx[2 * SEP_MAX_R + 1], wy[2 * SEP_MAX_R + 1];
};

__global__ __launch_bounds__(256) void blur_sep_down_generic_kernel(const SepDownGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.opitch, p.channels, 0, p.in, p.in_stride);   // q.y, q.x: the OUTPUT pixel
        const int y = p.oy + q.y * p.sy, x = p.ox + q.x * p.sx;
        unsigned sum = 0;
        for (int j = -p.ry; j <= p.ry; j++) {
            const int ny = min(max(y + j, 0), p.H - 1);
            const uint8_t *rowp = q.src + (size_t)ny * (size_t)p.pitch + q.c;
            unsigned h = 0;
            for (int i = -p.rx; i <= p.rx; i++) {
                const int nx = min(max(x + i, 0), p.width - 1);
                h += (unsigned)rowp[(size_t)nx * (size_t)p.channels] * p.wx[SEP_MAX_R + i];
            }
            sum += h * p.wy[SEP_MAX_R + j];
        }
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)(sum >> p.shift);
    }
}

// tile_aligned (kernel_common.h), stride 2 both ways, input rows of whole 32-byte chunk pairs.
bool down_tile_aligned(const LaunchDesc &d)
{
    const Filter &f = *d.filter;
    return tile_aligned(d) && f.down_sx == 2 && f.down_sy == 2 && (long long)d.width * d.channels % 32 == 0;
}

int launch_sep_down_tiled(const LaunchDesc &d)
{
    set_last_kernel("blur_sep_down_tiled_kernel");
    const Filter &f = *d.filter;
    const SepTaps &k = f.taps;
    SepDownTiledParams p{};
    // tiles of the INPUT image; strips of whole groups: 2 G input chunks each, at most TILE_NCOLS chunks per strip
    // 3 channels: 4 groups = 24 chunks per strip, so that 16 kept rows x 4 groups fill the 64 lanes of a wave-iteration of the horizontal pass
    const int unit = 2 * down_group(d.channels), max_units = d.channels == 3 ? 4 : TILE_NCOLS / unit;
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid, tile_grid(d.width * d.channels / 16, d.band_rows, unit, max_units))) return st;
    p.y1 = d.band_rows; p.oy = f.down_oy;             // y0 = 0: the whole image
    p.rx = k.rx; p.ry = k.ry; p.shift = k.shift;
    p.dlo = f.down_ox - k.rx; p.dhi = f.down_ox + k.rx;
    for (int D = p.dlo; D <= p.dhi; D++) p.wx[SEP_MAX_R + D] = k.wx[SEP_MAX_R + D - f.down_ox];
    for (int i = 0; i <= 2 * SEP_MAX_R; i++) p.wy2[i] = k.wy[i] | (k.wy[i] << 16);
    const dim3 block(TILE_THREADS);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto C) {
        return dispatch<4, 8, 16>(k.rx <= 4 ? 4 : k.rx <= 8 ? 8 : 16, [&](auto RB) {
            const int ncw = p.ncols + 2 * down_halo_chunks(C, RB);
            const size_t staged = (size_t)(TILE_TH + 2 * k.ry) * ncw * 16u, sums = (size_t)DOWN_TH * down_sum_row(ncw);
            return do_launch(blur_sep_down_tiled_kernel<C, RB>, grid, block, std::max(staged, sums), d, p);
        });
    });
}

int launch_sep_down_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_sep_down_generic_kernel");
    const Filter &f = *d.filter;
    const SepTaps &k = f.taps;
    SepDownGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    p.width = d.width;
    p.sx = f.down_sx; p.sy = f.down_sy; p.ox = f.down_ox; p.oy = f.down_oy;
    p.rx = k.rx; p.ry = k.ry; p.shift = k.shift;
    for (int i = 0; i <= 2 * SEP_MAX_R; i++) { p.wx[i] = k.wx[i]; p.wy[i] = k.wy[i]; }
    return do_launch(blur_sep_down_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

// A band's phase would depend on where it starts, so only whole images (launch_checks()); out_stride is measured against
// the DECIMATED image (dense_out()).
int launch_sep_down(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::SEP_DOWN, [&](const Filter &f) {
        const SepTaps &k = f.taps;
        const mi_blur_decimation dec{f.down_sx, f.down_sy, f.down_ox, f.down_oy};
        return k.rx >= 0 && k.rx <= SEP_MAX_R && k.ry >= 0 && k.ry <= SEP_MAX_R && k.shift >= 0 && k.shift <= 16 &&
               down_ok(&dec, d.width, d.band_rows);
    });
    if (st != LAUNCH_GO) return st;
    return down_tile_aligned(d) ? launch_sep_down_tiled(d) : launch_sep_down_generic(d);
}

}  // namespace mi_blur
