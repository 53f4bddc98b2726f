// sep_kernels.hip — gfx950 kernels of the separable integer blur of any radius up to 16 (mi_blur_enqueue_sep,
// include/mi_blur.h):
//   out[y][x][c] = ( sum_j wy[j] * sum_i wx[i] * in[clamp(y+j-ry)][clamp(x+i-rx)][c] ) >> (bx + by)
// Taps sum to 2^bx / 2^by <= 256, so a one-axis sum is <= 255 * 256 = 65280 (16 bits) and the full sum < 2^24: every
// order of evaluation gives the same bits, which licenses a vertical pass in packed 16-bit fields followed by a
// horizontal one in 32 bits.
//
// Tiled kernel (blur_sep_tiled_kernel<C, RB>): rows of whole 16-byte chunks, 16-byte aligned buffers and strides, 1-4
// channels.  One workgroup = one tile of TILE_TH output rows x ncols (<= 32) chunk columns:
//   * stage (TILE_TH + 2 ry) rows x (ncols + 2 HC) chunks in LDS (stage_tile, kernel_common.h), x-clamp included.  HC =
//     the halo chunks either side that the radius bucket RB needs (RB * C bytes);
//   * vertical pass: each thread takes one chunk column (halo chunks included) and SEP_RPG output rows, walks the
//     SEP_RPG + 2 ry staged rows once and adds every row into the outputs it belongs to — every dword split into its
//     even / odd bytes as two 16-bit fields, v_pk_mad_u16 with the row's tap (2 MACs per lane-op).  The sums replace the
//     staged bytes in LDS (16-bit, even / odd fields kept apart);
//   * horizontal pass: each thread takes one output chunk, reads the 2 HC + 1 chunks of sums around it and adds the
//     2 rx + 1 taps at byte offsets d * C (the field pairs are whole dwords or one v_alignbit of two) with v_dot2_u32_u16
//     against (w, 0) / (0, w); one shift, re-interleave, one 16-byte store.
//   Taps are kernel arguments (scalar loads), rx and ry runtime bounds; RB in {4, 8, 16} only sizes the registers of
//   the horizontal window.  4 channels x 3 buckets = 12 instantiations.
//
// Generic kernel (blur_sep_generic_kernel): one output byte per thread, any shape, runtime taps.  Correct everywhere,
// fast nowhere.
#include "kernel_common.h"

#include <algorithm>
#include <utility>

namespace mi_blur {

namespace {

constexpr int SEP_RPG = 8;          // output rows per thread in the vertical pass

constexpr int sep_halo_chunks(int C, int RB) { return (RB * C + 15) / 16; }

struct SepTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per band / output block
    int pitch, cpr;                   // bytes per row, 16-byte chunks per row
    int H, y0, y1;                    // band rows (clamp range), output rows [y0, y1)
    int ncols, nstrips, ntiles_y;
    int rx, ry, shift;
    unsigned nblocks;
    int xcd;                          // 1 = each XCD takes a contiguous run of tiles (halo rows stay in its L2)
    unsigned wx[2 * SEP_MAX_R + 1];   // centred horizontal taps
    unsigned wy2[2 * SEP_MAX_R + 1];  // centred vertical taps, the weight in both 16-bit halves
};

// Field pair at byte offset K from the PI-parity bytes of output dword I, out of the window of 16-bit sums: E[j] / O[j]
// hold the sums of window bytes 4j, 4j+2 / 4j+1, 4j+3, the window starting HC chunks left of the output chunk.
template <int HC, int K, int PI, int I, int N>
__device__ __forceinline__ uint32_t sep_tap(const uint32_t (&E)[N], const uint32_t (&O)[N])
{
    constexpr int q0 = 16 * HC + 4 * I + PI + K;
    static_assert(q0 >= 0 && q0 + 2 < 4 * N, "tap outside the window");
    constexpr int e0 = q0 >> 1, j = e0 >> 1;
    const uint32_t (&A)[N] = (q0 & 1) ? O : E;
    if constexpr ((e0 & 1) == 0) return A[j];
    else return __builtin_amdgcn_alignbit(A[j + 1], A[j], 16);
}

// One tap of the horizontal pass: the pixel d columns away (byte offset d * C), skipped beyond the runtime radius.
// v_dot2_u32_u16 against (w, 0) / (0, w) adds w times the low / high field of a field pair to a 32-bit sum.
template <int C, int HC, int D, int N>
__device__ __forceinline__ void sep_htap(const uint32_t (&E)[N], const uint32_t (&O)[N], const unsigned *wx, int rx,
                                         uint32_t (&lo)[2][4], uint32_t (&hi)[2][4])
{
    if (D < -rx || D > rx) return;                      // uniform
    const uint32_t w = wx[SEP_MAX_R + D];
    const u16x2 wl = pk16(w), wh = pk16(w << 16);
    auto mac = [&](uint32_t f, int PI, int I) {
        lo[PI][I] = __builtin_amdgcn_udot2(pk16(f), wl, lo[PI][I], false);
        hi[PI][I] = __builtin_amdgcn_udot2(pk16(f), wh, hi[PI][I], false);
    };
    mac(sep_tap<HC, D * C, 0, 0>(E, O), 0, 0); mac(sep_tap<HC, D * C, 1, 0>(E, O), 1, 0);
    mac(sep_tap<HC, D * C, 0, 1>(E, O), 0, 1); mac(sep_tap<HC, D * C, 1, 1>(E, O), 1, 1);
    mac(sep_tap<HC, D * C, 0, 2>(E, O), 0, 2); mac(sep_tap<HC, D * C, 1, 2>(E, O), 1, 2);
    mac(sep_tap<HC, D * C, 0, 3>(E, O), 0, 3); mac(sep_tap<HC, D * C, 1, 3>(E, O), 1, 3);
}
template <int C, int HC, int RB, int... Ds, int N>
__device__ __forceinline__ void sep_hpass(std::integer_sequence<int, Ds...>, const uint32_t (&E)[N], const uint32_t (&O)[N],
                                          const unsigned *wx, int rx, uint32_t (&lo)[2][4], uint32_t (&hi)[2][4])
{
    (sep_htap<C, HC, Ds - RB>(E, O, wx, rx, lo, hi), ...);
}

template <int C, int RB>
__global__ __launch_bounds__(TILE_THREADS) void blur_sep_tiled_kernel(const SepTiledParams p)
{
    constexpr int HC = sep_halo_chunks(C, RB);
    constexpr int NW = 4 * (2 * HC + 1);            // window dwords per parity
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x;
    const int ry = p.ry;
    const TileCoords tc = tile_coords<HC>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, p.y0, p.y1, ry);
    const int img = tc.img, ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc, ncw = tc.ncw;
    stage_tile<C, HC>(lds, p.in + (long long)img * p.in_stride, p.cpr, p.H, p.pitch, tc, ry, t);

    // ---- vertical pass: thread = (chunk column cc, row group g); every staged row read once
    const int ngrp = (rows_out + SEP_RPG - 1) / SEP_RPG;
    const bool vact = t < ncw * ngrp;
    const int g = t / ncw, vcc = t - g * ncw;
    uint32_t acc[SEP_RPG][8];
#pragma unroll
    for (int m = 0; m < SEP_RPG; m++)
#pragma unroll
        for (int k = 0; k < 8; k++) acc[m][k] = 0u;
    if (vact) {
        const uint8_t *lp = lds + ((size_t)g * SEP_RPG * ncw + vcc) * 16u;
        const int span = SEP_RPG + 2 * ry;
        for (int e = 0; e < span; e++) {                // staged rows g*RPG + e; rows past the tile feed unstored outputs only
            const uint4 x = *reinterpret_cast<const uint4 *>(lp + (size_t)e * ncw * 16u);
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
            uint32_t f[8];
#pragma unroll
            for (int k = 0; k < 4; k++) { f[k] = xs[k] & 0x00ff00ffu; f[4 + k] = (xs[k] >> 8) & 0x00ff00ffu; }
#pragma unroll
            for (int m = 0; m < SEP_RPG; m++) {
                const int j = e - m;                    // tap index 0..2ry of this row for output row g*RPG + m (uniform)
                if (j >= 0 && j <= 2 * ry) {
                    const u16x2 w = pk16(p.wy2[SEP_MAX_R - ry + j]);
#pragma unroll
                    for (int k = 0; k < 8; k++) acc[m][k] = pk32(pk16(f[k]) * w + pk16(acc[m][k]));
                }
            }
        }
    }
    __syncthreads();                                    // every staged byte read: the sums take the tile's place
    if (vact) {
#pragma unroll
        for (int m = 0; m < SEP_RPG; m++) {
            uint4 *vp = reinterpret_cast<uint4 *>(lds + ((size_t)(g * SEP_RPG + m) * ncw + vcc) * 32u);
            vp[0] = make_uint4(acc[m][0], acc[m][1], acc[m][2], acc[m][3]);
            vp[1] = make_uint4(acc[m][4], acc[m][5], acc[m][6], acc[m][7]);
        }
    }
    __syncthreads();

    // ---- horizontal pass: thread = one output chunk; 32-bit sums, one shift
    const int rx = p.rx, shift = p.shift;
    uint8_t *out_img = p.out + (long long)img * p.out_stride;
    for (int i = t; i < rows_out * nc; i += TILE_THREADS) {
        const int k = i / nc, col = i - k * nc;
        uint32_t E[NW], O[NW];
        const uint4 *vp = reinterpret_cast<const uint4 *>(lds + ((size_t)k * ncw + col) * 32u);
#pragma unroll
        for (int w = 0; w < 2 * HC + 1; w++) {
            const uint4 a = vp[2 * w], b = vp[2 * w + 1];
            E[4 * w] = a.x; E[4 * w + 1] = a.y; E[4 * w + 2] = a.z; E[4 * w + 3] = a.w;
            O[4 * w] = b.x; O[4 * w + 1] = b.y; O[4 * w + 2] = b.z; O[4 * w + 3] = b.w;
        }
        uint32_t lo[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, hi[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        sep_hpass<C, HC, RB>(std::make_integer_sequence<int, 2 * RB + 1>{}, E, O, p.wx, rx, lo, hi);
        uint32_t o[4];
#pragma unroll
        for (int I = 0; I < 4; I++)                     // bytes 4I, 4I+1, 4I+2, 4I+3 = even lo, odd lo, even hi, odd hi
            o[I] = (lo[0][I] >> shift) | ((lo[1][I] >> shift) << 8) | ((hi[0][I] >> shift) << 16) | ((hi[1][I] >> shift) << 24);
        uint8_t *op = out_img + (size_t)(ty0 - p.y0 + k) * (size_t)p.pitch + (size_t)(x0c + col) * 16u;
        u32x4 v; v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
        *reinterpret_cast<u32x4 *>(op) = v;
    }
}

struct SepGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per band (rows * pitch)
    int width, channels, pitch, H, y0;
    int rx, ry, shift;
    unsigned wx[2 * SEP_MAX_R + 1], wy[2 * SEP_MAX_R + 1];
};

__global__ __launch_bounds__(256) void blur_sep_generic_kernel(const SepGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.pitch, p.channels, p.y0, p.in, p.in_stride);
        unsigned sum = 0;
        for (int j = -p.ry; j <= p.ry; j++) {
            const int ny = min(max(q.y + j, 0), p.H - 1);
            const uint8_t *rowp = q.src + (size_t)ny * (size_t)p.pitch + q.c;
            unsigned h = 0;
            for (int i = -p.rx; i <= p.rx; i++) {
                const int nx = min(max(q.x + i, 0), p.width - 1);
                h += (unsigned)rowp[(size_t)nx * (size_t)p.channels] * p.wx[SEP_MAX_R + i];
            }
            sum += h * p.wy[SEP_MAX_R + j];
        }
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)(sum >> p.shift);
    }
}

int launch_sep_tiled(const LaunchDesc &d)
{
    set_last_kernel("blur_sep_tiled_kernel");
    const SepTaps &k = d.filter->taps;
    SepTiledParams p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid)) return st;
    p.rx = k.rx; p.ry = k.ry; p.shift = k.shift;
    for (int i = 0; i <= 2 * SEP_MAX_R; i++) { p.wx[i] = k.wx[i]; p.wy2[i] = k.wy[i] | (k.wy[i] << 16); }
    const dim3 block(TILE_THREADS);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto C) {
        return dispatch<4, 8, 16>(k.rx <= 4 ? 4 : k.rx <= 8 ? 8 : 16, [&](auto RB) {
            const int ncw = p.ncols + 2 * sep_halo_chunks(C, RB);      // sums: TILE_TH rows x ncw chunks x 32 B >= the staged bytes
            return do_launch(blur_sep_tiled_kernel<C, RB>, grid, block, (size_t)TILE_TH * ncw * 32u, d, p);
        });
    });
}

int launch_sep_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_sep_generic_kernel");
    const SepTaps &k = d.filter->taps;
    SepGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    p.rx = k.rx; p.ry = k.ry; p.shift = k.shift;
    for (int i = 0; i <= 2 * SEP_MAX_R; i++) { p.wx[i] = k.wx[i]; p.wy[i] = k.wy[i]; }
    return do_launch(blur_sep_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

int launch_sep(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::SEP, [](const Filter &f) {
        const SepTaps &k = f.taps;
        return k.rx >= 0 && k.rx <= SEP_MAX_R && k.ry >= 0 && k.ry <= SEP_MAX_R && k.shift >= 0 && k.shift <= 16;
    });
    if (st != LAUNCH_GO) return st;
    return tile_aligned(d) ? launch_sep_tiled(d) : launch_sep_generic(d);
}

}  // namespace mi_blur
