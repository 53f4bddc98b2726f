// conv_kernels.hip — gfx950 kernels of the 2-D convolution with signed integer taps (mi_blur_enqueue_conv, include/mi_blur.h):
// per channel, over the (2 rx + 1) x (2 ry + 1) window with clamp-to-edge,
//   acc = sum K[j][i] * v,  (MAG: acc2 = sum K2[j][i] * v),  out = clamp((acc | |acc| | |acc| + |acc2|) + bias >> shift, 0, 255)
// Correlation (no flip).  filter_conv bounds sum |K| by 65535, so |acc| < 2^24: 24-bit multiplies and 32-bit signed sums are
// exact and the bytes are those of the CPU device.  Not separable: every tap is multiplied for every output byte, but a
// tap costs a byte extraction (shared between the output bytes that read it) and one multiply-add, nothing else.
//
// Tiled kernel (blur_conv_tiled_kernel<C, RC, NT>): the shapes of blur_bilateral_tiled_kernel — rows of whole 16-byte
// chunks, 16-byte aligned buffers and strides, 1-4 channels.  One workgroup = one tile of TILE_TH output rows x ncols
// (<= 32) chunk columns:
//   * stage (TILE_TH + 2 ry) rows x (ncols + 2 HC) chunks in LDS (stage_tile, kernel_common.h), x-clamp included;
//   * a thread takes one output dword (4 bytes) at a time.  Per window row it reads the dwords that cover its
//     4 + 2 RC C window bytes; every tap is then at a compile-time byte of those registers.  The ROW loop runs over the
//     real 2 ry + 1; the COLUMN loop is unrolled for the radius class RC (1, 2, 3, 5 or 7: rx = 0 and 1 take class 1, so
//     the 3 x 3 presets pay for no zero column) with the tap row zero-padded to 2 RC + 1, read from the kernel arguments
//     through the scalar cache (taps are wave-uniform);
//   * NT = 2 (MAG) accumulates both tables from the same window registers in the same pass;
//   * int32 accumulators, one saturating pack.
// The tables travel BY VALUE in the kernel arguments (one dword per tap): no device allocation, nothing to free.
//
// Generic kernel (blur_conv_generic_kernel): one output byte per thread, any shape, both tables (int16) in LDS.
#include "kernel_common.h"

#include <algorithm>
#include <string.h>

namespace mi_blur {

namespace {

constexpr int CONV_MAX_R = MI_BLUR_CONV_MAX_RADIUS;
constexpr int CONV_SPAN = 2 * CONV_MAX_R + 1;         // the 15 x 15 frame Filter::conv_k is centred in

constexpr int conv_hc(int C, int RC) { return RC * C <= 16 ? 1 : 2; }   // rx C <= 28 bytes of halo
constexpr int conv_class(int rx) { return rx <= 1 ? 1 : rx <= 3 ? rx : rx <= 5 ? 5 : 7; }

template <int RC, int NT>
struct ConvTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per band / output block
    int pitch, cpr;                   // bytes per row, 16-byte chunks per row
    int H, y0, y1;                    // band rows (clamp range), output rows [y0, y1)
    int ncols, nstrips, ntiles_y;
    int ry, mode, shift, bias;
    unsigned nblocks;
    int xcd;                          // 1 = each XCD takes a contiguous run of tiles (halo rows stay in its L2)
    int32_t k[NT][CONV_SPAN][2 * RC + 1];   // k[t][j + ry][i + RC] = K[j][i] (t = 1: K2), 0 beyond rx; rows past 2 ry unused
};

// acc (and acc2 for MAG) -> the output byte.  bias + |acc| + |acc2| stays below 2^27; >> on int is the floor.
// The empty asm keeps the shift and the clamp apart: left together, hipcc fuses the shift-and-clamp of two neighbouring
// bytes into v_ashr_pk_u8_i32 and ORs the other two bytes onto its result as if the upper half of that register were
// zero.  On the MI355X a negative acc + bias in byte 1 then turned bytes 2 and 3 of the dword into 255 (K = [4], bias -64,
// shift 4, ABS): what an upper half that keeps the register's earlier content, the accumulator, gives.
__device__ __forceinline__ uint32_t conv_pack(int acc, int acc2, int mode, int shift, int bias)
{
    int a = mode == MI_BLUR_CONV_SAT ? acc : abs(acc);
    if (mode == MI_BLUR_CONV_MAG) a += abs(acc2);
    a = (a + bias) >> shift;
    asm volatile("" : "+v"(a));
    return (uint32_t)min(max(a, 0), 255);
}

template <int C, int RC, int NT>
__global__ __launch_bounds__(TILE_THREADS) void blur_conv_tiled_kernel(const ConvTiledParams<RC, NT> p)
{
    constexpr int HC = conv_hc(C, RC);
    extern __shared__ __attribute__((aligned(16))) uint8_t tile[];
    const int t = threadIdx.x;
    const int ry = p.ry;
    const TileCoords tc = tile_coords<HC>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, p.y0, p.y1, ry);
    const int img = tc.img, ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc, ncw = tc.ncw;
    stage_tile<C, HC>(tile, p.in + (long long)img * p.in_stride, p.cpr, p.H, p.pitch, tc, ry, t);

    // ---- the window: thread = one output dword; window row jj of output row k is staged row k + jj
    constexpr int PAD = (RC * C + 3) & ~3;              // bytes read left of the output dword (whole dwords)
    constexpr int OFF = PAD - RC * C;                   // the window's first byte within them
    constexpr int NW = (PAD + 4 + RC * C + 3) / 4;      // dwords that cover the 4 + 2 RC C window bytes
    static_assert(PAD <= 16 * HC, "halo smaller than the radius class");
    const int nq = nc * 4;
    const int rb = ncw * 16;
    uint8_t *out_tile = p.out + (long long)img * p.out_stride + (size_t)(ty0 - p.y0) * (size_t)p.pitch + (size_t)x0c * 16u;
    for (int i = t; i < rows_out * nq; i += TILE_THREADS) {
        const int k = i / nq, q = i - k * nq;
        const uint8_t *wp = tile + k * rb + 16 * HC + 4 * q;
        int acc[4] = {0, 0, 0, 0}, acc2[4] = {0, 0, 0, 0};
        for (int jj = 0; jj <= 2 * ry; jj++) {
            uint32_t W[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) W[w] = *reinterpret_cast<const uint32_t *>(wp + jj * rb - PAD + 4 * w);
#pragma unroll
            for (int g = 0; g <= 2 * RC; g++) {
                const int k0 = p.k[0][jj][g];           // wave-uniform: scalar loads
                const int k1 = NT == 2 ? p.k[NT - 1][jj][g] : 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int v = (int)window_byte(W, OFF + b + g * C);
                    acc[b] += __mul24(k0, v);                                   // |K| < 2^16, v < 2^8: exact
                    if (NT == 2) acc2[b] += __mul24(k1, v);
                }
            }
        }
        const int mode = NT == 2 ? (int)MI_BLUR_CONV_MAG : p.mode;
        const uint32_t o = conv_pack(acc[0], acc2[0], mode, p.shift, p.bias) | (conv_pack(acc[1], acc2[1], mode, p.shift, p.bias) << 8) |
                           (conv_pack(acc[2], acc2[2], mode, p.shift, p.bias) << 16) | (conv_pack(acc[3], acc2[3], mode, p.shift, p.bias) << 24);
        *reinterpret_cast<uint32_t *>(out_tile + (size_t)k * (size_t)p.pitch + 4 * q) = o;
    }
}

constexpr int CONV_TAB_DWORDS = (2 * CONV_SPAN * CONV_SPAN * 2 + 3) / 4;   // both int16 tables

struct ConvGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per band (rows * pitch)
    int width, channels, pitch, H, y0;
    int rx, ry, mode, shift, bias;
    uint32_t tab[CONV_TAB_DWORDS];                   // K, then K2, int16, each centred in the 15 x 15 frame
};

__global__ __launch_bounds__(256) void blur_conv_generic_kernel(const ConvGenericParams p)
{
    __shared__ uint32_t tab[CONV_TAB_DWORDS];
    if (threadIdx.x < CONV_TAB_DWORDS) tab[threadIdx.x] = p.tab[threadIdx.x];
    __syncthreads();
    const int16_t *kc = reinterpret_cast<const int16_t *>(tab) + CONV_MAX_R * CONV_SPAN + CONV_MAX_R;   // K[0][0]
    const int16_t *kc2 = kc + CONV_SPAN * CONV_SPAN;
    const int rx = p.rx, ry = p.ry;
    const bool mag = p.mode == MI_BLUR_CONV_MAG;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.pitch, p.channels, p.y0, p.in, p.in_stride);
        int acc = 0, acc2 = 0;
        for (int j = -ry; j <= ry; j++) {
            const int ny = min(max(q.y + j, 0), p.H - 1);
            const uint8_t *rowp = q.src + (size_t)ny * (size_t)p.pitch + q.c;
            for (int i = -rx; i <= rx; i++) {
                const int nx = min(max(q.x + i, 0), p.width - 1);
                const int v = rowp[(size_t)nx * (size_t)p.channels];
                acc += __mul24((int)kc[j * CONV_SPAN + i], v);
                if (mag) acc2 += __mul24((int)kc2[j * CONV_SPAN + i], v);
            }
        }
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)conv_pack(acc, acc2, p.mode, p.shift, p.bias);
    }
}
static_assert(CONV_TAB_DWORDS <= 256, "one thread per table dword");

template <int RC, int NT>
int launch_conv_tiled(const LaunchDesc &d)
{
    set_last_kernel("blur_conv_tiled_kernel");
    const Filter &f = *d.filter;
    const int rx = f.conv_rx, ry = f.conv_ry;
    ConvTiledParams<RC, NT> p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid)) return st;
    p.ry = ry; p.mode = f.conv_mode; p.shift = f.conv_shift; p.bias = f.conv_bias;
    for (int t = 0; t < NT; t++)
        for (int j = -ry; j <= ry; j++)
            for (int i = -rx; i <= rx; i++) p.k[t][j + ry][i + RC] = f.conv_k[t][(j + CONV_MAX_R) * CONV_SPAN + i + CONV_MAX_R];
    const dim3 block(TILE_THREADS);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto C) {
        const size_t lds = (size_t)(TILE_TH + 2 * ry) * (size_t)(p.ncols + 2 * conv_hc(C, RC)) * 16u;
        return do_launch(blur_conv_tiled_kernel<C, RC, NT>, grid, block, lds, d, p);
    });
}

int launch_conv_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_conv_generic_kernel");
    const Filter &f = *d.filter;
    ConvGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    p.rx = f.conv_rx; p.ry = f.conv_ry; p.mode = f.conv_mode; p.shift = f.conv_shift; p.bias = f.conv_bias;
    static_assert(sizeof(f.conv_k) <= sizeof(p.tab), "both tables fit");
    memcpy(p.tab, f.conv_k, sizeof(f.conv_k));
    return do_launch(blur_conv_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

int launch_conv(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::CONV, [](const Filter &f) {
        return f.conv_rx >= 0 && f.conv_rx <= CONV_MAX_R && f.conv_ry >= 0 && f.conv_ry <= CONV_MAX_R;
    });
    if (st != LAUNCH_GO) return st;
    const Filter &f = *d.filter;
    if (!tile_aligned(d)) return launch_conv_generic(d);
    return dispatch<1, 2, 3, 5, 7>(conv_class(f.conv_rx), [&](auto RC) {
        return f.conv_mode == MI_BLUR_CONV_MAG ? launch_conv_tiled<RC, 2>(d) : launch_conv_tiled<RC, 1>(d);
    });
}

}  // namespace mi_blur
