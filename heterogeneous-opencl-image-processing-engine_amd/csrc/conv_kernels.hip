// conv_kernels.hip — gfx950 kernels of the 2-D convolution with signed integer taps (mi_blur_enqueue_conv, include/mi_blur.h):
// per channel, over the (2 rx + 1) x (2 ry + 1) window with clamp-to-edge,
//   acc = sum K[j][i] * v,  (MAG: acc2 = sum K2[j][i] * v),  out = clamp((acc | |acc| | |acc| + |acc2|) + bias >> shift, 0, 255)
// Correlation (no flip).  filter_conv bounds sum |K| by 65535, so |acc| < 2^24: 24-bit multiplies and 32-bit signed sums are
// exact and the bytes are those of the CPU device.  Not separable: every tap is multiplied for every output byte, but a
// tap costs a byte extraction (shared between the output bytes that read it) and one multiply-add, nothing else.
//
// Tiled kernel (blur_conv_tiled_kernel<C, RC, NT>): the shapes of blur_bilateral_tiled_kernel — rows of whole 16-byte
// chunks, 16-byte aligned buffers and strides, 1-4 channels.  One workgroup = one tile of CONV_TH output rows x ncols
// (<= 32) chunk columns:
//   * stage (CONV_TH + 2 ry) rows x (ncols + 2 HC) chunks with global_load_lds_dwordx4, source rows clamped to the band,
//     halo chunks outside the image row filled with the edge pixel's channels: bilateral_kernels.hip's staging, step for
//     step (a twin, not a shared helper: the other kernels' code objects stay what they were);
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

constexpr int CONV_TH = 32;          // output rows per tile
constexpr int CONV_NCOLS = 32;       // at most this many output chunk columns per tile
constexpr int CONV_THREADS = 256;
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

// Byte idx of the window row held in the dwords W; idx is a constant wherever this is called (unrolled loops).
template <int N>
__device__ __forceinline__ int conv_byte(const uint32_t (&W)[N], int idx) { return (int)((W[idx >> 2] >> (8 * (idx & 3))) & 0xffu); }

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
__global__ __launch_bounds__(CONV_THREADS) void blur_conv_tiled_kernel(const ConvTiledParams<RC, NT> p)
{
    constexpr int HC = conv_hc(C, RC);
    extern __shared__ __attribute__((aligned(16))) uint8_t tile[];
    const int t = threadIdx.x;
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const int strip = (int)(L % (unsigned)p.nstrips);
    const unsigned t2 = L / (unsigned)p.nstrips;
    const int ty = (int)(t2 % (unsigned)p.ntiles_y);
    const int img = (int)(t2 / (unsigned)p.ntiles_y);

    const int ty0 = p.y0 + ty * CONV_TH;                // first output row of the tile (band coordinates)
    const int rows_out = min(CONV_TH, p.y1 - ty0);
    const int x0c = strip * p.ncols;
    const int nc = min(p.ncols, p.cpr - x0c);
    const int ncw = nc + 2 * HC;                        // staged chunk columns: tile chunk cc = row chunk x0c - HC + cc
    const int ry = p.ry;
    const int nrows = rows_out + 2 * ry;
    const uint8_t *img_in = p.in + (long long)img * p.in_stride;

    // ---- stage: slot s = row * ncw + cc; one wave-instruction moves 64 consecutive slots
    {
        const int lane = t & 63, wv = t >> 6;
        const int nslots = nrows * ncw;
        for (int u = wv; u * 64 < nslots; u += CONV_THREADS / 64) {
            const int s = u * 64 + lane;
            if (s < nslots) {
                const int row = s / ncw, cc = s - row * ncw;
                const int gc = x0c - HC + cc;
                if (gc >= 0 && gc < p.cpr) {
                    const int sr = min(max(ty0 - ry + row, 0), p.H - 1);
                    const uint8_t *g = img_in + ((unsigned)sr * (unsigned)p.pitch + (unsigned)gc * 16u);
                    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)g,
                                                     (void __attribute__((address_space(3))) *)(tile + (size_t)u * 64 * 16), 16, 0, 0);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // x-clamp: halo chunks outside the row get copies of the first / last pixel's channels (same channel, p mod C)
    if (x0c < HC || x0c + nc + HC > p.cpr) {
        const int nedge = nrows * 2 * HC;
        for (int i = t; i < nedge; i += CONV_THREADS) {
            const int row = i / (2 * HC), h = i - row * (2 * HC);
            const int cc = h < HC ? h : nc + h;         // the HC left halo chunks, then the HC right ones
            const int gc = x0c - HC + cc;
            if (gc >= 0 && gc < p.cpr) continue;
            uint8_t *rowl = tile + (size_t)row * ncw * 16u;
            const int base = (x0c - HC) * 16;           // row byte at tile byte 0
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t w = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int pos = gc * 16 + 4 * q + b;
                    const int src = pos < 0 ? ((pos % C) + C) % C : p.pitch - C + (pos - p.pitch) % C;
                    w |= (uint32_t)rowl[src - base] << (8 * b);
                }
                v[q] = w;
            }
            *reinterpret_cast<uint4 *>(rowl + cc * 16) = make_uint4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
    }

    // ---- the window: thread = one output dword; window row jj of output row k is staged row k + jj
    constexpr int PAD = (RC * C + 3) & ~3;              // bytes read left of the output dword (whole dwords)
    constexpr int OFF = PAD - RC * C;                   // the window's first byte within them
    constexpr int NW = (PAD + 4 + RC * C + 3) / 4;      // dwords that cover the 4 + 2 RC C window bytes
    static_assert(PAD <= 16 * HC, "halo smaller than the radius class");
    const int nq = nc * 4;
    const int rb = ncw * 16;
    uint8_t *out_tile = p.out + (long long)img * p.out_stride + (size_t)(ty0 - p.y0) * (size_t)p.pitch + (size_t)x0c * 16u;
    for (int i = t; i < rows_out * nq; i += CONV_THREADS) {
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
                    const int v = conv_byte(W, OFF + b + g * C);
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
        const long long img = idx / p.block;
        const long long rem = idx - img * p.block;
        const int y = p.y0 + (int)(rem / p.pitch);
        const int b = (int)(rem % p.pitch);
        const int x = b / p.channels, c = b - x * p.channels;
        const uint8_t *src = p.in + img * p.in_stride;
        int acc = 0, acc2 = 0;
        for (int j = -ry; j <= ry; j++) {
            const int ny = min(max(y + j, 0), p.H - 1);
            const uint8_t *rowp = src + (size_t)ny * (size_t)p.pitch + c;
            for (int i = -rx; i <= rx; i++) {
                const int nx = min(max(x + i, 0), p.width - 1);
                const int v = rowp[(size_t)nx * (size_t)p.channels];
                acc += __mul24((int)kc[j * CONV_SPAN + i], v);
                if (mag) acc2 += __mul24((int)kc2[j * CONV_SPAN + i], v);
            }
        }
        p.out[img * p.out_stride + rem] = (uint8_t)conv_pack(acc, acc2, p.mode, p.shift, p.bias);
    }
}
static_assert(CONV_TAB_DWORDS <= 256, "one thread per table dword");

template <int RC, int NT>
int launch_conv_tiled(const LaunchDesc &d)
{
    set_last_kernel("blur_conv_tiled_kernel");
    const Filter &f = *d.filter;
    const int rows = d.y1 - d.y0, rx = f.conv_rx, ry = f.conv_ry;
    ConvTiledParams<RC, NT> p{};
    fill_band(p, d);
    const int cpr = p.pitch / 16;
    p.cpr = cpr; p.y1 = d.y1;
    p.nstrips = (cpr + CONV_NCOLS - 1) / CONV_NCOLS;
    p.ncols = (cpr + p.nstrips - 1) / p.nstrips;
    p.ntiles_y = (rows + CONV_TH - 1) / CONV_TH;
    p.ry = ry; p.mode = f.conv_mode; p.shift = f.conv_shift; p.bias = f.conv_bias;
    for (int t = 0; t < NT; t++)
        for (int j = -ry; j <= ry; j++)
            for (int i = -rx; i <= rx; i++) p.k[t][j + ry][i + RC] = f.conv_k[t][(j + CONV_MAX_R) * CONV_SPAN + i + CONV_MAX_R];
    const long long nblocks = (long long)d.n_images * p.ntiles_y * p.nstrips;
    if (nblocks > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    p.nblocks = (unsigned)nblocks;
    p.xcd = nblocks >= 16 ? 1 : 0;
    const dim3 grid((unsigned)nblocks), block(CONV_THREADS);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto C) {
        const size_t lds = (size_t)(CONV_TH + 2 * ry) * (size_t)(p.ncols + 2 * conv_hc(C, RC)) * 16u;
        return do_launch(blur_conv_tiled_kernel<C, RC, NT>, grid, block, lds, d, p);
    });
}

int launch_conv_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_conv_generic_kernel");
    const Filter &f = *d.filter;
    ConvGenericParams p{};
    fill_band(p, d);
    p.block = dense_out(d);
    p.total = p.block * d.n_images;
    p.width = d.width; p.channels = d.channels;
    p.rx = f.conv_rx; p.ry = f.conv_ry; p.mode = f.conv_mode; p.shift = f.conv_shift; p.bias = f.conv_bias;
    static_assert(sizeof(f.conv_k) <= sizeof(p.tab), "both tables fit");
    memcpy(p.tab, f.conv_k, sizeof(f.conv_k));
    return do_launch(blur_conv_generic_kernel, byte_grid(p.total), dim3(256), 0, d, p);
}

}  // namespace

int launch_conv(const LaunchDesc &d)
{
    if (const int st = check_desc(d, FilterKind::CONV)) return st;
    const Filter &f = *d.filter;
    if (f.conv_rx < 0 || f.conv_rx > CONV_MAX_R || f.conv_ry < 0 || f.conv_ry > CONV_MAX_R) return MI_BLUR_ERR_INVALID;
    if (d.halo_top || d.halo_bottom) return MI_BLUR_ERR_UNSUPPORTED;
    if (strides_too_small(d)) return MI_BLUR_ERR_INVALID;
    if (d.n_images == 0) return MI_BLUR_OK;             // after the strides (launch(): before)
    const long long pitch = (long long)d.width * d.channels;
    const bool aligned = d.channels <= 4 && pitch % 16 == 0 && (uintptr_t)d.in % 16 == 0 && (uintptr_t)d.out % 16 == 0 &&
                         d.in_stride % 16 == 0 && d.out_stride % 16 == 0;
    if (!aligned) return launch_conv_generic(d);
    return dispatch<1, 2, 3, 5, 7>(conv_class(f.conv_rx), [&](auto RC) {
        return f.conv_mode == MI_BLUR_CONV_MAG ? launch_conv_tiled<RC, 2>(d) : launch_conv_tiled<RC, 1>(d);
    });
}

}  // namespace mi_blur
