// bilateral_kernels.hip — gfx950 kernels of the bilateral filter (mi_blur_enqueue_bilateral, include/mi_blur.h): per
// channel, with the spatial table S over the (2r+1) x (2r+1) window and the range table R over |v - v0|,
//   w = S[j][i] * R[|v - v0|],  den = sum w,  num = sum w * v,  out = (num + den / 2) / den
// v0 the sample itself, v its clamped neighbours.  Integer tables, 32-bit unsigned sums (filter_bilateral bounds sum S by
// 65535, so num + den / 2 < 2^32), one exact division: the bytes are those of the CPU device.  Not separable: every one
// of the (2r+1)^2 taps is looked up and multiplied for every output byte, so this is a VALU / LDS kernel, not an HBM one.
//
// Tiled kernel (blur_bilateral_tiled_kernel<C, RC>): the shapes of blur_sep_tiled_kernel — rows of whole 16-byte chunks,
// 16-byte aligned buffers and strides, 1-4 channels.  One workgroup = one tile of TILE_TH output rows x ncols (<= 32)
// chunk columns:
//   * the range table, 256 bytes, goes to the first 64 dwords of LDS once per workgroup;
//   * stage (TILE_TH + 2 r) rows x (ncols + 2 HC) chunks behind it (stage_tile, kernel_common.h), x-clamp included;
//   * a thread takes one output dword (4 bytes) at a time.  Per window row it reads the dwords that cover its 4 + 2 RC C
//     window bytes; every tap is then at a compile-time byte of those registers: |v - v0|, one ds_read_u8 of R, S * R,
//     two accumulations.  The ROW loop runs over the real radius; the COLUMN loop is unrolled for the radius class RC
//     (2, 4 or 8) with the spatial row zero-padded to 2 RC + 1, read from the kernel arguments through the scalar cache
//     (S is wave-uniform), so the classes cost columns of zero weight, never rows;
//   * the quotient is a float estimate (v_rcp_f32), at most one off either way (the true quotient is below 256, the
//     estimate's error below 2^-12), corrected by one multiply and two compares.
// The tables travel BY VALUE in the kernel arguments (the range table as 64 dwords, the spatial table as one dword per
// tap): no device allocation, nothing to free, the launch stays asynchronous.
//
// Generic kernel (blur_bilateral_generic_kernel): one output byte per thread, any shape, both tables in LDS.
#include "kernel_common.h"

#include <algorithm>
#include <string.h>

namespace mi_blur {

namespace {

constexpr int BIL_GC = 9;          // window columns whose range look-ups are in flight together
constexpr int BIL_MAX_R = MI_BLUR_BILATERAL_MAX_RADIUS;
constexpr int BIL_SPAN = 2 * BIL_MAX_R + 1;         // the 17 x 17 frame Filter::bil_s is centred in
constexpr int BIL_RANGE_BYTES = 256;                // LDS bytes in front of the tile

constexpr int bil_hc(int C, int RC) { return RC * C <= 16 ? 1 : (RC * C + 15) / 16; }
constexpr int bil_class(int r) { return r <= 2 ? 2 : r <= 4 ? 4 : 8; }

template <int RC>
struct BilTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per band / output block
    int pitch, cpr;                   // bytes per row, 16-byte chunks per row
    int H, y0, y1;                    // band rows (clamp range), output rows [y0, y1)
    int ncols, nstrips, ntiles_y;
    int r;
    unsigned nblocks;
    int xcd;                          // 1 = each XCD takes a contiguous run of tiles (halo rows stay in its L2)
    uint32_t range[BIL_RANGE_BYTES / 4];
    uint32_t s[BIL_SPAN][2 * RC + 1]; // s[j + r][i + RC] = S[j][i], 0 beyond the radius; rows past 2 r unused
};

// (num + den / 2) / den, exact.  den >= 1, the quotient is at most 255, q * den < 2^32 for q <= 256.
__device__ __forceinline__ uint32_t bil_div(uint32_t num, uint32_t den)
{
    const uint32_t n = num + (den >> 1);
    uint32_t q = (uint32_t)((float)n * __builtin_amdgcn_rcpf((float)den));
    const uint32_t qd = q * den;
    if (qd > n) q--;
    else if (n - qd >= den) q++;
    return q;
}

template <int C, int RC>
__global__ __launch_bounds__(TILE_THREADS) void blur_bilateral_tiled_kernel(const BilTiledParams<RC> p)
{
    constexpr int HC = bil_hc(C, RC);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *tile = lds + BIL_RANGE_BYTES;
    const int t = threadIdx.x;
    const int r = p.r;
    const TileCoords tc = tile_coords<HC>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, p.y0, p.y1, r);
    const int img = tc.img, ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc, ncw = tc.ncw;
    if (t < BIL_RANGE_BYTES / 4) reinterpret_cast<uint32_t *>(lds)[t] = p.range[t];
    stage_tile<C, HC>(tile, p.in + (long long)img * p.in_stride, p.cpr, p.H, p.pitch, tc, r, t);

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
        const uint32_t c0 = *reinterpret_cast<const uint32_t *>(wp + r * rb);
        uint32_t v0[4], num[4], den[4];
#pragma unroll
        for (int b = 0; b < 4; b++) { v0[b] = (c0 >> (8 * b)) & 0xffu; num[b] = 0u; den[b] = 0u; }
        for (int jj = 0; jj <= 2 * r; jj++) {
            uint32_t W[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) W[w] = *reinterpret_cast<const uint32_t *>(wp + jj * rb - PAD + 4 * w);
            // BIL_GC columns at a time: every look-up of the group is issued before the first one is used, so the
            // gathers are in flight together (taken tap by tap the loop waits out one LDS round trip per tap)
#pragma unroll
            for (int g0 = 0; g0 <= 2 * RC; g0 += BIL_GC) {
                constexpr int G = BIL_GC < 2 * RC + 1 ? BIL_GC : 2 * RC + 1;
                uint32_t R[G][4];
#pragma unroll
                for (int g = 0; g < G; g++) {
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        if (g0 + g > 2 * RC) continue;
                        const uint32_t v = window_byte(W, OFF + b + (g0 + g) * C);
                        R[g][b] = lds[v > v0[b] ? v - v0[b] : v0[b] - v];
                    }
                }
                asm volatile("" ::: "memory");          // the compiler keeps the loads above this line
#pragma unroll
                for (int g = 0; g < G; g++) {
                    if (g0 + g > 2 * RC) continue;
                    const uint32_t s = p.s[jj][g0 + g]; // wave-uniform: a scalar load
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const uint32_t w = __umul24(s, R[g][b]);                             // < 2^16
                        den[b] += w;
                        num[b] += __umul24(w, window_byte(W, OFF + b + (g0 + g) * C));          // w v < 2^24
                    }
                }
            }
        }
        const uint32_t o = bil_div(num[0], den[0]) | (bil_div(num[1], den[1]) << 8) | (bil_div(num[2], den[2]) << 16) |
                           (bil_div(num[3], den[3]) << 24);
        *reinterpret_cast<uint32_t *>(out_tile + (size_t)k * (size_t)p.pitch + 4 * q) = o;
    }
}

struct BilGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per band (rows * pitch)
    int width, channels, pitch, H, y0;
    int r;
    uint32_t tab[(BIL_SPAN * BIL_SPAN + BIL_RANGE_BYTES + 3) / 4];   // the range table, then S centred in the 17 x 17 frame
};

__global__ __launch_bounds__(256) void blur_bilateral_generic_kernel(const BilGenericParams p)
{
    constexpr int NT = (BIL_SPAN * BIL_SPAN + BIL_RANGE_BYTES + 3) / 4;
    __shared__ uint32_t tab[NT];
    if (threadIdx.x < NT) tab[threadIdx.x] = p.tab[threadIdx.x];
    __syncthreads();
    const uint8_t *range = reinterpret_cast<const uint8_t *>(tab);
    const uint8_t *sc = range + BIL_RANGE_BYTES + BIL_MAX_R * BIL_SPAN + BIL_MAX_R;   // S[0][0]
    const int r = p.r;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.pitch, p.channels, p.y0, p.in, p.in_stride);
        const uint32_t v0 = q.src[(size_t)q.y * (size_t)p.pitch + q.b];
        uint32_t num = 0u, den = 0u;
        for (int j = -r; j <= r; j++) {
            const int ny = min(max(q.y + j, 0), p.H - 1);
            const uint8_t *rowp = q.src + (size_t)ny * (size_t)p.pitch + q.c;
            for (int i = -r; i <= r; i++) {
                const int nx = min(max(q.x + i, 0), p.width - 1);
                const uint32_t v = rowp[(size_t)nx * (size_t)p.channels];
                const uint32_t d = v > v0 ? v - v0 : v0 - v;
                const uint32_t w = __umul24((uint32_t)sc[j * BIL_SPAN + i], (uint32_t)range[d]);
                den += w;
                num += __umul24(w, v);
            }
        }
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)bil_div(num, den);
    }
}
static_assert((BIL_SPAN * BIL_SPAN + BIL_RANGE_BYTES + 3) / 4 <= 256, "one thread per table dword");

template <int RC>
int launch_bilateral_tiled(const LaunchDesc &d)
{
    set_last_kernel("blur_bilateral_tiled_kernel");
    const Filter &f = *d.filter;
    const int r = f.bil_r;
    BilTiledParams<RC> p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid)) return st;
    p.r = r;
    memcpy(p.range, f.bil_range, BIL_RANGE_BYTES);
    for (int j = -r; j <= r; j++)
        for (int i = -r; i <= r; i++) p.s[j + r][i + RC] = f.bil_s[(j + BIL_MAX_R) * BIL_SPAN + i + BIL_MAX_R];
    const dim3 block(TILE_THREADS);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto C) {
        const size_t lds = BIL_RANGE_BYTES + (size_t)(TILE_TH + 2 * r) * (size_t)(p.ncols + 2 * bil_hc(C, RC)) * 16u;
        return do_launch(blur_bilateral_tiled_kernel<C, RC>, grid, block, lds, d, p);
    });
}

int launch_bilateral_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_bilateral_generic_kernel");
    const Filter &f = *d.filter;
    BilGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    p.r = f.bil_r;
    uint8_t *tab = reinterpret_cast<uint8_t *>(p.tab);
    memcpy(tab, f.bil_range, BIL_RANGE_BYTES);
    memcpy(tab + BIL_RANGE_BYTES, f.bil_s, BIL_SPAN * BIL_SPAN);
    return do_launch(blur_bilateral_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

int launch_bilateral(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::BILATERAL, [](const Filter &f) { return f.bil_r >= 1 && f.bil_r <= BIL_MAX_R; });
    if (st != LAUNCH_GO) return st;
    if (!tile_aligned(d)) return launch_bilateral_generic(d);
    return dispatch<2, 4, 8>(bil_class(d.filter->bil_r), [&](auto RC) { return launch_bilateral_tiled<RC>(d); });
}

}  // namespace mi_blur
