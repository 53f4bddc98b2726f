// bilateral_kernels.hip — gfx950 kernels of the bilateral filter (mi_blur_enqueue_bilateral, include/mi_blur.h): per
// channel, with the spatial table S over the (2r+1) x (2r+1) window and the range table R over |v - v0|,
//   w = S[j][i] * R[|v - v0|],  den = sum w,  num = sum w * v,  out = (num + den / 2) / den
// v0 the sample itself, v its clamped neighbours.  Integer tables, 32-bit unsigned sums (filter_bilateral bounds sum S by
// 65535, so num + den / 2 < 2^32), one exact division: the bytes are those of the CPU device.  Not separable: every one
// of the (2r+1)^2 taps is looked up and multiplied for every output byte, so this is a VALU / LDS kernel, not an HBM one.
//
// Tiled kernel (blur_bilateral_tiled_kernel<C, RC>): the shapes of blur_sep_tiled_kernel — rows of whole 16-byte chunks,
// 16-byte aligned buffers and strides, 1-4 channels.  One workgroup = one tile of BIL_TH output rows x ncols (<= 32)
// chunk columns:
//   * the range table, 256 bytes, goes to the first 64 dwords of LDS once per workgroup;
//   * stage (BIL_TH + 2 r) rows x (ncols + 2 HC) chunks behind it with global_load_lds_dwordx4, source rows clamped to the
//     band, halo chunks outside the image row filled with the edge pixel's channels: morph_kernels.hip's staging, step for
//     step (a twin, not a shared helper: the other kernels' code objects stay what they were);
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

constexpr int BIL_TH = 32;          // output rows per tile
constexpr int BIL_NCOLS = 32;       // at most this many output chunk columns per tile
constexpr int BIL_THREADS = 256;
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

// Byte idx of the window row held in the dwords W; idx is a constant wherever this is called (unrolled loops).
template <int N>
__device__ __forceinline__ uint32_t bil_byte(const uint32_t (&W)[N], int idx) { return (W[idx >> 2] >> (8 * (idx & 3))) & 0xffu; }

template <int C, int RC>
__global__ __launch_bounds__(BIL_THREADS) void blur_bilateral_tiled_kernel(const BilTiledParams<RC> p)
{
    constexpr int HC = bil_hc(C, RC);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *tile = lds + BIL_RANGE_BYTES;
    const int t = threadIdx.x;
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const int strip = (int)(L % (unsigned)p.nstrips);
    const unsigned t2 = L / (unsigned)p.nstrips;
    const int ty = (int)(t2 % (unsigned)p.ntiles_y);
    const int img = (int)(t2 / (unsigned)p.ntiles_y);

    const int ty0 = p.y0 + ty * BIL_TH;                 // first output row of the tile (band coordinates)
    const int rows_out = min(BIL_TH, p.y1 - ty0);
    const int x0c = strip * p.ncols;
    const int nc = min(p.ncols, p.cpr - x0c);
    const int ncw = nc + 2 * HC;                        // staged chunk columns: tile chunk cc = row chunk x0c - HC + cc
    const int r = p.r;
    const int nrows = rows_out + 2 * r;
    const uint8_t *img_in = p.in + (long long)img * p.in_stride;

    if (t < BIL_RANGE_BYTES / 4) reinterpret_cast<uint32_t *>(lds)[t] = p.range[t];
    // ---- stage: slot s = row * ncw + cc; one wave-instruction moves 64 consecutive slots
    {
        const int lane = t & 63, wv = t >> 6;
        const int nslots = nrows * ncw;
        for (int u = wv; u * 64 < nslots; u += BIL_THREADS / 64) {
            const int s = u * 64 + lane;
            if (s < nslots) {
                const int row = s / ncw, cc = s - row * ncw;
                const int gc = x0c - HC + cc;
                if (gc >= 0 && gc < p.cpr) {
                    const int sr = min(max(ty0 - r + row, 0), p.H - 1);
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
        for (int i = t; i < nedge; i += BIL_THREADS) {
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
    for (int i = t; i < rows_out * nq; i += BIL_THREADS) {
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
                        const uint32_t v = bil_byte(W, OFF + b + (g0 + g) * C);
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
                        num[b] += __umul24(w, bil_byte(W, OFF + b + (g0 + g) * C));          // w v < 2^24
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
        const long long img = idx / p.block;
        const long long rem = idx - img * p.block;
        const int y = p.y0 + (int)(rem / p.pitch);
        const int b = (int)(rem % p.pitch);
        const int x = b / p.channels, c = b - x * p.channels;
        const uint8_t *src = p.in + img * p.in_stride;
        const uint32_t v0 = src[(size_t)y * (size_t)p.pitch + b];
        uint32_t num = 0u, den = 0u;
        for (int j = -r; j <= r; j++) {
            const int ny = min(max(y + j, 0), p.H - 1);
            const uint8_t *rowp = src + (size_t)ny * (size_t)p.pitch + c;
            for (int i = -r; i <= r; i++) {
                const int nx = min(max(x + i, 0), p.width - 1);
                const uint32_t v = rowp[(size_t)nx * (size_t)p.channels];
                const uint32_t d = v > v0 ? v - v0 : v0 - v;
                const uint32_t w = __umul24((uint32_t)sc[j * BIL_SPAN + i], (uint32_t)range[d]);
                den += w;
                num += __umul24(w, v);
            }
        }
        p.out[img * p.out_stride + rem] = (uint8_t)bil_div(num, den);
    }
}
static_assert((BIL_SPAN * BIL_SPAN + BIL_RANGE_BYTES + 3) / 4 <= 256, "one thread per table dword");

template <int RC>
int launch_bilateral_tiled(const LaunchDesc &d)
{
    set_last_kernel("blur_bilateral_tiled_kernel");
    const Filter &f = *d.filter;
    const int rows = d.y1 - d.y0, r = f.bil_r;
    BilTiledParams<RC> p{};
    fill_band(p, d);
    const int cpr = p.pitch / 16;
    p.cpr = cpr; p.y1 = d.y1;
    p.nstrips = (cpr + BIL_NCOLS - 1) / BIL_NCOLS;
    p.ncols = (cpr + p.nstrips - 1) / p.nstrips;
    p.ntiles_y = (rows + BIL_TH - 1) / BIL_TH;
    p.r = r;
    memcpy(p.range, f.bil_range, BIL_RANGE_BYTES);
    for (int j = -r; j <= r; j++)
        for (int i = -r; i <= r; i++) p.s[j + r][i + RC] = f.bil_s[(j + BIL_MAX_R) * BIL_SPAN + i + BIL_MAX_R];
    const long long nblocks = (long long)d.n_images * p.ntiles_y * p.nstrips;
    if (nblocks > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    p.nblocks = (unsigned)nblocks;
    p.xcd = nblocks >= 16 ? 1 : 0;
    const dim3 grid((unsigned)nblocks), block(BIL_THREADS);
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto C) {
        const size_t lds = BIL_RANGE_BYTES + (size_t)(BIL_TH + 2 * r) * (size_t)(p.ncols + 2 * bil_hc(C, RC)) * 16u;
        return do_launch(blur_bilateral_tiled_kernel<C, RC>, grid, block, lds, d, p);
    });
}

int launch_bilateral_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_bilateral_generic_kernel");
    const Filter &f = *d.filter;
    BilGenericParams p{};
    fill_band(p, d);
    p.block = dense_out(d);
    p.total = p.block * d.n_images;
    p.width = d.width; p.channels = d.channels;
    p.r = f.bil_r;
    uint8_t *tab = reinterpret_cast<uint8_t *>(p.tab);
    memcpy(tab, f.bil_range, BIL_RANGE_BYTES);
    memcpy(tab + BIL_RANGE_BYTES, f.bil_s, BIL_SPAN * BIL_SPAN);
    return do_launch(blur_bilateral_generic_kernel, byte_grid(p.total), dim3(256), 0, d, p);
}

}  // namespace

int launch_bilateral(const LaunchDesc &d)
{
    if (const int st = check_desc(d, FilterKind::BILATERAL)) return st;
    const Filter &f = *d.filter;
    if (f.bil_r < 1 || f.bil_r > BIL_MAX_R) return MI_BLUR_ERR_INVALID;
    if (d.halo_top || d.halo_bottom) return MI_BLUR_ERR_UNSUPPORTED;
    if (strides_too_small(d)) return MI_BLUR_ERR_INVALID;
    if (d.n_images == 0) return MI_BLUR_OK;             // after the strides (launch(): before)
    const long long pitch = (long long)d.width * d.channels;
    const bool aligned = d.channels <= 4 && pitch % 16 == 0 && (uintptr_t)d.in % 16 == 0 && (uintptr_t)d.out % 16 == 0 &&
                         d.in_stride % 16 == 0 && d.out_stride % 16 == 0;
    if (!aligned) return launch_bilateral_generic(d);
    return dispatch<2, 4, 8>(bil_class(f.bil_r), [&](auto RC) { return launch_bilateral_tiled<RC>(d); });
}

}  // namespace mi_blur
