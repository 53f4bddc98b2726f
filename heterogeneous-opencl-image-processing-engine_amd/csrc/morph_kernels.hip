// morph_kernels.hip — gfx950 kernels of greyscale morphology (mi_blur_enqueue_morph, include/mi_blur.h): per channel the
// minimum (ERODE), the maximum (DILATE) or their difference (GRADIENT) of the (2 rx + 1) x (2 ry + 1) window, edges clamped:
//   lo[y][x][c] = min { in[clamp(y+j)][clamp(x+i)][c] : |i| <= rx, |j| <= ry },  hi = max of the same set
// min and max are separable and independent of the order of evaluation, so a vertical pass followed by a horizontal one
// gives the same bytes as the 2-D window.
//
// Tiled kernel (blur_morph_tiled_kernel<C, OP, HC>): the shapes of blur_sep_tiled_kernel — rows of whole 16-byte chunks,
// 16-byte aligned buffers and strides, 1-4 channels.  One workgroup = one tile of TILE_TH output rows x ncols (<= 32)
// chunk columns:
//   * stage (TILE_TH + 2 ry) rows x (ncols + 2 HC) chunks in LDS (stage_tile, kernel_common.h), x-clamp included.
//     HC = ceil(rx * C / 16) halo chunks either side, at least 1;
//   * the extrema live in 16-bit fields: a dword x carries its odd bytes as the HIGH bytes of its two fields already, and
//     x << 8 carries the even ones there.  The high byte of v_pk_min_u16 / v_pk_max_u16 of two fields is the min / max of
//     their high bytes whatever the low bytes hold, so one lane-operation reduces two bytes and nothing is ever masked;
//   * vertical pass: each thread takes one chunk column (halo chunks included) and MORPH_RPG = 8 output rows.  Their
//     windows are rows m .. m + 2 ry of the 8 + 2 ry staged rows the thread walks once.  ry >= 4: rows 7 .. 2 ry are in all
//     eight windows and are reduced once (the core); rows 0 .. 6 are taken downwards as a running suffix extremum, rows
//     2 ry + 1 .. 2 ry + 7 upwards as a running prefix (van Herk / Gil-Werman with one block per thread): 2 ry + 21
//     combinations for eight outputs instead of 8 (2 ry + 1).  ry <= 3: straight taps (at most 7 per output).  The
//     results replace the staged bytes in LDS, ONE byte per sample (two planes for GRADIENT);
//   * horizontal pass: each thread takes MORPH_NCH = 2 adjacent output chunks and the window of bytes around them, as
//     even / odd field arrays.  Doubling in place: w1 = the bytes, w2[q] = min(w1[q], w1[q + C]), w4[q] = min(w2[q],
//     w2[q + 2 C]), ... up to the largest 2^k <= 2 rx + 1, every level only over the bytes the next one needs; then two
//     overlapping windows of 2^k cover the 2 rx + 1 taps: out[q] = min(wk[q - rx C], wk[q + (rx + 1 - 2^k) C]).  Field
//     pairs at a byte offset are whole dwords or one v_alignbit of two.  k + 1 combinations per byte (6 at rx = 16)
//     instead of 2 rx.  rx is a runtime value: a wave-uniform switch picks the unrolled pass of that radius; HC, which
//     sizes LDS and the window registers, is the template argument.  GRADIENT subtracts its two planes at the end: every
//     byte of hi is >= its byte of lo, so the dword difference never borrows.
//
// Generic kernel (blur_morph_generic_kernel): one output byte per thread, any shape.  Correct everywhere, fast nowhere.
#include "kernel_common.h"

#include <algorithm>
#include <utility>

namespace mi_blur {

namespace {

template <bool MX>
__device__ __forceinline__ uint32_t ext2(uint32_t a, uint32_t b)
{
    return pk32(MX ? __builtin_elementwise_max(pk16(a), pk16(b)) : __builtin_elementwise_min(pk16(a), pk16(b)));
}
// Bytes back from the field form: the odd bytes from o, the even ones from the high bytes of e's fields.
__device__ __forceinline__ uint32_t unfield(uint32_t e, uint32_t o) { return (o & 0xff00ff00u) | ((e >> 8) & 0x00ff00ffu); }

constexpr int MORPH_RPG = 8;        // output rows per thread in the vertical pass
constexpr int MORPH_NCH = 2;        // output chunks per thread in the horizontal pass

constexpr int morph_hc(int C, int rx) { return rx * C <= 16 ? 1 : (rx * C + 15) / 16; }
constexpr int morph_log2(int n) { int k = 0; while ((2 << k) <= n) k++; return k; }   // largest k with 2^k <= n
constexpr bool morph_min(int op) { return op != MI_BLUR_MORPH_DILATE; }
constexpr bool morph_max(int op) { return op != MI_BLUR_MORPH_ERODE; }

struct MorphTiledParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per band / output block
    int pitch, cpr;                   // bytes per row, 16-byte chunks per row
    int H, y0, y1;                    // band rows (clamp range), output rows [y0, y1)
    int ncols, nstrips, ntiles_y;
    int rx, ry;
    unsigned nblocks;
    int xcd;                          // 1 = each XCD takes a contiguous run of tiles (halo rows stay in its L2)
};

// One staged row of one chunk column as fields: f[0..3] the even bytes (x << 8), f[4..7] the odd ones (x itself).
__device__ __forceinline__ void morph_row(const uint8_t *lp, uint32_t (&f)[8])
{
    const uint4 x = *reinterpret_cast<const uint4 *>(lp);
    f[0] = x.x << 8; f[1] = x.y << 8; f[2] = x.z << 8; f[3] = x.w << 8;
    f[4] = x.x; f[5] = x.y; f[6] = x.z; f[7] = x.w;
}

// Running extrema of one chunk column in field form: the minimum and / or the maximum, as OP needs (what it does not
// need is never computed: the members are dead).
template <int OP>
struct MorphExt {
    uint32_t lo[8], hi[8];
    __device__ __forceinline__ void set(const uint32_t (&f)[8])
    {
#pragma unroll
        for (int k = 0; k < 8; k++) { lo[k] = f[k]; hi[k] = f[k]; }
    }
    __device__ __forceinline__ void identity()
    {
#pragma unroll
        for (int k = 0; k < 8; k++) { lo[k] = 0xffffffffu; hi[k] = 0u; }
    }
    __device__ __forceinline__ void add(const uint32_t (&f)[8])
    {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if constexpr (morph_min(OP)) lo[k] = ext2<false>(lo[k], f[k]);
            if constexpr (morph_max(OP)) hi[k] = ext2<true>(hi[k], f[k]);
        }
    }
    __device__ __forceinline__ void add(const MorphExt &o)
    {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if constexpr (morph_min(OP)) lo[k] = ext2<false>(lo[k], o.lo[k]);
            if constexpr (morph_max(OP)) hi[k] = ext2<true>(hi[k], o.hi[k]);
        }
    }
};

// Field pair of window bytes q, q + 2 out of the even / odd field arrays (E[j]: bytes 4j, 4j+2; O[j]: 4j+1, 4j+3).
// q is a constant wherever this is called (unrolled loops).  Pairs past the window read as 0: only bytes no output needs.
template <int N>
__device__ __forceinline__ uint32_t morph_pair(const uint32_t (&E)[N], const uint32_t (&O)[N], int q)
{
    const int e0 = q >> 1, j = e0 >> 1;
    const uint32_t (&A)[N] = (q & 1) ? O : E;
    const uint32_t a = j < N ? A[j] : 0u;
    if ((e0 & 1) == 0) return a;
    const uint32_t b = j + 1 < N ? A[j + 1] : 0u;
    return __builtin_amdgcn_alignbit(b, a, 16);
}

// Doubling level L of the horizontal pass, in place: w(2^(L+1))[q] = ext(w(2^L)[q], w(2^L)[q + C 2^L]) for the window
// bytes [LO, hi) the later levels need.  Ascending dwords: a dword's partners lie in itself and above it, and both its
// new values are formed before either is written.
template <int C, int RX, int L, int K, int LO, int HIK, bool MX, int N>
__device__ __forceinline__ void morph_levels(uint32_t (&E)[N], uint32_t (&O)[N])
{
    if constexpr (L < K) {
        constexpr int S = C << L;
        constexpr int hi = HIK + C * ((1 << K) - (2 << L));
        constexpr int j0 = LO >> 2, j1 = (hi + 3) >> 2 < N ? (hi + 3) >> 2 : N;
#pragma unroll
        for (int j = j0; j < j1; j++) {
            const uint32_t ne = ext2<MX>(E[j], morph_pair(E, O, 4 * j + S));
            const uint32_t no = ext2<MX>(O[j], morph_pair(E, O, 4 * j + 1 + S));
            E[j] = ne; O[j] = no;
        }
        morph_levels<C, RX, L + 1, K, LO, HIK, MX>(E, O);
    }
}

// Horizontal pass of one thread: the min (MX = false) or max of the 2 RX + 1 taps for MORPH_NCH output chunks, from the
// plane of vertical results at lp (the window's first chunk: HC chunks left of the first output chunk).  res: bytes.
template <int C, int HC, int RX, bool MX>
__device__ __forceinline__ void morph_hpass(const uint8_t *lp, uint32_t (&res)[4 * MORPH_NCH])
{
    constexpr int NWC = MORPH_NCH + 2 * HC, N = 4 * NWC;      // window chunks, dwords per parity
    constexpr int P0 = 16 * HC, NOUT = 16 * MORPH_NCH;
    constexpr int K = morph_log2(2 * RX + 1);
    constexpr int LO = P0 - RX * C;                           // first window byte any output needs
    constexpr int S1 = (RX + 1 - (1 << K)) * C;               // the second window of 2^K starts this far from the output byte
    constexpr int HIK = P0 + NOUT + S1;                       // level K is needed on [LO, HIK)
    constexpr int HI0 = P0 + NOUT + RX * C;                   // the bytes themselves on [LO, HI0)
    static_assert(LO >= 0 && HI0 <= 16 * NWC, "window smaller than the radius");
    uint32_t E[N], O[N];
#pragma unroll
    for (int w = 0; w < NWC; w++) {
        if (16 * (w + 1) > LO && 16 * w < HI0) {
            const uint4 x = *reinterpret_cast<const uint4 *>(lp + 16 * w);
            O[4 * w] = x.x; O[4 * w + 1] = x.y; O[4 * w + 2] = x.z; O[4 * w + 3] = x.w;
            E[4 * w] = x.x << 8; E[4 * w + 1] = x.y << 8; E[4 * w + 2] = x.z << 8; E[4 * w + 3] = x.w << 8;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) { O[4 * w + i] = 0u; E[4 * w + i] = 0u; }
        }
    }
    morph_levels<C, RX, 0, K, LO, HIK, MX>(E, O);
#pragma unroll
    for (int j = 0; j < 4 * MORPH_NCH; j++) {
        const int q = P0 + 4 * j;
        const uint32_t e = ext2<MX>(morph_pair(E, O, q - RX * C), morph_pair(E, O, q + S1));
        const uint32_t o = ext2<MX>(morph_pair(E, O, q + 1 - RX * C), morph_pair(E, O, q + 1 + S1));
        res[j] = unfield(e, o);
    }
}

// The horizontal pass of the whole tile at radius RX — instantiated only in the kernel whose HC is that radius's.
template <int C, int OP, int HC, int RX>
__device__ __forceinline__ void morph_htile(const MorphTiledParams &p, const uint8_t *lds, uint8_t *out_tile, int rows_out, int nc,
                                            int ncw, int t)
{
    if constexpr (morph_hc(C, RX) == HC) {
        const int npairs = (nc + MORPH_NCH - 1) / MORPH_NCH;
        for (int i = t; i < rows_out * npairs; i += TILE_THREADS) {
            const int k = i / npairs, col = (i - k * npairs) * MORPH_NCH;
            const uint8_t *lp = lds + ((size_t)k * ncw + col) * 16u;
            uint32_t r[4 * MORPH_NCH];
            if constexpr (OP == MI_BLUR_MORPH_GRADIENT) {
                uint32_t lo[4 * MORPH_NCH];
                morph_hpass<C, HC, RX, false>(lp, lo);
                morph_hpass<C, HC, RX, true>(lp + (size_t)TILE_TH * ncw * 16u, r);
#pragma unroll
                for (int j = 0; j < 4 * MORPH_NCH; j++) r[j] -= lo[j];     // bytewise hi >= lo: no borrow
            } else {
                morph_hpass<C, HC, RX, OP == MI_BLUR_MORPH_DILATE>(lp, r);
            }
            uint8_t *op = out_tile + (size_t)k * (size_t)p.pitch + (size_t)col * 16u;
#pragma unroll
            for (int c = 0; c < MORPH_NCH; c++) {
                if (col + c < nc) {
                    u32x4 v; v.x = r[4 * c]; v.y = r[4 * c + 1]; v.z = r[4 * c + 2]; v.w = r[4 * c + 3];
                    *reinterpret_cast<u32x4 *>(op + 16 * c) = v;
                }
            }
        }
    }
}
template <int C, int OP, int HC, int... RXs>
__device__ __forceinline__ void morph_hswitch(std::integer_sequence<int, RXs...>, const MorphTiledParams &p, const uint8_t *lds,
                                              uint8_t *out_tile, int rows_out, int nc, int ncw, int t)
{
    (void)(... || (p.rx == RXs && (morph_htile<C, OP, HC, RXs>(p, lds, out_tile, rows_out, nc, ncw, t), true)));   // uniform
}

template <int C, int OP, int HC>
__global__ __launch_bounds__(TILE_THREADS) void blur_morph_tiled_kernel(const MorphTiledParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x;
    const int ry = p.ry;
    const TileCoords tc = tile_coords<HC>(p.xcd, p.nblocks, p.nstrips, p.ntiles_y, p.ncols, p.cpr, p.y0, p.y1, ry);
    const int img = tc.img, ty0 = tc.ty0, rows_out = tc.rows_out, x0c = tc.x0c, nc = tc.nc, ncw = tc.ncw;
    stage_tile<C, HC>(lds, p.in + (long long)img * p.in_stride, p.cpr, p.H, p.pitch, tc, ry, t);

    // ---- vertical pass: thread = (chunk column cc, row group g); every staged row read once
    const int ngrp = (rows_out + MORPH_RPG - 1) / MORPH_RPG;
    const bool vact = t < ncw * ngrp;
    const int g = t / ncw, vcc = t - g * ncw;
    MorphExt<OP> acc[MORPH_RPG];
    if (vact) {
        // staged rows g*RPG + e, e = 0 .. RPG + 2 ry - 1; rows past the tile feed unstored outputs only
        const uint8_t *lp = lds + ((size_t)g * MORPH_RPG * ncw + vcc) * 16u;
        const size_t rb = (size_t)ncw * 16u;
        uint32_t f[8];
        if (ry < 4) {                                   // straight taps: output m takes rows m .. m + 2 ry
#pragma unroll
            for (int m = 0; m < MORPH_RPG; m++) acc[m].identity();
            for (int e = 0; e < MORPH_RPG + 2 * ry; e++) {
                morph_row(lp + e * rb, f);
#pragma unroll
                for (int m = 0; m < MORPH_RPG; m++)
                    if (e - m >= 0 && e - m <= 2 * ry) acc[m].add(f);          // uniform
            }
        } else {
            MorphExt<OP> run;
#pragma unroll
            for (int m = MORPH_RPG - 2; m >= 0; m--) {  // rows 6 .. 0: suffix extrema, acc[m] = rows m .. 6
                morph_row(lp + m * rb, f);
                if (m == MORPH_RPG - 2) run.set(f); else run.add(f);
                acc[m] = run;
            }
            morph_row(lp + (MORPH_RPG - 1) * rb, f);    // rows 7 .. 2 ry: in every window
            run.set(f);
            for (int e = MORPH_RPG; e <= 2 * ry; e++) { morph_row(lp + e * rb, f); run.add(f); }
            acc[MORPH_RPG - 1] = run;
#pragma unroll
            for (int m = 0; m < MORPH_RPG - 1; m++) acc[m].add(run);
#pragma unroll
            for (int m = 1; m < MORPH_RPG; m++) {       // rows 2 ry + 1 .. 2 ry + 7: prefix extrema
                morph_row(lp + (2 * ry + m) * rb, f);
                if (m == 1) run.set(f); else run.add(f);
                acc[m].add(run);
            }
        }
    }
    __syncthreads();                                    // every staged byte read: the extrema take the tile's place
    if (vact) {
#pragma unroll
        for (int m = 0; m < MORPH_RPG; m++) {
            uint8_t *vp = lds + ((size_t)(g * MORPH_RPG + m) * ncw + vcc) * 16u;
            const uint32_t(&a)[8] = morph_min(OP) ? acc[m].lo : acc[m].hi;
            *reinterpret_cast<uint4 *>(vp) = make_uint4(unfield(a[0], a[4]), unfield(a[1], a[5]), unfield(a[2], a[6]), unfield(a[3], a[7]));
            if constexpr (OP == MI_BLUR_MORPH_GRADIENT) {
                const uint32_t(&b)[8] = acc[m].hi;      // second plane: TILE_TH rows further on
                *reinterpret_cast<uint4 *>(vp + (size_t)TILE_TH * ncw * 16u) =
                    make_uint4(unfield(b[0], b[4]), unfield(b[1], b[5]), unfield(b[2], b[6]), unfield(b[3], b[7]));
            }
        }
    }
    __syncthreads();

    // ---- horizontal pass: thread = MORPH_NCH output chunks of one row
    uint8_t *out_tile = p.out + (long long)img * p.out_stride + (size_t)(ty0 - p.y0) * (size_t)p.pitch + (size_t)x0c * 16u;
    morph_hswitch<C, OP, HC>(std::make_integer_sequence<int, MI_BLUR_MORPH_MAX_RADIUS + 1>{}, p, lds, out_tile, rows_out, nc, ncw, t);
}

struct MorphGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per band (rows * pitch)
    int width, channels, pitch, H, y0;
    int op, rx, ry;
};

__global__ __launch_bounds__(256) void blur_morph_generic_kernel(const MorphGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.pitch, p.channels, p.y0, p.in, p.in_stride);
        unsigned lo = 255u, hi = 0u;
        for (int j = -p.ry; j <= p.ry; j++) {
            const int ny = min(max(q.y + j, 0), p.H - 1);
            const uint8_t *rowp = q.src + (size_t)ny * (size_t)p.pitch + q.c;
            for (int i = -p.rx; i <= p.rx; i++) {
                const int nx = min(max(q.x + i, 0), p.width - 1);
                const unsigned v = rowp[(size_t)nx * (size_t)p.channels];
                lo = min(lo, v); hi = max(hi, v);
            }
        }
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)(p.op == MI_BLUR_MORPH_ERODE ? lo : p.op == MI_BLUR_MORPH_DILATE ? hi : hi - lo);
    }
}

int launch_morph_tiled(const LaunchDesc &d)
{
    set_last_kernel("blur_morph_tiled_kernel");
    const Filter &f = *d.filter;
    MorphTiledParams p{};
    dim3 grid;
    if (const int st = fill_tiles(p, d, &grid)) return st;
    p.rx = f.morph_rx; p.ry = f.morph_ry;
    const dim3 block(TILE_THREADS);
    const int hc = morph_hc(d.channels, p.rx);
    // the staged rows, then in their place one plane of TILE_TH rows per extremum; the last thread of a row of the
    // horizontal pass may read one chunk past its plane (an output chunk it does not store)
    const size_t row_bytes = (size_t)(p.ncols + 2 * hc) * 16u;
    const size_t planes = f.morph_op == MI_BLUR_MORPH_GRADIENT ? 2 : 1;
    const size_t lds = std::max((size_t)(TILE_TH + 2 * p.ry), planes * TILE_TH) * row_bytes + 16u;
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto C) {
        return dispatch<MI_BLUR_MORPH_ERODE, MI_BLUR_MORPH_DILATE, MI_BLUR_MORPH_GRADIENT>(f.morph_op, [&](auto OP) {
            return dispatch<1, 2, 3, 4>(hc, [&](auto HC) {
                if constexpr (HC <= C) return do_launch(blur_morph_tiled_kernel<C, OP, HC>, grid, block, lds, d, p);
                else return (int)MI_BLUR_ERR_INVALID;    // morph_hc(C, 16) = C: never asked for
            });
        });
    });
}

int launch_morph_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_morph_generic_kernel");
    const Filter &f = *d.filter;
    MorphGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    p.op = f.morph_op; p.rx = f.morph_rx; p.ry = f.morph_ry;
    return do_launch(blur_morph_generic_kernel, grid, dim3(256), 0, d, p);
}

}  // namespace

int launch_morph(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::MORPH, [](const Filter &f) {
        return f.morph_op >= MI_BLUR_MORPH_ERODE && f.morph_op <= MI_BLUR_MORPH_GRADIENT && f.morph_rx >= 0 &&
               f.morph_rx <= MI_BLUR_MORPH_MAX_RADIUS && f.morph_ry >= 0 && f.morph_ry <= MI_BLUR_MORPH_MAX_RADIUS;
    });
    if (st != LAUNCH_GO) return st;
    return tile_aligned(d) ? launch_morph_tiled(d) : launch_morph_generic(d);
}

}  // namespace mi_blur
