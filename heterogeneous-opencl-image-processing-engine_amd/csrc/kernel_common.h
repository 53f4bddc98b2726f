// kernel_common.h — internal (not part of the C ABI): what the .hip files share below launch(): the launch call, the
// blockIdx -> tile maps, the template dispatch, the argument checks and parameter fill every family repeats, the host side of the direct layout,
// the flat grid and the 16-pixel group of the families outside Filter (fill_flat(), load_group(), store_group()),
// the tile of all seven tiled kernels (its coordinates and its launch geometry: fill_tiles(), on tile_grid() of filter.h), the
// staging of the sep, morph, bilateral, conv and sep_down kernels' LDS tile (stage_tile) and of the resize and warp kernels'
// footprint (stage_box), and the v_mad_u32_u24 form of the bilinear blend (lerp24).
// Everything here has internal linkage, so libmi_blur.so exports nothing from it.
#pragma once
#include "blur_launch.h"
#include "../../include/mi_blur.h"

#include <hip/hip_ext.h>
#include <limits.h>
#include <stdint.h>
#include <type_traits>

namespace mi_blur {

// ----------------------------------------------------------------------------------
// device side
// ----------------------------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// blockIdx -> tile.  Blocks b and b+8 share an XCD (round-robin dispatch); give each XCD a contiguous run of the
// n tiles so tile-edge halo rows are L2 hits.  A bijection of [0, n).  Speed only.
__device__ __forceinline__ unsigned xcd_contiguous(unsigned L, unsigned n)
{
    const unsigned q = n >> 3, r = n & 7u, x = L & 7u, k = L >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}
// The same idea at a finer grain: runs of `run` consecutive tiles (tiles that share halo rows: an image, a few tile rows)
// are dealt to the XCDs in turn, so an XCD's tiles still find their neighbours' rows in its own L2 while its stream walks
// the WHOLE buffer instead of one eighth of it.  A bijection of [0, n): the last n mod 8*run tiles map to themselves.
__device__ __forceinline__ unsigned xcd_runs(unsigned L, unsigned n, unsigned run)
{
    const unsigned span = 8u * run, full = n - n % span;
    if (L >= full) return L;
    const unsigned x = L & 7u, k = L >> 3, j = k / run, o = k - j * run;
    return (j * 8u + x) * run + o;
}
__device__ __forceinline__ unsigned xcd_map(unsigned L, unsigned n, int mode)
{
    return mode == 0 ? L : mode == 1 ? xcd_contiguous(L, n) : xcd_runs(L, n, (unsigned)mode);
}

// The flat rule's group g of an image (color_flat_ok(), filter.h): N chunks of 16 bytes, as 4 N dwords of a local array.
// The hist, arith and CLAHE kernels.  blur_color_tiled_kernel and blur_integral_tiled_kernel write the same loops out:
// with these helpers their code objects come out in another instruction order
// (profiles/r25_table_api_code_objects.md).
template <int N>
__device__ __forceinline__ void load_group(uint32_t (&w)[4 * N], const uint8_t *img, unsigned g)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(img + (size_t)g * (16u * N));
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint4 v = src[j];
        w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
    }
}
template <int N>
__device__ __forceinline__ void store_group(const uint32_t (&r)[4 * N], uint8_t *img, unsigned g)
{
    uint4 *dst = reinterpret_cast<uint4 *>(img + (size_t)g * (16u * N));
#pragma unroll
    for (int j = 0; j < N; j++) dst[j] = make_uint4(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]);
}

__device__ __forceinline__ u16x2 pk16(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ uint32_t pk32(u16x2 x) { return __builtin_bit_cast(uint32_t, x); }
// Byte idx of a window row held in the dwords W; idx is a constant wherever this is called (unrolled loops).
template <int N>
__device__ __forceinline__ uint32_t window_byte(const uint32_t (&W)[N], int idx) { return (W[idx >> 2] >> (8 * (idx & 3))) & 0xffu; }

// The LDS tile blur_sep_tiled_kernel, blur_morph_tiled_kernel, blur_bilateral_tiled_kernel, blur_conv_tiled_kernel and
// (in input coordinates) blur_sep_down_tiled_kernel work on: rows of whole 16-byte chunks, one workgroup of TILE_THREADS = one tile of TILE_TH output rows x ncols
// (<= TILE_NCOLS) chunk columns, staged with ry rows above and below and HC halo chunks either side.  blur_resize_tiled_kernel
// and blur_warp_tiled_kernel take the tile from the same tile_coords (HC = 0, ry = 0, on the OUTPUT image) and stage the
// input box under it with stage_box.  The helpers take
// the kernel arguments they need as scalars: handed the parameter struct by reference the kernels grow by a third.
// TILE_TH rows x at most TILE_NCOLS chunk columns (filter.h).
constexpr int TILE_THREADS = 256;

struct TileCoords {
    int img;                        // image of the batch
    int ty0, rows_out;              // first output row of the tile (band coordinates), output rows (<= TILE_TH)
    int x0c, nc;                    // first output chunk column, output chunk columns (<= ncols)
    int ncw, nrows;                 // staged chunk columns (tile chunk cc = row chunk x0c - HC + cc) and rows
};
// blockIdx -> tile (fill_tiles() is the host side: strips fastest, then tile rows, then images).
template <int HC>
__device__ __forceinline__ TileCoords tile_coords(int xcd, unsigned nblocks, int nstrips, int ntiles_y, int ncols, int cpr, int y0,
                                                  int y1, int ry)
{
    const unsigned L = xcd ? xcd_contiguous(blockIdx.x, nblocks) : blockIdx.x;
    const int strip = (int)(L % (unsigned)nstrips);
    const unsigned t2 = L / (unsigned)nstrips;
    const int ty = (int)(t2 % (unsigned)ntiles_y);
    TileCoords tc;
    tc.img = (int)(t2 / (unsigned)ntiles_y);
    tc.ty0 = y0 + ty * TILE_TH;
    tc.rows_out = min(TILE_TH, y1 - tc.ty0);
    tc.x0c = strip * ncols;
    tc.nc = min(ncols, cpr - tc.x0c);
    tc.ncw = tc.nc + 2 * HC;
    tc.nrows = tc.rows_out + 2 * ry;
    return tc;
}

// Stages tc's nrows x ncw chunks of the image at img_in (rows of cpr chunks, `pitch` bytes; source rows clamped to
// [0, H)) at `tile` and returns after the barrier that makes them visible to thread t's workgroup.
//   * slot s = row * ncw + cc; global_load_lds_dwordx4 (LDS-DMA, 16 B per lane) moves 64 consecutive slots per
//     wave-instruction: their LDS image is the 64 lanes in order;
//   * halo chunks outside the image row are not loaded: they get copies of the first / last pixel's channels (same
//     channel, position mod C), so the x-clamp costs the passes nothing.  A row narrower than the halo has them on both
//     sides of its only strip; their source is the row itself, which no thread of this loop writes.
template <int C, int HC>
__device__ __forceinline__ void stage_tile(uint8_t *tile, const uint8_t *img_in, int cpr, int H, int pitch, const TileCoords &tc, int ry, int t)
{
    const int ty0 = tc.ty0, x0c = tc.x0c, nc = tc.nc, ncw = tc.ncw, nrows = tc.nrows;
    {
        const int lane = t & 63, wv = t >> 6;
        const int nslots = nrows * ncw;
        for (int u = wv; u * 64 < nslots; u += TILE_THREADS / 64) {
            const int s = u * 64 + lane;
            if (s < nslots) {
                const int row = s / ncw, cc = s - row * ncw;
                const int gc = x0c - HC + cc;
                if (gc >= 0 && gc < cpr) {
                    const int sr = min(max(ty0 - ry + row, 0), H - 1);
                    const uint8_t *g = img_in + ((unsigned)sr * (unsigned)pitch + (unsigned)gc * 16u);
                    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)g,
                                                     (void __attribute__((address_space(3))) *)(tile + (size_t)u * 64 * 16), 16, 0, 0);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (x0c < HC || x0c + nc + HC > cpr) {
        const int nedge = nrows * 2 * HC;
        for (int i = t; i < nedge; i += TILE_THREADS) {
            const int row = i / (2 * HC), h = i - row * (2 * HC);
            const int cc = h < HC ? h : nc + h;         // the HC left halo chunks, then the HC right ones
            const int gc = x0c - HC + cc;
            if (gc >= 0 && gc < cpr) continue;
            uint8_t *rowl = tile + (size_t)row * ncw * 16u;
            const int base = (x0c - HC) * 16;           // row byte at tile byte 0
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t w = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int pos = gc * 16 + 4 * q + b;
                    const int src = pos < 0 ? ((pos % C) + C) % C : pitch - C + (pos - pitch) % C;
                    w |= (uint32_t)rowl[src - base] << (8 * b);
                }
                v[q] = w;
            }
            *reinterpret_cast<uint4 *>(rowl + cc * 16) = make_uint4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
    }
}

// Stages nsr rows x nsc chunks that lie inside the image (no clamp), from src = the first chunk of the first row, rows
// `pitch` bytes apart, at dst: slot s = row * nsc + chunk (filter.h, "Tile geometry").  No barrier: the caller's follows.
__device__ __forceinline__ void stage_box(uint8_t *dst, const uint8_t *src, int pitch, int nsr, int nsc, int t)
{
    const int nslots = nsr * nsc;
#pragma unroll 2
    for (int s = t; s < nslots; s += TILE_THREADS) {
        const int row = s / nsc, cc = s - row * nsc;
        const uint4 v = *reinterpret_cast<const uint4 *>(src + ((unsigned)row * (unsigned)pitch + (unsigned)cc * 16u));
        *reinterpret_cast<uint4 *>(dst + (size_t)s * 16u) = v;
    }
}

// bilinear_blend() (filter.h) one axis at a time, for operands below 2^24 (bytes, or the first axis' sums < 2^20), so
// that each product is one v_mad_u32_u24: (BLEND_ONE - f) * a + f * b, and the same with the rounding of the second axis.
__device__ __forceinline__ uint32_t lerp24(uint32_t a, uint32_t b, uint32_t f) { return __umul24(a, BLEND_ONE - f) + __umul24(b, f); }
__device__ __forceinline__ uint32_t lerp24_round(uint32_t a, uint32_t b, uint32_t f) { return (lerp24(a, b, f) + BLEND_BIAS) >> BLEND_SHIFT; }

// Pixels xa and xa + 1 of a staged row, pixel xa starting at byte offset `off` of the footprint: a (and b) = their C
// bytes, lowest channel lowest.  Two dword reads at the 4-byte aligned address below `off` (one ds_read2_b32) and a 64-bit
// shift; 3 channels can straddle a third dword (bytes 3 .. 8 of the two): warp_read_bytes(C) bytes in all, the extent
// warp_tap() (filter.h) states and WARP_LDS_SLACK keeps inside the launch's LDS.  The warp, perspective and remap tiled kernels.
template <int C>
__device__ __forceinline__ void warp_taps(const uint8_t *lds, int off, uint32_t &a, uint32_t &b)
{
    constexpr uint32_t PIX = C == 4 ? 0xffffffffu : (1u << (8 * (C & 3))) - 1u;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(lds + (off & ~3));
    const int sh = 8 * (off & 3);
    const uint64_t v = (((uint64_t)q[1] << 32) | q[0]) >> sh;
    a = (uint32_t)v & PIX;
    if constexpr (C == 3) {
        const uint64_t v2 = (((uint64_t)q[2] << 32) | q[1]) >> sh;      // the bytes from off + 4 on; pixel b starts at off + 3
        b = (((uint32_t)v >> 24) | ((uint32_t)v2 << 8)) & PIX;
    } else {
        b = (uint32_t)(v >> (8 * C)) & PIX;
    }
}

// Output byte idx of a byte-per-thread (generic) kernel: block = output bytes per band, so idx = img * block + rem and
// rem = (y - y0) * pitch + b, b = x * channels + c (pitch: of the OUTPUT row, where that is not the input's).  src = the image's band.
struct BytePos {
    long long img, rem;
    int y, b, x, c;
    const uint8_t *src;
};
__device__ __forceinline__ BytePos byte_pos(long long idx, long long block, int pitch, int channels, int y0, const uint8_t *in, long long in_stride)
{
    BytePos q;
    q.img = idx / block;
    q.rem = idx - q.img * block;
    q.y = y0 + (int)(q.rem / pitch);
    q.b = (int)(q.rem % pitch);
    q.x = q.b / channels; q.c = q.b - q.x * channels;
    q.src = in + q.img * in_stride;
    return q;
}

// ----------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------
static inline int hip_status(hipError_t e) { return e == hipSuccess ? MI_BLUR_OK : MI_BLUR_ERR_HIP_BASE - (int)e; }

// One kernel launch.  On a LaunchDesc: the timestamped form exactly when the caller gave a start or stop event.
template <typename K, typename... A>
static int do_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A &...args)
{
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return hip_status(hipGetLastError());
}
template <typename K, typename... A>
static int do_launch(K kernel, dim3 grid, dim3 block, size_t lds, const LaunchDesc &d, const A &...args)
{
    if (d.start || d.stop)
        hipExtLaunchKernelGGL(kernel, grid, block, lds, d.stream, d.start, d.stop, 0, args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, lds, d.stream, args...);
    return hip_status(hipGetLastError());
}

// Runtime value -> template argument: dispatch<1, 2, 3, 4>(channels, [&](auto C) { return do_launch(kernel<C>, ...); })
// calls f with std::integral_constant<int, V> for the listed V that equals v and returns its status;
// MI_BLUR_ERR_INVALID when v is not listed.  Only the listed values are instantiated, in list order — which is the order
// of the kernels in the code object, so a list such as <16, 4, 8> keeps the order its `case` table had.
template <int... Vs, typename F>
static int dispatch(int v, F &&f)
{
    int status = MI_BLUR_ERR_INVALID;
    (void)(... || (v == Vs && (status = f(std::integral_constant<int, Vs>{}), true)));   // a left fold: instantiates in list order
    return status;
}

// The argument checks launch() and launch_checks() share; every one of them is MI_BLUR_ERR_INVALID.
static inline int check_desc(const LaunchDesc &d, FilterKind kind)
{
    if (!d.filter || d.filter->kind != kind || !d.in || !d.out || d.in == d.out) return MI_BLUR_ERR_INVALID;
    if (d.width <= 0 || d.band_rows <= 0 || d.channels <= 0 || d.n_images < 0) return MI_BLUR_ERR_INVALID;
    if (d.y0 < 0 || d.y1 > d.band_rows || d.y0 >= d.y1) return MI_BLUR_ERR_INVALID;
    if ((long long)d.width * d.channels > INT_MAX / 2) return MI_BLUR_ERR_INVALID;
    if ((long long)d.width * d.channels * d.band_rows > INT_MAX) return MI_BLUR_ERR_INVALID;  // per-image 32-bit
    return MI_BLUR_OK;
}
// Dense sizes of one band and one output block (out_shape(), filter.h: d.filter is set), and whether a stride given is
// negative or smaller than that.
static inline long long dense_in(const LaunchDesc &d) { return (long long)d.band_rows * d.width * d.channels; }
static inline long long dense_out(const LaunchDesc &d)
{
    const OutShape o = out_shape(*d.filter, d.width, d.band_rows, d.channels, d.y0, d.y1);
    return (long long)o.rows * o.width * o.channels;
}
static inline bool strides_too_small(const LaunchDesc &d)
{
    return d.in_stride < 0 || d.out_stride < 0 || (d.in_stride && d.in_stride < dense_in(d)) || (d.out_stride && d.out_stride < dense_out(d));
}
// What every family but the box blur answers before it chooses a kernel, in this order: check_desc, the family's own
// check of the filter (filter_ok(filter) false: MI_BLUR_ERR_INVALID; a whole_image_only family checks it against the
// image of d there too), the forms it does not take (halo pointers; rows other than the whole image for a
// whole_image_only filter: MI_BLUR_ERR_UNSUPPORTED), the strides, and only then the empty batch (MI_BLUR_OK; launch()
// answers it before the strides).  LAUNCH_GO, which is no status: there is something to launch.
constexpr int LAUNCH_GO = 1;
template <typename F>
static int launch_checks(const LaunchDesc &d, FilterKind kind, F &&filter_ok)
{
    if (const int st = check_desc(d, kind)) return st;
    if (!filter_ok(*d.filter)) return MI_BLUR_ERR_INVALID;
    if (d.halo_top || d.halo_bottom) return MI_BLUR_ERR_UNSUPPORTED;
    if (whole_image_only(*d.filter) && (d.y0 != 0 || d.y1 != d.band_rows)) return MI_BLUR_ERR_UNSUPPORTED;
    if (strides_too_small(d)) return MI_BLUR_ERR_INVALID;
    return d.n_images == 0 ? MI_BLUR_OK : LAUNCH_GO;
}
// Rows of whole 16-byte chunks, 1-4 channels, 16-byte aligned buffers and strides: what the tiled kernels (and the
// median's register-window kernel) take.
static inline bool tile_aligned(const LaunchDesc &d)
{
    return d.channels <= 4 && (long long)d.width * d.channels % 16 == 0 && (uintptr_t)d.in % 16 == 0 && (uintptr_t)d.out % 16 == 0 &&
           d.in_stride % 16 == 0 && d.out_stride % 16 == 0;
}

// Bytes of one output row: the input's, or the output image's of a whole_image_only filter (out_shape(), filter.h).
static inline int out_pitch(const LaunchDesc &d)
{
    const OutShape o = out_shape(*d.filter, d.width, d.band_rows, d.channels, d.y0, d.y1);
    return o.width * o.channels;
}

// The members most kernels' parameter structs have under the same names (a template, not a base struct: the structs'
// names and layouts are the kernels' mangled names and kernarg layouts).  Stride 0 = laid end to end.  A struct with
// `opitch` belongs to a whole_image_only filter: it gets the output pitch, and its launch sets the y0 (0), y1 or width it carries.
template <typename P, typename = void> struct has_opitch : std::false_type {};
template <typename P> struct has_opitch<P, std::void_t<decltype(P::opitch)>> : std::true_type {};
template <typename P>
static void fill_band(P &p, const LaunchDesc &d)
{
    p.in = d.in; p.out = d.out;
    p.pitch = d.width * d.channels; p.H = d.band_rows;
    if constexpr (has_opitch<P>::value) p.opitch = out_pitch(d);
    else p.y0 = d.y0;
    p.in_stride = d.in_stride ? d.in_stride : dense_in(d);
    p.out_stride = d.out_stride ? d.out_stride : dense_out(d);
}

// The flat grid of the kernels that number their workgroups (image, workgroup of the image), one workgroup each:
// p.nblocks, and p.xcd = the XCD-contiguous order for grids of 16 workgroups and more (the kernels decode it with
// xcd_contiguous()).  MI_BLUR_ERR_INVALID when the workgroups do not number in 31 bits.
template <typename P>
static int fill_flat(P &p, long long n_images, long long per_image)
{
    const long long nblocks = n_images * per_image;
    if (nblocks > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    p.nblocks = (unsigned)nblocks;
    p.xcd = nblocks >= 16 ? 1 : 0;
    return MI_BLUR_OK;
}

// fill_band plus the tile decomposition g of the tiled kernels' parameter structs (tile_coords() is the device side) and
// the grid, one workgroup per tile.  MI_BLUR_ERR_INVALID when the tiles do not number in 31 bits.  Without g: the rows
// [y0, y1) of the band and the chunks of its rows, in strips of up to TILE_NCOLS chunks.
template <typename P>
static int fill_tiles(P &p, const LaunchDesc &d, dim3 *grid, const TileGrid &g)
{
    fill_band(p, d);
    if constexpr (!has_opitch<P>::value) p.y1 = d.y1;
    p.cpr = g.cpr; p.nstrips = g.nstrips; p.ncols = g.ncols; p.ntiles_y = g.ntiles_y;
    if (const int st = fill_flat(p, d.n_images, (long long)p.ntiles_y * p.nstrips)) return st;
    *grid = dim3(p.nblocks);
    return MI_BLUR_OK;
}
template <typename P>
static int fill_tiles(P &p, const LaunchDesc &d, dim3 *grid) { return fill_tiles(p, d, grid, tile_grid(d.width * d.channels / 16, d.y1 - d.y0)); }

static inline bool aligned16(const void *q) { return (uintptr_t)q % 16 == 0; }
// Workgroups of 256 threads for `threads` threads, none of them spare; 0 when they do not number in 31 bits.
static inline unsigned blocks_of(long long threads) { const long long b = (threads + 255) / 256; return b > 0x7fffffffLL ? 0u : (unsigned)b; }

// Grid of a byte-per-thread kernel: 256 threads per block, capped; the kernel grid-strides the rest.
static inline dim3 byte_grid(long long total)
{
    const long long blocks = (total + 255) / 256;
    return dim3((unsigned)(blocks > 256LL * 64 ? 256LL * 64 : blocks));
}
// fill_band plus what byte_pos() takes, for the generic kernels' parameter structs; returns the grid.
template <typename P>
static dim3 fill_generic(P &p, const LaunchDesc &d)
{
    fill_band(p, d);
    p.block = dense_out(d);
    p.total = p.block * d.n_images;
    p.channels = d.channels;
    if constexpr (!has_opitch<P>::value) p.width = d.width;
    return byte_grid(p.total);
}

// The direct layout (blur_direct_kernel, blur_median_fast_kernel): lanes are consecutive 16-byte chunk columns of the
// flattened (image, band of bh rows, chunk column) space, 62 computing lanes per wave, 4 waves per block.  Its work is
// numbered in 32 bits: direct_fits() is that bound for the shortest band any of these kernels uses (4 rows).
static inline bool direct_fits(const LaunchDesc &d)
{
    const long long cpr = (long long)d.width * d.channels / 16, rows = d.y1 - d.y0;
    return (long long)d.n_images * ((rows + 3) / 4) * cpr < 0x7fffffffLL;
}
// Fills p.nbands, p.total and p.nblocks (p.cpr is set) and returns the grid.
template <typename P>
static dim3 direct_grid(P &p, const LaunchDesc &d, int bh)
{
    p.nbands = (d.y1 - d.y0 + bh - 1) / bh;
    p.total = (long long)d.n_images * p.nbands * p.cpr;
    const long long waves = (p.total + 61) / 62;
    p.nblocks = (unsigned)((waves + 3) / 4);
    return dim3(p.nblocks);
}

}  // namespace mi_blur
