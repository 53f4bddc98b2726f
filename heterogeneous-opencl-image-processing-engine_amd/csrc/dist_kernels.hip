// dist_kernels.hip — gfx950 kernels of the exact distance transform (include/mi_blur.h, "Exact distance transform"):
// mi_blur_enqueue_dist and mi_blur_enqueue_dist_u8.  Integers only.  A candidate is dist_cand(), a search dist_search() or
// dist_search_plain(), the value it starts from and ends with dist_start() / dist_final(), a byte dist_byte() (filter.h),
// which the host export and the CPU device use too.
//
// ONE RULE: no workgroup here ever waits for another.  There is no flag and no ticket: what one band of rows hands the
// next crosses a dispatch boundary on the stream, through the work buffer.  Every loop has a bound known at launch.
//
// The column pass, three dispatches, one thread per column and channel (threads run along W * C: any shape, any alignment):
//   blur_dist_bands_kernel: per (image, band of rows) the first and the last site row of the column, or the marker, to
//     carry[image][band][first, last][W * C].
//   blur_dist_carry_kernel: per image the walk over the bands, down and then up, in place: `last` becomes the last site
//     row above the band, `first` the first site row below it.
//   blur_dist_cols_kernel: per (image, band) down the band from `last`, then up it from `first`: g[image][y][W * C], the
//     distance along the column to its nearest site; with a limit, the marker above it.
// The row pass, one dispatch:
//   blur_dist_tiled_kernel<CHUNK, OUT> (rows of whole 16-byte chunks of g, at most DIST_MAX_ROW elements, an aligned
//     output): a workgroup owns dist_rows() consecutive rows of the batch (g of all images is one array of rows, and a row
//     needs nothing of its neighbours).  It copies them to LDS with 16-byte loads, one plane per row and channel padded
//     with the marker to whole chunks of CHUNK columns, takes every chunk's minimum, and a thread owns 4 consecutive
//     elements of a row at a time: dist_search() per element (the nearest columns one by one, then chunk by chunk), then
//     one 16-byte store (OUT 0: the table) or one 4-byte store (OUT 1: bytes).
//   blur_dist_generic_kernel<OUT>: one element per thread of a capped grid that strides; dist_search_plain() on g in
//     global memory.
#include "kernel_common.h"

namespace mi_blur {

namespace {

struct DistColsParams {
    const uint8_t *in;
    uint16_t *g;
    uint16_t *carry;
    unsigned wc;                      // W * C
    unsigned nbands;
    int H, band;
    int nonzero;                      // a site is in != 0
    uint32_t cap;                     // dist_cap(limit)
    long long total;                  // threads: n_images * nbands * wc (bands, cols) or n_images * wc (carry)
};

__device__ __forceinline__ bool is_site(uint8_t v, int nonzero) { return (v != 0) == (nonzero != 0); }

__global__ __launch_bounds__(256) void blur_dist_bands_kernel(const DistColsParams p)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.total) return;
    const long long ib = t / p.wc;                                       // image * nbands + band
    const unsigned e = (unsigned)(t - ib * p.wc), b = (unsigned)(ib % p.nbands);
    const long long img = ib / p.nbands;
    const int y0 = (int)b * p.band, y1 = min(y0 + p.band, p.H);
    const uint8_t *src = p.in + ((size_t)img * p.H + y0) * p.wc + e;
    uint32_t first = DIST_G_NONE, last = DIST_G_NONE;
    for (int y = y0; y < y1; y++, src += p.wc)
        if (is_site(*src, p.nonzero)) {
            first = first == DIST_G_NONE ? (uint32_t)y : first;
            last = (uint32_t)y;
        }
    uint16_t *dst = p.carry + (size_t)ib * 2 * p.wc + e;
    dst[0] = (uint16_t)first;
    dst[p.wc] = (uint16_t)last;
}

__global__ __launch_bounds__(256) void blur_dist_carry_kernel(const DistColsParams p)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.total) return;
    const long long img = t / p.wc;
    const unsigned e = (unsigned)(t - img * p.wc);
    const size_t step = (size_t)2 * p.wc;
    uint16_t *q = p.carry + (size_t)img * p.nbands * step + e;
    uint32_t run = DIST_G_NONE;
    for (unsigned b = 0; b < p.nbands; b++) {                            // down: the last site row above band b
        uint16_t *last = q + b * step + p.wc;
        const uint32_t v = *last;
        *last = (uint16_t)run;
        run = v == DIST_G_NONE ? run : v;
    }
    run = DIST_G_NONE;
    for (unsigned b = p.nbands; b-- > 0;) {                              // up: the first site row below band b
        uint16_t *first = q + b * step;
        const uint32_t v = *first;
        *first = (uint16_t)run;
        run = v == DIST_G_NONE ? run : v;
    }
}

__global__ __launch_bounds__(256) void blur_dist_cols_kernel(const DistColsParams p)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.total) return;
    const long long ib = t / p.wc;
    const unsigned e = (unsigned)(t - ib * p.wc), b = (unsigned)(ib % p.nbands);
    const long long img = ib / p.nbands;
    const int y0 = (int)b * p.band, y1 = min(y0 + p.band, p.H);
    const size_t at = ((size_t)img * p.H + y0) * p.wc + e;
    const uint16_t *c = p.carry + (size_t)ib * 2 * p.wc + e;
    const uint8_t *src = p.in + at;
    uint16_t *g = p.g + at;
    uint32_t site = c[p.wc];                                             // the nearest site row so far, above
    for (int y = y0; y < y1; y++, src += p.wc, g += p.wc) {
        site = is_site(*src, p.nonzero) ? (uint32_t)y : site;
        *g = (uint16_t)(site == DIST_G_NONE ? DIST_G_NONE : (uint32_t)y - site);
    }
    site = c[0];                                                         // ... and below
    for (int y = y1 - 1; y >= y0; y--) {
        g -= p.wc;
        uint32_t d = *g;
        site = d == 0 ? (uint32_t)y : site;
        const uint32_t up = site == DIST_G_NONE ? DIST_G_NONE : site - (uint32_t)y;
        d = up < d ? up : d;                                             // the marker is the largest 16-bit value
        *g = (uint16_t)dist_g_cap(d, p.cap);
    }
}

struct DistRowParams {
    const uint16_t *g;
    uint32_t *table;                  // OUT 0
    uint8_t *out;                     // OUT 1
    long long rows;                   // n_images * H
    unsigned wc;                      // W * C
    int W, C;
    int rpg;                          // tiled: rows per workgroup
    int nch;                          // tiled: chunks per plane
    int metric, byte_op, invert;
    uint32_t start;                   // dist_start(metric, limit)
    long long total;                  // generic: elements
};

template <int CHUNK>
__device__ __forceinline__ uint32_t search_plane(int metric, const uint16_t *g, const uint16_t *cm, int nch, int x, uint32_t start)
{
    if (metric == MI_BLUR_DIST_L2) return dist_search<MI_BLUR_DIST_L2, CHUNK>(g, cm, nch, x, start);
    if (metric == MI_BLUR_DIST_L1) return dist_search<MI_BLUR_DIST_L1, CHUNK>(g, cm, nch, x, start);
    return dist_search<MI_BLUR_DIST_LINF, CHUNK>(g, cm, nch, x, start);
}

template <int CHUNK, int OUT>
__global__ __launch_bounds__(DIST_THREADS) void blur_dist_tiled_kernel(const DistRowParams p)
{
    extern __shared__ uint4 dist_lds[];
    uint16_t *plane = reinterpret_cast<uint16_t *>(dist_lds);           // [row][c][nch * CHUNK]
    const unsigned t = threadIdx.x, wp = (unsigned)p.nch * CHUNK, C = (unsigned)p.C, W = (unsigned)p.W;
    const long long r0 = (long long)blockIdx.x * p.rpg;
    const unsigned nr = (unsigned)min((long long)p.rpg, p.rows - r0);
    const unsigned planes = nr * C;
    uint16_t *cm = plane + (size_t)planes * wp;                          // [row][c][nch]
    const uint16_t *src = p.g + (size_t)r0 * p.wc;
    for (unsigned q = t; q < nr * p.wc / 8; q += DIST_THREADS) {         // 8 elements of g to their planes
        const uint4 v = reinterpret_cast<const uint4 *>(src)[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const unsigned row = q * 8 / p.wc, e0 = q * 8 - row * p.wc;      // wc is a multiple of 8: one row
        unsigned x = e0 / C, c = e0 - x * C;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            plane[(row * C + c) * wp + x] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
            if (++c == C) { c = 0; x++; }
        }
    }
    const unsigned pad = wp - W;                                         // the last chunk's columns beyond the row
    for (unsigned q = t; q < planes * pad; q += DIST_THREADS) plane[(q / pad) * wp + W + q % pad] = (uint16_t)DIST_G_NONE;
    __syncthreads();
    for (unsigned q = t; q < planes * (unsigned)p.nch; q += DIST_THREADS) {   // planes are whole chunks: chunk q starts at q * CHUNK
        const uint16_t *s = plane + (size_t)q * CHUNK;
        uint32_t m = DIST_G_NONE;
#pragma unroll
        for (int j = 0; j < CHUNK; j++) m = s[j] < m ? s[j] : m;
        cm[q] = (uint16_t)m;
    }
    __syncthreads();
    const unsigned quads = p.wc / 4;
    for (unsigned q = t; q < nr * quads; q += DIST_THREADS) {
        const unsigned row = q / quads, e0 = (q - row * quads) * 4;
        unsigned x = e0 / C, c = e0 - x * C;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned pl = row * C + c;
            v[j] = dist_final(search_plane<CHUNK>(p.metric, plane + (size_t)pl * wp, cm + (size_t)pl * p.nch, p.nch, (int)x, p.start), p.start);
            if (++c == C) { c = 0; x++; }
        }
        const size_t at = (size_t)(r0 + row) * p.wc + e0;
        if (OUT == 0) {
            *reinterpret_cast<uint4 *>(p.table + at) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) word |= (uint32_t)dist_byte(p.metric, p.byte_op, p.invert, v[j]) << (8 * j);
            *reinterpret_cast<uint32_t *>(p.out + at) = word;
        }
    }
}

template <int OUT>
__global__ __launch_bounds__(256) void blur_dist_generic_kernel(const DistRowParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const long long row = idx / p.wc;
        const int e = (int)(idx - row * p.wc), x = e / p.C, c = e - x * p.C;
        const uint16_t *g = p.g + (size_t)row * p.wc + c;
        const uint32_t best = p.metric == MI_BLUR_DIST_L2   ? dist_search_plain<MI_BLUR_DIST_L2>(g, p.C, p.W, x, p.start)
                              : p.metric == MI_BLUR_DIST_L1 ? dist_search_plain<MI_BLUR_DIST_L1>(g, p.C, p.W, x, p.start)
                                                            : dist_search_plain<MI_BLUR_DIST_LINF>(g, p.C, p.W, x, p.start);
        const uint32_t T = dist_final(best, p.start);
        if (OUT == 0) p.table[idx] = T;
        else p.out[idx] = (uint8_t)dist_byte(p.metric, p.byte_op, p.invert, T);
    }
}

}  // namespace

int launch_dist(const uint8_t *in, uint32_t *table, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_dist &k, void *work, hipStream_t stream)
{
    const bool bytes = out != nullptr;
    if ((table != nullptr) == bytes || !work || !aligned16(work)) return MI_BLUR_ERR_INVALID;
    if (!dist_args_ok(in, bytes ? (const void *)out : (const void *)table, W, H, C, n_images, &k, bytes, 16)) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const Tunables tun = tunables();
    const int band = tun.dist_band;
    const unsigned nbands = (unsigned)dist_bands(H, band);
    const long long wc = (long long)W * C, rows = (long long)n_images * H;
    const long long band_threads = (long long)n_images * nbands * wc, carry_threads = (long long)n_images * wc;
    if (!blocks_of(band_threads) || rows > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    DistColsParams pc{};
    pc.in = in; pc.g = static_cast<uint16_t *>(work);
    pc.carry = reinterpret_cast<uint16_t *>(static_cast<uint8_t *>(work) + dist_g_bytes(W, H, C, n_images));
    pc.wc = (unsigned)wc; pc.nbands = nbands; pc.H = H; pc.band = band; pc.nonzero = k.sites_nonzero; pc.cap = dist_cap(k.limit);
    pc.total = band_threads;
    if (const int rc = do_launch(blur_dist_bands_kernel, dim3(blocks_of(band_threads)), dim3(256), 0, stream, pc)) return rc;
    pc.total = carry_threads;
    if (const int rc = do_launch(blur_dist_carry_kernel, dim3(blocks_of(carry_threads)), dim3(256), 0, stream, pc)) return rc;
    pc.total = band_threads;
    if (const int rc = do_launch(blur_dist_cols_kernel, dim3(blocks_of(band_threads)), dim3(256), 0, stream, pc)) return rc;

    DistRowParams pr{};
    pr.g = pc.g; pr.table = table; pr.out = out; pr.rows = rows; pr.wc = (unsigned)wc; pr.W = W; pr.C = C;
    pr.metric = k.metric; pr.byte_op = k.byte_op; pr.invert = k.invert; pr.start = dist_start(k.metric, k.limit);
    pr.total = rows * wc;
    const int chunk = 1 << tun.dist_chunk_log2;
    const int rpg = dist_rows(W, C);
    const size_t lds = dist_lds_bytes(W, C, rpg, chunk);
    const long long groups = (rows + rpg - 1) / rpg;
    if (dist_tiled_ok(W, C) && (!bytes || aligned16(out)) && lds <= 65536 && groups <= 0x7fffffffLL) {
        pr.rpg = rpg; pr.nch = dist_chunks(W, chunk);
        set_last_kernel("blur_dist_tiled_kernel");
        const dim3 grid((unsigned)groups), block(DIST_THREADS);
        return dispatch<16, 8, 32>(chunk, [&](auto CH) {
            constexpr int ch = decltype(CH)::value;
            return bytes ? do_launch(blur_dist_tiled_kernel<ch, 1>, grid, block, lds, stream, pr) : do_launch(blur_dist_tiled_kernel<ch, 0>, grid, block, lds, stream, pr);
        });
    }
    set_last_kernel("blur_dist_generic_kernel");
    return bytes ? do_launch(blur_dist_generic_kernel<1>, byte_grid(pr.total), dim3(256), 0, stream, pr)
                 : do_launch(blur_dist_generic_kernel<0>, byte_grid(pr.total), dim3(256), 0, stream, pr);
}

}  // namespace mi_blur
