// clahe_kernels.hip — gfx950 kernels of CLAHE (include/mi_blur.h, "CLAHE"): the tile histograms and tile tables
// (mi_blur_enqueue_clahe_tables) and the look-up through the four tables around every pixel (mi_blur_enqueue_clahe_apply).
// Integers only; the arithmetic is clahe_edge(), clahe_bin(), clahe_entry(), clahe_axis() and bilinear_blend() of
// filter.h, which the host exports and the CPU device use too.
//
// blur_clahe_tables_tiled_kernel<C>: W a multiple of 16 and a 16-byte aligned input.  One workgroup of CLAHE_THREADS
// threads per (image, tile); blockIdx -> (image, tile) in the XCD-contiguous order for grids of 16 workgroups and more.
// The tile's rows are cut into the groups of 16 pixels that touch it (C chunks of 16 bytes each, aligned); a thread takes
// items t, t + CLAHE_THREADS, ... of (row, group).  A group that straddles a tile edge is read by both neighbours and
// masked per pixel.  Bins: one set of C x 256 uint32 counters PER WAVE in LDS, added to with ds_add_u32, with the
// histogram kernel's shortcuts for a group that lies inside the tile: a thread whose 16 pixels agree adds 16 once, and
// where a ballot shows that every active lane holds the same value one lane adds 16 x lanes.  Then tile_tables(): the
// waves' sets are summed, and thread v = bin v writes the raw histogram, adds what its bins hold over the clip to a
// counter per channel, takes its share of the excess back (closed form: no loop), and after a prefix sum over the bins
// (in LDS, 8 steps, all channels at once; a tile has fewer than 2^31 pixels, so 32 bits hold every sum) writes the
// tables' bytes.  No global atomic, no memset, no wait for another workgroup.
//
// blur_clahe_tables_generic_kernel: any shape and alignment; one byte per thread and step, one set of counters, the same
// tile_tables(); at most CLAHE_GENERIC_BLOCKS workgroups, which stride over the (image, tile) jobs.
//
// blur_clahe_apply_tiled_kernel<C>: the same rule with the output aligned too, and the LDS rule clahe_apply_tiled_ok().
// A workgroup owns, for one image, up to CLAHE_ROWS rows of one row class (the rows between two tile-row centres: both
// tile rows are constant there) and a span of CLAHE_SPAN pixels.  It stages the tables of both tile rows for the tile
// columns the span touches (two contiguous runs of d_tables; in LDS the tables lie CLAHE_LDS_TABLE = 260 bytes apart, so
// that lanes reading the same byte of different tiles' tables, as on a flat image, do not all hit one bank) and one entry
// per column of the span (the column's first table, whether the second is the next one, and fx) and per row (fy) in LDS.
// A thread takes items of (row, group of 16 pixels): C loads of 16 bytes, per byte four LDS byte look-ups and one blend,
// C stores of 16 bytes.
//
// blur_clahe_apply_generic_kernel: one byte per thread, grid-stride under byte_grid(), the tables read from device memory.
#include "kernel_common.h"

namespace mi_blur {

namespace {

constexpr int BINS = MI_BLUR_HIST_BINS;

struct ClaheTablesParams {
    const uint8_t *in;
    uint32_t *hist;                   // uint32[n][TY][TX][C][256]
    uint8_t *tables;                  // uint8[n][TY][TX][C][256]
    long long in_stride;              // bytes per image
    int W, H, channels, TX, TY;
    int clip_q8, mask;                // mask without the "0 = all" form
    unsigned nblocks;                 // the jobs, one per tile: n * TY * TX
    int xcd;
};

// A job's tile: its pixels [x0, x1) x [y0, y1) and its image.
struct ClaheTile {
    unsigned img;
    int x0, x1, y0, y1;
};
__device__ __forceinline__ ClaheTile clahe_tile(unsigned job, int W, int H, int TX, int TY)
{
    const unsigned per = (unsigned)(TX * TY);
    ClaheTile q;
    q.img = job / per;
    const unsigned tile = job - q.img * per, ty = tile / (unsigned)TX, tx = tile - ty * (unsigned)TX;
    q.x0 = clahe_edge(W, TX, (int)tx); q.x1 = clahe_edge(W, TX, (int)tx + 1);
    q.y0 = clahe_edge(H, TY, (int)ty); q.y1 = clahe_edge(H, TY, (int)ty + 1);
    return q;
}

// Thread v = bin v of a workgroup of CLAHE_THREADS: the tile's counts bins[C][256] (LDS, visible to all) -> its raw
// histogram and its tables.  scan = uint32[2][C][256], exc = uint32[C], both LDS.  Every thread calls it.
__device__ __forceinline__ void tile_tables(const uint32_t *bins, uint32_t *scan, uint32_t *exc, int C, uint32_t A, int clip_q8, int mask,
                                            uint32_t *hist_out, uint8_t *tab_out)
{
    const int v = threadIdx.x;
    const uint32_t clip = clahe_clip(A, clip_q8);
    if (v < C) exc[v] = 0;
    __syncthreads();
    for (int c = 0; c < C; c++) {
        const uint32_t h = bins[c * BINS + v];
        hist_out[c * BINS + v] = h;
        const uint32_t over = clahe_over(h, clip);
        if (over) atomicAdd(&exc[c], over);
    }
    __syncthreads();
    for (int c = 0; c < C; c++) scan[c * BINS + v] = clahe_bin(bins[c * BINS + v], clip, exc[c], v);
    __syncthreads();
    int b = 0;
    for (int d = 1; d < BINS; d <<= 1, b ^= 1) {          // 8 steps: the sums end in scan[0]
        for (int c = 0; c < C; c++) {
            uint32_t x = scan[(b * C + c) * BINS + v];
            if (v >= d) x += scan[(b * C + c) * BINS + v - d];
            scan[((b ^ 1) * C + c) * BINS + v] = x;
        }
        __syncthreads();
    }
    for (int c = 0; c < C; c++) tab_out[c * BINS + v] = (mask >> c) & 1 ? clahe_entry(scan[c * BINS + v], A) : (uint8_t)v;
}

template <int C>
__global__ __launch_bounds__(CLAHE_THREADS) void blur_clahe_tables_tiled_kernel(const ClaheTablesParams p)
{
    constexpr int WAVES = CLAHE_THREADS / 64;
    __shared__ uint32_t bins[WAVES * C * BINS];
    __shared__ uint32_t scan[2 * C * BINS];
    __shared__ uint32_t exc[C];
    const int t = threadIdx.x;
    for (int i = t; i < WAVES * C * BINS; i += CLAHE_THREADS) bins[i] = 0;
    __syncthreads();
    const unsigned job = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const ClaheTile q = clahe_tile(job, p.W, p.H, p.TX, p.TY);
    const uint8_t *src = p.in + (long long)q.img * p.in_stride;
    uint32_t *mine = bins + (t >> 6) * (C * BINS);
    const unsigned g0 = (unsigned)q.x0 / COLOR_GROUP, ngx = ((unsigned)q.x1 + COLOR_GROUP - 1) / COLOR_GROUP - g0;
    const unsigned items = ngx * (unsigned)(q.y1 - q.y0);                          // at most W * H / 16 + H

    for (unsigned i = (unsigned)t; i < items; i += CLAHE_THREADS) {
        const unsigned r = i / ngx, g = g0 + (i - r * ngx);
        const uint8_t *chunk = src + ((size_t)(q.y0 + (int)r) * p.W + (size_t)g * COLOR_GROUP) * C;
        uint32_t w[4 * C];
        load_group<C>(w, chunk, 0);
        const int px0 = (int)g * COLOR_GROUP;
        const bool full = px0 >= q.x0 && px0 + COLOR_GROUP <= q.x1;               // the whole group lies inside the tile
        const unsigned long long active = __ballot(1);
        const bool lead = (unsigned)(t & 63) == (unsigned)__builtin_ctzll(active);
#pragma unroll
        for (int c = 0; c < C; c++) {
            uint32_t v[COLOR_GROUP], diff = 0;
#pragma unroll
            for (int px = 0; px < COLOR_GROUP; px++) {
                v[px] = window_byte(w, px * C + c);
                diff |= v[px] ^ v[0];
            }
            uint32_t *b = mine + c * BINS;
            const uint32_t first_v = (uint32_t)__builtin_amdgcn_readfirstlane((int)v[0]);
            if (__ballot(full && diff == 0 && v[0] == first_v) == active) {       // the whole wave agrees: one add for all of it
                if (lead) atomicAdd(&b[first_v], (uint32_t)COLOR_GROUP * (uint32_t)__popcll(active));
            } else if (full && diff == 0) {                                        // this thread's 16 pixels agree
                atomicAdd(&b[v[0]], (uint32_t)COLOR_GROUP);
            } else {
#pragma unroll
                for (int px = 0; px < COLOR_GROUP; px++)
                    if (full || (px0 + px >= q.x0 && px0 + px < q.x1)) atomicAdd(&b[v[px]], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = t; i < C * BINS; i += CLAHE_THREADS) {                             // thread i owns counter i of every set
        uint32_t s = 0;
#pragma unroll
        for (int wv = 0; wv < WAVES; wv++) s += bins[wv * (C * BINS) + i];
        bins[i] = s;
    }
    __syncthreads();
    const uint32_t A = (uint32_t)(q.x1 - q.x0) * (uint32_t)(q.y1 - q.y0);
    tile_tables(bins, scan, exc, C, A, p.clip_q8, p.mask, p.hist + (size_t)job * (C * BINS), p.tables + (size_t)job * (C * BINS));
}

__global__ __launch_bounds__(CLAHE_THREADS) void blur_clahe_tables_generic_kernel(const ClaheTablesParams p)
{
    __shared__ uint32_t bins[MI_BLUR_COLOR_MAX_CHANNELS * BINS];
    __shared__ uint32_t scan[2 * MI_BLUR_COLOR_MAX_CHANNELS * BINS];
    __shared__ uint32_t exc[MI_BLUR_COLOR_MAX_CHANNELS];
    const int t = threadIdx.x, C = p.channels;
    const unsigned pitch = (unsigned)(p.W * C);
    for (unsigned job = blockIdx.x; job < p.nblocks; job += gridDim.x) {
        for (int i = t; i < C * BINS; i += CLAHE_THREADS) bins[i] = 0;
        __syncthreads();
        const ClaheTile q = clahe_tile(job, p.W, p.H, p.TX, p.TY);
        const uint8_t *src = p.in + (long long)q.img * p.in_stride + ((size_t)q.y0 * p.W + (size_t)q.x0) * C;
        const unsigned rowb = (unsigned)(q.x1 - q.x0) * (unsigned)C, total = rowb * (unsigned)(q.y1 - q.y0);    // bytes of the tile: <= INT_MAX
        for (unsigned i = (unsigned)t; i < total; i += CLAHE_THREADS) {
            const unsigned r = i / rowb, b = i - r * rowb;
            atomicAdd(&bins[(b % (unsigned)C) * BINS + src[(size_t)r * pitch + b]], 1u);
        }
        __syncthreads();
        const uint32_t A = (uint32_t)(q.x1 - q.x0) * (uint32_t)(q.y1 - q.y0);
        tile_tables(bins, scan, exc, C, A, p.clip_q8, p.mask, p.hist + (size_t)job * (C * BINS), p.tables + (size_t)job * (C * BINS));
        __syncthreads();
    }
}

struct ClaheApplyParams {
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *tables;            // uint8[n][TY][TX][C][256], any alignment
    long long stride;                 // bytes per image, in and out
    int W, H, TX, TY;
    int nspans, slices;               // spans of CLAHE_SPAN pixels of a row; slices of up to CLAHE_ROWS rows of an image
    int max_cols;                     // the most tile columns a span needs: the LDS holds 2 * max_cols * C tables
    unsigned nblocks;
    int xcd;
};

// An entry of a span's column: fx, whether t1 = t0 + 1, and t0 counted from the span's first tile column.
constexpr int XENT_STEP_BIT = 11, XENT_COL_SHIFT = 12;

extern __shared__ __attribute__((aligned(16))) uint8_t clahe_lds[];

template <int C>
__global__ __launch_bounds__(CLAHE_THREADS) void blur_clahe_apply_tiled_kernel(const ClaheApplyParams p)
{
    const int t = threadIdx.x;
    // blockIdx -> (image, slice of rows, span): spans fastest
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const int span = (int)(L % (unsigned)p.nspans);
    const unsigned u = L / (unsigned)p.nspans;
    const unsigned img = u / (unsigned)p.slices;
    int s = (int)(u - img * (unsigned)p.slices);
    // the slice's row class k and its rows [lo, hi): clahe_slices() counted the same way, so the slice exists
    int k = 0, lo = 0, hi = clahe_class_lo(p.H, p.TY, 1);
    for (; k < p.TY; k++, lo = hi, hi = clahe_class_lo(p.H, p.TY, k + 1)) {
        const int ns = (hi - lo + CLAHE_ROWS - 1) / CLAHE_ROWS;
        if (s < ns) break;
        s -= ns;
    }
    lo += s * CLAHE_ROWS;
    if (lo >= hi) return;                                                        // the whole workgroup: nothing was shared yet
    hi = min(hi, lo + CLAHE_ROWS);
    const int ty0 = max(k - 1, 0), ty1 = min(k, p.TY - 1);
    const int xa = span * CLAHE_SPAN, xb = min(xa + CLAHE_SPAN, p.W) - 1;       // the span's pixels [xa, xb]
    int ta, tb, unused, f;
    clahe_axis(p.W, p.TX, xa, ta, unused, f);
    clahe_axis(p.W, p.TX, xb, unused, tb, f);
    const int ntab = (tb - ta + 1) * C;                                          // tables of one tile row: <= max_cols * C
    const int rowbytes = ntab * CLAHE_LDS_TABLE;

    uint8_t *lut = clahe_lds;                                                    // [2][ntab] tables, CLAHE_LDS_TABLE bytes apart
    uint32_t *xent = reinterpret_cast<uint32_t *>(clahe_lds + clahe_apply_lds_tables(p.max_cols, C));
    uint32_t *yent = xent + CLAHE_SPAN;
    const uint8_t *tab = p.tables + (size_t)img * p.TY * p.TX * (C * BINS);
    const uint8_t *s0 = tab + ((size_t)ty0 * p.TX + ta) * (C * BINS), *s1 = tab + ((size_t)ty1 * p.TX + ta) * (C * BINS);
    if ((uintptr_t)p.tables % 4 == 0) {                                          // every table starts at a multiple of 256
        uint32_t *l0 = reinterpret_cast<uint32_t *>(lut), *l1 = reinterpret_cast<uint32_t *>(lut + rowbytes);
        for (int i = t; i < ntab * (BINS / 4); i += CLAHE_THREADS) {
            const int at = (i / (BINS / 4)) * (CLAHE_LDS_TABLE / 4) + i % (BINS / 4);
            l0[at] = reinterpret_cast<const uint32_t *>(s0)[i];
            l1[at] = reinterpret_cast<const uint32_t *>(s1)[i];
        }
    } else {
        for (int i = t; i < ntab * BINS; i += CLAHE_THREADS) {
            const int at = (i / BINS) * CLAHE_LDS_TABLE + i % BINS;
            lut[at] = s0[i];
            lut[rowbytes + at] = s1[i];
        }
    }
    if (xa + t <= xb) {
        int t0, t1, fx;
        clahe_axis(p.W, p.TX, xa + t, t0, t1, fx);
        xent[t] = (uint32_t)fx | (uint32_t)(t1 - t0) << XENT_STEP_BIT | (uint32_t)(t0 - ta) << XENT_COL_SHIFT;
    }
    if (t < hi - lo) {
        int t0, t1, fy;
        clahe_axis(p.H, p.TY, lo + t, t0, t1, fy);
        yent[t] = (uint32_t)fy;
    }
    __syncthreads();

    const int ng = (xb - xa + 1) / COLOR_GROUP, items = (hi - lo) * (CLAHE_SPAN / COLOR_GROUP);
    const uint8_t *src = p.in + (long long)img * p.stride;
    uint8_t *dst = p.out + (long long)img * p.stride;
    for (int i = t; i < items; i += CLAHE_THREADS) {
        const int r = i / (CLAHE_SPAN / COLOR_GROUP), g = i % (CLAHE_SPAN / COLOR_GROUP);
        if (g >= ng) continue;                                                   // the last span of a row may be short
        const size_t at = ((size_t)(lo + r) * p.W + (size_t)(xa + g * COLOR_GROUP)) * C;
        uint32_t w[4 * C], o[4 * C], e[COLOR_GROUP];
        load_group<C>(w, src + at, 0);
#pragma unroll
        for (int j = 0; j < COLOR_GROUP / 4; j++) {
            const uint4 v = reinterpret_cast<const uint4 *>(xent + g * COLOR_GROUP)[j];
            e[4 * j] = v.x; e[4 * j + 1] = v.y; e[4 * j + 2] = v.z; e[4 * j + 3] = v.w;
        }
        const unsigned fy = yent[r];
#pragma unroll
        for (int j = 0; j < 4 * C; j++) o[j] = 0;
#pragma unroll
        for (int j = 0; j < COLOR_GROUP * C; j++) {
            const int px = j / C, c = j % C;
            const unsigned fx = e[px] & (BLEND_ONE - 1u);
            const int next = (int)((e[px] >> XENT_STEP_BIT) & 1u) * (C * CLAHE_LDS_TABLE);
            const uint8_t *b0 = lut + ((int)(e[px] >> XENT_COL_SHIFT) * C + c) * CLAHE_LDS_TABLE + (int)window_byte(w, j);
            const unsigned q = bilinear_blend(b0[0], b0[next], b0[rowbytes], b0[rowbytes + next], fx, fy);
            o[j >> 2] |= q << (8 * (j & 3));
        }
        store_group<C>(o, dst + at, 0);
    }
}

struct ClaheApplyGenericParams {
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *tables;
    long long bytes, total;           // bytes per image, bytes of the launch
    int W, H, channels, TX, TY;
};

__global__ __launch_bounds__(256) void blur_clahe_apply_generic_kernel(const ClaheApplyGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    const unsigned C = (unsigned)p.channels, pitch = (unsigned)p.W * C;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const long long img = idx / p.bytes;
        const unsigned rem = (unsigned)(idx - img * p.bytes), y = rem / pitch, b = rem - y * pitch, x = b / C, c = b - x * C;
        int tx0, tx1, fx, ty0, ty1, fy;
        clahe_axis(p.W, p.TX, (int)x, tx0, tx1, fx);
        clahe_axis(p.H, p.TY, (int)y, ty0, ty1, fy);
        const uint8_t *tab = p.tables + ((size_t)img * p.TY * p.TX * C + c) * BINS + p.in[idx];
        const size_t tile = (size_t)C * BINS, r0 = (size_t)ty0 * p.TX * tile, r1 = (size_t)ty1 * p.TX * tile;
        p.out[idx] = (uint8_t)bilinear_blend(tab[r0 + tx0 * tile], tab[r0 + tx1 * tile], tab[r1 + tx0 * tile], tab[r1 + tx1 * tile],
                                             (unsigned)fx, (unsigned)fy);
    }
}

}  // namespace

int launch_clahe_tables(const uint8_t *in, uint32_t *hist, uint8_t *tables, int W, int H, int C, int n_images, const mi_blur_clahe &k,
                        hipStream_t stream)
{
    if (!in || !hist || !tables || !aligned16(hist) || !hist_image_ok(W, H, C) || !clahe_ok(&k, W, H, C) || n_images < 0) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    ClaheTablesParams p{};
    if (const int st = fill_flat(p, n_images, (long long)k.tiles_y * k.tiles_x)) return st;       // the generic kernel does not read p.xcd
    p.in = in; p.hist = hist; p.tables = tables; p.in_stride = (long long)W * H * C;
    p.W = W; p.H = H; p.channels = C; p.TX = k.tiles_x; p.TY = k.tiles_y;
    p.clip_q8 = k.clip_q8; p.mask = tone_mask(k.channel_mask, C);
    if (clahe_tiled_ok(W) && aligned16(in)) {
        set_last_kernel("blur_clahe_tables_tiled_kernel");
        return dispatch<1, 2, 3, 4>(C, [&](auto CC) {
            return do_launch(blur_clahe_tables_tiled_kernel<CC>, dim3(p.nblocks), dim3(CLAHE_THREADS), 0, stream, p);
        });
    }
    set_last_kernel("blur_clahe_tables_generic_kernel");
    const unsigned blocks = p.nblocks > (unsigned)CLAHE_GENERIC_BLOCKS ? (unsigned)CLAHE_GENERIC_BLOCKS : p.nblocks;
    return do_launch(blur_clahe_tables_generic_kernel, dim3(blocks), dim3(CLAHE_THREADS), 0, stream, p);
}

int launch_clahe_apply(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_clahe &k, const uint8_t *tables,
                       hipStream_t stream)
{
    if (!in || !out || in == out || !tables || !hist_image_ok(W, H, C) || !clahe_ok(&k, W, H, C) || n_images < 0) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const long long bytes = (long long)W * H * C;
    if (aligned16(in) && aligned16(out) && clahe_apply_tiled_ok(W, k.tiles_x, C)) {
        ClaheApplyParams p{};
        p.in = in; p.out = out; p.tables = tables; p.stride = bytes;
        p.W = W; p.H = H; p.TX = k.tiles_x; p.TY = k.tiles_y;
        p.nspans = clahe_spans(W); p.slices = clahe_slices(H, k.tiles_y);
        p.max_cols = clahe_span_cols(W, k.tiles_x);
        if (const int st = fill_flat(p, n_images, (long long)p.slices * p.nspans)) return st;
        const size_t lds = clahe_apply_lds_tables(p.max_cols, C) + (size_t)(CLAHE_SPAN + CLAHE_ROWS) * sizeof(uint32_t);
        set_last_kernel("blur_clahe_apply_tiled_kernel");
        return dispatch<1, 2, 3, 4>(C, [&](auto CC) {
            return do_launch(blur_clahe_apply_tiled_kernel<CC>, dim3(p.nblocks), dim3(CLAHE_THREADS), lds, stream, p);
        });
    }
    ClaheApplyGenericParams p{};
    p.in = in; p.out = out; p.tables = tables; p.bytes = bytes; p.total = bytes * n_images;
    p.W = W; p.H = H; p.channels = C; p.TX = k.tiles_x; p.TY = k.tiles_y;
    set_last_kernel("blur_clahe_apply_generic_kernel");
    return do_launch(blur_clahe_apply_generic_kernel, byte_grid(p.total), dim3(256), 0, stream, p);
}

}  // namespace mi_blur
