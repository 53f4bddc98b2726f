// hist_kernels.hip — gfx950 kernels of the histogram family (include/mi_blur.h, "Histogram, and tone tables made from
// it"): the per-image, per-channel histogram (mi_blur_enqueue_hist), the tone tables made from it on the device
// (blur_tone_table_kernel, inside mi_blur_enqueue_tone) and the look-up through one table per image and channel
// (mi_blur_enqueue_tables).  Integers only, no counter narrower than 32 bits; the tables' arithmetic is tone_entry() and
// its predicates (filter.h), which the host export and the CPU device use too.
//
// blur_hist_tiled_kernel<C>: the colour kernel's flat rule (W * H a multiple of 16, a 16-byte aligned input).  A
// workgroup of HIST_THREADS threads owns a run of HIST_RUN consecutive groups of 16 pixels of one image (an image of more
// than HIST_IMAGE_BLOCKS runs has that many workgroups, each taking every HIST_IMAGE_BLOCKS-th run: the flushes of one
// image all land on the same C KiB, and that row takes them one after the other); blockIdx -> (image, workgroup) in the
// XCD-contiguous order for grids of 16 workgroups and more.  A thread takes groups t, t + HIST_THREADS, ... of the run:
// C loads of 16 bytes, byte j of the group belonging to channel j % C (a compile-time pick).  Bins: one set
// of C x 256 uint32 counters PER WAVE in LDS (4 C KiB), added to with ds_add_u32.  Flat data is the hard case (64 lanes
// adding to one counter serialise), so per channel a thread first looks whether its 16 pixels agree: then it adds 16
// once, and where a ballot shows that every active lane of the wave holds the same value one lane adds 16 x lanes.
// At the end of the run the workgroup sums the waves' sets and adds the non-zero counters to hist[image][c][v] with
// atomicAdd: thread t takes counters t, t + 256, ..., so a wave's adds are 256 contiguous bytes.  The output is zeroed
// on the stream before the launch.  No scratch.
//
// blur_hist_generic_kernel: any shape and alignment; a workgroup takes every parts-th stretch of 256 bytes of one image,
// one byte per thread and step, one set of counters, the same flush.
//
// blur_tone_table_kernel: one workgroup of 256 threads per table (per image and channel, or per image when joint), thread
// v = bin v: a 64-bit prefix sum over the bins in LDS, lo and hi as counts of the predicates across the workgroup, then tone_entry().
//
// blur_tables_tiled_kernel<C>: the flat rule with both pointers aligned and the runs of the histogram kernel, one
// workgroup per run; the image's C x 256 table goes to LDS once per workgroup, a thread's group is C loads of 16 bytes, 16 C byte look-ups and C stores.  blur_tables_generic_kernel: one
// byte per thread, the table read from device memory.
#include "kernel_common.h"

namespace mi_blur {

namespace {

constexpr int BINS = MI_BLUR_HIST_BINS;

struct HistTiledParams {
    const uint8_t *in;
    uint32_t *hist;
    long long in_stride;              // bytes per image
    unsigned groups, runs;            // groups of 16 pixels and runs of HIST_RUN groups per image
    unsigned per_image;               // workgroups per image: min(runs, HIST_IMAGE_BLOCKS)
    unsigned nblocks;
    int xcd;
};

template <int C>
__global__ __launch_bounds__(HIST_THREADS) void blur_hist_tiled_kernel(const HistTiledParams p)
{
    constexpr int WAVES = HIST_THREADS / 64;
    __shared__ uint32_t bins[WAVES * C * BINS];
    const int t = threadIdx.x;
    for (int i = t; i < WAVES * C * BINS; i += HIST_THREADS) bins[i] = 0;
    __syncthreads();
    // blockIdx -> (image, workgroup of the image): workgroups fastest, then images
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const unsigned img = L / p.per_image, first = L - img * p.per_image;
    const uint8_t *src = p.in + (long long)img * p.in_stride;
    uint32_t *mine = bins + (t >> 6) * (C * BINS);

    for (unsigned run = first; run < p.runs; run += p.per_image) {      // one run, or every per_image-th of a large image
        const unsigned g0 = run * HIST_RUN, g1 = min(g0 + (unsigned)HIST_RUN, p.groups);   // the last run of an image may be short
        for (unsigned g = g0 + (unsigned)t; g < g1; g += HIST_THREADS) {
            uint32_t w[4 * C];
            load_group<C>(w, src, g);
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
                if (__ballot(diff == 0 && v[0] == first_v) == active) {    // the whole wave agrees: one add for all of it
                    if (lead) atomicAdd(&b[first_v], (uint32_t)COLOR_GROUP * (uint32_t)__popcll(active));
                } else if (diff == 0) {                                    // this thread's 16 pixels agree
                    atomicAdd(&b[v[0]], (uint32_t)COLOR_GROUP);
                } else {
#pragma unroll
                    for (int px = 0; px < COLOR_GROUP; px++) atomicAdd(&b[v[px]], 1u);
                }
            }
        }
    }
    __syncthreads();
    uint32_t *dst = p.hist + (size_t)img * (C * BINS);
    for (int i = t; i < C * BINS; i += HIST_THREADS) {
        uint32_t s = 0;
#pragma unroll
        for (int wv = 0; wv < WAVES; wv++) s += bins[wv * (C * BINS) + i];
        if (s) atomicAdd(dst + i, s);
    }
}

struct HistGenericParams {
    const uint8_t *in;
    uint32_t *hist;
    long long in_stride;              // bytes per image
    unsigned bytes, parts;            // bytes per image (<= INT_MAX); workgroups per image
    int channels;
};

__global__ __launch_bounds__(HIST_THREADS) void blur_hist_generic_kernel(const HistGenericParams p)
{
    __shared__ uint32_t bins[MI_BLUR_COLOR_MAX_CHANNELS * BINS];
    const int t = threadIdx.x;
    for (int i = t; i < MI_BLUR_COLOR_MAX_CHANNELS * BINS; i += HIST_THREADS) bins[i] = 0;
    __syncthreads();
    const unsigned img = blockIdx.x / p.parts, part = blockIdx.x - img * p.parts;
    const uint8_t *src = p.in + (long long)img * p.in_stride;
    const unsigned C = (unsigned)p.channels, step = p.parts * HIST_THREADS;          // bytes + step < 2^32: parts <= 256
    for (unsigned idx = part * HIST_THREADS + (unsigned)t; idx < p.bytes; idx += step) atomicAdd(&bins[(idx % C) * BINS + src[idx]], 1u);
    __syncthreads();
    uint32_t *dst = p.hist + (size_t)img * (C * BINS);
    for (unsigned i = (unsigned)t; i < C * BINS; i += HIST_THREADS)
        if (bins[i]) atomicAdd(dst + i, bins[i]);
}

struct ToneTableParams {
    const uint32_t *hist;             // uint32[n][C][256]
    uint8_t *tables;                  // uint8[n][C][256]
    int channels;
    int mode, clip_lo, clip_hi, joint, mask;   // a valid mi_blur_tone; mask without the "0 = all" form
};

__global__ __launch_bounds__(BINS) void blur_tone_table_kernel(const ToneTableParams p)
{
    __shared__ uint64_t scan[2][BINS];
    const int v = threadIdx.x, C = p.channels;
    const int jobs = p.joint ? 1 : C;                   // a job = one table: of channel j, or the joint one
    const int img = (int)blockIdx.x / jobs, j = (int)blockIdx.x - img * jobs;
    const uint32_t *hist = p.hist + (size_t)img * (C * BINS);
    uint8_t *tab = p.tables + (size_t)img * (C * BINS);
    const int takes = p.joint ? p.mask : 1 << j;        // the channels that get this job's table
    if (!(takes & p.mask)) {                            // a channel that is not transformed: the identity
        tab[j * BINS + v] = (uint8_t)v;
        return;
    }
    uint64_t h = 0;
    for (int c = 0; c < C; c++)
        if ((takes >> c) & 1) h += hist[c * BINS + v];
    scan[0][v] = h;
    __syncthreads();
    int b = 0;
    for (int d = 1; d < BINS; d <<= 1, b ^= 1) {        // 8 steps: the sums end in scan[0]
        uint64_t x = scan[b][v];
        if (v >= d) x += scan[b][v - d];
        scan[b ^ 1][v] = x;
        __syncthreads();
    }
    const uint64_t cv = scan[0][v], c_prev = v ? scan[0][v - 1] : 0, N = scan[0][BINS - 1];
    uint8_t e = (uint8_t)v;
    if (N) {
        const int lo = __syncthreads_count(tone_below_lo(cv, tone_clip_count(N, p.clip_lo)));
        const int hi = __syncthreads_count(tone_upto_hi(N, c_prev, tone_clip_count(N, p.clip_hi))) - 1;
        e = tone_entry(p.mode, v, cv, N, lo, hi, scan[0][lo]);
    }
    for (int c = 0; c < C; c++)
        if (p.joint) tab[c * BINS + v] = (takes >> c) & 1 ? e : (uint8_t)v;
        else if (c == j) tab[c * BINS + v] = e;
}

struct TablesTiledParams {
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *tables;            // uint8[n][C][256]
    long long stride;                 // bytes per image, in and out
    unsigned groups, runs;
    unsigned nblocks;
    int xcd;
};

template <int C>
__global__ __launch_bounds__(HIST_THREADS) void blur_tables_tiled_kernel(const TablesTiledParams p)
{
    __shared__ uint32_t lut_w[C * BINS / 4];
    uint8_t *lut = reinterpret_cast<uint8_t *>(lut_w);
    const int t = threadIdx.x;
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const unsigned img = L / p.runs, run = L - img * p.runs;
    const uint8_t *tab = p.tables + (size_t)img * (C * BINS);
    for (int i = t; i < C * BINS; i += HIST_THREADS) lut[i] = tab[i];
    __syncthreads();
    const unsigned g0 = run * HIST_RUN, g1 = min(g0 + (unsigned)HIST_RUN, p.groups);
    const uint8_t *src = p.in + (long long)img * p.stride;
    uint8_t *out = p.out + (long long)img * p.stride;
    for (unsigned g = g0 + (unsigned)t; g < g1; g += HIST_THREADS) {
        uint32_t w[4 * C], r[4 * C];
        load_group<C>(w, src, g);
#pragma unroll
        for (int q = 0; q < 4 * C; q++) r[q] = 0;
#pragma unroll
        for (int j = 0; j < 16 * C; j++) r[j >> 2] |= (uint32_t)lut[(j % C) * BINS + (int)window_byte(w, j)] << (8 * (j & 3));
        store_group<C>(r, out, g);
    }
}

struct TablesGenericParams {
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *tables;
    long long bytes, total;           // bytes per image, bytes of the launch
    int channels;
};

__global__ __launch_bounds__(256) void blur_tables_generic_kernel(const TablesGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const long long img = idx / p.bytes;
        const unsigned c = (unsigned)(idx - img * p.bytes) % (unsigned)p.channels;
        p.out[idx] = p.tables[(img * p.channels + c) * BINS + p.in[idx]];
    }
}

// The groups and runs of an image and the flat grid of the two tiled kernels, per_image workgroups an image.
template <typename P>
int fill_runs(P &p, int W, int H, int n_images, unsigned per_image)
{
    p.groups = (unsigned)((long long)W * H / COLOR_GROUP);
    p.runs = (unsigned)hist_runs(W, H);
    return fill_flat(p, n_images, per_image);
}

}  // namespace

int launch_hist(const uint8_t *in, uint32_t *hist, int W, int H, int C, int n_images, hipStream_t stream)
{
    if (!in || !hist || !aligned16(hist) || !hist_image_ok(W, H, C) || n_images < 0) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const long long bytes = (long long)W * H * C;
    if (const hipError_t e = hipMemsetAsync(hist, 0, (size_t)n_images * C * BINS * sizeof(uint32_t), stream)) {
        (void)hipGetLastError();
        return hip_status(e);
    }
    if (color_flat_ok(W, H) && aligned16(in)) {
        HistTiledParams p{};
        p.in = in; p.hist = hist; p.in_stride = bytes;
        p.per_image = (unsigned)hist_blocks(W, H);
        if (const int st = fill_runs(p, W, H, n_images, p.per_image)) return st;
        set_last_kernel("blur_hist_tiled_kernel");
        return dispatch<1, 2, 3, 4>(C, [&](auto CC) {
            return do_launch(blur_hist_tiled_kernel<CC>, dim3(p.nblocks), dim3(HIST_THREADS), 0, stream, p);
        });
    }
    HistGenericParams p{};
    p.in = in; p.hist = hist; p.in_stride = bytes; p.bytes = (unsigned)bytes; p.channels = C;
    const long long parts = (bytes + 64 * HIST_THREADS - 1) / (64 * HIST_THREADS);      // about 64 bytes per thread
    p.parts = (unsigned)(parts > 256 ? 256 : parts);
    if ((long long)n_images * p.parts > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    set_last_kernel("blur_hist_generic_kernel");
    return do_launch(blur_hist_generic_kernel, dim3((unsigned)n_images * p.parts), dim3(HIST_THREADS), 0, stream, p);
}

int launch_tone_tables(const uint32_t *hist, uint8_t *tables, int C, int n_images, const mi_blur_tone &t, hipStream_t stream)
{
    if (!hist || !tables || !tone_ok(&t, C) || n_images < 0) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    ToneTableParams p{};
    p.hist = hist; p.tables = tables; p.channels = C;
    p.mode = t.mode; p.clip_lo = t.clip_lo; p.clip_hi = t.clip_hi; p.joint = t.joint; p.mask = tone_mask(t.channel_mask, C);
    set_last_kernel("blur_tone_table_kernel");
    const long long nblocks = (long long)n_images * (t.joint ? 1 : C);
    if (nblocks > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    return do_launch(blur_tone_table_kernel, dim3((unsigned)nblocks), dim3(BINS), 0, stream, p);
}

int launch_tables(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const uint8_t *tables, hipStream_t stream)
{
    if (!in || !out || in == out || !tables || !hist_image_ok(W, H, C) || n_images < 0) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const long long bytes = (long long)W * H * C;
    if (color_flat_ok(W, H) && aligned16(in) && aligned16(out)) {
        TablesTiledParams p{};
        p.in = in; p.out = out; p.tables = tables; p.stride = bytes;
        if (const int st = fill_runs(p, W, H, n_images, (unsigned)hist_runs(W, H))) return st;
        set_last_kernel("blur_tables_tiled_kernel");
        return dispatch<1, 2, 3, 4>(C, [&](auto CC) {
            return do_launch(blur_tables_tiled_kernel<CC>, dim3(p.nblocks), dim3(HIST_THREADS), 0, stream, p);
        });
    }
    TablesGenericParams p{};
    p.in = in; p.out = out; p.tables = tables; p.bytes = bytes; p.total = bytes * n_images; p.channels = C;
    set_last_kernel("blur_tables_generic_kernel");
    return do_launch(blur_tables_generic_kernel, byte_grid(p.total), dim3(256), 0, stream, p);
}

}  // namespace mi_blur
