// match_kernels.hip — gfx950 kernels of template matching and of the peak search (include/mi_blur.h, "Template matching
// and peak search"): mi_blur_enqueue_match and mi_blur_enqueue_match_peak.  Integers only; a score is match_score()
// (filter.h), which the host export and the CPU device use too.  No workgroup here ever waits for another.
//
// blur_match_prep_kernel: one workgroup per template: its rows zero-padded to MATCH_ROW_PAD bytes (what the tiled kernel
//   reads) and its sums (sum_t, sum_tt), into the work buffer.
// blur_match_tiled_kernel<METHOD> (SQDIFF, CCORR, SAD; aligned images, rows of whole 16-byte chunks): a row is W * C
//   bytes and a template row tw * C bytes, output x starts at byte x * C, so the channels are summed for nothing.  A
//   workgroup owns MATCH_TX x MATCH_TY outputs: a lane owns a column, a wave MATCH_R consecutive output rows.  The input
//   rows of a band of template rows are staged in LDS (stage_box); a thread forms four input bytes at its byte offset from
//   two LDS dwords (v_alignbyte_b32), four dwords at a time, and every such dword serves its MATCH_R output rows against
//   MATCH_R template rows: CCORR one v_dot4_u32_u8, SAD one v_sad_u8, SQDIFF two dot products (a t and a a).  The
//   template's dwords are uniform across a wave: scalar loads of the padded template.  The dwords past a template row's
//   last byte are masked out of the input, so SAD and sum a^2 see nothing there.
// blur_match_generic_kernel: one output entry per thread, plain loops, any shape and alignment, every raw method.
// blur_match_score_kernel: one entry per thread: the window's sum_a and sum_aa from four reads of S and of Q per channel
//   (the -1 indices guarded), sum_at from the CCORR table, the template's sums, match_score().
// blur_match_peak_kernel / blur_match_peak_final_kernel: MI_BLUR_MATCH_PEAK_PARTS workgroups per image reduce their
//   share of the table to a minimum key (value << 32 | index) and a maximum key (value << 32 | ~index), one workgroup per
//   image reduces those and decodes.  The first entry in row-major order wins a tie by construction.
#include "kernel_common.h"

#include <algorithm>

namespace mi_blur {

namespace {

struct MatchPrepParams {
    const uint8_t *t;
    uint32_t *sums;                   // [templates][4]
    uint8_t *pad;                     // [templates][th][row_pad]
    int tb, th, row_pad;              // bytes of a template row, rows, bytes of a padded row
};

__global__ __launch_bounds__(256) void blur_match_prep_kernel(const MatchPrepParams p)
{
    __shared__ uint32_t part[2][4];
    const uint8_t *src = p.t + (size_t)blockIdx.x * p.th * p.tb;
    uint8_t *dst = p.pad + (size_t)blockIdx.x * p.th * p.row_pad;
    uint32_t s = 0, q = 0;
    const int total = p.th * p.row_pad;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int row = i / p.row_pad, b = i - row * p.row_pad;
        const uint32_t v = b < p.tb ? src[row * p.tb + b] : 0u;
        dst[i] = (uint8_t)v;
        s += v;
        q += v * v;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        s += __shfl_down(s, d);
        q += __shfl_down(q, d);
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = s; part[1][threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t *o = p.sums + (size_t)blockIdx.x * 4;
        o[0] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        o[1] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        o[2] = 0;
        o[3] = 0;
    }
}

struct MatchParams {
    const uint8_t *in, *t;            // t: the templates as given (generic) or zero-padded (tiled)
    const uint32_t *sums;             // tiled SQDIFF: [templates][4]
    uint32_t *out;
    int W, H, C, tw, th, Wo, Ho;
    int method, t_shared;
    int tb, row_pad;                  // bytes of a template row, of a padded one
    int tiles_x, tiles_y;
    long long total;                  // generic: entries
};

__global__ __launch_bounds__(256) void blur_match_generic_kernel(const MatchParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    const long long image_e = (long long)p.Wo * p.Ho;
    const size_t row_e = (size_t)p.W * p.C;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const long long img = idx / image_e, rem = idx - img * image_e;
        const int y = (int)(rem / p.Wo), x = (int)(rem - (long long)y * p.Wo);
        const uint8_t *a = p.in + ((size_t)img * p.H + y) * row_e + (size_t)x * p.C;
        const uint8_t *t = p.t + (p.t_shared ? 0 : (size_t)img * p.th * p.tb);
        uint32_t acc = 0;
        for (int dy = 0; dy < p.th; dy++, a += row_e, t += p.tb)
            for (int b = 0; b < p.tb; b++) {
                const int av = a[b], tv = t[b], d = av - tv;
                acc += p.method == MI_BLUR_MATCH_CCORR ? (uint32_t)(av * tv) : p.method == MI_BLUR_MATCH_SQDIFF ? (uint32_t)(d * d) : (uint32_t)(d < 0 ? -d : d);
            }
        p.out[idx] = acc;
    }
}

template <int METHOD>
__global__ __launch_bounds__(MATCH_THREADS) void blur_match_tiled_kernel(const MatchParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t tile[];
    constexpr int R = MATCH_R;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const unsigned tile_x = blockIdx.x % (unsigned)p.tiles_x, t2 = blockIdx.x / (unsigned)p.tiles_x;
    const unsigned tile_y = t2 % (unsigned)p.tiles_y, img = t2 / (unsigned)p.tiles_y;
    const int x0 = (int)tile_x * MATCH_TX, ty0 = (int)tile_y * MATCH_TY;
    const int pitch = p.W * p.C, cpr = pitch / 16;
    // The staged columns: from the chunk of the tile's first byte to the one of the last byte any lane reads, in the row.
    const int c0 = x0 * p.C / 16;
    const int last = (x0 + MATCH_TX - 1) * p.C + p.row_pad + 4;         // one byte past the last one read
    const int nsc = min((last + 15) / 16, cpr) - c0;
    const int lpitch = nsc * 16;
    const int rows_fit = MATCH_LDS_BYTES / lpitch;                      // >= MATCH_TY: lpitch <= 1 328
    const int band = min(p.th, rows_fit - (MATCH_TY - 1));
    const uint8_t *img_in = p.in + (size_t)img * p.H * pitch;
    const uint8_t *tp = p.t + (p.t_shared ? 0 : (size_t)img * p.th * p.row_pad);
    const int x = x0 + lane;
    const int off = min(x, p.Wo - 1) * p.C - c0 * 16;                   // the lane's first byte of a staged row; lanes past the last output read its bytes
    const int sh = off & 3;
    const int tdw = (p.tb + 3) / 4;                                     // dwords of a template row that hold bytes
    const uint32_t tail_mask = (p.tb & 3) ? (1u << (8 * (p.tb & 3))) - 1u : 0xffffffffu;
    const int npd = p.row_pad / 4;

    uint32_t acc[R], acc2[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = acc2[r] = 0;

    for (int dy0 = 0; dy0 < p.th; dy0 += band) {
        const int nb = min(band, p.th - dy0);                           // template rows of this band
        const int first = ty0 + dy0;                                    // image row of staged row 0
        const int nsr = min(nb + MATCH_TY - 1, p.H - first);
        if (dy0) __syncthreads();
        stage_box(tile, img_in + (size_t)first * pitch + (size_t)c0 * 16, pitch, nsr, nsc, t);
        __syncthreads();
        // Staged row wave * R + ir is the input row of output row r against template row dy0 + ir - r.
        for (int ir = 0; ir < nb + R - 1; ir++) {
            const int srow = wave * R + ir;
            if (srow >= nsr) break;                                     // rows below the image: outputs that do not exist
            const uint32_t *lrow = reinterpret_cast<const uint32_t *>(tile + srow * lpitch + (off & ~3));
            for (int j0 = 0; j0 < npd; j0 += 4) {
                uint32_t w[5], a[4];
#pragma unroll
                for (int j = 0; j < 5; j++) w[j] = lrow[j0 + j];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int jj = j0 + j;
                    const uint32_t m = jj < tdw - 1 ? 0xffffffffu : jj == tdw - 1 ? tail_mask : 0u;
                    a[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], (uint32_t)sh) & m;
                }
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int dyr = ir - r;
                    if (dyr < 0 || dyr >= nb) continue;                 // uniform across the wave
                    const uint32_t *trow = reinterpret_cast<const uint32_t *>(tp + (size_t)(dy0 + dyr) * p.row_pad) + j0;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t tv = trow[j];
                        if (METHOD == MI_BLUR_MATCH_SAD) {
                            acc[r] = __builtin_amdgcn_sad_u8(a[j], tv, acc[r]);
                        } else {
                            acc[r] = __builtin_amdgcn_udot4(a[j], tv, acc[r], false);
                            if (METHOD == MI_BLUR_MATCH_SQDIFF) acc2[r] = __builtin_amdgcn_udot4(a[j], a[j], acc2[r], false);
                        }
                    }
                }
            }
        }
    }
    if (x >= p.Wo) return;
    const uint32_t stt = METHOD == MI_BLUR_MATCH_SQDIFF ? p.sums[(p.t_shared ? 0 : (size_t)img) * 4 + 1] : 0u;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int y = ty0 + wave * R + r;
        if (y >= p.Ho) break;
        const uint32_t v = METHOD == MI_BLUR_MATCH_SQDIFF ? acc2[r] + stt - 2u * acc[r] : acc[r];
        p.out[((size_t)img * p.Ho + y) * p.Wo + x] = v;
    }
}

struct MatchScoreParams {
    const uint32_t *ccorr, *S, *Q, *sums;
    int32_t *out;
    int W, H, C, tw, th, Wo, Ho;
    int method, t_shared;
    uint32_t A;
    long long total;
};

// The sum over the tw x th window at (x, y), all channels, from the integral table T of one image.
__device__ __forceinline__ uint32_t match_window(const uint32_t *T, int W, int C, int x, int y, int tw, int th)
{
    const size_t row_e = (size_t)W * C;
    const uint32_t *lo = T + (size_t)(y + th - 1) * row_e, *hi = T + (size_t)(y > 0 ? y - 1 : 0) * row_e;
    const size_t right = (size_t)(x + tw - 1) * C, left = (size_t)(x > 0 ? x - 1 : 0) * C;
    uint32_t s = 0;
    for (int c = 0; c < C; c++) {
        uint32_t v = lo[right + c];
        if (x > 0) v -= lo[left + c];
        if (y > 0) v -= hi[right + c];
        if (x > 0 && y > 0) v += hi[left + c];
        s += v;
    }
    return s;
}

__global__ __launch_bounds__(256) void blur_match_score_kernel(const MatchScoreParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    const long long image_e = (long long)p.Wo * p.Ho;
    const size_t table_e = (size_t)p.W * p.H * p.C;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const long long img = idx / image_e, rem = idx - img * image_e;
        const int y = (int)(rem / p.Wo), x = (int)(rem - (long long)y * p.Wo);
        const uint32_t *sums = p.sums + (p.t_shared ? 0 : (size_t)img * 4);
        const uint32_t sa = p.method == MI_BLUR_MATCH_ZNCC ? match_window(p.S + (size_t)img * table_e, p.W, p.C, x, y, p.tw, p.th) : 0u;
        const uint32_t saa = match_window(p.Q + (size_t)img * table_e, p.W, p.C, x, y, p.tw, p.th);
        p.out[idx] = match_score(p.method, p.A, p.ccorr[idx], sa, saa, sums[0], sums[1]);
    }
}

struct MatchPeakParams {
    const uint32_t *table;
    unsigned long long *parts;        // [n][MI_BLUR_MATCH_PEAK_PARTS][2]
    long long *peaks;                 // [n][6]
    unsigned entries;                 // Wo * Ho
    int Wo;
    uint32_t bias;                    // 2^31 when signed
};

// The workgroup's minimum of lo and maximum of hi, in thread 0.
__device__ __forceinline__ void peak_reduce(unsigned long long &lo, unsigned long long &hi)
{
    __shared__ unsigned long long part[2][MATCH_PEAK_THREADS / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long l2 = __shfl_down(lo, d), h2 = __shfl_down(hi, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = lo; part[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < MATCH_PEAK_THREADS / 64; w++) {
            lo = part[0][w] < lo ? part[0][w] : lo;
            hi = part[1][w] > hi ? part[1][w] : hi;
        }
}

__global__ __launch_bounds__(MATCH_PEAK_THREADS) void blur_match_peak_kernel(const MatchPeakParams p)
{
    const unsigned part = blockIdx.x % MI_BLUR_MATCH_PEAK_PARTS, img = blockIdx.x / MI_BLUR_MATCH_PEAK_PARTS;
    const uint32_t *src = p.table + (size_t)img * p.entries;
    unsigned long long lo = ~0ull, hi = 0ull;                           // no entry has either key: an index is below 2^31
    for (unsigned long long i = (unsigned long long)part * MATCH_PEAK_THREADS + threadIdx.x; i < p.entries;
         i += (unsigned long long)MI_BLUR_MATCH_PEAK_PARTS * MATCH_PEAK_THREADS) {
        const unsigned long long v = (unsigned long long)(src[i] ^ p.bias) << 32;
        const unsigned long long kl = v | (uint32_t)i, kh = v | (uint32_t)~(uint32_t)i;
        lo = kl < lo ? kl : lo;
        hi = kh > hi ? kh : hi;
    }
    peak_reduce(lo, hi);
    if (threadIdx.x == 0) {
        p.parts[2 * (size_t)blockIdx.x] = lo;
        p.parts[2 * (size_t)blockIdx.x + 1] = hi;
    }
}

__global__ __launch_bounds__(MATCH_PEAK_THREADS) void blur_match_peak_final_kernel(const MatchPeakParams p)
{
    static_assert(MI_BLUR_MATCH_PEAK_PARTS <= MATCH_PEAK_THREADS, "a thread of the final workgroup takes one part");
    const unsigned long long *src = p.parts + 2 * (size_t)blockIdx.x * MI_BLUR_MATCH_PEAK_PARTS;
    unsigned long long lo = ~0ull, hi = 0ull;
    if (threadIdx.x < MI_BLUR_MATCH_PEAK_PARTS) { lo = src[2 * threadIdx.x]; hi = src[2 * threadIdx.x + 1]; }
    peak_reduce(lo, hi);
    if (threadIdx.x == 0) {
        long long *o = p.peaks + 6 * (size_t)blockIdx.x;
        const uint32_t vl = (uint32_t)(lo >> 32) ^ p.bias, vh = (uint32_t)(hi >> 32) ^ p.bias;
        const uint32_t il = (uint32_t)lo, ih = ~(uint32_t)hi;
        o[0] = p.bias ? (long long)(int32_t)vl : (long long)vl;
        o[1] = il % (uint32_t)p.Wo;
        o[2] = il / (uint32_t)p.Wo;
        o[3] = p.bias ? (long long)(int32_t)vh : (long long)vh;
        o[4] = ih % (uint32_t)p.Wo;
        o[5] = ih / (uint32_t)p.Wo;
    }
}

// The raw launch on buffers that are known to be good: tiled where it may, else generic.  pad and sums: the prepared
// work buffer, or null when only the generic kernel may run.
int launch_match_raw(const uint8_t *in, const uint8_t *t, const uint8_t *pad, const uint32_t *sums, uint32_t *out, int W, int H, int C, int n_images,
                     int method, const mi_blur_match &k, hipStream_t stream)
{
    MatchParams p{};
    p.in = in; p.out = out; p.sums = sums; p.W = W; p.H = H; p.C = C; p.tw = k.tw; p.th = k.th; p.Wo = W - k.tw + 1; p.Ho = H - k.th + 1;
    p.method = method; p.t_shared = k.t_shared; p.tb = k.tw * C; p.row_pad = (int)match_row_pad(k, C);
    p.total = (long long)n_images * p.Wo * p.Ho;
    p.tiles_x = (p.Wo + MATCH_TX - 1) / MATCH_TX;
    p.tiles_y = (p.Ho + MATCH_TY - 1) / MATCH_TY;
    const long long groups = (long long)n_images * p.tiles_x * p.tiles_y;
    if (pad && tunables().match_tiled && match_tiled_ok(W, C) && aligned16(in) && groups <= 0x7fffffffLL) {
        p.t = pad;
        // LDS: the widest tile's rows, as many as the template needs or MATCH_LDS_BYTES hold.
        const int cpr = W * C / 16;
        const int lpitch = std::min((MATCH_TX * C + p.row_pad + 4 + 15 + 15) / 16 + 1, cpr) * 16;
        // A workgroup stages at most th + MATCH_TY - 1 rows of its own pitch (<= lpitch) and at most MATCH_LDS_BYTES.
        const size_t lds = std::min((size_t)(k.th + MATCH_TY - 1) * lpitch, (size_t)MATCH_LDS_BYTES) + MATCH_LDS_SLACK;
        set_last_kernel("blur_match_tiled_kernel");
        return dispatch<MI_BLUR_MATCH_SQDIFF, MI_BLUR_MATCH_CCORR, MI_BLUR_MATCH_SAD>(method, [&](auto M) {
            return do_launch(blur_match_tiled_kernel<decltype(M)::value>, dim3((unsigned)groups), dim3(MATCH_THREADS), lds, stream, p);
        });
    }
    p.t = t;
    set_last_kernel("blur_match_generic_kernel");
    return do_launch(blur_match_generic_kernel, byte_grid(p.total), dim3(256), 0, stream, p);
}

}  // namespace

int launch_match(const uint8_t *in, const uint8_t *t, void *out, int W, int H, int C, int n_images, const mi_blur_match &k, void *work, hipStream_t stream)
{
    if (!match_args_ok(in, t, out, W, H, C, n_images, &k, 16) || !work || !aligned16(work)) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    uint8_t *base = static_cast<uint8_t *>(work);
    uint32_t *sums = reinterpret_cast<uint32_t *>(base);
    uint8_t *pad = base + match_round16(match_sums_bytes(k, n_images));
    MatchPrepParams pp{};
    pp.t = t; pp.sums = sums; pp.pad = pad; pp.tb = k.tw * C; pp.th = k.th; pp.row_pad = (int)match_row_pad(k, C);
    if (const int rc = do_launch(blur_match_prep_kernel, dim3((unsigned)match_templates(k, n_images)), dim3(256), 0, stream, pp)) return rc;
    if (!match_is_score(k.method)) return launch_match_raw(in, t, pad, sums, static_cast<uint32_t *>(out), W, H, C, n_images, k.method, k, stream);

    const size_t table = match_round16(integral_words(W, H, C, n_images) * sizeof(uint32_t));
    uint8_t *q = pad + match_round16(match_pad_bytes(k, C, n_images));
    uint32_t *ccorr = reinterpret_cast<uint32_t *>(q);
    q += match_table_bytes(k, W, H, n_images);
    uint32_t *S = reinterpret_cast<uint32_t *>(q), *Q = reinterpret_cast<uint32_t *>(q + table);
    if (const int rc = launch_integral(in, S, Q, W, H, C, n_images, q + 2 * table, stream)) return rc;
    if (const int rc = launch_match_raw(in, t, pad, sums, ccorr, W, H, C, n_images, MI_BLUR_MATCH_CCORR, k, stream)) return rc;
    MatchScoreParams ps{};
    ps.ccorr = ccorr; ps.S = S; ps.Q = Q; ps.sums = sums; ps.out = static_cast<int32_t *>(out);
    ps.W = W; ps.H = H; ps.C = C; ps.tw = k.tw; ps.th = k.th; ps.Wo = W - k.tw + 1; ps.Ho = H - k.th + 1;
    ps.method = k.method; ps.t_shared = k.t_shared; ps.A = (uint32_t)(k.tw * k.th * C);
    ps.total = (long long)n_images * ps.Wo * ps.Ho;
    return do_launch(blur_match_score_kernel, byte_grid(ps.total), dim3(256), 0, stream, ps);
}

int launch_match_peak(const void *table, int is_signed, int Wo, int Ho, int n_images, int64_t *peaks, void *work, hipStream_t stream)
{
    if (!match_peak_args_ok(table, is_signed, Wo, Ho, n_images, peaks, 16, 16) || !work || !aligned16(work)) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    if ((long long)n_images * MI_BLUR_MATCH_PEAK_PARTS > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
    MatchPeakParams p{};
    p.table = static_cast<const uint32_t *>(table); p.parts = static_cast<unsigned long long *>(work); p.peaks = reinterpret_cast<long long *>(peaks);
    p.entries = (unsigned)((long long)Wo * Ho); p.Wo = Wo; p.bias = is_signed ? 0x80000000u : 0u;
    set_last_kernel("blur_match_peak_kernel");
    if (const int rc = do_launch(blur_match_peak_kernel, dim3((unsigned)n_images * MI_BLUR_MATCH_PEAK_PARTS), dim3(MATCH_PEAK_THREADS), 0, stream, p)) return rc;
    return do_launch(blur_match_peak_final_kernel, dim3((unsigned)n_images), dim3(MATCH_PEAK_THREADS), 0, stream, p);
}

}  // namespace mi_blur
