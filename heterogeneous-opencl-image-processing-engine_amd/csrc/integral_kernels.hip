// integral_kernels.hip — gfx950 kernels of the integral images and of the box filters made from them (include/mi_blur.h,
// "Integral images, and box filters"): mi_blur_enqueue_integral and mi_blur_enqueue_box_from_integral.  Integers only,
// every table entry modulo 2^32; a window's sum is box_window() and an output byte box_byte() (filter.h), which the host
// export and the CPU device use too.
//
// ONE RULE: no workgroup here ever waits for another.  There is no look-back, no flag and no ticket: what one band of rows
// hands the next crosses a dispatch boundary on the stream, through the work buffer.
//
// The tiled integral (W a multiple of INTEGRAL_PIXELS, W <= INTEGRAL_MAX_W, an aligned input), three dispatches:
//   blur_integral_bands_kernel<MODE>: a thread owns one 16-byte chunk column of one band of rows of one image and walks down
//     it: 16 column sums of the bytes (MODE 0), of their squares (1) or both (2), to work[image][band][table][W * C].  The
//     channel count does not enter: a column of bytes is a column of one channel.
//   blur_integral_band_prefix_kernel: one thread per column walks the bands of its image: the exclusive prefix, in place.
//   blur_integral_tiled_kernel<C, MODE>: one workgroup per (image, band), of the fewest whole waves whose threads, 16 pixels
//     each, cover the row.  A thread keeps the running column sums of its 16 C bytes in registers (seeded from the work
//     buffer), adds each row to them (the next row's C loads of 16 bytes are already in flight) and takes the prefix
//     along the row: its own totals per channel, an inclusive scan of those across the wave by lane shifts (one per
//     channel and table), the waves' totals through LDS (two sets, by row parity: one barrier per row), then the running
//     sums again from that offset, stored as 4 C chunks of 16 bytes per table.  Channel picks are compile-time.
// The generic integral (any shape and alignment), two dispatches, no work buffer:
//   blur_integral_generic_kernel: one wave per row, 64 pixels a step: the prefix along the row into the tables.
//   blur_integral_generic_cols_kernel: one thread per column and channel walks down the tables, in place.
//
// blur_box_tiled_kernel<OP, N> (rows of whole 16-byte chunks, aligned output and input): a thread owns N = 4 consecutive
// output bytes of a row ("box_bytes" 16: N = 16), which is N consecutive dwords at each corner of the window, fetched as
// 16-byte loads at 4-byte alignment: with N = 4 the loads of a wave are contiguous.  Where all of its pixels are more than
// rx columns and ry rows from every border: corner - corner - corner + corner; elsewhere box_window() per byte.  blur_box_generic_kernel: one output byte
// per thread, box_window() everywhere.
#include "kernel_common.h"

namespace mi_blur {

namespace {

constexpr int MODE_S = 0, MODE_Q = 1, MODE_BOTH = 2;

__device__ __forceinline__ void put4(uint32_t *dst, const uint32_t *v) { *reinterpret_cast<uint4 *>(dst) = make_uint4(v[0], v[1], v[2], v[3]); }

struct IntegralBandsParams {
    const uint8_t *in;
    uint32_t *work;
    long long in_stride;              // bytes per image
    unsigned cpr;                     // 16-byte chunks per row
    unsigned nbands;
    int H, band;
    unsigned total;                   // n_images * nbands * cpr threads
};

template <int MODE>
__global__ __launch_bounds__(256) void blur_integral_bands_kernel(const IntegralBandsParams p)
{
    constexpr int NT = MODE == MODE_BOTH ? 2 : 1;
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= p.total) return;
    const unsigned col = g % p.cpr, t2 = g / p.cpr, b = t2 % p.nbands, img = t2 / p.nbands;
    const int y0 = (int)b * p.band, y1 = min(y0 + p.band, p.H);
    const size_t pitch = (size_t)p.cpr * 16u;
    const uint8_t *src = p.in + (long long)img * p.in_stride + (size_t)y0 * pitch + (size_t)col * 16u;
    uint32_t s[16], q[16];
#pragma unroll
    for (int j = 0; j < 16; j++) s[j] = q[j] = 0;
    for (int y = y0; y < y1; y++, src += pitch) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t e = window_byte(w, j);
            if (MODE != MODE_Q) s[j] += e;
            if (MODE != MODE_S) q[j] += e * e;
        }
    }
    uint32_t *dst = p.work + ((size_t)img * p.nbands + b) * NT * pitch + (size_t)col * 16u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        put4(dst + 4 * j, MODE == MODE_Q ? q + 4 * j : s + 4 * j);
        if (MODE == MODE_BOTH) put4(dst + pitch + 4 * j, q + 4 * j);
    }
}

struct IntegralPrefixParams {
    uint32_t *work;
    unsigned row;                     // dwords of one band: tables * W * C
    unsigned nbands;
    unsigned total;                   // n_images * row threads
};

__global__ __launch_bounds__(256) void blur_integral_band_prefix_kernel(const IntegralPrefixParams p)
{
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= p.total) return;
    const unsigned img = g / p.row, e = g - img * p.row;
    uint32_t *q = p.work + (size_t)img * p.nbands * p.row + e;
    uint32_t run = 0;
    for (unsigned b = 0; b < p.nbands; b++, q += p.row) {
        const uint32_t v = *q;
        *q = run;
        run += v;
    }
}

struct IntegralScanParams {
    const uint8_t *in;
    uint32_t *sum, *sqsum;
    const uint32_t *work;
    long long in_stride;              // bytes per image
    int W, H, band;
    unsigned nbands;
};

template <int C, int MODE>
__global__ __launch_bounds__(INTEGRAL_MAX_THREADS) void blur_integral_tiled_kernel(const IntegralScanParams p)
{
    constexpr int NT = MODE == MODE_BOTH ? 2 : 1;
    constexpr int E = INTEGRAL_PIXELS * C;                              // bytes of a thread per row
    __shared__ uint32_t wave_tot[2][INTEGRAL_MAX_THREADS / 64][NT * C];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned img = blockIdx.x / p.nbands, b = blockIdx.x - img * p.nbands;
    const bool active = INTEGRAL_PIXELS * t < p.W;                      // the last wave may reach beyond the row
    const size_t row_e = (size_t)p.W * C;
    const int y0 = (int)b * p.band, y1 = min(y0 + p.band, p.H);

    uint32_t col[NT][E];                                                // the running column sums
#pragma unroll
    for (int k = 0; k < NT; k++)
#pragma unroll
        for (int j = 0; j < E; j++) col[k][j] = 0;
    uint32_t w[4 * C];
#pragma unroll
    for (int j = 0; j < 4 * C; j++) w[j] = 0;
    const uint8_t *src = p.in + (long long)img * p.in_stride + (size_t)y0 * row_e + (size_t)t * E;
    if (active) {
        const uint32_t *seed = p.work + ((size_t)img * p.nbands + b) * NT * row_e + (size_t)t * E;
#pragma unroll
        for (int k = 0; k < NT; k++)
#pragma unroll
            for (int j = 0; j < 4 * C; j++) {
                const uint4 v = reinterpret_cast<const uint4 *>(seed + k * row_e)[j];
                col[k][4 * j] = v.x; col[k][4 * j + 1] = v.y; col[k][4 * j + 2] = v.z; col[k][4 * j + 3] = v.w;
            }
#pragma unroll
        for (int j = 0; j < C; j++) {
            const uint4 v = reinterpret_cast<const uint4 *>(src)[j];
            w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
        }
    }
    const size_t first = ((size_t)img * p.H + y0) * row_e + (size_t)t * E;
    uint32_t *dst[NT];
    dst[0] = (MODE == MODE_Q ? p.sqsum : p.sum) + first;
    if (MODE == MODE_BOTH) dst[NT - 1] = p.sqsum + first;

    for (int y = y0; y < y1; y++) {
        uint32_t nw[4 * C];                                             // the next row, in flight while this one is scanned
#pragma unroll
        for (int j = 0; j < 4 * C; j++) nw[j] = 0;
        src += row_e;
        if (active && y + 1 < y1) {
#pragma unroll
            for (int j = 0; j < C; j++) {
                const uint4 v = reinterpret_cast<const uint4 *>(src)[j];
                nw[4 * j] = v.x; nw[4 * j + 1] = v.y; nw[4 * j + 2] = v.z; nw[4 * j + 3] = v.w;
            }
        }
        uint32_t tot[NT][C];
#pragma unroll
        for (int k = 0; k < NT; k++)
#pragma unroll
            for (int c = 0; c < C; c++) tot[k][c] = 0;
#pragma unroll
        for (int j = 0; j < E; j++) {
            const uint32_t e = window_byte(w, j);
            if (MODE != MODE_Q) col[0][j] += e;
            if (MODE != MODE_S) col[NT - 1][j] += e * e;
#pragma unroll
            for (int k = 0; k < NT; k++) tot[k][j % C] += col[k][j];
        }
        uint32_t off[NT][C];
#pragma unroll
        for (int k = 0; k < NT; k++)
#pragma unroll
            for (int c = 0; c < C; c++) {
                uint32_t inc = tot[k][c];                               // inclusive scan of the lanes' totals
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t v = __shfl_up(inc, d);
                    if (lane >= d) inc += v;
                }
                if (lane == 63) wave_tot[y & 1][wave][k * C + c] = inc;
                off[k][c] = inc - tot[k][c];
            }
        __syncthreads();
        for (int wv = 0; wv < wave; wv++)
#pragma unroll
            for (int k = 0; k < NT; k++)
#pragma unroll
                for (int c = 0; c < C; c++) off[k][c] += wave_tot[y & 1][wv][k * C + c];
        if (active) {
#pragma unroll
            for (int k = 0; k < NT; k++) {
#pragma unroll
                for (int j4 = 0; j4 < 4 * C; j4++) {
                    uint32_t v[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int j = 4 * j4 + e;
                        off[k][j % C] += col[k][j];
                        v[e] = off[k][j % C];
                    }
                    put4(dst[k] + 4 * j4, v);
                }
                dst[k] += row_e;
            }
        }
#pragma unroll
        for (int j = 0; j < 4 * C; j++) w[j] = nw[j];
    }
}

struct IntegralGenericParams {
    const uint8_t *in;
    uint32_t *sum, *sqsum;            // either may be null
    int W, H, C;
    long long rows;                   // n_images * H
    long long cols;                   // n_images * W * C
};

__global__ __launch_bounds__(256) void blur_integral_generic_kernel(const IntegralGenericParams p)
{
    const int lane = threadIdx.x & 63;
    const size_t row_e = (size_t)p.W * p.C;
    for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < p.rows; row += (long long)gridDim.x * 4) {
        const uint8_t *src = p.in + (size_t)row * row_e;
        uint32_t carry_s[MI_BLUR_COLOR_MAX_CHANNELS] = {0, 0, 0, 0}, carry_q[MI_BLUR_COLOR_MAX_CHANNELS] = {0, 0, 0, 0};
        for (int x0 = 0; x0 < p.W; x0 += 64) {
            const int x = x0 + lane;
            const bool ok = x < p.W;
#pragma unroll
            for (int c = 0; c < MI_BLUR_COLOR_MAX_CHANNELS; c++) {
                if (c >= p.C) break;
                const uint32_t e = ok ? src[(size_t)x * p.C + c] : 0u;
                uint32_t s = e, q = e * e;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t vs = __shfl_up(s, d), vq = __shfl_up(q, d);
                    if (lane >= d) { s += vs; q += vq; }
                }
                s += carry_s[c];
                q += carry_q[c];
                const size_t at = (size_t)row * row_e + (size_t)x * p.C + c;
                if (ok && p.sum) p.sum[at] = s;
                if (ok && p.sqsum) p.sqsum[at] = q;
                carry_s[c] = __shfl(s, 63);                             // lanes beyond the row added 0: lane 63 has the total
                carry_q[c] = __shfl(q, 63);
            }
        }
    }
}

__global__ __launch_bounds__(256) void blur_integral_generic_cols_kernel(const IntegralGenericParams p)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= p.cols) return;
    const size_t row_e = (size_t)p.W * p.C;
    const long long img = g / (long long)row_e;
    const size_t at = (size_t)img * p.H * row_e + (size_t)(g - img * (long long)row_e);
    for (int k = 0; k < 2; k++) {
        uint32_t *q = k ? p.sqsum : p.sum;
        if (!q) continue;
        q += at;
        uint32_t run = 0;
        for (int y = 0; y < p.H; y++, q += row_e) {
            run += *q;
            *q = run;
        }
    }
}

struct BoxParams {
    const uint8_t *in;                // THRESHOLD only
    const uint32_t *sum, *sqsum;      // sqsum: STDDEV only
    uint8_t *out;
    int W, H, C;
    int op, rx, ry, offset, invert;
    uint32_t A;
    float inv_2a;
    double inv_a;
    unsigned per_row;                 // tiled: threads per row
    long long total;                  // tiled: threads of the launch; generic: bytes
};

// N consecutive dwords from a 4-byte aligned address, as 16-byte loads.
template <int N>
__device__ __forceinline__ void load_run(uint32_t (&v)[N], const uint32_t *src)
{
#pragma unroll
    for (int i = 0; i < N / 4; i++) {
        u32x4 q;
        __builtin_memcpy(&q, src + 4 * i, 16);
        v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
    }
}
// The N window sums of a thread in the interior: corner - corner - corner + corner, modulo 2^32.
template <int N>
__device__ __forceinline__ void corner_sums(uint32_t (&s)[N], const uint32_t *T, size_t row_e, int y, int b0, const BoxParams &p)
{
    const uint32_t *lo = T + (size_t)(y + p.ry) * row_e + b0, *hi = T + (size_t)(y - p.ry - 1) * row_e + b0;
    const int right = p.rx * p.C, left = -(p.rx + 1) * p.C;
    uint32_t v[N];
    load_run(s, lo + right);
    load_run(v, lo + left);
#pragma unroll
    for (int j = 0; j < N; j++) s[j] -= v[j];
    load_run(v, hi + right);
#pragma unroll
    for (int j = 0; j < N; j++) s[j] -= v[j];
    load_run(v, hi + left);
#pragma unroll
    for (int j = 0; j < N; j++) s[j] += v[j];
}

// N = the consecutive output bytes of a row one thread owns: 16 (four 16-byte loads per corner, the lanes of a wave 64
// bytes apart) or 4 (one 16-byte load per corner, the lanes of a wave contiguous).
template <int OP, int N>
__global__ __launch_bounds__(BOX_THREADS) void blur_box_tiled_kernel(const BoxParams p)
{
    const long long g = (long long)blockIdx.x * BOX_THREADS + threadIdx.x;
    if (g >= p.total) return;
    const long long r = g / p.per_row;
    const int b0 = (int)(g - r * p.per_row) * N;                        // the thread's first byte of its row
    const long long img = r / p.H;
    const int y = (int)(r - img * p.H);
    const size_t row_e = (size_t)p.W * p.C;
    const size_t image_e = (size_t)p.H * row_e;
    const uint32_t *S = p.sum + (size_t)img * image_e;
    const uint32_t *Q = OP == MI_BLUR_BOX_STDDEV ? p.sqsum + (size_t)img * image_e : nullptr;
    const size_t at = (size_t)img * image_e + (size_t)y * row_e + b0;
    uint32_t a[N / 4], o[N / 4];                                        // the centre bytes and the output bytes
#pragma unroll
    for (int i = 0; i < N / 4; i++) {
        a[i] = OP == MI_BLUR_BOX_THRESHOLD ? reinterpret_cast<const uint32_t *>(p.in + at)[i] : 0u;
        o[i] = 0;
    }
    const int x_first = b0 / p.C, x_last = (b0 + N - 1) / p.C;
    if (x_first > p.rx && x_last + p.rx < p.W && y > p.ry && y + p.ry < p.H) {
        uint32_t s[N], q[N];
        corner_sums(s, S, row_e, y, b0, p);
        if (OP == MI_BLUR_BOX_STDDEV) corner_sums(q, Q, row_e, y, b0, p);
#pragma unroll
        for (int j = 0; j < N; j++)
            o[j >> 2] |= (uint32_t)box_byte(OP, p.offset, p.invert, p.A, p.inv_2a, p.inv_a, s[j], OP == MI_BLUR_BOX_STDDEV ? q[j] : 0u,
                                            (int)window_byte(a, j)) << (8 * (j & 3));
    } else {
#pragma unroll
        for (int i = 0; i < N / 4; i++) {                               // words under a constant index, bytes in a loop: no scratch
            uint32_t word = 0;
            for (int e = 0; e < 4; e++) {
                const int b = b0 + 4 * i + e, x = b / p.C, c = b - x * p.C;
                const uint32_t s = box_window(S, p.W, p.H, p.C, x, y, c, p.rx, p.ry);
                const uint32_t q = OP == MI_BLUR_BOX_STDDEV ? box_window(Q, p.W, p.H, p.C, x, y, c, p.rx, p.ry) : 0u;
                word |= (uint32_t)box_byte(OP, p.offset, p.invert, p.A, p.inv_2a, p.inv_a, s, q, (int)(a[i] >> (8 * e) & 0xffu)) << (8 * e);
            }
            o[i] = word;
        }
    }
#pragma unroll
    for (int i = 0; i < N / 4; i++) reinterpret_cast<uint32_t *>(p.out + at)[i] = o[i];
}

__global__ __launch_bounds__(256) void blur_box_generic_kernel(const BoxParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    const long long row_e = (long long)p.W * p.C, image_e = row_e * p.H;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const long long img = idx / image_e, rem = idx - img * image_e;
        const int y = (int)(rem / row_e), b = (int)(rem - (long long)y * row_e), x = b / p.C, c = b - x * p.C;
        const uint32_t s = box_window(p.sum + (size_t)img * image_e, p.W, p.H, p.C, x, y, c, p.rx, p.ry);
        const uint32_t q = p.op == MI_BLUR_BOX_STDDEV ? box_window(p.sqsum + (size_t)img * image_e, p.W, p.H, p.C, x, y, c, p.rx, p.ry) : 0u;
        const int a = p.op == MI_BLUR_BOX_THRESHOLD ? p.in[idx] : 0;
        p.out[idx] = (uint8_t)box_byte(p.op, p.offset, p.invert, p.A, p.inv_2a, p.inv_a, s, q, a);
    }
}

}  // namespace

int launch_integral(const uint8_t *in, uint32_t *sum, uint32_t *sqsum, int W, int H, int C, int n_images, void *work, hipStream_t stream)
{
    if (!integral_args_ok(in, sum, sqsum, W, H, C, n_images, 16) || !work || !aligned16(work)) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const int mode = sum && sqsum ? MODE_BOTH : sum ? MODE_S : MODE_Q, nt = mode == MODE_BOTH ? 2 : 1;
    const long long bytes = (long long)W * H * C;
    if (integral_tiled_ok(W) && aligned16(in)) {
        const int band = tunables().integral_band;
        const unsigned nbands = (unsigned)integral_bands(H, band), cpr = (unsigned)((long long)W * C / 16);
        const long long band_threads = (long long)n_images * nbands * cpr, prefix_threads = (long long)n_images * nt * W * C;
        const long long groups = (long long)n_images * nbands;
        if (band_threads > 0xffffffffLL || prefix_threads > 0xffffffffLL || groups > 0x7fffffffLL) return MI_BLUR_ERR_INVALID;
        IntegralBandsParams pb{};
        pb.in = in; pb.work = static_cast<uint32_t *>(work); pb.in_stride = bytes; pb.cpr = cpr; pb.nbands = nbands; pb.H = H; pb.band = band;
        pb.total = (unsigned)band_threads;
        if (const int rc = dispatch<MODE_S, MODE_Q, MODE_BOTH>(mode, [&](auto M) {
                return do_launch(blur_integral_bands_kernel<M>, dim3(blocks_of(band_threads)), dim3(256), 0, stream, pb);
            }))
            return rc;
        IntegralPrefixParams pp{};
        pp.work = pb.work; pp.row = (unsigned)(nt * W * C); pp.nbands = nbands; pp.total = (unsigned)prefix_threads;
        if (const int rc = do_launch(blur_integral_band_prefix_kernel, dim3(blocks_of(prefix_threads)), dim3(256), 0, stream, pp)) return rc;
        IntegralScanParams ps{};
        ps.in = in; ps.sum = sum; ps.sqsum = sqsum; ps.work = pb.work; ps.in_stride = bytes; ps.W = W; ps.H = H; ps.band = band; ps.nbands = nbands;
        set_last_kernel("blur_integral_tiled_kernel");
        const dim3 grid((unsigned)groups), block((unsigned)integral_threads(W));
        return dispatch<1, 2, 3, 4>(C, [&](auto CC) {
            constexpr int c = decltype(CC)::value;
            return dispatch<MODE_S, MODE_Q, MODE_BOTH>(mode, [&](auto M) {
                return do_launch(blur_integral_tiled_kernel<c, decltype(M)::value>, grid, block, 0, stream, ps);
            });
        });
    }
    IntegralGenericParams p{};
    p.in = in; p.sum = sum; p.sqsum = sqsum; p.W = W; p.H = H; p.C = C; p.rows = (long long)n_images * H; p.cols = (long long)n_images * W * C;
    const long long row_blocks = (p.rows + 3) / 4;
    if (!blocks_of(p.cols)) return MI_BLUR_ERR_INVALID;
    set_last_kernel("blur_integral_generic_kernel");
    if (const int rc = do_launch(blur_integral_generic_kernel, dim3((unsigned)(row_blocks > 65536 ? 65536 : row_blocks)), dim3(256), 0, stream, p)) return rc;
    return do_launch(blur_integral_generic_cols_kernel, dim3(blocks_of(p.cols)), dim3(256), 0, stream, p);
}

int launch_box_from_integral(const uint8_t *in, const uint32_t *sum, const uint32_t *sqsum, uint8_t *out, int W, int H, int C, int n_images,
                             const mi_blur_box &k, hipStream_t stream)
{
    if (!box_from_args_ok(in, sum, sqsum, out, W, H, C, n_images, &k)) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const BoxConst bc = box_const(k);
    BoxParams p{};
    p.in = in; p.sum = sum; p.sqsum = sqsum; p.out = out; p.W = W; p.H = H; p.C = C;
    p.op = k.op; p.rx = k.rx; p.ry = k.ry; p.offset = k.offset; p.invert = k.invert;
    p.A = bc.A; p.inv_2a = bc.inv_2a; p.inv_a = bc.inv_a;
    const long long bytes = (long long)W * H * C * n_images;
    const int own = tunables().box_bytes;                               // output bytes per thread: 4 | 16
    if (box_tiled_ok(W, C) && aligned16(out) && aligned16(in) && blocks_of(bytes / own)) {
        p.per_row = (unsigned)((long long)W * C / own);
        p.total = bytes / own;
        static_assert(BOX_THREADS == 256, "blocks_of() counts workgroups of 256");
        set_last_kernel("blur_box_tiled_kernel");
        return dispatch<MI_BLUR_BOX_MEAN, MI_BLUR_BOX_STDDEV, MI_BLUR_BOX_THRESHOLD>(k.op, [&](auto OP) {
            constexpr int op = decltype(OP)::value;
            const dim3 grid(blocks_of(p.total)), block(BOX_THREADS);
            return own == 4 ? do_launch(blur_box_tiled_kernel<op, 4>, grid, block, 0, stream, p) : do_launch(blur_box_tiled_kernel<op, 16>, grid, block, 0, stream, p);
        });
    }
    p.total = bytes;
    set_last_kernel("blur_box_generic_kernel");
    return do_launch(blur_box_generic_kernel, byte_grid(p.total), dim3(256), 0, stream, p);
}

}  // namespace mi_blur
