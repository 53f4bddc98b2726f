// arith_kernels.hip — gfx950 kernels of the two-image arithmetic (mi_blur_enqueue_arith, include/mi_blur.h, "Two-image
// arithmetic"): out = A op B, or the blend of A and B through a mask M.  Integers only; every output byte is arith_byte()
// (filter.h), which the host export and the CPU device use too.  Streaming kernels: no LDS, no barrier.
//
// blur_arith_flat_kernel<OP> (6 instances): every operand has the image's channel count, W * H * C is a multiple of 16
// and all pointers are 16-byte aligned.  The operation is bytewise then, so an image is a flat run of W * H * C bytes cut
// into chunks of 16 and the channel count does not enter the kernel.  A thread owns ONE chunk: one 16-byte load per
// operand and one 16-byte store, lane after lane, so every wave instruction moves 1 KiB contiguously.  A workgroup owns
// a run of ARITH_RUN consecutive chunks of one image; blockIdx -> (image, run) in the XCD-contiguous order for grids of
// 16 workgroups and more.  A shared operand has an image stride of 0.  The weights sit in scalar registers; a byte is
// extracted from its dword, goes through arith_byte() with the constant OP and is ORed back into place.
//
// blur_arith_plane_kernel<OP, C, B_PLANE, M_PLANE> (24 instances: five operations x C 2..4 with a plane B, LERP with
// its three flag pairs x C 2..4): the colour kernel's flat rule (W * H a multiple of 16, aligned pointers).  A thread
// owns a group of 16 pixels: C chunks of every full operand, one chunk of every plane operand, C stores; byte j of the
// group belongs to pixel j / C, a compile-time pick from the plane chunk.
//
// blur_arith_generic_kernel: one output byte per thread, grid-strided, any shape and alignment.
//
// In place: a thread reads all the bytes of its chunk (group, byte) before it stores them, and no thread reads another
// thread's output bytes in the allowed cases (out == A; out == B where B has the output's extent).
#include "kernel_common.h"

namespace mi_blur {

namespace {

struct ArithWeights {
    int32_t wa, wb, bias;
    int shift;
};

struct ArithTiledParams {
    const uint8_t *a, *b, *m;
    uint8_t *out;
    long long stride;                 // bytes per image of A and of the output
    long long b_stride, m_stride;     // bytes per image of B and M; 0 for a shared operand
    unsigned units, runs;             // per image: chunks (flat) or groups of 16 pixels (plane), and runs of them
    unsigned nblocks;
    int xcd;
    ArithWeights k;
};

// The 16 bytes of four dwords through arith_byte(), byte by byte.
template <int OP>
__device__ __forceinline__ uint4 arith_chunk(const ArithWeights &k, const uint4 a, const uint4 b, const uint4 m)
{
    const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w}, wm[4] = {m.x, m.y, m.z, m.w};
    uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++)
        r[j >> 2] |= (uint32_t)arith_byte(OP, k.wa, k.wb, k.bias, k.shift, (int)window_byte(wa, j), (int)window_byte(wb, j), (int)window_byte(wm, j))
                     << (8 * (j & 3));
    return make_uint4(r[0], r[1], r[2], r[3]);
}

template <int OP>
__global__ __launch_bounds__(ARITH_THREADS) void blur_arith_flat_kernel(const ArithTiledParams p)
{
    // blockIdx -> (image, run): runs fastest, then images
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const unsigned img = L / p.runs, run = L - img * p.runs;
    const unsigned ch = run * ARITH_RUN + threadIdx.x;
    if (ch >= p.units) return;                                  // the last run of an image may be short
    const size_t off = (size_t)ch * ARITH_CHUNK;
    const uint4 a = *reinterpret_cast<const uint4 *>(p.a + (long long)img * p.stride + off);
    const uint4 b = *reinterpret_cast<const uint4 *>(p.b + (long long)img * p.b_stride + off);
    uint4 m = make_uint4(0, 0, 0, 0);
    if constexpr (OP == MI_BLUR_ARITH_LERP) m = *reinterpret_cast<const uint4 *>(p.m + (long long)img * p.m_stride + off);
    *reinterpret_cast<uint4 *>(p.out + (long long)img * p.stride + off) = arith_chunk<OP>(p.k, a, b, m);
}

template <int OP, int C, int B_PLANE, int M_PLANE>
__global__ __launch_bounds__(ARITH_THREADS) void blur_arith_plane_kernel(const ArithTiledParams p)
{
    constexpr bool LERP = OP == MI_BLUR_ARITH_LERP;
    constexpr int NB = B_PLANE ? 1 : C, NM = !LERP ? 1 : M_PLANE ? 1 : C;
    const unsigned L = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    const unsigned img = L / p.runs, run = L - img * p.runs;
    const unsigned g = run * ARITH_PLANE_RUN + threadIdx.x;
    if (g >= p.units) return;
    uint32_t a[4 * C], b[4 * NB], m[4 * NM], r[4 * C];
    load_group<C>(a, p.a + (long long)img * p.stride, g);          // C chunks of a full operand, 1 of a plane
    load_group<NB>(b, p.b + (long long)img * p.b_stride, g);
    if constexpr (LERP) load_group<NM>(m, p.m + (long long)img * p.m_stride, g);
    else m[0] = m[1] = m[2] = m[3] = 0;
#pragma unroll
    for (int q = 0; q < 4 * C; q++) r[q] = 0;
#pragma unroll
    for (int j = 0; j < 16 * C; j++) {
        const int vb = (int)window_byte(b, B_PLANE ? j / C : j);
        const int vm = LERP ? (int)window_byte(m, M_PLANE ? j / C : j) : 0;
        r[j >> 2] |= (uint32_t)arith_byte(OP, p.k.wa, p.k.wb, p.k.bias, p.k.shift, (int)window_byte(a, j), vb, vm) << (8 * (j & 3));
    }
    store_group<C>(r, p.out + (long long)img * p.stride, g);
}

struct ArithGenericParams {
    const uint8_t *a, *b, *m;
    uint8_t *out;
    long long bytes, total;           // bytes per image of A, bytes of the launch
    long long b_stride, m_stride;     // bytes per image of B and M; 0 for a shared operand
    int channels, op, b_plane, m_plane;
    ArithWeights k;
};

__global__ __launch_bounds__(256) void blur_arith_generic_kernel(const ArithGenericParams p)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const long long img = idx / p.bytes;
        const unsigned rem = (unsigned)(idx - img * p.bytes), px = rem / (unsigned)p.channels;
        const int b = p.b[img * p.b_stride + (p.b_plane ? px : rem)];
        const int m = p.op == MI_BLUR_ARITH_LERP ? p.m[img * p.m_stride + (p.m_plane ? px : rem)] : 0;
        p.out[idx] = (uint8_t)arith_byte(p.op, p.k.wa, p.k.wb, p.k.bias, p.k.shift, p.a[idx], b, m);
    }
}

}  // namespace

int launch_arith(const uint8_t *a, const uint8_t *b, const uint8_t *m, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_arith &k,
                 hipStream_t stream)
{
    if (!arith_args_ok(a, b, m, out, W, H, C, n_images, &k)) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const mi_blur_arith q = arith_normalised(k, C, n_images);
    const bool lerp = q.op == MI_BLUR_ARITH_LERP;
    const long long bytes = arith_image_bytes(W, H, C, 0);
    const long long b_stride = q.b_shared ? 0 : arith_image_bytes(W, H, C, q.b_plane);
    const long long m_stride = !lerp || q.m_shared ? 0 : arith_image_bytes(W, H, C, q.m_plane);
    const ArithWeights wts{q.wa, q.wb, q.bias, q.shift};
    const bool plane = q.b_plane || q.m_plane;
    const bool aligned = aligned16(a) && aligned16(b) && aligned16(out) && (!lerp || aligned16(m));
    if (aligned && (plane ? color_flat_ok(W, H) : arith_flat_ok(W, H, C))) {
        ArithTiledParams p{};
        p.a = a; p.b = b; p.m = m; p.out = out;
        p.stride = bytes; p.b_stride = b_stride; p.m_stride = m_stride;
        p.units = (unsigned)(plane ? (long long)W * H / COLOR_GROUP : bytes / ARITH_CHUNK);
        p.runs = (unsigned)(plane ? arith_plane_runs(W, H) : arith_flat_runs(W, H, C));
        if (const int st = fill_flat(p, n_images, p.runs)) return st;
        p.k = wts;
        const dim3 grid(p.nblocks), block(ARITH_THREADS);
        if (!plane) {
            set_last_kernel("blur_arith_flat_kernel");
            return dispatch<0, 1, 2, 3, 4, 5>(q.op, [&](auto OP) { return do_launch(blur_arith_flat_kernel<OP>, grid, block, 0, stream, p); });
        }
        set_last_kernel("blur_arith_plane_kernel");
        return dispatch<0, 1, 2, 3, 4, 5>(q.op, [&](auto OP) {
            return dispatch<2, 3, 4>(C, [&](auto CC) {
                if constexpr (decltype(OP)::value == MI_BLUR_ARITH_LERP)
                    return dispatch<1, 2, 3>(2 * q.b_plane + q.m_plane, [&](auto F) {
                        constexpr int f = decltype(F)::value;
                        return do_launch(blur_arith_plane_kernel<MI_BLUR_ARITH_LERP, decltype(CC)::value, (f >> 1) & 1, f & 1>, grid, block, 0, stream, p);
                    });
                else
                    return do_launch(blur_arith_plane_kernel<decltype(OP)::value, decltype(CC)::value, 1, 0>, grid, block, 0, stream, p);
            });
        });
    }
    ArithGenericParams p{};
    p.a = a; p.b = b; p.m = m; p.out = out;
    p.bytes = bytes; p.total = bytes * n_images; p.b_stride = b_stride; p.m_stride = m_stride;
    p.channels = C; p.op = q.op; p.b_plane = q.b_plane; p.m_plane = q.m_plane;
    p.k = wts;
    set_last_kernel("blur_arith_generic_kernel");
    return do_launch(blur_arith_generic_kernel, byte_grid(p.total), dim3(256), 0, stream, p);
}

}  // namespace mi_blur
