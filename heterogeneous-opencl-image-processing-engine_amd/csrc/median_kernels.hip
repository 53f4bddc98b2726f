// median_kernels.hip — gfx950 kernels of the median blur, radius 1..7 (mi_blur_enqueue_median, include/mi_blur.h):
//   out[y][x][c] = the k-th smallest (k = ((2r+1)^2 - 1) / 2) of in[clamp(y+j)][clamp(x+i)][c], -r <= i, j <= r
// The window count is odd, so the result is one exact byte; every kernel here computes it with min / max only (or an
// exact count), so all of them agree with the CPU device byte for byte.
//
// Fast kernel (blur_median_fast_kernel<C, R>), radius 1 and 2: rows of whole 16-byte chunks, 16-byte aligned buffers and
// strides, 1-4 channels.  The direct kernel's layout (blur_kernels.hip; its host side is shared, kernel_common.h): a lane owns one 16-byte chunk column and BH (8 | 4)
// output rows, loads the BH + 2R rows of it straight into registers, takes the 8 bytes either side from the
// neighbouring lanes (DPP wave shifts; lanes 0 and 63 only supply them, 62 lanes per wave compute), and replaces them by
// copies of the edge pixel's channels at the row ends (one v_perm of its own first / last dword).  No LDS, no barrier.
// Every byte is unpacked to its own 32-bit register (v_bfe_u32) and the selection runs on whole registers, where min3 /
// max3 / med3 are single instructions:
//   * R = 1: per byte column of the three rows, lo = min3, mid = med3, hi = max3 (sorted once, used by three outputs);
//     out = med3(max3(lo[-C], lo[0], lo[+C]), med3(mid[-C], mid[0], mid[+C]), min3(hi[-C], hi[0], hi[+C])).
//     About 7 min/max-class instructions per output byte plus the unpack and the repack.
//   * R = 2: per byte column the five rows are sorted (Batcher network, 9 compare-exchanges); the sorted column pairs
//     (p, p+C) are merged once (odd-even merge, shared by the two outputs that use that pair); an output merges its two
//     pairs (ranks 7..12 of the 20 are all it needs) and takes rank 12 of that list and its own sorted column as
//     min over i of max(col[i-1], merged[12-i]).  The networks are written out in full over registers padded with
//     0xffffffff; the compiler folds the padding away and drops every comparator the result does not depend on.
//
// Generic kernel (blur_median_generic_kernel<R>): one output byte per thread, any shape, radius 1..7.  The window is held in
// registers as 16-bit fields, two per dword, and the result found bit by bit from the top: t = ans | bit is kept when at
// most k window values are below t, counted two fields per subtraction.  Correct everywhere, fast nowhere.
#include "kernel_common.h"

#include <utility>

namespace mi_blur {

namespace {

constexpr int med_bh(int R) { return R == 1 ? 8 : 4; }   // output rows per lane, fast kernel (radius 2: registers)
constexpr uint32_t MED_PAD = 0xffffffffu;

__device__ __forceinline__ uint32_t mn(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t mx(uint32_t a, uint32_t b) { return a < b ? b : a; }
__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) { return mn(mn(a, b), c); }
__device__ __forceinline__ uint32_t max3u(uint32_t a, uint32_t b, uint32_t c) { return mx(mx(a, b), c); }
__device__ __forceinline__ uint32_t med3u(uint32_t a, uint32_t b, uint32_t c) { return mx(mn(a, b), mn(mx(a, b), c)); }
__device__ __forceinline__ void cex(uint32_t &a, uint32_t &b) { const uint32_t l = mn(a, b), h = mx(a, b); a = l; b = h; }

// Batcher's odd-even merge of sorted runs of P into runs of 2P over N slots, as a compile-time comparator table.
struct MedCe { int a, b; };
template <int N, int P>
constexpr int oe_count()
{
    int n = 0;
    for (int k = P; k >= 1; k >>= 1)
        for (int j = k % P; j <= N - 1 - k; j += 2 * k)
            for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); i++)
                if ((i + j) / (2 * P) == (i + j + k) / (2 * P)) n++;
    return n;
}
template <int N, int P> struct OeTable { MedCe ce[oe_count<N, P>()]; };
template <int N, int P>
constexpr OeTable<N, P> oe_table()
{
    OeTable<N, P> t{};
    int n = 0;
    for (int k = P; k >= 1; k >>= 1)
        for (int j = k % P; j <= N - 1 - k; j += 2 * k)
            for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); i++)
                if ((i + j) / (2 * P) == (i + j + k) / (2 * P)) { t.ce[n].a = i + j; t.ce[n].b = i + j + k; n++; }
    return t;
}
template <int N, int P, size_t... I>
__device__ __forceinline__ void oe_apply(uint32_t (&v)[N], std::index_sequence<I...>)
{
    constexpr OeTable<N, P> t = oe_table<N, P>();
    (cex(v[t.ce[I].a], v[t.ce[I].b]), ...);
}
template <int N, int P>
__device__ __forceinline__ void oe_merge(uint32_t (&v)[N])
{
    oe_apply<N, P>(v, std::make_index_sequence<oe_count<N, P>()>{});
}

struct MedFastParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride;  // bytes per band / output block
    long long total;                  // n_images * nbands * cpr chunk columns of work
    int pitch, cpr;
    int H, y0, y1;
    int nbands;
    unsigned nblocks;
    int xcd;
};

// v_perm_b32 selector that fills a halo dword from the edge dword x of the row (same channel, position mod C).
// LEFT: halo dword h (0: row bytes -8..-5, 1: -4..-1) from the row's first dword; right: h (0: bytes 16..19 of the last
// chunk, 1: 20..23) from its last dword.
template <int C, bool LEFT, int h>
constexpr uint32_t med_edge_sel()
{
    uint32_t s = 0;
    for (int b = 0; b < 4; b++) {
        int src = 0;
        if (LEFT) { const int pos = -8 + 4 * h + b; src = ((pos % C) + C) % C; }
        else { const int pos = 4 * h + b; src = 4 - C + pos % C; }
        s |= (uint32_t)src << (8 * b);
    }
    return s;
}

// Byte at row position q (-8 <= q < 24) of the 8-dword window (2 halo dwords, the chunk, 2 halo dwords).
__device__ __forceinline__ uint32_t med_byte(const uint32_t (&w)[8], int q)
{
    const int i = q + 8;
    return __builtin_amdgcn_ubfe(w[i >> 2], (i & 3) * 8, 8);
}

template <typename F, int... I>
__device__ __forceinline__ void med_unrolled(F &f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}

template <int C, int R, int BH>
__global__ __launch_bounds__(256) void blur_median_fast_kernel(const MedFastParams p)
{
    constexpr int NR = BH + 2 * R, HB = R * C;          // rows loaded, halo bytes used either side
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned B = p.xcd ? xcd_contiguous(blockIdx.x, p.nblocks) : blockIdx.x;
    // (this lane decode and the DPP window below have a twin in blur_direct_kernel: a shared helper changed the generated code)
    const long long fl = (long long)(B * 4u + (unsigned)wave) * 62 - 1 + lane;
    const bool inrange = fl >= 0 && fl < p.total;
    const unsigned f = (unsigned)(fl < 0 ? 0 : (fl >= p.total ? p.total - 1 : fl));
    const unsigned col = f % (unsigned)p.cpr, t2 = f / (unsigned)p.cpr;
    const unsigned band = t2 % (unsigned)p.nbands;
    const long long img = (long long)(t2 / (unsigned)p.nbands);
    const bool compute = inrange && lane >= 1 && lane <= 62;
    const int row0 = p.y0 + (int)band * BH;
    const int rows_out = compute ? min(BH, p.y1 - row0) : 0;
    const bool at_start = col == 0, at_end = (int)col == p.cpr - 1;
    const uint8_t *src = p.in + img * p.in_stride + (size_t)col * 16u;
    uint8_t *dst = p.out + img * p.out_stride + (size_t)(row0 - p.y0) * (size_t)p.pitch + (size_t)col * 16u;

    uint4 rows[NR];
#pragma unroll
    for (int j = 0; j < NR; j++)
        rows[j] = *reinterpret_cast<const uint4 *>(src + (size_t)min(max(row0 - R + j, 0), p.H - 1) * (size_t)p.pitch);

    uint32_t w[NR][8];
#pragma unroll
    for (int j = 0; j < NR; j++) {
        const uint4 c = rows[j];
        w[j][2] = c.x; w[j][3] = c.y; w[j][4] = c.z; w[j][5] = c.w;
        const uint32_t l0 = __builtin_amdgcn_update_dpp(0u, c.z, 0x138, 0xf, 0xf, false);   // wave_shr:1: lane i-1's last two
        const uint32_t l1 = __builtin_amdgcn_update_dpp(0u, c.w, 0x138, 0xf, 0xf, false);
        const uint32_t r0 = __builtin_amdgcn_update_dpp(0u, c.x, 0x130, 0xf, 0xf, false);   // wave_shl:1: lane i+1's first two
        const uint32_t r1 = __builtin_amdgcn_update_dpp(0u, c.y, 0x130, 0xf, 0xf, false);
        w[j][0] = at_start ? __builtin_amdgcn_perm(c.x, c.x, med_edge_sel<C, true, 0>()) : l0;
        w[j][1] = at_start ? __builtin_amdgcn_perm(c.x, c.x, med_edge_sel<C, true, 1>()) : l1;
        w[j][6] = at_end ? __builtin_amdgcn_perm(c.w, c.w, med_edge_sel<C, false, 0>()) : r0;
        w[j][7] = at_end ? __builtin_amdgcn_perm(c.w, c.w, med_edge_sel<C, false, 1>()) : r1;
    }

    // one output row per call, i a compile-time constant: a body this size is past what `#pragma unroll` unrolls, and a
    // runtime row index would put the window w[][] in scratch
    auto out_row = [&](auto row_index) {
        constexpr int i = decltype(row_index)::value;
        uint32_t o[16];
        if constexpr (R == 1) {
            uint32_t lo[16 + 2 * HB], mid[16 + 2 * HB], hi[16 + 2 * HB];
#pragma unroll
            for (int q = -HB; q < 16 + HB; q++) {
                const uint32_t a = med_byte(w[i], q), b = med_byte(w[i + 1], q), c = med_byte(w[i + 2], q);
                lo[q + HB] = min3u(a, b, c); mid[q + HB] = med3u(a, b, c); hi[q + HB] = max3u(a, b, c);
            }
#pragma unroll
            for (int x = 0; x < 16; x++) {
                const int q = x + HB;
                o[x] = med3u(max3u(lo[q - C], lo[q], lo[q + C]), med3u(mid[q - C], mid[q], mid[q + C]),
                             min3u(hi[q - C], hi[q], hi[q + C]));
            }
        } else {
            // sorted columns at row positions [-2C, 16 + 2C), merged pairs (p, p + C) at [-2C, 16 + C)
            uint32_t s[16 + 2 * HB][5];
#pragma unroll
            for (int q = -HB; q < 16 + HB; q++) {
                uint32_t v[8];
#pragma unroll
                for (int e = 0; e < 5; e++) v[e] = med_byte(w[i + e], q);
                v[5] = v[6] = v[7] = MED_PAD;
                oe_merge<8, 1>(v); oe_merge<8, 2>(v); oe_merge<8, 4>(v);
#pragma unroll
                for (int e = 0; e < 5; e++) s[q + HB][e] = v[e];
            }
            uint32_t m[16 + HB + C][10];
#pragma unroll
            for (int q = 0; q < 16 + HB + C; q++) {          // pair of columns q - HB and q - HB + C
                uint32_t v[16];
#pragma unroll
                for (int e = 0; e < 5; e++) { v[e] = s[q][e]; v[8 + e] = s[q + C][e]; }
                v[5] = v[6] = v[7] = v[13] = v[14] = v[15] = MED_PAD;
                oe_merge<16, 8>(v);
#pragma unroll
                for (int e = 0; e < 10; e++) m[q][e] = v[e];
            }
#pragma unroll
            for (int x = 0; x < 16; x++) {
                const int q = x + HB;                            // own column; pairs at q - 2C and q + C
                uint32_t a[32];
#pragma unroll
                for (int e = 0; e < 32; e++) a[e] = MED_PAD;
#pragma unroll
                for (int e = 0; e < 10; e++) { a[e] = m[q - 2 * C][e]; a[16 + e] = m[q + C][e]; }
                oe_merge<32, 16>(a);                             // ranks 7..12 of the 20 are all that is used
                // rank 12 of (a[0..20) U s[q][0..5)): the smallest over i = 0..5 of max(s[q][i-1], a[12-i])
                uint32_t r = a[12];
#pragma unroll
                for (int e = 1; e <= 5; e++) r = mn(r, mx(s[q][e - 1], a[12 - e]));
                o[x] = r;
            }
        }
        if (i < rows_out) {
            u32x4 st;
            st.x = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
            st.y = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
            st.z = o[8] | (o[9] << 8) | (o[10] << 16) | (o[11] << 24);
            st.w = o[12] | (o[13] << 8) | (o[14] << 16) | (o[15] << 24);
            *reinterpret_cast<u32x4 *>(dst + (size_t)i * (size_t)p.pitch) = st;
        }
    };
    med_unrolled(out_row, std::make_integer_sequence<int, BH>{});
}

struct MedGenericParams {
    const uint8_t *in;
    uint8_t *out;
    long long in_stride, out_stride, block, total;   // block = output bytes per band (rows * pitch)
    int width, channels, pitch, H, y0;
};

template <int R>
__global__ __launch_bounds__(256) void blur_median_generic_kernel(const MedGenericParams p)
{
    constexpr int D = 2 * R + 1, N = D * D, NW = (N + 1) / 2, K = (N - 1) / 2;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        const BytePos q = byte_pos(idx, p.block, p.pitch, p.channels, p.y0, p.in, p.in_stride);
        const uint8_t *src = q.src + q.c;
        uint32_t V[NW];
#pragma unroll
        for (int e = 0; e < NW; e++) V[e] = 0u;
        V[NW - 1] = 255u << 16;                         // N is odd: the spare field holds 255, never below a candidate
#pragma unroll
        for (int j = 0; j < D; j++) {
            const uint8_t *rowp = src + (size_t)min(max(q.y + j - R, 0), p.H - 1) * (size_t)p.pitch;
#pragma unroll
            for (int i = 0; i < D; i++) {
                const int e = j * D + i;
                const uint32_t v = rowp[(size_t)min(max(q.x + i - R, 0), p.width - 1) * (size_t)p.channels];
                V[e >> 1] |= v << (16 * (e & 1));
            }
        }
        // (0xff + t - v) in a 16-bit field has bit 8 set exactly when v < t (0 <= v, t <= 255): no borrow between fields
        uint32_t ans = 0;
#pragma unroll
        for (int bit = 7; bit >= 0; bit--) {
            const uint32_t t = ans | (1u << bit);
            const uint32_t T = 0x00ff00ffu + (t | (t << 16));
            uint32_t acc = 0;
#pragma unroll
            for (int e = 0; e < NW; e++) acc += (T - V[e]) & 0x01000100u;
            const uint32_t below = ((acc & 0xffffu) + (acc >> 16)) >> 8;
            if (below <= (uint32_t)K) ans = t;
        }
        p.out[q.img * p.out_stride + q.rem] = (uint8_t)ans;
    }
}

int launch_median_fast(const LaunchDesc &d)
{
    set_last_kernel("blur_median_fast_kernel");
    MedFastParams p{};
    fill_band(p, d);
    p.cpr = p.pitch / 16; p.y1 = d.y1;
    const dim3 grid = direct_grid(p, d, med_bh(d.filter->radius)), block(256);
    p.xcd = p.nblocks >= 16 ? 1 : 0;
    return dispatch<1, 2, 3, 4>(d.channels, [&](auto C) {
        return dispatch<1, 2>(d.filter->radius, [&](auto R) { return do_launch(blur_median_fast_kernel<C, R, med_bh(R)>, grid, block, 0, d, p); });
    });
}

int launch_median_generic(const LaunchDesc &d)
{
    set_last_kernel("blur_median_generic_kernel");
    MedGenericParams p{};
    const dim3 grid = fill_generic(p, d);
    return dispatch<1, 2, 3, 4, 5, 6, 7>(d.filter->radius, [&](auto R) {
        return do_launch(blur_median_generic_kernel<R>, grid, dim3(256), 0, d, p);
    });
}

}  // namespace

int launch_median(const LaunchDesc &d)
{
    const int st = launch_checks(d, FilterKind::MEDIAN, [](const Filter &f) { return f.radius >= 1 && f.radius <= MI_BLUR_MEDIAN_MAX_RADIUS; });
    if (st != LAUNCH_GO) return st;
    const bool fast = d.filter->radius <= 2 && tile_aligned(d) && direct_fits(d);
    return fast ? launch_median_fast(d) : launch_median_generic(d);
}

}  // namespace mi_blur
