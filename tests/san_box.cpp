// host-only sanitizer run of the integral images and the box filters, in three parts:
//   1. the arithmetic the kernels share with the host (filter.h): box_div() against the division at every rounding
//      boundary of every window area, box_root() against the comparison it is defined by around every threshold, and
//      box_axis() against a clamped walk along one axis for every position, extent and radius of a spread;
//   2. the units of blur_integral_tiled_kernel and blur_box_tiled_kernel walked as the kernels walk them: every 16-byte
//      chunk a thread touches inside its row, every pixel of a row owned exactly once, the work buffer's size;
//   3. the CPU device (cpu_integral, cpu_box_from_integral) against loops written here from the header's text: 64-bit
//      running sums reduced modulo 2^32 and a clamped walk over every window, exact-size heap buffers (ASan sees any
//      over-read or over-write, UBSan any signed overflow), one table or both, in place for THRESHOLD.
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mi_blur;

static uint32_t rng_state = 24681357u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int fail(const char *what, long long a, long long b, long long c)
{
    printf("FAILED %s %lld %lld %lld\n", what, a, b, c);
    return 1;
}

// Part 1.
static int arithmetic()
{
    int bad = 0;
    for (int rx = 0; rx <= MI_BLUR_BOX_MAX_RADIUS; rx++)
        for (int ry = 0; ry <= rx; ry++) {
            const mi_blur_box k{MI_BLUR_BOX_MEAN, rx, ry, 0, 0};
            const BoxConst bc = box_const(k);
            const uint32_t A = bc.A;
            if (A != (uint32_t)((2 * rx + 1) * (2 * ry + 1))) bad += fail("area", rx, ry, A);
            for (uint32_t v = 1; v <= 255; v++) {                       // 2 Sum + A = 2 A v is the boundary; it is odd + odd: never met
                const uint32_t first = (A * (2 * v - 1) + 1) / 2;
                for (uint32_t s = first - 1; s <= first; s++) {
                    const uint32_t n = 2 * s + A;
                    if (box_div(n, 2 * A, bc.inv_2a) != n / (2 * A) || n / (2 * A) != v - (first - s)) bad += fail("box_div", A, s, v);
                }
            }
            if (box_div(A, 2 * A, bc.inv_2a) != 0 || box_div(511 * A, 2 * A, bc.inv_2a) != 255) bad += fail("box_div ends", A, 0, 0);
            for (int s = 1; s <= 128; s++) {
                const uint64_t T = ((uint64_t)(2 * s - 1) * (2 * s - 1) * A * A + 3) / 4;
                for (uint64_t D = T - 1; D <= T; D++)
                    if (box_root(D, A, bc.inv_a) != s - (int)(T - D)) bad += fail("box_root", A, s, (long long)D);
            }
            if (box_root(0, A, bc.inv_a) != 0 || box_root((uint64_t)65025 * A * A, A, bc.inv_a) != 128) bad += fail("box_root ends", A, 0, 0);
        }
    const int extents[] = {1, 2, 3, 7, 16, 100, 255, 256, 300}, radii[] = {0, 1, 2, 7, 16, 126, 127};
    for (int N : extents)
        for (int r : radii) {
            std::vector<long long> F(N);
            long long run = 0;
            for (int i = 0; i < N; i++) { run += 1 + (i * 37 + N) % 255; F[i] = run; }
            for (int X = 0; X < N; X++) {
                long long want = 0;
                for (int d = -r; d <= r; d++) { const int i = X + d < 0 ? 0 : X + d > N - 1 ? N - 1 : X + d; want += F[i] - (i ? F[i - 1] : 0); }
                const BoxAxis ax = box_axis(X, N, r);
                long long got = 0;
                for (int t = 0; t < 5; t++) {
                    if (ax.idx[t] < 0 || ax.idx[t] >= N) bad += fail("axis index", N, r, X);
                    else got += (long long)ax.coef[t] * F[ax.idx[t]];
                }
                if (got != want) bad += fail("axis sum", N, r, X);
            }
        }
    return bad;
}

// Part 2 for one shape.
static int walk(int W, int H, int C, int n_images)
{
    int bad = 0;
    if (!hist_image_ok(W, H, C)) return fail("image refused", W, H, C);
    const long long row_e = (long long)W * C;
    if (integral_tiled_ok(W)) {
        const int threads = integral_threads(W);
        if (threads % 64 || threads > INTEGRAL_MAX_THREADS || threads * INTEGRAL_PIXELS < W || (threads - 64) * INTEGRAL_PIXELS >= W) bad += fail("threads", W, threads, 0);
        std::vector<uint8_t> seen((size_t)W, 0);
        for (int t = 0; t < threads; t++) {
            if (INTEGRAL_PIXELS * t >= W) continue;                     // the kernel's `active`
            const long long first = (long long)t * INTEGRAL_PIXELS * C;  // bytes of the input row, dwords of a table row
            if (first % 16 || first + 16 * C > row_e) bad += fail("thread's run", W, C, t);
            for (int px = 0; px < INTEGRAL_PIXELS; px++) seen[(size_t)t * INTEGRAL_PIXELS + px]++;
        }
        for (int x = 0; x < W; x++)
            if (seen[x] != 1) bad += fail("pixel not owned once", W, x, seen[x]);
        for (int band : {1, 8, INTEGRAL_BAND, 64, 256}) {
            const int nb = integral_bands(H, band);
            if ((long long)nb * band < H || (long long)(nb - 1) * band >= H) bad += fail("bands", H, band, nb);
            for (int tables = 1; tables <= 2; tables++)
                if (integral_work_bytes(W, H, C, n_images, tables, band) != (size_t)n_images * nb * tables * row_e * 4) bad += fail("work bytes", W, H, band);
        }
    }
    if (box_tiled_ok(W, C)) {
        const long long cpr = row_e / 16;
        for (int rx : {0, 1, 16, 127})
            for (long long col = 0; col < cpr; col++) {
                const int b0 = (int)col * 16, x_first = b0 / C, x_last = (b0 + 15) / C;
                if (x_last >= W) bad += fail("chunk beyond the row", W, C, col);
                if (x_first > rx && x_last + rx < W) {                  // the interior: all four runs of 16 dwords inside the row
                    const long long left = b0 - (long long)(rx + 1) * C, right = b0 + (long long)rx * C;
                    if (left < 0 || right + 16 > row_e) bad += fail("corner run", W, C, col);
                }
            }
    }
    return bad;
}

// Part 3 for one case.
static int run_case(int W, int H, int C, int n_images, int op, int rx, int ry, int n_threads)
{
    mi_blur_box k{op, rx, ry, 0, 0};
    if (op == MI_BLUR_BOX_THRESHOLD) { k.offset = rnd_range(-255, 255); k.invert = (int)(rnd() & 1); }
    if (!box_ok(&k)) return fail("struct refused", op, rx, ry);
    const size_t px = (size_t)W * H, words = (size_t)n_images * px * C;
    uint8_t *in = (uint8_t *)malloc(words), *out = (uint8_t *)malloc(words);
    uint32_t *S = (uint32_t *)malloc(words * 4), *Q = (uint32_t *)malloc(words * 4), *alone = (uint32_t *)malloc(words * 4);
    const int flat = (int)(rnd() % 4);
    for (size_t i = 0; i < words; i++) in[i] = (uint8_t)(flat == 0 ? 255 : flat == 1 ? 100 + rnd() % 3 : rnd());
    int bad = 0;
    // the tables
    std::vector<uint32_t> wantS(words), wantQ(words);
    for (int i = 0; i < n_images; i++)
        for (int c = 0; c < C; c++)
            for (int y = 0; y < H; y++) {
                uint64_t rs = 0, rq = 0;
                for (int x = 0; x < W; x++) {
                    const size_t e = (((size_t)i * H + y) * W + x) * C + c;
                    rs += in[e]; rq += (uint64_t)in[e] * in[e];
                    const uint64_t us = y ? wantS[e - (size_t)W * C] : 0, uq = y ? wantQ[e - (size_t)W * C] : 0;
                    wantS[e] = (uint32_t)(us + rs); wantQ[e] = (uint32_t)(uq + rq);
                }
            }
    if (!integral_args_ok(in, S, Q, W, H, C, n_images, 4)) bad += fail("arguments refused", W, H, C);
    if (!cpu_integral(in, S, Q, W, H, C, n_images, n_threads)) bad += fail("no memory", W, H, C);
    if (memcmp(S, wantS.data(), words * 4) || memcmp(Q, wantQ.data(), words * 4)) bad += fail("tables differ", W, H, C);
    if (!cpu_integral(in, alone, nullptr, W, H, C, n_images, n_threads) || memcmp(alone, wantS.data(), words * 4)) bad += fail("S alone differs", W, H, C);
    if (!cpu_integral(in, nullptr, alone, W, H, C, n_images, n_threads) || memcmp(alone, wantQ.data(), words * 4)) bad += fail("Q alone differs", W, H, C);
    // the windows, by a clamped walk
    std::vector<uint8_t> want(words);
    const long long A = (long long)(2 * rx + 1) * (2 * ry + 1);
    for (int i = 0; i < n_images; i++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                for (int c = 0; c < C; c++) {
                    long long s = 0, q = 0;
                    for (int dy = -ry; dy <= ry; dy++) {
                        const int yy = y + dy < 0 ? 0 : y + dy > H - 1 ? H - 1 : y + dy;
                        for (int dx = -rx; dx <= rx; dx++) {
                            const int xx = x + dx < 0 ? 0 : x + dx > W - 1 ? W - 1 : x + dx;
                            const long long v = in[(((size_t)i * H + yy) * W + xx) * C + c];
                            s += v; q += v * v;
                        }
                    }
                    const size_t e = (((size_t)i * H + y) * W + x) * C + c;
                    int v;
                    if (op == MI_BLUR_BOX_MEAN) v = (int)((2 * s + A) / (2 * A));
                    else if (op == MI_BLUR_BOX_STDDEV) {
                        const long long D = A * q - s * s;
                        for (v = 0; v < 128 && (long long)(2 * v + 1) * (2 * v + 1) * A * A <= 4 * D; v++) {}
                    } else v = (A * (in[e] + k.offset) > s) != (k.invert != 0) ? 255 : 0;
                    want[e] = (uint8_t)v;
                }
    const uint8_t *img = op == MI_BLUR_BOX_THRESHOLD ? in : nullptr;
    const uint32_t *sq = op == MI_BLUR_BOX_STDDEV ? Q : nullptr;
    if (!box_from_args_ok(img, S, sq, out, W, H, C, n_images, &k) && ((uintptr_t)S % 16 == 0 && (uintptr_t)Q % 16 == 0)) bad += fail("box arguments refused", W, H, C);
    cpu_box_from_integral(img, S, sq, out, W, H, C, n_images, k, n_threads);
    if (memcmp(out, want.data(), words)) bad += fail("bytes differ", W, H, op);
    if (op == MI_BLUR_BOX_THRESHOLD) {                                  // in place: the image is read only at the byte that is written
        cpu_box_from_integral(in, S, nullptr, in, W, H, C, n_images, k, n_threads);
        if (memcmp(in, want.data(), words)) bad += fail("bytes differ in place", W, H, op);
    }
    free(in); free(out); free(S); free(Q); free(alone);
    return bad;
}

int main()
{
    int bad = arithmetic();
    if (!bad) printf("arithmetic clean\n");

    int before = bad;
    const int shapes[][2] = {{16, 1}, {1008, 3}, {1024, INTEGRAL_BAND}, {1040, INTEGRAL_BAND + 1}, {INTEGRAL_MAX_W, 2 * INTEGRAL_BAND + 1}, {4112, 4097}, {48, 40},
                             {272, 260}, {1920, 1080}, {20, 7}, {17, 5}};
    for (const auto &s : shapes)
        for (int C = 1; C <= 4; C++) bad += walk(s[0], s[1], C, 3);
    if (integral_tiled_ok(INTEGRAL_MAX_W + 16) || integral_tiled_ok(17) || !integral_tiled_ok(INTEGRAL_MAX_W)) bad += fail("tiled rule", 0, 0, 0);
    if (bad == before) printf("geometry clean\n");

    before = bad;
    const int sizes[][2] = {{1, 1}, {1, 9}, {9, 1}, {16, 4}, {13, 5}, {40, 33}};
    const int radii[][2] = {{0, 0}, {1, 1}, {1, 7}, {16, 16}, {127, 0}, {0, 127}, {127, 127}};
    for (int op = 0; op <= MI_BLUR_BOX_THRESHOLD; op++)
        for (const auto &s : sizes)
            for (const auto &r : radii)
                if (s[0] * s[1] <= 100 || r[0] + r[1] <= 200)              // the walk over 255 x 255 windows: the small images only
                    bad += run_case(s[0], s[1], 1 + (int)(rnd() % 4), 1 + (int)(rnd() % 2), op, r[0], r[1], 1 + (int)(rnd() % 4));
    for (int rep = 0; rep < 30; rep++)
        bad += run_case(rnd_range(1, 60), rnd_range(1, 50), rnd_range(1, 4), rnd_range(1, 3), rnd_range(0, 2), rnd_range(0, 9), rnd_range(0, 9), rnd_range(1, 5));
    bad += run_case(70, 300, 3, 2, MI_BLUR_BOX_STDDEV, 3, 5, 4);        // more rows than one band of the CPU device
    if (bad == before) printf("integral and box cases clean\n");
    return bad ? 1 : 0;
}
