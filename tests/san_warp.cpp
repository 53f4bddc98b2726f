// host-only sanitizer run: the CPU device's affine warp (cpu_blur_batch with a WARP filter) against a scalar loop written
// here from the header's text, on random small shapes, on edge maps (the range limits, far-away and degenerate maps) and
// on the maps at the header's limits that the GPU tests run (LIMIT_MAPS of tests/warp_ref.py), with exact-size heap buffers so ASan sees any over-read / over-write and UBSan any overflow of the coordinate arithmetic.
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

typedef long long i64;

static i64 floor_shift(i64 v, int s) { return v >= 0 ? v >> s : -((-v + ((i64)1 << s) - 1) >> s); }   // floor(v / 2^s) without shifting a negative

static i64 tap(const uint8_t *img, i64 W, i64 H, int C, int c, int border, int fill, i64 y, i64 x)
{
    if (border == MI_BLUR_WARP_CONSTANT && (x < 0 || x > W - 1 || y < 0 || y > H - 1)) return fill;
    x = x < 0 ? 0 : x > W - 1 ? W - 1 : x;
    y = y < 0 ? 0 : y > H - 1 ? H - 1 : y;
    return img[(y * W + x) * C + c];
}

static int run_case(int W, int H, int C, int n, int nt, const mi_blur_warp &w, unsigned *seed)
{
    auto rnd = [&](int k) { *seed = *seed * 1664525u + 1013904223u; return (int)((*seed >> 8) % (unsigned)k); };
    const int Wo = w.out_width, Ho = w.out_height;
    const size_t isz = (size_t)W * H * C, osz = (size_t)Wo * Ho * C;
    uint8_t *in = (uint8_t *)malloc(isz * n), *out = (uint8_t *)malloc(osz * n), *want = (uint8_t *)malloc(osz * n);
    for (size_t i = 0; i < isz * n; i++) in[i] = (uint8_t)rnd(256);
    memset(out, 0xA5, osz * n);
    mi_blur::Filter f;
    if (mi_blur::filter_warp(&w, &f) != MI_BLUR_OK || !mi_blur::warp_ok(&w, W, H, C)) { printf("REFUSED W%d H%d Wo%d Ho%d\n", W, H, Wo, Ho); return 1; }
    mi_blur::cpu_blur_batch(in, out, W, H, C, f, n, 0, H, nt, 0, 0);
    for (int i = 0; i < n; i++)
        for (int Y = 0; Y < Ho; Y++)
            for (int X = 0; X < Wo; X++) {
                const i64 sx = w.m[0] * X + w.m[1] * Y + w.m[2], sy = w.m[3] * X + w.m[4] * Y + w.m[5];
                for (int c = 0; c < C; c++) {
                    const uint8_t *p = in + i * isz;
                    i64 v;
                    if (w.mode == MI_BLUR_RESIZE_NEAREST) {
                        v = tap(p, W, H, C, c, w.border, w.fill, floor_shift(sy + 32768, 16), floor_shift(sx + 32768, 16));
                    } else {
                        const i64 px = floor_shift(sx + 16, 5), py = floor_shift(sy + 16, 5);
                        const i64 x0 = floor_shift(px, 11), y0 = floor_shift(py, 11), fx = px - x0 * 2048, fy = py - y0 * 2048;
                        const i64 top = (2048 - fx) * tap(p, W, H, C, c, w.border, w.fill, y0, x0) + fx * tap(p, W, H, C, c, w.border, w.fill, y0, x0 + 1);
                        const i64 bot = (2048 - fx) * tap(p, W, H, C, c, w.border, w.fill, y0 + 1, x0) + fx * tap(p, W, H, C, c, w.border, w.fill, y0 + 1, x0 + 1);
                        v = ((2048 - fy) * top + fy * bot + (1 << 21)) >> 22;
                    }
                    want[i * osz + ((size_t)Y * Wo + X) * C + c] = (uint8_t)v;
                }
            }
    const int bad = memcmp(out, want, osz * n);
    if (bad) printf("MISMATCH W%d H%d Wo%d Ho%d C%d n%d nt%d mode%d border%d m %lld %lld %lld %lld %lld %lld\n", W, H, Wo, Ho, C, n, nt, w.mode, w.border,
                    (i64)w.m[0], (i64)w.m[1], (i64)w.m[2], (i64)w.m[3], (i64)w.m[4], (i64)w.m[5]);
    free(in); free(out); free(want);
    return bad ? 1 : 0;
}

int main()
{
    unsigned s = 8642;
    auto rnd = [&](int n) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (unsigned)n); };
    const i64 Q = 65536, LIN = (i64)1 << 26, OFF = (i64)1 << 46;
    int cases = 0;
    for (int it = 0; it < 300; it++) {
        const int W = 1 + rnd(40), H = 1 + rnd(40), C = 1 + rnd(5), n = 1 + rnd(3), nt = 1 + rnd(3);
        mi_blur_warp w{1 + rnd(40), 1 + rnd(40), rnd(2), rnd(2), rnd(256), {}};
        for (int i = 0; i < 6; i++) w.m[i] = i % 3 == 2 ? (i64)rnd(120 * 65536) - 40 * Q : (i64)rnd(4 * 65536) - 2 * Q;
        if (run_case(W, H, C, n, nt, w, &s)) return 1;
        cases++;
    }
    // edge maps: the limits in every sign, everything far outside on each side, a constant position, one-pixel images
    const i64 edge[][6] = {{LIN, LIN, OFF, LIN, LIN, OFF}, {-LIN, -LIN, -OFF, -LIN, -LIN, -OFF}, {LIN, -LIN, -OFF, -LIN, LIN, OFF}, {0, 0, 0, 0, 0, 0},
                           {0, 0, OFF, 0, 0, -OFF}, {Q, 0, -OFF, 0, Q, 0}, {Q, 0, 0, 0, Q, OFF}, {1, 0, -1, 0, 1, -1}, {Q, 0, -16, 0, Q, -17},
                           {Q, 0, -2 * Q, 0, Q, -2 * Q}, {Q, 0, -2 * Q - 17, 0, Q, 9 * Q - 16}, {-Q, 0, 8 * Q + 15, 0, -Q, 8 * Q + 16}, {LIN, 0, -LIN * 3, 0, LIN, -LIN * 2}};
    for (const auto &m : edge)
        for (int mode = 0; mode < 2; mode++)
            for (int border = 0; border < 2; border++)
                for (int shape = 0; shape < 3; shape++) {
                    const int W = shape == 0 ? 1 : shape == 1 ? 9 : 16, H = shape == 0 ? 1 : shape == 1 ? 8 : 3;
                    mi_blur_warp w{shape == 0 ? 1 : 7, shape == 0 ? 1 : 6, mode, border, 200, {}};
                    for (int i = 0; i < 6; i++) w.m[i] = m[i];
                    if (run_case(W, H, 1 + shape, 2, 2, w, &s)) return 1;
                    cases++;
                }
    // the maps of tests/warp_ref.py's LIMIT_MAPS on its shapes: 64 x 64 to 80 x 40 (96 x 40 for 3 channels), 1-4 channels
    const i64 limits[][6] = {{LIN, 0, 0, 0, LIN, 0}, {-LIN, LIN, 63 * Q, LIN, -LIN, 63 * Q}, {LIN, 0, -79 * LIN + 5 * Q, 0, LIN, -39 * LIN + 7 * Q + 123},
                             {Q, 0, OFF, 0, Q, OFF}, {-Q, 0, -OFF, 0, -Q, -OFF}, {Q, 0, -OFF, 0, Q, 3 * Q}, {LIN, LIN, OFF, -LIN, -LIN, -OFF},
                             {0, 0, 10 * Q + 777, 0, 0, 20 * Q + 31111}, {Q, 0, 0, Q, 0, Q / 3}, {1, 0, 5 * Q, 0, 1, 6 * Q + 65535},
                             {LIN, 0, -40 * LIN + 30 * Q, 0, Q, 0}, {Q, 0, 0, LIN, Q, -20 * LIN}};
    for (const auto &m : limits)
        for (int mode = 0; mode < 2; mode++)
            for (int border = 0; border < 2; border++)
                for (int C = 1; C <= 4; C++) {
                    mi_blur_warp w{C == 3 ? 96 : 80, 40, mode, border, 173, {}};
                    for (int i = 0; i < 6; i++) w.m[i] = m[i];
                    if (run_case(64, 64, C, 2, 3, w, &s)) return 1;
                    cases++;
                }
    printf("%d random and edge warp cases clean\n", cases);
    return 0;
}
