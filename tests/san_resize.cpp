// host-only sanitizer run: the CPU device's resize (cpu_blur_batch with a RESIZE filter) against a scalar loop written
// here from the header's text, on random small shapes, exact-size heap buffers so ASan sees any over-read / over-write.
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

// One axis, in 64-bit signed arithmetic with an explicit floor.
static void axis(long long n_in, long long n_out, int mode, long long X, long long *a, long long *b, long long *f)
{
    const long long den = 2 * n_out;
    if (mode == MI_BLUR_RESIZE_NEAREST) { *a = *b = ((2 * X + 1) * n_in) / den; *f = 0; return; }
    const long long num = (2 * X + 1) * n_in - n_out;
    long long i0 = num / den;
    if (num % den < 0) i0--;                             // floor towards minus infinity
    const long long rem = num - i0 * den;
    *f = (rem * 2048 + n_out) / den;
    *a = i0 < 0 ? 0 : i0 > n_in - 1 ? n_in - 1 : i0;
    *b = i0 + 1 < 0 ? 0 : i0 + 1 > n_in - 1 ? n_in - 1 : i0 + 1;
}

int main()
{
    unsigned s = 4321;
    auto rnd = [&](int n) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (unsigned)n); };
    int cases = 0;
    for (int it = 0; it < 400; it++) {
        const int W = 1 + rnd(40), H = 1 + rnd(40), Wo = 1 + rnd(40), Ho = 1 + rnd(40), C = 1 + rnd(5), n = 1 + rnd(3), nt = 1 + rnd(3);
        const int mode = rnd(2);
        const size_t isz = (size_t)W * H * C, osz = (size_t)Wo * Ho * C;
        uint8_t *in = (uint8_t *)malloc(isz * n), *out = (uint8_t *)malloc(osz * n), *want = (uint8_t *)malloc(osz * n);
        for (size_t i = 0; i < isz * n; i++) in[i] = (uint8_t)rnd(256);
        memset(out, 0xA5, osz * n);
        const mi_blur_resize r{Wo, Ho, mode};
        mi_blur::Filter f;
        if (mi_blur::filter_resize(&r, &f) != MI_BLUR_OK || !mi_blur::resize_ok(&r, W, H, C)) { printf("REFUSED W%d H%d Wo%d Ho%d\n", W, H, Wo, Ho); return 1; }
        mi_blur::cpu_blur_batch(in, out, W, H, C, f, n, 0, H, nt, 0, 0);
        for (int i = 0; i < n; i++)
            for (int Y = 0; Y < Ho; Y++)
                for (int X = 0; X < Wo; X++) {
                    long long xa, xb, fx, ya, yb, fy;
                    axis(W, Wo, mode, X, &xa, &xb, &fx);
                    axis(H, Ho, mode, Y, &ya, &yb, &fy);
                    for (int c = 0; c < C; c++) {
                        const uint8_t *p = in + i * isz + c;
                        const long long top = (2048 - fx) * p[(ya * W + xa) * C] + fx * p[(ya * W + xb) * C];
                        const long long bot = (2048 - fx) * p[(yb * W + xa) * C] + fx * p[(yb * W + xb) * C];
                        const long long v = mode == MI_BLUR_RESIZE_NEAREST ? p[(ya * W + xa) * C] : ((2048 - fy) * top + fy * bot + (1 << 21)) >> 22;
                        want[i * osz + ((size_t)Y * Wo + X) * C + c] = (uint8_t)v;
                    }
                }
        if (memcmp(out, want, osz * n)) { printf("MISMATCH W%d H%d Wo%d Ho%d C%d n%d nt%d mode%d\n", W, H, Wo, Ho, C, n, nt, mode); return 1; }
        free(in); free(out); free(want); cases++;
    }
    printf("%d random resize cases clean\n", cases);
    return 0;
}
