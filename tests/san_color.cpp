// host-only sanitizer run of the colour transform, in three parts:
//   1. the units of blur_color_tiled_kernel (filter.h) walked over a spread of launches as the kernel walks them: every
//      16-byte chunk a thread loads against the input image, every chunk it stores against the output image, every
//      group taken exactly once;
//   2. the CPU device (cpu_blur_batch with a COLOR filter) against a scalar loop written here from the header's text,
//      random transforms of every (C, Co, lut) at 1 x 1, 1 x 17 and 5 x 13 in exact-size heap buffers, so ASan sees any
//      over-read or over-write;
//   3. the same with the limit weights: rows that sum to 2^18, biases of +-2^26, shifts 0 and 16.
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mi_blur;

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int fail(const char *what, int W, int H, int C, int Co, int lut)
{
    printf("FAILED %s W%d H%d C%d Co%d lut%d\n", what, W, H, C, Co, lut);
    return 1;
}

// Part 1 for one launch; 0 when clean.
static int walk(int W, int H, int C, int Co, int n_images)
{
    if (!color_flat_ok(W, H) || !color_image_ok(Co, W, H, C)) return fail("not a tiled launch", W, H, C, Co, 0);
    const long long groups = (long long)W * H / COLOR_GROUP, in_bytes = (long long)W * H * C, out_bytes = (long long)W * H * Co;
    const int runs = color_runs(W, H);
    if ((long long)runs * COLOR_RUN < groups || (long long)(runs - 1) * COLOR_RUN >= groups) return fail("runs", W, H, C, Co, 0);
    std::vector<uint8_t> seen((size_t)groups, 0);
    for (long long L = 0; L < (long long)n_images * runs; L++) {
        const long long img = L / runs, run = L - img * runs;
        if (img >= n_images) return fail("image", W, H, C, Co, 0);
        for (int t = 0; t < COLOR_RUN; t++) {
            const long long g = run * COLOR_RUN + t;
            if (g >= groups) continue;
            if (g * 16 * C + 16 * C > in_bytes) return fail("input chunk", W, H, C, Co, 0);
            if (g * 16 * Co + 16 * Co > out_bytes) return fail("output chunk", W, H, C, Co, 0);
            if (img == 0) seen[(size_t)g]++;
        }
    }
    for (long long g = 0; g < groups; g++)
        if (seen[(size_t)g] != 1) return fail("group not taken once", W, H, C, Co, 0);
    return 0;
}

// The header's text, in 64 bits.
static uint8_t scalar(const mi_blur_color &k, int C, const uint8_t *px, int o)
{
    long long acc = k.bias[o];
    for (int i = 0; i < C; i++) acc += (long long)k.m[o][i] * px[i];
    long long v = acc >> k.shift;
    v = v < 0 ? 0 : v > 255 ? 255 : v;
    return k.lut_on ? k.lut[o][v] : (uint8_t)v;
}

static mi_blur_color make(int Co, int shift, int lut, bool limit)
{
    mi_blur_color k{};
    memset(&k, 0x7b, sizeof k);                                 // rows beyond Co hold garbage
    k.out_channels = Co; k.shift = shift; k.lut_on = lut;
    for (int o = 0; o < Co; o++) {
        if (limit) {
            const int big = rnd_range(0, 3);
            long long rest = COLOR_ROW_MAX;
            for (int i = 0; i < 4; i++) {
                if (i == big) continue;
                k.m[o][i] = rnd_range(-30000, 30000);
                rest -= k.m[o][i] < 0 ? -k.m[o][i] : k.m[o][i];
            }
            k.m[o][big] = (int32_t)(rnd() & 1 ? rest : -rest);
            k.bias[o] = (int32_t)(rnd() & 1 ? COLOR_BIAS_MAX : -COLOR_BIAS_MAX);
        } else {
            const int unit = 1 << shift;
            for (int i = 0; i < 4; i++) k.m[o][i] = rnd_range(-unit, unit);
            k.bias[o] = rnd_range(-200, 200) * unit;
        }
        for (int v = 0; v < 256; v++) k.lut[o][v] = (uint8_t)(rnd() & 0xff);
    }
    return k;
}

// Parts 2 and 3 for one case; 0 when clean.
static int run_case(int W, int H, int C, const mi_blur_color &k, int n_images, int n_threads)
{
    const int Co = k.out_channels;
    Filter f;
    if (filter_color(&k, &f) != MI_BLUR_OK || !color_image_ok(Co, W, H, C)) return fail("refused", W, H, C, Co, k.lut_on);
    const size_t in_n = (size_t)n_images * W * H * C, out_n = (size_t)n_images * W * H * Co;
    uint8_t *in = (uint8_t *)malloc(in_n), *out = (uint8_t *)malloc(out_n);
    for (size_t i = 0; i < in_n; i++) in[i] = (uint8_t)(rnd() % 5 == 0 ? (rnd() & 1 ? 255 : 0) : rnd() & 0xff);
    memset(out, 0xA5, out_n);
    cpu_blur_batch(in, out, W, H, C, f, n_images, 0, H, n_threads);
    int bad = 0;
    for (size_t p = 0; p < (size_t)n_images * W * H && !bad; p++)
        for (int o = 0; o < Co; o++)
            if (out[p * Co + o] != scalar(k, C, in + p * C, o)) { bad = fail("bytes differ", W, H, C, Co, k.lut_on); break; }
    free(in); free(out);
    return bad;
}

int main()
{
    int bad = 0;
    const int flat[][2] = {{4, 4}, {24, 2}, {16, 255}, {16, 256}, {16, 257}, {64, 128}, {16, 513}, {1, 16}, {1920, 1080}};
    for (const auto &s : flat)
        for (int C = 1; C <= 4; C++)
            for (int Co = 1; Co <= 4; Co++) bad += walk(s[0], s[1], C, Co, 3);
    if (!bad) printf("tile geometry clean\n");

    const int sizes[][2] = {{1, 1}, {17, 1}, {13, 5}};
    int before = bad;
    for (int C = 1; C <= 4; C++)
        for (int Co = 1; Co <= 4; Co++)
            for (int lut = 0; lut <= 1; lut++)
                for (const auto &s : sizes)
                    for (int shift : {0, 7, 16}) bad += run_case(s[0], s[1], C, make(Co, shift, lut, false), 3, 1 + (int)(rnd() % 4));
    if (bad == before) printf("random color cases clean\n");

    before = bad;
    for (int C = 1; C <= 4; C++)
        for (int Co = 1; Co <= 4; Co++)
            for (int lut = 0; lut <= 1; lut++)
                for (const auto &s : sizes)
                    for (int shift : {0, 16}) bad += run_case(s[0], s[1], C, make(Co, shift, lut, true), 2, 3);
    if (bad == before) printf("limit color cases clean\n");
    return bad ? 1 : 0;
}
