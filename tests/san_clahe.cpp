// host-only sanitizer run of CLAHE, in three parts:
//   1. the geometry of blur_clahe_tables_tiled_kernel and blur_clahe_apply_tiled_kernel (filter.h) walked over a spread
//      of launches as the kernels walk them: every 16-byte chunk against the image, every pixel of a tile counted exactly
//      once, every group of an image written exactly once, every LDS table index inside what the launch asks for;
//   2. the CPU device (cpu_clahe_tables, cpu_clahe_apply, cpu_clahe) against scalar loops written here, random shapes of
//      every channel count in exact-size heap buffers, so ASan sees any over-read or over-write;
//   3. clahe_table() on extreme histograms in unsigned __int128: one level, areas up to 2^31 - 1, every clip's ends.
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mi_blur;

static uint32_t rng_state = 2424u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int fail(const char *what, int W, int H, int C, int TX, int TY)
{
    printf("FAILED %s W%d H%d C%d tiles %d x %d\n", what, W, H, C, TX, TY);
    return 1;
}

// Part 1 for one image; 0 when clean.
static int walk(int W, int H, int C, int TX, int TY)
{
    const mi_blur_clahe k{TX, TY, 512, 0};
    if (!clahe_tiled_ok(W) || !hist_image_ok(W, H, C) || !clahe_ok(&k, W, H, C)) return fail("not a tiled launch", W, H, C, TX, TY);
    const long long bytes = (long long)W * H * C;
    // the table kernel: a workgroup per tile, items of (row, group that touches the tile), masked per pixel
    std::vector<uint8_t> counted((size_t)W * H, 0);
    for (int ty = 0; ty < TY; ty++)
        for (int tx = 0; tx < TX; tx++) {
            const int x0 = clahe_edge(W, TX, tx), x1 = clahe_edge(W, TX, tx + 1), y0 = clahe_edge(H, TY, ty), y1 = clahe_edge(H, TY, ty + 1);
            if (x0 >= x1 || y0 >= y1) return fail("empty tile", W, H, C, TX, TY);
            const unsigned g0 = (unsigned)x0 / COLOR_GROUP, ngx = ((unsigned)x1 + COLOR_GROUP - 1) / COLOR_GROUP - g0;
            for (unsigned i = 0; i < ngx * (unsigned)(y1 - y0); i++) {
                const unsigned r = i / ngx, g = g0 + (i - r * ngx);
                const long long at = ((long long)(y0 + (int)r) * W + (long long)g * COLOR_GROUP) * C;
                if (at < 0 || at + 16 * C > bytes || at % 16) return fail("table chunk", W, H, C, TX, TY);
                for (int px = 0; px < COLOR_GROUP; px++) {
                    const int x = (int)g * COLOR_GROUP + px;
                    if (x >= x0 && x < x1) counted[(size_t)(y0 + (int)r) * W + x]++;
                }
            }
        }
    for (size_t i = 0; i < counted.size(); i++)
        if (counted[i] != 1) return fail("pixel not counted once", W, H, C, TX, TY);
    // the look-up kernel: (slice of a row class, span); the staged tables and the entries
    if (!clahe_apply_tiled_ok(W, TX, C)) return 0;
    const int nspans = clahe_spans(W), slices = clahe_slices(H, TY), max_cols = clahe_span_cols(W, TX);
    std::vector<uint8_t> written((size_t)(W / COLOR_GROUP) * H, 0);
    for (int slice = 0; slice < slices; slice++)
        for (int span = 0; span < nspans; span++) {
            int s = slice, kk = 0, lo = 0, hi = clahe_class_lo(H, TY, 1);
            for (; kk < TY; kk++, lo = hi, hi = clahe_class_lo(H, TY, kk + 1)) {
                const int ns = (hi - lo + CLAHE_ROWS - 1) / CLAHE_ROWS;
                if (s < ns) break;
                s -= ns;
            }
            lo += s * CLAHE_ROWS;
            if (lo >= hi) return fail("empty slice", W, H, C, TX, TY);
            hi = hi < lo + CLAHE_ROWS ? hi : lo + CLAHE_ROWS;
            const int ty0 = kk - 1 > 0 ? kk - 1 : 0, ty1 = kk < TY - 1 ? kk : TY - 1;
            const int xa = span * CLAHE_SPAN, xb = (xa + CLAHE_SPAN < W ? xa + CLAHE_SPAN : W) - 1;
            int ta, tb, unused, f;
            clahe_axis(W, TX, xa, ta, unused, f);
            clahe_axis(W, TX, xb, unused, tb, f);
            if (tb - ta + 1 > max_cols || ta < 0 || tb >= TX) return fail("columns of a span", W, H, C, TX, TY);
            for (int y = lo; y < hi; y++) {
                int t0, t1, fy;
                clahe_axis(H, TY, y, t0, t1, fy);
                if (fy && (t0 != ty0 || t1 != ty1)) return fail("row class", W, H, C, TX, TY);
                if (!fy && t0 != ty0) return fail("row class at a centre", W, H, C, TX, TY);
                for (int x = xa; x <= xb; x++) {
                    int c0, c1, fx;
                    clahe_axis(W, TX, x, c0, c1, fx);
                    if (c0 - ta < 0 || c1 - ta > tb - ta || c1 - c0 < 0 || c1 - c0 > 1 || fx < 0 || fx >= (int)BLEND_ONE) return fail("column entry", W, H, C, TX, TY);
                }
                for (int g = 0; g < (xb - xa + 1) / COLOR_GROUP; g++) {
                    const long long at = ((long long)y * W + xa + g * COLOR_GROUP) * C;
                    if (at + 16 * C > bytes || at % 16) return fail("look-up chunk", W, H, C, TX, TY);
                    written[(size_t)y * (W / COLOR_GROUP) + (xa / COLOR_GROUP + g)]++;
                }
            }
        }
    for (size_t i = 0; i < written.size(); i++)
        if (written[i] != 1) return fail("group not written once", W, H, C, TX, TY);
    return 0;
}

// The header's text for one table, in unsigned __int128 so that nothing here can overflow.
typedef unsigned __int128 u128;
static void scalar_table(const uint32_t *h, uint32_t A, int clip_q8, uint8_t *lut)
{
    u128 hp[256];
    for (int v = 0; v < 256; v++) hp[v] = h[v];
    if (clip_q8) {
        u128 clip = (u128)clip_q8 * A / 65536, excess = 0;
        if (clip < 1) clip = 1;
        for (int v = 0; v < 256; v++) excess += h[v] > clip ? h[v] - clip : 0;
        const u128 residual = excess % 256;
        for (int v = 0; v < 256; v++) hp[v] = (h[v] < clip ? h[v] : clip) + excess / 256;
        if (residual > 0) {
            u128 step = 256 / residual;
            if (step < 1) step = 1;
            for (int v = 0; v < 256; v++)
                if (v % step == 0 && v / step < residual) hp[v]++;
        }
    }
    u128 run = 0;
    for (int v = 0; v < 256; v++) { run += hp[v]; lut[v] = (uint8_t)((510 * run + A) / (2 * (u128)A)); }
    if (run != A) printf("FAILED the clipped bins do not sum to the area\n");
}

// Part 2 for one case; 0 when clean.
static int run_case(int W, int H, int C, int TX, int TY, int clip_q8, int mask, int n_images, int n_threads)
{
    const mi_blur_clahe k{TX, TY, clip_q8, mask};
    if (!clahe_ok(&k, W, H, C)) return fail("refused", W, H, C, TX, TY);
    const size_t px = (size_t)W * H, bytes = (size_t)n_images * px * C, words = clahe_tables_of(n_images, k, C) * 256;
    uint8_t *in = (uint8_t *)malloc(bytes), *out = (uint8_t *)malloc(bytes), *step = (uint8_t *)malloc(bytes);
    uint32_t *work = (uint32_t *)malloc(words * 5), *work2 = (uint32_t *)malloc(words * 5);
    const int span = rnd_range(1, 256), base = rnd_range(0, 256 - span);
    for (size_t i = 0; i < bytes; i++) in[i] = (uint8_t)(base + (int)(rnd() % (uint32_t)span));
    std::vector<uint32_t> hist(words, 0);
    std::vector<uint8_t> tabs(words);
    const int on = mask ? mask : (1 << C) - 1;
    for (int i = 0; i < n_images; i++)
        for (int ty = 0; ty < TY; ty++)
            for (int tx = 0; tx < TX; tx++) {
                const int x0 = tx * W / TX, x1 = (tx + 1) * W / TX, y0 = ty * H / TY, y1 = (ty + 1) * H / TY;
                const size_t at = ((((size_t)i * TY + ty) * TX + tx) * C) * 256;
                for (int y = y0; y < y1; y++)
                    for (int x = x0; x < x1; x++)
                        for (int c = 0; c < C; c++) hist[at + c * 256 + in[(((size_t)i * H + y) * W + x) * C + c]]++;
                for (int c = 0; c < C; c++) {
                    if ((on >> c) & 1) scalar_table(&hist[at + c * 256], (uint32_t)((x1 - x0) * (y1 - y0)), clip_q8, &tabs[at + c * 256]);
                    else for (int v = 0; v < 256; v++) tabs[at + c * 256 + v] = (uint8_t)v;
                }
            }
    memset(out, 0xA5, bytes);
    memset(work, 0xFF, words * 5);
    cpu_clahe(in, out, W, H, C, n_images, k, work, n_threads);
    int bad = 0;
    if (memcmp(work, hist.data(), words * 4)) bad += fail("work: histograms differ", W, H, C, TX, TY);
    if (memcmp(work + words, tabs.data(), words)) bad += fail("work: tables differ", W, H, C, TX, TY);
    cpu_clahe_tables(in, work2, reinterpret_cast<uint8_t *>(work2 + words), W, H, C, n_images, k, n_threads);
    if (memcmp(work, work2, words * 5)) bad += fail("the tables step differs", W, H, C, TX, TY);
    cpu_clahe_apply(in, step, W, H, C, n_images, k, tabs.data(), n_threads);
    if (memcmp(out, step, bytes)) bad += fail("clahe is not tables, apply", W, H, C, TX, TY);
    for (size_t i = 0; i < bytes && !bad; i++) {
        const size_t img = i / (px * C), rem = i % (px * C);
        const int y = (int)(rem / ((size_t)W * C)), x = (int)(rem % ((size_t)W * C)) / C, c = (int)(rem % C);
        int x0, x1, fx, y0, y1, fy;
        clahe_axis(W, TX, x, x0, x1, fx);
        clahe_axis(H, TY, y, y0, y1, fy);
        auto L = [&](int ty, int tx) { return (u128)tabs[((((size_t)img * TY + ty) * TX + tx) * C + c) * 256 + in[i]]; };
        const u128 v = ((u128)(2048 - fx) * (2048 - fy) * L(y0, x0) + (u128)fx * (2048 - fy) * L(y0, x1) + (u128)(2048 - fx) * fy * L(y1, x0) +
                        (u128)fx * fy * L(y1, x1) + (1u << 21)) >> 22;
        if (out[i] != (uint8_t)v) bad += fail("bytes differ", W, H, C, TX, TY);
    }
    free(in); free(out); free(step); free(work); free(work2);
    return bad;
}

// Part 3: clahe_table() against scalar_table() on one histogram at every clip's ends.
static int extreme(const uint32_t *h, const char *what)
{
    u128 A = 0;
    for (int v = 0; v < 256; v++) A += h[v];
    if (A == 0 || A > 0x7fffffffu) { printf("FAILED extreme %s: area\n", what); return 1; }
    int bad = 0;
    for (int clip_q8 : {0, 1, 2, 255, 256, 257, 512, 10240, 65535, 65536}) {
        uint8_t got[256], want[256];
        memset(got, 0xA5, sizeof got);
        clahe_table(h, (uint32_t)A, clip_q8, got);
        scalar_table(h, (uint32_t)A, clip_q8, want);
        if (memcmp(got, want, 256) || got[255] != 255) { printf("FAILED extreme %s clip %d\n", what, clip_q8); bad++; }
    }
    return bad;
}

int main()
{
    int bad = 0;
    const int shapes[][4] = {{16, 4, 1, 1}, {48, 9, 3, 3}, {48, 9, 5, 2}, {16, 16, 16, 16}, {96, 96, 1, 1}, {64, 40, 8, 8}, {32, 32, 3, 3}, {1024, 2, 64, 2},
                             {1024, 2, 50, 1}, {1920, 1080, 8, 8}, {1920, 1080, 16, 16}, {256, 256, 8, 8}, {272, 77, 64, 64}, {4096, 130, 8, 64}, {4096, 70, 64, 1},
                             {32768, 3, 64, 3}, {32768, 2, 1, 1}, {16, 4099, 16, 64}, {80, 33, 7, 5}};
    for (const auto &s : shapes)
        for (int C = 1; C <= 4; C++) bad += walk(s[0], s[1], C, s[2], s[3]);
    for (int rep = 0; rep < 60; rep++) {
        const int W = 16 * rnd_range(1, 40), H = rnd_range(1, 150);
        bad += walk(W, H, rnd_range(1, 4), rnd_range(1, W < 64 ? W : 64), rnd_range(1, H < 64 ? H : 64));
    }
    if (!bad) printf("tile geometry clean\n");

    int before = bad;
    const int sizes[][4] = {{1, 1, 1, 1}, {7, 5, 7, 5}, {40, 13, 3, 4}, {64, 48, 8, 8}, {64, 48, 1, 1}, {17, 9, 3, 2}, {300, 97, 64, 64}};
    for (int C = 1; C <= 4; C++)
        for (const auto &s : sizes)
            for (int clip_q8 : {0, 512, 65536}) bad += run_case(s[0], s[1], C, s[2], s[3], clip_q8, rnd_range(0, (1 << C) - 1), 1 + (int)(rnd() % 3), 1 + (int)(rnd() % 4));
    for (int rep = 0; rep < 12; rep++) {
        const int W = rnd_range(1, 90), H = rnd_range(1, 70), C = rnd_range(1, 4);
        bad += run_case(W, H, C, rnd_range(1, W < 64 ? W : 64), rnd_range(1, H < 64 ? H : 64), rnd_range(0, 65536), rnd_range(0, (1 << C) - 1), rnd_range(1, 4), rnd_range(1, 5));
    }
    if (bad == before) printf("cpu device cases clean\n");

    before = bad;
    std::vector<uint32_t> h(256);
    auto clear = [&] { std::fill(h.begin(), h.end(), 0u); };
    clear(); h[9] = 0x7fffffffu;
    bad += extreme(h.data(), "one level of 2^31 - 1");
    clear(); h[0] = 0x3fffffffu; h[255] = 0x40000000u;
    bad += extreme(h.data(), "both ends, 2^31 - 1 in all");
    clear(); h[255] = 1;
    bad += extreme(h.data(), "area 1 at 255");
    clear(); h[0] = 1;
    bad += extreme(h.data(), "area 1 at 0");
    clear(); for (int v = 0; v < 256; v++) h[v] = 1;
    bad += extreme(h.data(), "every level once");
    clear(); for (int v = 0; v < 256; v++) h[v] = 0x7fffffu;
    bad += extreme(h.data(), "every level 2^23 - 1");
    clear(); for (int v = 0; v < 256; v++) h[v] = 254; h[77] = 767; h[3] = 1;
    bad += extreme(h.data(), "a residual of 255 at clip 256");
    for (int rep = 0; rep < 60; rep++) {
        clear();
        for (int v = 0; v < 256; v++) h[v] = rnd() % 3 ? 0 : (rnd() << (rnd() % 8)) >> 10;
        h[rnd() % 256] += 1;
        bad += extreme(h.data(), "random sparse");
    }
    if (bad == before) printf("extreme histograms clean\n");
    return bad ? 1 : 0;
}
