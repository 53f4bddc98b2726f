// host-only sanitizer run of the histogram family, in three parts:
//   1. the units of blur_hist_tiled_kernel / blur_tables_tiled_kernel (filter.h) walked over a spread of launches as the
//      kernels walk them: every 16-byte chunk a thread touches against the image, every group taken exactly once;
//   2. the CPU device (cpu_hist, cpu_tables, cpu_tone) against scalar loops written here, random shapes of every channel
//      count in exact-size heap buffers, so ASan sees any over-read or over-write;
//   3. tone_tables() on extreme histograms: one level, the ends of the range, all levels, counts at the top of 32 bits
//      summed over four channels (UBSan sees an overflow), the largest clips.
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mi_blur;

static uint32_t rng_state = 2468u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int fail(const char *what, int W, int H, int C)
{
    printf("FAILED %s W%d H%d C%d\n", what, W, H, C);
    return 1;
}

// Part 1 for one launch; 0 when clean.
static int walk(int W, int H, int C, int n_images)
{
    if (!color_flat_ok(W, H) || !hist_image_ok(W, H, C)) return fail("not a tiled launch", W, H, C);
    const long long groups = (long long)W * H / COLOR_GROUP, bytes = (long long)W * H * C;
    const int runs = hist_runs(W, H);
    if ((long long)runs * HIST_RUN < groups || (long long)(runs - 1) * HIST_RUN >= groups) return fail("runs", W, H, C);
    // blur_tables_tiled_kernel: one workgroup per run; blur_hist_tiled_kernel: at most HIST_IMAGE_BLOCKS per image, each
    // taking every per_image-th run
    const int per_image = hist_blocks(W, H);
    if (per_image > HIST_IMAGE_BLOCKS || per_image > runs || (runs <= HIST_IMAGE_BLOCKS && per_image != runs)) return fail("workgroups per image", W, H, C);
    std::vector<uint8_t> seen((size_t)groups, 0), seen_hist((size_t)groups, 0);
    for (long long L = 0; L < (long long)n_images * runs; L++) {
        const long long img = L / runs, run = L - img * runs;
        if (img >= n_images) return fail("image", W, H, C);
        const long long g0 = run * HIST_RUN, g1 = g0 + HIST_RUN < groups ? g0 + HIST_RUN : groups;
        for (int t = 0; t < HIST_THREADS; t++)
            for (long long g = g0 + t; g < g1; g += HIST_THREADS) {
                if (g * 16 * C + 16 * C > bytes) return fail("chunk", W, H, C);
                if (img == 0) seen[(size_t)g]++;
            }
    }
    for (long long L = 0; L < (long long)n_images * per_image; L++) {
        const long long img = L / per_image, first = L - img * per_image;
        if (img >= n_images) return fail("image", W, H, C);
        for (long long run = first; run < runs; run += per_image) {
            const long long g0 = run * HIST_RUN, g1 = g0 + HIST_RUN < groups ? g0 + HIST_RUN : groups;
            for (int t = 0; t < HIST_THREADS; t++)
                for (long long g = g0 + t; g < g1; g += HIST_THREADS) {
                    if (g * 16 * C + 16 * C > bytes) return fail("chunk", W, H, C);
                    if (img == 0) seen_hist[(size_t)g]++;
                }
        }
    }
    for (long long g = 0; g < groups; g++)
        if (seen_hist[(size_t)g] != 1) return fail("group not counted once", W, H, C);
    for (long long g = 0; g < groups; g++)
        if (seen[(size_t)g] != 1) return fail("group not taken once", W, H, C);
    return 0;
}

// The header's text for one table, in unsigned __int128 so that nothing here can overflow.
typedef unsigned __int128 u128;
static void scalar_table(const mi_blur_tone &t, const u128 *h, uint8_t *lut)
{
    u128 N = 0, cum[256];
    for (int v = 0; v < 256; v++) { N += h[v]; cum[v] = N; }
    for (int v = 0; v < 256; v++) lut[v] = (uint8_t)v;
    if (N == 0) return;
    if (t.mode == MI_BLUR_TONE_EQUALIZE) {
        int m = 0;
        while (h[m] == 0) m++;
        const u128 D = N - h[m];
        if (D == 0) return;
        for (int v = 0; v < 256; v++) lut[v] = v < m ? 0 : (uint8_t)((510 * (cum[v] - h[m]) + D) / (2 * D));
        return;
    }
    const u128 k_lo = N * (u128)t.clip_lo / 65536, k_hi = N * (u128)t.clip_hi / 65536;
    int lo = 0, hi = 255;
    while (!(cum[lo] > k_lo)) lo++;
    while (!(N - (hi ? cum[hi - 1] : 0) > k_hi)) hi--;
    if (lo > hi) { printf("FAILED lo > hi\n"); return; }
    if (lo == hi) return;
    const int d = hi - lo;
    for (int v = 0; v < 256; v++) lut[v] = v <= lo ? 0 : v >= hi ? 255 : (uint8_t)((510 * (v - lo) + d) / (2 * d));
}
static void scalar_tables(const mi_blur_tone &t, const uint32_t *hist, int C, uint8_t *tables)
{
    const int mask = t.channel_mask ? t.channel_mask : (1 << C) - 1;
    for (int c = 0; c < C; c++) {
        uint8_t *lut = tables + c * 256;
        for (int v = 0; v < 256; v++) lut[v] = (uint8_t)v;
        if (!((mask >> c) & 1)) continue;
        u128 h[256];
        for (int v = 0; v < 256; v++) {
            h[v] = 0;
            for (int k = 0; k < C; k++)
                if (t.joint ? (mask >> k) & 1 : k == c) h[v] += hist[k * 256 + v];
        }
        scalar_table(t, h, lut);
    }
}

static mi_blur_tone random_tone(int C)
{
    mi_blur_tone t{};
    t.mode = rnd() & 1;
    if (t.mode == MI_BLUR_TONE_STRETCH) { t.clip_lo = rnd_range(0, TONE_CLIP_MAX); t.clip_hi = rnd_range(0, TONE_CLIP_MAX); }
    t.joint = rnd() & 1;
    t.channel_mask = rnd_range(0, (1 << C) - 1);
    return t;
}

// Part 2 for one case; 0 when clean.
static int run_case(int W, int H, int C, int n_images, int n_threads)
{
    const size_t px = (size_t)W * H, bytes = (size_t)n_images * px * C, words = (size_t)n_images * C * 256;
    uint8_t *in = (uint8_t *)malloc(bytes), *out = (uint8_t *)malloc(bytes), *step = (uint8_t *)malloc(bytes);
    uint32_t *hist = (uint32_t *)malloc(words * 4), *work = (uint32_t *)malloc(words * 5);
    std::vector<uint32_t> want(words, 0);
    const int span = rnd_range(1, 256), base = rnd_range(0, 256 - span);
    for (size_t i = 0; i < bytes; i++) in[i] = (uint8_t)(base + (int)(rnd() % (uint32_t)span));
    for (int i = 0; i < n_images; i++)
        for (size_t p = 0; p < px; p++)
            for (int c = 0; c < C; c++) want[((size_t)i * C + c) * 256 + in[((size_t)i * px + p) * C + c]]++;
    memset(hist, 0xFF, words * 4);
    cpu_hist(in, hist, W, H, C, n_images, n_threads);
    int bad = memcmp(hist, want.data(), words * 4) ? fail("histogram differs", W, H, C) : 0;

    const mi_blur_tone t = random_tone(C);
    if (!tone_ok(&t, C)) bad += fail("tone refused", W, H, C);
    std::vector<uint8_t> tabs(words);
    for (int i = 0; i < n_images; i++) scalar_tables(t, want.data() + (size_t)i * C * 256, C, tabs.data() + (size_t)i * C * 256);
    memset(out, 0xA5, bytes);
    cpu_tone(in, out, W, H, C, n_images, t, work, n_threads);
    if (memcmp(work, want.data(), words * 4)) bad += fail("work: histograms differ", W, H, C);
    if (memcmp(work + words, tabs.data(), words)) bad += fail("work: tables differ", W, H, C);
    cpu_tables(in, step, W, H, C, n_images, tabs.data(), n_threads);
    if (memcmp(out, step, bytes)) bad += fail("tone is not hist, tables, apply", W, H, C);
    for (size_t i = 0; i < bytes && !bad; i++)
        if (out[i] != tabs[((i / (px * C)) * C + i % C) * 256 + in[i]]) bad += fail("bytes differ", W, H, C);
    free(in); free(out); free(step); free(hist); free(work);
    return bad;
}

// Part 3: tone_tables() against scalar_tables() on one extreme histogram, every mode, joint and a few clips.
static int extreme(const uint32_t *hist, int C, const char *what)
{
    int bad = 0;
    const int clips[][2] = {{0, 0}, {1, 1}, {TONE_CLIP_MAX, TONE_CLIP_MAX}, {TONE_CLIP_MAX, 0}, {0, TONE_CLIP_MAX}, {655, 1310}};
    for (int mode = 0; mode <= 1; mode++)
        for (int joint = 0; joint <= 1; joint++)
            for (int mask = 0; mask < (1 << C); mask += (C > 2 ? 3 : 1))
                for (const auto &cl : clips) {
                    if (mode == MI_BLUR_TONE_EQUALIZE && (cl[0] || cl[1])) continue;
                    const mi_blur_tone t{mode, cl[0], cl[1], joint, mask};
                    std::vector<uint8_t> got((size_t)C * 256, 0xA5), want((size_t)C * 256);
                    if (!tone_ok(&t, C)) { bad += fail(what, mode, joint, C); continue; }
                    tone_tables(t, hist, C, got.data());
                    scalar_tables(t, hist, C, want.data());
                    if (got != want) { printf("FAILED extreme %s mode%d joint%d mask%d clips %d %d\n", what, mode, joint, mask, cl[0], cl[1]); bad++; }
                }
    return bad;
}

int main()
{
    int bad = 0;
    const int flat[][2] = {{4, 4}, {24, 2}, {16, HIST_RUN - 1}, {16, HIST_RUN}, {16, HIST_RUN + 1}, {16, 2 * HIST_RUN + 1}, {1, 16}, {1920, 1080}, {2048, 2 * HIST_RUN}, {112, 18797}, {2048, 2052}, {4097, 4096}};
    for (const auto &s : flat)
        for (int C = 1; C <= 4; C++) bad += walk(s[0], s[1], C, 3);
    if (!bad) printf("tile geometry clean\n");

    int before = bad;
    const int sizes[][2] = {{1, 1}, {17, 1}, {13, 5}, {7, 5}, {300, 97}};
    for (int C = 1; C <= 4; C++)
        for (const auto &s : sizes)
            for (int rep = 0; rep < 3; rep++) bad += run_case(s[0], s[1], C, 1 + rep, 1 + (int)(rnd() % 4));
    for (int rep = 0; rep < 12; rep++) bad += run_case(rnd_range(1, 90), rnd_range(1, 70), rnd_range(1, 4), rnd_range(1, 5), rnd_range(1, 5));
    if (bad == before) printf("hist and tables cases clean\n");

    before = bad;
    std::vector<uint32_t> h(4 * 256);
    auto clear = [&] { std::fill(h.begin(), h.end(), 0u); };
    clear(); for (int c = 0; c < 4; c++) h[c * 256 + 77] = 0xFFFFFFFFu;
    bad += extreme(h.data(), 4, "one level at the top of 32 bits");
    clear(); for (int c = 0; c < 4; c++) { h[c * 256] = 0xFFFFFFFFu; h[c * 256 + 255] = 0xFFFFFFFFu; }
    bad += extreme(h.data(), 4, "both ends at the top of 32 bits");
    clear(); for (int c = 0; c < 4; c++) { h[c * 256 + 255] = 5; }
    bad += extreme(h.data(), 4, "first level 255");
    clear(); for (int c = 0; c < 4; c++) { h[c * 256] = 5; }
    bad += extreme(h.data(), 4, "last level 0");
    clear(); for (size_t i = 0; i < h.size(); i++) h[i] = 1;
    bad += extreme(h.data(), 4, "every level once");
    clear(); for (size_t i = 0; i < h.size(); i++) h[i] = 0xFFFFFFFFu;
    bad += extreme(h.data(), 4, "every level at the top of 32 bits");
    clear();
    bad += extreme(h.data(), 4, "empty");
    clear(); h[3] = 1 << 26; for (int v = 0; v < 256; v++) h[256 + v] = (1 << 26) / 256; h[2 * 256 + 255] = 1; h[2 * 256 + 254] = (1 << 26) - 1;
    bad += extreme(h.data(), 3, "4096 x 4096");
    for (int rep = 0; rep < 40; rep++) {
        const int C = rnd_range(1, 4);
        clear();
        for (int i = 0; i < C * 256; i++) h[i] = rnd() % 3 ? 0 : rnd() << (rnd() % 9);
        bad += extreme(h.data(), C, "random sparse");
    }
    if (bad == before) printf("extreme histograms clean\n");
    return bad ? 1 : 0;
}
