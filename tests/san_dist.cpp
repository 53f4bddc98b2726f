// host-only sanitizer run of the distance transform, in four parts:
//   1. the arithmetic the kernels share with the host (filter.h): dist_root() against the comparison it is defined by at
//      every rounding boundary, dist_cand() at the largest operands, dist_start() / dist_final() around every limit of a
//      spread, dist_byte() at its ends, and the tiled kernel's LDS size at its widest rows;
//   2. the CPU device (cpu_dist) on the named cases of the header's text against a brute force over all sites written
//      here: exact-size heap buffers (ASan sees any over-read or over-write, UBSan any signed overflow), the table and
//      both byte forms, in place for the bytes;
//   3. the extremes: the longest row, the longest column and two columns of 32768 rows with the only site at one end;
//   4. random shapes, densities, metrics, conventions and limits against the same brute force.
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mi_blur;

static uint32_t rng_state = 97531u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int fail(const char *what, long long a, long long b, long long c)
{
    printf("FAILED %s %lld %lld %lld\n", what, a, b, c);
    return 1;
}

static long long metric_of(int metric, long long dx, long long dy) { return metric == MI_BLUR_DIST_L2 ? dx * dx + dy * dy : metric == MI_BLUR_DIST_L1 ? dx + dy : dx > dy ? dx : dy; }

// Part 1.
static int arithmetic()
{
    int bad = 0;
    for (int s = 1; s <= 255; s++) {
        const uint32_t first = (uint32_t)(((2 * s - 1) * (2 * s - 1) + 3) / 4);
        if (dist_root(first) != s || dist_root(first - 1) != s - 1) bad += fail("dist_root", s, first, dist_root(first));
    }
    for (uint32_t T = 0; T < 70000; T++) {
        int s = 0;
        while (s < 255 && (uint64_t)(2 * s + 1) * (2 * s + 1) <= 4ull * T) s++;
        if (dist_root(T) != s) bad += fail("dist_root against the comparison", T, s, dist_root(T));
    }
    if (dist_root(2147352578u) != 255 || dist_root(0xFFFFFFFEu) != 255) bad += fail("dist_root ends", 0, 0, 0);
    if (dist_cand(MI_BLUR_DIST_L2, 32767u, 32767u) != 2147352578u || dist_cand(MI_BLUR_DIST_L1, 32767u, 32767u) != 65534u ||
        dist_cand(MI_BLUR_DIST_LINF, 32767u, 32766u) != 32767u || dist_max(MI_BLUR_DIST_L2) != 2147352578u)
        bad += fail("dist_cand ends", 0, 0, 0);
    for (int metric = 0; metric <= MI_BLUR_DIST_LINF; metric++) {
        if (dist_start(metric, 0) != MI_BLUR_DIST_NONE || dist_final(dist_max(metric), MI_BLUR_DIST_NONE) != dist_max(metric)) bad += fail("no limit", metric, 0, 0);
        for (int limit : {1, 2, 5, 255, 300, 32766, 32767}) {
            const uint32_t start = dist_start(metric, limit), at = (uint32_t)metric_of(metric, limit, 0);
            if (start != at + 1 || dist_final(at, start) != at || dist_final(at + 1, start) != MI_BLUR_DIST_NONE || dist_final(start, start) != MI_BLUR_DIST_NONE)
                bad += fail("limit", metric, limit, start);
            if (dist_g_cap((uint32_t)limit, dist_cap(limit)) != (uint32_t)limit || dist_g_cap((uint32_t)limit + 1, dist_cap(limit)) != DIST_G_NONE) bad += fail("g cap", limit, 0, 0);
        }
        if (dist_byte(metric, MI_BLUR_DIST_BYTE, 0, MI_BLUR_DIST_NONE) != 255 || dist_byte(metric, MI_BLUR_DIST_BYTE, 0, 0) != 0 ||
            dist_byte(metric, MI_BLUR_DIST_WITHIN, 0, 0) != 255 || dist_byte(metric, MI_BLUR_DIST_WITHIN, 1, 0) != 0 ||
            dist_byte(metric, MI_BLUR_DIST_WITHIN, 0, MI_BLUR_DIST_NONE) != 0 || dist_byte(metric, MI_BLUR_DIST_WITHIN, 1, MI_BLUR_DIST_NONE) != 255)
            bad += fail("dist_byte ends", metric, 0, 0);
    }
    if (dist_g_cap(DIST_G_NONE, dist_cap(0)) != DIST_G_NONE || dist_g_cap(32767u, dist_cap(0)) != 32767u) bad += fail("g cap without a limit", 0, 0, 0);
    for (int C = 1; C <= 4; C++)                                         // the widest rows the tiled kernel takes, every chunk size
        for (int W = DIST_MAX_ROW / C - 40; W <= DIST_MAX_ROW / C; W++)
            for (int chunk : {8, 16, 32})
                if (dist_tiled_ok(W, C) && (dist_rows(W, C) != 1 || dist_lds_bytes(W, C, 1, chunk) > 65536)) bad += fail("lds", W, C, chunk);
    for (int W : {1, 2, 8, 100, 512, 513, 4096})
        for (int C = 1; C <= 4; C++) {
            const int r = dist_rows(W, C);
            if (r < 1 || r > DIST_MAX_ROWS || (r > 1 && (long long)r * W * C > DIST_TILE_ELEMS) || dist_lds_bytes(W, C, r, 8) > 65536) bad += fail("rows", W, C, r);
        }
    return bad;
}

// The definition for one image batch.
static void brute(const uint8_t *in, int W, int H, int C, int n, const mi_blur_dist &k, std::vector<uint32_t> &T)
{
    T.assign((size_t)n * W * H * C, MI_BLUR_DIST_NONE);
    const long long bound = k.limit ? metric_of(k.metric, k.limit, 0) : (1ll << 62) - 1;      // no site leaves 1 << 62: beyond every bound
    std::vector<int> sx, sy;
    for (int i = 0; i < n; i++)
        for (int c = 0; c < C; c++) {
            sx.clear(); sy.clear();
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++)
                    if ((in[(((size_t)i * H + y) * W + x) * C + c] != 0) == (k.sites_nonzero != 0)) { sx.push_back(x); sy.push_back(y); }
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    long long best = 1ll << 62;
                    for (size_t s = 0; s < sx.size(); s++) {
                        const long long d = metric_of(k.metric, llabs((long long)x - sx[s]), llabs((long long)y - sy[s]));
                        best = d < best ? d : best;
                    }
                    if (best <= bound) T[(((size_t)i * H + y) * W + x) * C + c] = (uint32_t)best;
                }
        }
}

static int byte_of(const mi_blur_dist &k, uint32_t T)
{
    if (k.byte_op == MI_BLUR_DIST_WITHIN) return (T != MI_BLUR_DIST_NONE) != (k.invert != 0) ? 255 : 0;
    if (T == MI_BLUR_DIST_NONE) return 255;
    if (k.metric != MI_BLUR_DIST_L2) return T > 255 ? 255 : (int)T;
    int s = 0;
    while (s < 255 && (uint64_t)(2 * s + 1) * (2 * s + 1) <= 4ull * T) s++;
    return s;
}

// cpu_dist on `in` (exact-size heap copies) against `want`, the table and the byte form(s) of it, in place too.
static int check(const std::vector<uint8_t> &img, int W, int H, int C, int n, mi_blur_dist k, const std::vector<uint32_t> &want, int n_threads)
{
    int bad = 0;
    const size_t size = img.size();
    uint8_t *in = (uint8_t *)malloc(size), *out = (uint8_t *)malloc(size);
    uint32_t *table = (uint32_t *)malloc(size * 4);
    memcpy(in, img.data(), size);
    k.byte_op = 0; k.invert = 0;
    if (!dist_args_ok(in, table, W, H, C, n, &k, false, 4)) bad += fail("table arguments refused", W, H, C);
    if (!cpu_dist(in, table, nullptr, W, H, C, n, k, n_threads)) bad += fail("no memory", W, H, C);
    for (size_t e = 0; e < size; e++)
        if (table[e] != want[e]) { bad += fail("table differs", (long long)e, table[e], want[e]); break; }
    for (int form = 0; form < (k.limit ? 3 : 1); form++) {
        k.byte_op = form ? MI_BLUR_DIST_WITHIN : MI_BLUR_DIST_BYTE; k.invert = form == 2;
        if (!dist_args_ok(in, out, W, H, C, n, &k, true, 1) || !dist_args_ok(in, in, W, H, C, n, &k, true, 1)) bad += fail("byte arguments refused", W, H, form);
        if (!cpu_dist(in, nullptr, out, W, H, C, n, k, n_threads)) bad += fail("no memory", W, H, C);
        for (size_t e = 0; e < size; e++)
            if (out[e] != byte_of(k, want[e])) { bad += fail("bytes differ", (long long)e, out[e], form); break; }
        if (form == (k.limit ? 2 : 0)) {                                 // the last form in place
            if (!cpu_dist(in, nullptr, in, W, H, C, n, k, n_threads) || memcmp(in, out, size)) bad += fail("bytes differ in place", W, H, form);
        }
    }
    free(in); free(out); free(table);
    return bad;
}

static int run_case(const std::vector<uint8_t> &img, int W, int H, int C, int n, int metric, int nonzero, int limit, int n_threads)
{
    const mi_blur_dist k{metric, nonzero, limit, 0, 0};
    if (!dist_ok(&k, false)) return fail("struct refused", metric, nonzero, limit);
    std::vector<uint32_t> want;
    brute(img.data(), W, H, C, n, k, want);
    return check(img, W, H, C, n, k, want, n_threads);
}

// Part 2.
static int named()
{
    int bad = 0;
    for (int metric = 0; metric <= MI_BLUR_DIST_LINF; metric++) {
        for (int v = 0; v < 2; v++) bad += run_case(std::vector<uint8_t>(1, (uint8_t)v), 1, 1, 1, 1, metric, 0, 0, 1);      // 1 x 1 with and without a site
        const int shapes[][3] = {{23, 1, 1}, {1, 23, 1}, {11, 7, 2}, {40, 9, 3}, {17, 33, 4}};
        for (const auto &s : shapes) {
            const int W = s[0], H = s[1], C = s[2];
            for (int corner = 0; corner < 4; corner++) {                 // a single site at each corner, channel 0 only
                std::vector<uint8_t> img((size_t)W * H * C, 255);
                img[((size_t)(corner & 2 ? H - 1 : 0) * W + (corner & 1 ? W - 1 : 0)) * C] = 0;
                for (int limit : {0, 5}) bad += run_case(img, W, H, C, 1, metric, 0, limit, 2);
            }
        }
        std::vector<uint8_t> two((size_t)2 * 6 * 10 * 3, 0);             // image 0 full of sites, image 1 empty
        for (size_t e = two.size() / 2; e < two.size(); e++) two[e] = 9;
        bad += run_case(two, 10, 6, 3, 2, metric, 0, 0, 3) + run_case(two, 10, 6, 3, 2, metric, 1, 4, 3);
        std::vector<uint8_t> tri(12 * 12, 255);                          // the 3-4-5 triangle
        tri[2 * 12 + 3] = 0;
        for (int limit : {3, 4, 5, 6, 7}) bad += run_case(tri, 12, 12, 1, 1, metric, 0, limit, 1);
        std::vector<uint8_t> row(8 * 9, 255);                            // own column g = 5, a neighbour 3 columns away g = 0
        row[0 * 9 + 2] = 0; row[5 * 9 + 5] = 0;
        bad += run_case(row, 9, 8, 1, 1, metric, 0, 0, 1);
        std::vector<uint8_t> ties(9 * 9, 255);
        ties[4 * 9 + 0] = ties[4 * 9 + 8] = ties[0 * 9 + 4] = ties[8 * 9 + 4] = 0;
        bad += run_case(ties, 9, 9, 1, 1, metric, 0, 0, 2);
        std::vector<uint8_t> far((size_t)3 * 200, 255);                  // the nearest site several chunks away, and a far chunk that wins by one
        far[0 * 200 + 150] = 0; far[2 * 200 + 20] = 0;
        bad += run_case(far, 200, 3, 1, 1, metric, 0, 0, 1);
    }
    return bad;
}

// Part 3: the site at (0, 0); the wanted value of (x, y) is the metric of (x, y) itself.
static int extremes()
{
    int bad = 0;
    const int shapes[][2] = {{32768, 1}, {1, 32768}, {2, 32768}};
    for (const auto &s : shapes) {
        const int W = s[0], H = s[1];
        std::vector<uint8_t> img((size_t)W * H, 1);
        img[0] = 0;
        for (int metric = 0; metric <= MI_BLUR_DIST_LINF; metric++)
            for (int limit : {0, 32767}) {
                std::vector<uint32_t> want((size_t)W * H);
                const long long bound = limit ? metric_of(metric, limit, 0) : (1ll << 62);
                for (int y = 0; y < H; y++)
                    for (int x = 0; x < W; x++) {
                        const long long d = metric_of(metric, x, y);
                        want[(size_t)y * W + x] = d <= bound ? (uint32_t)d : MI_BLUR_DIST_NONE;
                    }
                if (metric == MI_BLUR_DIST_L2 && want.back() != (W == 2 ? (limit ? MI_BLUR_DIST_NONE : 32767u * 32767u + 1u) : 32767u * 32767u)) bad += fail("extreme value", W, H, limit);
                bad += check(img, W, H, 1, 1, mi_blur_dist{metric, 0, limit, 0, 0}, want, 3);
            }
    }
    return bad;
}

int main()
{
    int bad = arithmetic();
    if (!bad) printf("arithmetic clean\n");

    int before = bad;
    bad += named();
    if (bad == before) printf("named cases clean\n");

    before = bad;
    bad += extremes();
    if (bad == before) printf("extremes clean\n");

    before = bad;
    for (int rep = 0; rep < 60; rep++) {
        const int W = rnd_range(1, 70), H = rnd_range(1, 50), C = rnd_range(1, 4), n = rnd_range(1, 2);
        static const int densities[] = {0, 3, 20, 200, 1000}, limits[] = {0, 0, 1, 5, 300};
        const int per_mille = densities[rnd() % 5];
        std::vector<uint8_t> img((size_t)n * W * H * C);
        for (auto &v : img) v = (int)(rnd() % 1000) < per_mille ? 0 : (uint8_t)(1 + rnd() % 255);
        bad += run_case(img, W, H, C, n, rnd_range(0, 2), (int)(rnd() & 1), limits[rnd() % 5], rnd_range(1, 5));
    }
    {
        std::vector<uint8_t> tall((size_t)40 * 300 * 2, 7);             // more rows than one band of the CPU device
        tall[(size_t)(150 * 40 + 7) * 2] = 0; tall[(size_t)(299 * 40 + 39) * 2 + 1] = 0;
        bad += run_case(tall, 40, 300, 2, 1, MI_BLUR_DIST_L2, 0, 0, 4);
    }
    if (bad == before) printf("random cases clean\n");
    return bad ? 1 : 0;
}
