// host-only sanitizer run of the two-image arithmetic, in three parts:
//   1. the units of blur_arith_flat_kernel / blur_arith_plane_kernel (filter.h) walked over a spread of launches as the
//      kernels walk them: every 16-byte chunk a thread touches against its operand, every unit taken exactly once; and
//      the run counts of the largest images the family takes;
//   2. the CPU device (cpu_arith) against a scalar loop written here from the header's table in 64-bit integers with a
//      division for LERP, random structs at the limits of their fields (UBSan sees an overflow), every flag combination,
//      exact-size heap buffers (ASan sees any over-read or over-write), in place where that is allowed;
//   3. the aliasing and argument checks (arith_alias_ok, arith_args_ok).
#include "cpu_device.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mi_blur;

static uint32_t rng_state = 97531u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int fail(const char *what, int W, int H, int C)
{
    printf("FAILED %s W%d H%d C%d\n", what, W, H, C);
    return 1;
}

// Part 1 for one image shape; 0 when clean.
static int walk(int W, int H, int C, int n_images)
{
    if (!hist_image_ok(W, H, C)) return fail("image refused", W, H, C);
    const long long bytes = (long long)W * H * C, pixels = (long long)W * H;
    if (arith_flat_ok(W, H, C)) {
        const long long chunks = bytes / ARITH_CHUNK, runs = arith_flat_runs(W, H, C);
        if (runs * ARITH_RUN < chunks || (runs - 1) * ARITH_RUN >= chunks) return fail("flat runs", W, H, C);
        std::vector<uint8_t> seen((size_t)chunks, 0);
        for (long long L = 0; L < n_images * runs; L++) {
            const long long img = L / runs, run = L - img * runs;
            if (img >= n_images) return fail("flat image", W, H, C);
            for (int t = 0; t < ARITH_THREADS; t++) {
                const long long ch = run * ARITH_RUN + t;
                if (ch >= chunks) continue;
                if (ch * ARITH_CHUNK + ARITH_CHUNK > bytes) return fail("flat chunk", W, H, C);
                if (img == n_images - 1) seen[(size_t)ch]++;
            }
        }
        for (long long ch = 0; ch < chunks; ch++)
            if (seen[(size_t)ch] != 1) return fail("chunk not taken once", W, H, C);
    }
    if (color_flat_ok(W, H) && C >= 2) {
        const long long groups = pixels / COLOR_GROUP, runs = arith_plane_runs(W, H);
        if (runs * ARITH_PLANE_RUN < groups || (runs - 1) * ARITH_PLANE_RUN >= groups) return fail("plane runs", W, H, C);
        std::vector<uint8_t> seen((size_t)groups, 0);
        for (long long L = 0; L < n_images * runs; L++) {
            const long long img = L / runs, run = L - img * runs;
            for (int t = 0; t < ARITH_THREADS; t++) {
                const long long g = run * ARITH_PLANE_RUN + t;
                if (g >= groups) continue;
                if (g * 16 * C + 16 * C > bytes || g * 16 + 16 > pixels) return fail("plane group", W, H, C);
                if (img == 0) seen[(size_t)g]++;
            }
        }
        for (long long g = 0; g < groups; g++)
            if (seen[(size_t)g] != 1) return fail("group not taken once", W, H, C);
    }
    return 0;
}

// The header's table for one byte, in 64 bits and with the division LERP is defined by.
static int scalar_byte(const mi_blur_arith &k, int a, int b, int m)
{
    const auto fin = [&](long long acc) {
        const long long one = 1LL << k.shift;
        long long v = acc >= 0 ? acc / one : -((-acc + one - 1) / one);            // floor
        return (int)(v < 0 ? 0 : v > 255 ? 255 : v);
    };
    switch (k.op) {
    case MI_BLUR_ARITH_LINEAR: return fin((long long)k.wa * a + (long long)k.wb * b + k.bias);
    case MI_BLUR_ARITH_ABSDIFF: return fin((long long)k.wa * abs(a - b) + k.bias);
    case MI_BLUR_ARITH_MIN: return a < b ? a : b;
    case MI_BLUR_ARITH_MAX: return a > b ? a : b;
    case MI_BLUR_ARITH_MUL: return fin((long long)k.wa * a * b + k.bias);
    default: return (int)((2LL * (a * m + b * (255 - m)) + 255) / 510);
    }
}

static int32_t at_limit(int32_t lim) { return rnd() & 1 ? (rnd() & 1 ? lim : -lim) : (int32_t)rnd_range(-lim, lim); }
static mi_blur_arith random_struct(int op)
{
    mi_blur_arith k{};
    k.op = op;
    if (op == MI_BLUR_ARITH_LINEAR || op == MI_BLUR_ARITH_ABSDIFF || op == MI_BLUR_ARITH_MUL) {
        k.wa = at_limit(op == MI_BLUR_ARITH_MUL ? ARITH_MAX_W_MUL : ARITH_MAX_W);
        if (op == MI_BLUR_ARITH_LINEAR) k.wb = at_limit(ARITH_MAX_W);
        k.bias = at_limit(ARITH_MAX_BIAS);
        k.shift = rnd() % 3 ? rnd_range(0, ARITH_MAX_SHIFT) : (rnd() & 1 ? 0 : ARITH_MAX_SHIFT);
    }
    k.b_plane = rnd() & 1; k.b_shared = rnd() & 1;
    if (op == MI_BLUR_ARITH_LERP) { k.m_plane = rnd() & 1; k.m_shared = rnd() & 1; }
    return k;
}

// Part 2 for one case; 0 when clean.  in_place: 0 none, 1 out == a, 2 out == b (where B has the output's extent).
static int run_case(int W, int H, int C, int n_images, int op, int n_threads, int in_place)
{
    const mi_blur_arith k = random_struct(op);
    if (!arith_ok(&k)) return fail("struct refused", W, H, C);
    const size_t px = (size_t)W * H, bytes = (size_t)n_images * px * C;
    const size_t bc = k.b_plane ? 1 : C, mc = k.m_plane ? 1 : C;
    const size_t b_bytes = (k.b_shared ? 1 : n_images) * px * bc, m_bytes = (k.m_shared ? 1 : n_images) * px * mc;
    uint8_t *a = (uint8_t *)malloc(bytes), *b = (uint8_t *)malloc(b_bytes), *m = op == MI_BLUR_ARITH_LERP ? (uint8_t *)malloc(m_bytes) : nullptr;
    uint8_t *out = (uint8_t *)malloc(bytes);
    for (size_t i = 0; i < bytes; i++) a[i] = (uint8_t)(rnd() % 5 ? rnd() : (rnd() & 1 ? 0 : 255));
    for (size_t i = 0; i < b_bytes; i++) b[i] = (uint8_t)(rnd() % 5 ? rnd() : (rnd() & 1 ? 0 : 255));
    for (size_t i = 0; m && i < m_bytes; i++) m[i] = (uint8_t)(rnd() % 5 ? rnd() : (rnd() & 1 ? 0 : 255));
    std::vector<uint8_t> want(bytes);
    for (int i = 0; i < n_images; i++)
        for (size_t p = 0; p < px; p++)
            for (int c = 0; c < C; c++) {
                const int vb = b[((k.b_shared ? 0 : (size_t)i * px) + p) * bc + (k.b_plane ? 0 : c)];
                const int vm = m ? m[((k.m_shared ? 0 : (size_t)i * px) + p) * mc + (k.m_plane ? 0 : c)] : 0;
                want[((size_t)i * px + p) * C + c] = (uint8_t)scalar_byte(k, a[((size_t)i * px + p) * C + c], vb, vm);
            }
    const mi_blur_arith q = arith_normalised(k, C, n_images);
    if (in_place == 2 && (q.b_plane || q.b_shared)) in_place = 0;
    uint8_t *dst = in_place == 1 ? a : in_place == 2 ? b : out;
    int bad = 0;
    if (!arith_args_ok(a, b, m, dst, W, H, C, n_images, &k)) bad += fail("arguments refused", W, H, C);
    else {
        cpu_arith(a, b, m, dst, W, H, C, n_images, k, n_threads);
        if (memcmp(dst, want.data(), bytes)) bad += fail("bytes differ", W, H, C);
    }
    free(a); free(b); free(m); free(out);
    return bad;
}

// Part 3.
static int aliasing()
{
    int bad = 0;
    const int W = 12, H = 10, C = 3, n = 4;
    const size_t bytes = (size_t)n * W * H * C, plane = (size_t)W * H;
    std::vector<uint8_t> room(3 * bytes);
    uint8_t *base = room.data() + bytes;
    std::vector<uint8_t> other(bytes), mask(bytes);
    mi_blur_arith add{MI_BLUR_ARITH_LINEAR, 1, 1, 0, 0, 0, 0, 0, 0}, lerp{MI_BLUR_ARITH_LERP, 0, 0, 0, 0, 0, 0, 0, 0};
    const auto expect = [&](bool got, bool want, const char *what) { if (got != want) { printf("FAILED aliasing: %s\n", what); bad++; } };
    expect(arith_args_ok(base, other.data(), nullptr, base, W, H, C, n, &add), true, "out == a");
    expect(arith_args_ok(other.data(), base, nullptr, base, W, H, C, n, &add), true, "out == b");
    expect(arith_args_ok(base, base, nullptr, base, W, H, C, n, &add), true, "out == a == b");
    for (long long d : {1LL, 16LL, (long long)bytes - 1}) {
        expect(arith_args_ok(base + d, other.data(), nullptr, base, W, H, C, n, &add), false, "a above out");
        expect(arith_args_ok(base - d, other.data(), nullptr, base, W, H, C, n, &add), false, "a below out");
        expect(arith_args_ok(other.data(), base + d, nullptr, base, W, H, C, n, &add), false, "b above out");
        expect(arith_args_ok(other.data(), base - d, nullptr, base, W, H, C, n, &add), false, "b below out");
        expect(arith_args_ok(other.data(), mask.data(), base + d, base, W, H, C, n, &lerp), false, "m above out");
        expect(arith_args_ok(other.data(), mask.data(), base - d, base, W, H, C, n, &lerp), false, "m below out");
    }
    expect(arith_args_ok(base + bytes, base - bytes, nullptr, base, W, H, C, n, &add), true, "end to end");
    expect(arith_args_ok(other.data(), mask.data(), base, base, W, H, C, n, &lerp), false, "out == m");
    mi_blur_arith k = add;
    k.b_shared = 1;
    expect(arith_args_ok(other.data(), base, nullptr, base, W, H, C, n, &k), false, "out == shared b");
    expect(arith_args_ok(other.data(), base, nullptr, base, W, H, C, 1, &k), true, "out == shared b, one image");
    expect(arith_args_ok(other.data(), base - bytes / n, nullptr, base, W, H, C, n, &k), true, "shared b before out: one image long");
    expect(arith_args_ok(other.data(), base - bytes / n + 1, nullptr, base, W, H, C, n, &k), false, "shared b reaches out");
    expect(arith_args_ok(other.data(), base + bytes - 1, nullptr, base, W, H, C, n, &k), false, "shared b on out's last byte");
    k = add;
    k.b_plane = 1;
    expect(arith_args_ok(other.data(), base, nullptr, base, W, H, C, n, &k), false, "out == plane b");
    expect(arith_args_ok(other.data(), base, nullptr, base, W, H, C, 1, &k), false, "out == plane b, one image of three channels");
    expect(arith_args_ok(other.data(), base, nullptr, base, W, H, 1, n, &k), true, "out == plane b, one channel");
    expect(arith_args_ok(other.data(), base - n * plane, nullptr, base, W, H, C, n, &k), true, "plane b before out: n planes long");
    expect(arith_args_ok(other.data(), base - n * plane + 1, nullptr, base, W, H, C, n, &k), false, "plane b reaches out");
    k = lerp;
    k.m_plane = k.m_shared = 1;
    expect(arith_args_ok(other.data(), mask.data(), base - plane, base, W, H, C, n, &k), true, "shared plane m before out");
    expect(arith_args_ok(other.data(), mask.data(), base - plane + 1, base, W, H, C, n, &k), false, "shared plane m reaches out");
    expect(arith_args_ok(other.data(), mask.data(), nullptr, base, W, H, C, n, &lerp), false, "LERP without m");
    expect(arith_args_ok(other.data(), mask.data(), mask.data(), base, W, H, C, n, &add), false, "m without LERP");
    expect(arith_args_ok(other.data(), mask.data(), nullptr, base, W, H, C, 0, &add), true, "empty batch");
    expect(arith_args_ok(other.data(), mask.data(), nullptr, base, W, H, C, -1, &add), false, "negative batch");
    expect(arith_args_ok(other.data(), mask.data(), nullptr, base, 32768, 32768, 3, 1, &add), false, "image over the byte limit");
    expect(arith_args_ok(other.data(), mask.data(), nullptr, base, 32769, 1, 1, 1, &add), false, "width over the limit");
    return bad;
}

int main()
{
    int bad = 0;
    const int shapes[][2] = {{4, 4}, {1, 16}, {24, 2}, {16, ARITH_RUN - 1}, {16, ARITH_RUN}, {16, ARITH_RUN + 1}, {16, 2 * ARITH_RUN + 1}, {5, 7}, {4, 2},
                             {1920, 1080}, {4097, 4096}};
    for (const auto &s : shapes)
        for (int C = 1; C <= 4; C++) bad += walk(s[0], s[1], C, 3);
    // the largest images: the run counts and the workgroups of a large batch stay in 64 bits, far below their types' ends
    const int big[][3] = {{32768, 32768, 1}, {32768, 16383, 4}, {32768, 21845, 3}, {16384, 32767, 4}};
    for (const auto &s : big) {
        if (!hist_image_ok(s[0], s[1], s[2])) { bad += fail("largest image refused", s[0], s[1], s[2]); continue; }
        const long long bytes = (long long)s[0] * s[1] * s[2];
        if (bytes > INT_MAX) bad += fail("bytes", s[0], s[1], s[2]);
        if (arith_flat_ok(s[0], s[1], s[2]) && arith_flat_runs(s[0], s[1], s[2]) != (bytes / 16 + ARITH_RUN - 1) / ARITH_RUN) bad += fail("flat runs of the largest", s[0], s[1], s[2]);
        if (arith_plane_runs(s[0], s[1]) * ARITH_PLANE_RUN * COLOR_GROUP < (long long)s[0] * s[1]) bad += fail("plane runs of the largest", s[0], s[1], s[2]);
        if (arith_operand_bytes(s[0], s[1], s[2], 1 << 20, 0, 0) != bytes << 20) bad += fail("operand bytes", s[0], s[1], s[2]);
    }
    if (!bad) printf("geometry clean\n");

    int before = bad;
    const int sizes[][2] = {{1, 1}, {17, 1}, {13, 5}, {16, 16}, {300, 97}};
    for (int op = 0; op <= MI_BLUR_ARITH_LERP; op++)
        for (int C = 1; C <= 4; C++)
            for (const auto &s : sizes)
                for (int rep = 0; rep < 3; rep++) bad += run_case(s[0], s[1], C, 1 + rep, op, 1 + (int)(rnd() % 4), rep);
    for (int rep = 0; rep < 40; rep++)
        bad += run_case(rnd_range(1, 90), rnd_range(1, 70), rnd_range(1, 4), rnd_range(1, 5), rnd_range(0, 5), rnd_range(1, 5), rnd_range(0, 2));
    if (bad == before) printf("arith cases clean\n");

    before = bad;
    bad += aliasing();
    if (bad == before) printf("aliasing clean\n");
    return bad ? 1 : 0;
}
