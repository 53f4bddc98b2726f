// host-only sanitizer run of template matching and the peak search, in three parts:
//   1. the CPU device (cpu_match) against loops written here from the header's text, in exact-size heap buffers (ASan sees
//      any over-read or over-write, UBSan any signed overflow): every method, 1-4 channels, shared and per-image
//      templates, templates as large as the image, the all-255 extreme whose sums pass 2^31;
//   2. cpu_match_peak against a plain scan, signed and unsigned, tables of one row and of one column;
//   3. match_score() (filter.h) against the comparison it is defined by, on sums of random two-level windows and on the
//      half-way cases: k is the largest integer in 0..16384 with k = 0 or (2k - 1)^2 D <= 2^30 N^2.
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

typedef unsigned __int128 u128;

// The definition: N and D of the header, then the largest k by a walk down from 16384.
static bool holds(int k, u128 D, u128 rhs) { const u128 o = (u128)(2 * k - 1); return o * o * D <= rhs; }
static int32_t score_by_definition(int method, uint64_t A, uint64_t at, uint64_t sa, uint64_t saa, uint64_t st, uint64_t stt)
{
    __int128 N;
    u128 D;
    if (method == MI_BLUR_MATCH_NCC) { N = (__int128)at; D = (u128)saa * stt; }
    else { N = (__int128)(A * at) - (__int128)(sa * st); D = (u128)(A * saa - sa * sa) * (u128)(A * stt - st * st); }
    if (D == 0 || N == 0) return 0;
    const u128 n = (u128)(N < 0 ? -N : N), rhs = (n * n) << 30;
    int lo = 0, hi = MI_BLUR_MATCH_ONE;                                 // holds() is monotone: the largest k by bisection
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (holds(mid, D, rhs)) lo = mid; else hi = mid - 1;
    }
    return N < 0 ? -lo : lo;
}

static int one_match(int W, int H, int C, int n, int tw, int th, int shared, int fill, int n_threads)
{
    int bad = 0;
    const int Wo = W - tw + 1, Ho = H - th + 1, tb = tw * C;
    const size_t nt = shared ? 1 : (size_t)n;
    std::vector<uint8_t> in((size_t)n * H * W * C), t(nt * th * tb);
    for (auto &v : in) v = fill >= 0 ? (uint8_t)fill : (uint8_t)rnd();
    for (auto &v : t) v = fill >= 0 ? (uint8_t)fill : (uint8_t)rnd();
    for (int method = MI_BLUR_MATCH_SQDIFF; method <= MI_BLUR_MATCH_ZNCC; method++) {
        const mi_blur_match k{method, tw, th, shared};
        if (!match_ok(&k, W, H, C)) return fail("spec", W, H, tw);
        std::vector<uint32_t> out((size_t)n * Ho * Wo, 0x5A5A5A5Au);
        cpu_match(in.data(), t.data(), out.data(), W, H, C, n, k, n_threads);
        for (int img = 0; img < n; img++) {
            const uint8_t *T = t.data() + (shared ? 0 : (size_t)img * th * tb);
            uint64_t st = 0, stt = 0;
            for (int i = 0; i < th * tb; i++) { st += T[i]; stt += (uint64_t)T[i] * T[i]; }
            for (int y = 0; y < Ho; y++)
                for (int x = 0; x < Wo; x++) {
                    uint64_t at = 0, sq = 0, sad = 0, sa = 0, saa = 0;
                    for (int dy = 0; dy < th; dy++)
                        for (int b = 0; b < tb; b++) {
                            const int64_t a = in[(((size_t)img * H + y + dy) * W + x) * C + b], tv = T[dy * tb + b];
                            at += (uint64_t)(a * tv); sq += (uint64_t)((a - tv) * (a - tv)); sad += (uint64_t)(a < tv ? tv - a : a - tv);
                            sa += (uint64_t)a; saa += (uint64_t)(a * a);
                        }
                    if ((at | sq | sad) >> 32) return fail("a raw sum passes 32 bits", (long long)at, (long long)sq, (long long)sad);
                    uint32_t want;
                    switch (method) {
                    case MI_BLUR_MATCH_SQDIFF: want = (uint32_t)sq; break;
                    case MI_BLUR_MATCH_CCORR: want = (uint32_t)at; break;
                    case MI_BLUR_MATCH_SAD: want = (uint32_t)sad; break;
                    default: want = (uint32_t)score_by_definition(method, (uint64_t)th * tb, at, sa, saa, st, stt); break;
                    }
                    const uint32_t got = out[((size_t)img * Ho + y) * Wo + x];
                    if (got != want) bad += fail("match", method, (long long)got, (long long)want);
                }
        }
    }
    return bad;
}

static int match_cases()
{
    int bad = 0;
    for (int i = 0; i < 60; i++) {
        const int C = rnd_range(1, 4), W = rnd_range(1, 40), H = rnd_range(1, 24), n = rnd_range(1, 3);
        bad += one_match(W, H, C, n, rnd_range(1, W), rnd_range(1, H), (int)(rnd() & 1), -1, rnd_range(1, 5));
    }
    bad += one_match(37, 23, 3, 2, 37, 23, 1, -1, 2);                   // a single output
    bad += one_match(130, 129, 4, 1, 128, 128, 1, 255, 3);              // 255^2 * 65536: the largest sum there is
    bad += one_match(300, 2, 1, 1, 255, 1, 0, -1, 2);
    bad += one_match(2, 300, 1, 1, 1, 255, 0, -1, 2);
    if (!bad) printf("match cases clean\n");
    return bad;
}

static int peak_cases()
{
    int bad = 0;
    for (int i = 0; i < 200; i++) {
        const int Wo = i % 3 == 0 ? 1 : rnd_range(1, 30), Ho = i % 3 == 1 ? 1 : rnd_range(1, 20), n = rnd_range(1, 4), is_signed = (int)(rnd() & 1);
        std::vector<uint32_t> table((size_t)n * Wo * Ho);
        const uint32_t spread = i % 4 == 0 ? 3u : 0xffffffffu;          // few values: many ties
        for (auto &v : table) v = ((rnd() << 8) ^ rnd()) & spread;
        if (i % 4 == 0 && is_signed) for (auto &v : table) v -= 1u;    // ... around zero
        std::vector<int64_t> peaks((size_t)n * 6, -1);
        cpu_match_peak(table.data(), is_signed, Wo, Ho, n, peaks.data(), rnd_range(1, 4));
        for (int img = 0; img < n; img++) {
            int64_t want[6] = {0, 0, 0, 0, 0, 0};
            for (int e = 0; e < Wo * Ho; e++) {
                const uint32_t w = table[(size_t)img * Wo * Ho + e];
                const int64_t v = is_signed ? (int64_t)(int32_t)w : (int64_t)w;
                if (e == 0 || v < want[0]) { want[0] = v; want[1] = e % Wo; want[2] = e / Wo; }
                if (e == 0 || v > want[3]) { want[3] = v; want[4] = e % Wo; want[5] = e / Wo; }
            }
            if (memcmp(want, peaks.data() + 6 * (size_t)img, sizeof(want))) bad += fail("peak", i, img, is_signed);
        }
    }
    if (!bad) printf("peak cases clean\n");
    return bad;
}

static int score_cases()
{
    int bad = 0;
    for (int i = 0; i < 200000; i++) {
        const uint64_t A = i & 1 ? (uint64_t)rnd_range(1, 65536) : (uint64_t)rnd_range(1, 64);
        const uint64_t na = rnd() % (A + 1), nt = i % 5 == 0 ? na : rnd() % (A + 1);
        uint64_t a1 = rnd() & 255, a2 = rnd() & 255, t1 = rnd() & 255, t2 = rnd() & 255;
        if (i % 3 == 0) { t1 = a1; t2 = a2; }
        const uint64_t lo = na < nt ? na : nt, hi = na < nt ? nt : na;
        const uint64_t at = a1 * t1 * lo + (na > nt ? a1 * t2 : a2 * t1) * (hi - lo) + a2 * t2 * (A - hi);
        const uint64_t sa = a1 * na + a2 * (A - na), saa = a1 * a1 * na + a2 * a2 * (A - na);
        const uint64_t st = t1 * nt + t2 * (A - nt), stt = t1 * t1 * nt + t2 * t2 * (A - nt);
        for (int method = MI_BLUR_MATCH_NCC; method <= MI_BLUR_MATCH_ZNCC; method++) {
            const int32_t got = match_score(method, (uint32_t)A, (uint32_t)at, (uint32_t)sa, (uint32_t)saa, (uint32_t)st, (uint32_t)stt);
            const int32_t want = score_by_definition(method, A, at, sa, saa, st, stt);
            if (got != want) bad += fail("score", method, got, want);
        }
    }
    for (uint64_t m = 1; m <= 127; m += 2)                              // exactly half way, and one unit of N to either side
        for (int k = 1; k <= MI_BLUR_MATCH_ONE; k += k < 64 ? 1 : 509) {
            const uint64_t s = m << 15, N = (uint64_t)(2 * k - 1) * m;
            for (uint64_t at = N - 1; at <= N + 1 && at <= s; at++) {
                const int32_t got = match_score(MI_BLUR_MATCH_NCC, 65536u, (uint32_t)at, 0u, (uint32_t)s, 0u, (uint32_t)s);
                if (got != score_by_definition(MI_BLUR_MATCH_NCC, 65536, at, 0, s, 0, s) || (at == N && got != k)) bad += fail("half", (long long)m, k, got);
            }
        }
    if (!bad) printf("score cases clean\n");
    return bad;
}

int main()
{
    const int bad = match_cases() + peak_cases() + score_cases();
    return bad ? 1 : 0;
}
