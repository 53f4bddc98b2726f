// host-only sanitizer run of the area resize, in three parts:
//   1. the tile geometry of blur_area_tiled_kernel (filter.h) walked over a spread of launches as the kernel walks it:
//      every LDS position of the x table and the V rows against the size the host asks for, every input chunk and row a
//      thread loads against the image, every output dword against the output row;
//   2. the CPU device (cpu_blur_batch with an AREA filter) against a scalar loop written here from the header's text, on
//      random small shapes in exact-size heap buffers, so ASan sees any over-read or over-write;
//   3. the same on edge shapes: one row, one column, the ratio cap on either axis, one output pixel.
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mi_blur;

// w(X, i) of the header, in 64-bit signed arithmetic.
static long long weight(long long n_in, long long n_out, long long X, long long i)
{
    const long long hi = (X + 1) * n_in < (i + 1) * n_out ? (X + 1) * n_in : (i + 1) * n_out;
    const long long lo = X * n_in > i * n_out ? X * n_in : i * n_out;
    return hi > lo ? hi - lo : 0;
}

static int fail(const char *what, int W, int H, int Wo, int Ho, int C)
{
    printf("FAILED %s W%d H%d Wo%d Ho%d C%d\n", what, W, H, Wo, Ho, C);
    return 1;
}

// Part 1 for one launch; 0 when clean.
static int walk(int W, int H, int Wo, int Ho, int C)
{
    if (!area_ok(Wo, Ho, W, H, C) || Wo > W || Ho > H || (long long)W * C % 16 || (long long)Wo * C % 16) return fail("not a tiled launch", W, H, Wo, Ho, C);
    const AreaTiles t = area_tiles(W, Wo, Ho, C);
    if (!area_tiles_fit(t)) return fail("span over AREA_MAX_SPAN", W, H, Wo, Ho, C);
    if (t.span < t.max_nsc || (t.span != 64 && t.span != 128 && t.span != 256)) return fail("group narrower than the span", W, H, Wo, Ho, C);
    const long long lds = (long long)area_lds_bytes(t), xtab_dwords = area_xtab_bytes(t) / 4, vrow = area_v_row(t.max_nsc);
    const int groups = AREA_THREADS / t.span, rows_per_group = AREA_TH / groups, in_cpr = W * C / 16;
    if (lds > 65536 || xtab_dwords * 4 + groups * vrow * 4 != lds || area_xtab_bytes(t) % 16) return fail("LDS size", W, H, Wo, Ho, C);
    if (t.g.ncols % warp_unit(C) || t.g.ncols < 1 || (long long)t.g.nstrips * t.g.ncols < t.g.cpr || (long long)(t.g.nstrips - 1) * t.g.ncols >= t.g.cpr)
        return fail("strips", W, H, Wo, Ho, C);
    if ((long long)t.g.ntiles_y * AREA_TH < Ho || (long long)(t.g.ntiles_y - 1) * AREA_TH >= Ho) return fail("tile rows", W, H, Wo, Ho, C);
    long long covered = 0;
    for (int s = 0; s < t.g.nstrips; s++) {
        const int x0c = s * t.g.ncols, nc = t.g.cpr - x0c < t.g.ncols ? t.g.cpr - x0c : t.g.ncols;
        const Span sc = area_stage_chunks(W, Wo, C, x0c, nc);
        if (sc.lo < 0 || sc.hi >= in_cpr || sc.n() > t.max_nsc) return fail("span outside the row", W, H, Wo, Ho, C);
        for (int col = 0; col < sc.n(); col++)
            for (int e = 0; e < 16; e++)
                if ((long long)area_v_pos(col * 16 + e) >= vrow) return fail("V write", W, H, Wo, Ho, C);
        for (int ob = 0; ob < nc * 16; ob++) {
            if (2 * ob + 1 >= xtab_dwords) return fail("x table", W, H, Wo, Ho, C);
            const int gb = x0c * 16 + ob, X = gb / C, c = gb - X * C;
            if (X >= Wo) return fail("pixel outside the output", W, H, Wo, Ho, C);
            const AreaAxis ax = area_axis(W, Wo, X);
            const uint32_t e0 = area_x_entry0(ax, C, c, sc.lo), e1 = area_x_entry1(ax);
            const int q0 = (int)(e0 & 0xffffu), n = (int)(e0 >> 16);
            if (q0 != ax.i_lo * C + c - sc.lo * 16 || n != ax.i_hi - ax.i_lo + 1 || (int)(e1 & 0xffffu) != ax.w_lo || (int)(e1 >> 16) != ax.w_hi)
                return fail("x entry fields", W, H, Wo, Ho, C);
            for (int i = 0; i < n; i++) {
                const int q = q0 + i * C;
                if (q < 0 || q >= sc.n() * 16 || (long long)area_v_pos(q) >= vrow) return fail("V read", W, H, Wo, Ho, C);
            }
            covered++;
        }
        for (int od = 0; od < nc * 4; od++)
            if ((long long)x0c * 16 + od * 4 + 4 > (long long)Wo * C) return fail("output dword", W, H, Wo, Ho, C);
    }
    if (covered != (long long)Wo * C) return fail("output bytes not covered once", W, H, Wo, Ho, C);
    long long rows = 0;
    for (int ty = 0; ty < t.g.ntiles_y; ty++) {
        const int ty0 = ty * AREA_TH, rows_out = Ho - ty0 < AREA_TH ? Ho - ty0 : AREA_TH;
        for (int g = 0; g < groups; g++)
            for (int k = 0; k < rows_per_group; k++) {
                const int Y = ty0 + g * rows_per_group + k;
                if (Y >= ty0 + rows_out) continue;
                const AreaAxis ay = area_axis(H, Ho, Y);
                if (ay.i_lo < 0 || ay.i_hi >= H || ay.i_hi < ay.i_lo) return fail("input rows", W, H, Wo, Ho, C);
                rows++;
            }
    }
    if (rows != Ho) return fail("output rows not covered once", W, H, Wo, Ho, C);
    return 0;
}

// Parts 2 and 3 for one shape; 0 when clean.
static int run(int W, int H, int Wo, int Ho, int C, int n, int nt, unsigned *seed)
{
    auto rnd = [&](int m) { *seed = *seed * 1664525u + 1013904223u; return (int)((*seed >> 8) % (unsigned)m); };
    const size_t isz = (size_t)W * H * C, osz = (size_t)Wo * Ho * C;
    uint8_t *in = (uint8_t *)malloc(isz * n), *out = (uint8_t *)malloc(osz * n);
    for (size_t i = 0; i < isz * n; i++) in[i] = (uint8_t)rnd(256);
    memset(out, 0xA5, osz * n);
    const mi_blur_area r{Wo, Ho};
    Filter f;
    if (filter_area(&r, &f) != MI_BLUR_OK || !area_ok(&r, W, H, C)) return fail("refused", W, H, Wo, Ho, C);
    cpu_blur_batch(in, out, W, H, C, f, n, 0, H, nt, 0, 0);
    const long long D = (long long)W * H;
    int bad = 0;
    for (int i = 0; i < n && !bad; i++)
        for (int Y = 0; Y < Ho && !bad; Y++)
            for (int X = 0; X < Wo && !bad; X++)
                for (int c = 0; c < C; c++) {
                    long long S = 0;
                    for (long long y = (long long)Y * H / Ho; y <= ((long long)(Y + 1) * H - 1) / Ho; y++)
                        for (long long x = (long long)X * W / Wo; x <= ((long long)(X + 1) * W - 1) / Wo; x++)
                            S += weight(H, Ho, Y, y) * weight(W, Wo, X, x) * in[i * isz + ((size_t)y * W + x) * C + c];
                    if (out[i * osz + ((size_t)Y * Wo + X) * C + c] != (uint8_t)((2 * S + D) / (2 * D))) { bad = 1; break; }
                }
    free(in); free(out);
    return bad ? fail("MISMATCH", W, H, Wo, Ho, C) : 0;
}

int main()
{
    // ---- 1: the tile geometry
    int launches = 0;
    static const int WIDTHS[] = {16, 32, 48, 64, 112, 256, 1008, 1024, 1920, 4096, 32768};
    for (int C = 1; C <= 4; C++)
        for (int W : WIDTHS) {
            if ((long long)W * C % 16) continue;
            const int step = C == 3 || C == 1 ? 16 : C == 2 ? 8 : 4;                   // output widths of whole chunks
            for (int Wo = step; Wo <= W; Wo += (Wo < 20 * step ? step : 37 * step)) {
                if (W > MI_BLUR_AREA_MAX_RATIO * Wo) continue;
                static const int HS[][2] = {{1, 1}, {7, 7}, {9, 4}, {64, 1}, {67, 5}, {1080, 270}};
                for (const auto &h : HS) { if (walk(W, h[0], Wo, h[1], C)) return 1; launches++; }
            }
            if (walk(W, 13, W, 13, C)) return 1;                                         // equal size
            if (W % (16 * MI_BLUR_AREA_MAX_RATIO) == 0 && walk(W, 128, W / MI_BLUR_AREA_MAX_RATIO, 2, C)) return 1;   // the ratio cap
            launches += 2;
        }
    printf("%d launches: tile geometry clean\n", launches);

    // ---- 2: the CPU device on random shapes, enlargements included
    unsigned s = 8765;
    auto rnd = [&](int n) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (unsigned)n); };
    int cases = 0;
    for (int it = 0; it < 300; it++) {
        const int W = 1 + rnd(40), H = 1 + rnd(40), Wo = 1 + rnd(40), Ho = 1 + rnd(40), C = 1 + rnd(5), n = 1 + rnd(3), nt = 1 + rnd(3);
        if (run(W, H, Wo, Ho, C, n, nt, &s)) return 1;
        cases++;
    }
    printf("%d random area cases clean\n", cases);

    // ---- 3: one row, one column, the ratio cap, one output pixel
    static const int EDGE[][5] = {{1, 1, 1, 1, 3}, {50, 1, 7, 1, 3}, {1, 50, 1, 7, 2}, {50, 1, 50, 9, 1}, {1, 50, 9, 50, 1}, {64, 64, 1, 1, 5}, {128, 3, 2, 3, 3},
                                  {3, 128, 3, 2, 4}, {192, 130, 3, 3, 1}, {65, 2, 2, 1, 1}, {1, 1, 17, 23, 2}, {33, 1, 1, 1, 1}, {1, 33, 1, 1, 1}};
    cases = 0;
    for (const auto &e : EDGE)
        for (int nt = 1; nt <= 3; nt += 2) {
            if (run(e[0], e[1], e[2], e[3], e[4], 2, nt, &s)) return 1;
            cases++;
        }
    printf("%d edge area cases clean\n", cases);
    return 0;
}
