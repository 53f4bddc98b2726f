// host-only sanitizer run of the perspective warp, two parts:
//   1. the CPU device (cpu_blur_batch with a WARP_PERSP filter) against a scalar loop written here from the header's text
//      (plain 64-bit floor divisions), on random small shapes, on the maps at the header's limits and on the extreme
//      shapes of tests/warp_perspective_ref.py, with exact-size heap buffers, so ASan sees any over-read / over-write and
//      UBSan any overflow of the coordinate arithmetic (the double estimate of floor_div_clamped() included);
//   2. the tile walk of blur_warp_persp_tiled_kernel on the CPU: for every tile of every aligned case, every pixel's taps
//      must lie in the tile's box (the corner rule of persp_footprint()) and every warp_tap() offset plus
//      warp_read_bytes(C) inside the LDS that persp_tiles_max_bytes() sizes.
// argv[1], optional: a file of further cases, one per line: W H C Wo Ho h0 .. h8 (the named maps, which need the setter).
#include "cpu_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef long long i64;
using namespace mi_blur;

static i64 fdiv(i64 a, i64 b) { i64 q = a / b; if (a % b != 0 && a < 0) q--; return q; }     // floor(a / b), b > 0
static i64 fshift(i64 v, int s) { return fdiv(v, (i64)1 << s); }

static i64 tap(const uint8_t *img, i64 W, i64 H, int C, int c, int border, int fill, i64 y, i64 x)
{
    if (border == MI_BLUR_WARP_CONSTANT && (x < 0 || x > W - 1 || y < 0 || y > H - 1)) return fill;
    x = x < 0 ? 0 : x > W - 1 ? W - 1 : x;
    y = y < 0 ? 0 : y > H - 1 ? H - 1 : y;
    return img[(y * W + x) * C + c];
}

struct Case { int W, H, C; mi_blur_warp_perspective w; };

static void describe(const char *what, const Case &k)
{
    printf("%s W%d H%d C%d Wo%d Ho%d mode%d border%d h", what, k.W, k.H, k.C, k.w.out_width, k.w.out_height, k.w.mode, k.w.border);
    for (int i = 0; i < 9; i++) printf(" %lld", (i64)k.w.h[i]);
    printf("\n");
}

static int run_case(const Case &k, int n, int nt, unsigned *seed)
{
    auto rnd = [&](int m) { *seed = *seed * 1664525u + 1013904223u; return (int)((*seed >> 8) % (unsigned)m); };
    const mi_blur_warp_perspective &w = k.w;
    const int W = k.W, H = k.H, C = k.C, Wo = w.out_width, Ho = w.out_height;
    const size_t isz = (size_t)W * H * C, osz = (size_t)Wo * Ho * C;
    uint8_t *in = (uint8_t *)malloc(isz * n), *out = (uint8_t *)malloc(osz * n), *want = (uint8_t *)malloc(osz * n);
    for (size_t i = 0; i < isz * n; i++) in[i] = (uint8_t)rnd(256);
    memset(out, 0xA5, osz * n);
    Filter f;
    if (filter_warp_persp(&w, &f) != MI_BLUR_OK || !persp_ok(&w, W, H, C)) { describe("REFUSED", k); return 1; }
    cpu_blur_batch(in, out, W, H, C, f, n, 0, H, nt, 0, 0);
    for (int i = 0; i < n; i++)
        for (int Y = 0; Y < Ho; Y++)
            for (int X = 0; X < Wo; X++) {
                const i64 nx = w.h[0] * X + w.h[1] * Y + w.h[2], ny = w.h[3] * X + w.h[4] * Y + w.h[5], d = w.h[6] * X + w.h[7] * Y + w.h[8];
                for (int c = 0; c < C; c++) {
                    const uint8_t *p = in + i * isz;
                    i64 v;
                    if (w.mode == MI_BLUR_RESIZE_NEAREST) {
                        v = tap(p, W, H, C, c, w.border, w.fill, fdiv(2 * ny + d, 2 * d), fdiv(2 * nx + d, 2 * d));
                    } else {
                        const i64 px = fdiv(nx * 4096 + d, 2 * d), py = fdiv(ny * 4096 + d, 2 * d);
                        const i64 x0 = fshift(px, 11), y0 = fshift(py, 11), fx = px - x0 * 2048, fy = py - y0 * 2048;
                        const i64 top = (2048 - fx) * tap(p, W, H, C, c, w.border, w.fill, y0, x0) + fx * tap(p, W, H, C, c, w.border, w.fill, y0, x0 + 1);
                        const i64 bot = (2048 - fx) * tap(p, W, H, C, c, w.border, w.fill, y0 + 1, x0) + fx * tap(p, W, H, C, c, w.border, w.fill, y0 + 1, x0 + 1);
                        v = ((2048 - fy) * top + fy * bot + (1 << 21)) >> 22;
                    }
                    want[i * osz + ((size_t)Y * Wo + X) * C + c] = (uint8_t)v;
                }
            }
    const int bad = memcmp(out, want, osz * n);
    if (bad) describe("MISMATCH", k);
    free(in); free(out); free(want);
    return bad ? 1 : 0;
}

// Part 2.  Returns -1 on a failure, else 1 when the case is aligned and its largest box fits (walked), 0 when not.
static int walk_tiles(const Case &k, long long *taps)
{
    const mi_blur_warp_perspective &w = k.w;
    const int W = k.W, H = k.H, C = k.C, Wo = w.out_width, Ho = w.out_height;
    if (C > 4 || (W * C) % 16 || (Wo * C) % 16) return 0;
    const TileGrid g = warp_grid(Wo * C / 16, Ho, C);
    const long long max_bytes = persp_tiles_max_bytes(g, w.h, w.border, W, H, Ho, C);
    if (max_bytes > WARP_LDS_MAX) return 0;
    const long long lds = max_bytes + WARP_LDS_SLACK;
    for (int ty = 0; ty < g.ntiles_y; ty++)
        for (int s = 0; s < g.nstrips; s++) {
            const Tile tl = tile_at(g, Ho, s, ty);
            const WarpBox b = persp_tile_box(w.h, w.border, W, H, C, tl.ty0, tl.rows_out, tl.x0c, tl.nc);
            const Span px = tile_pixels(tl.x0c, tl.nc, C);
            if (px.hi > Wo - 1) { describe("FAILED (a tile's pixels pass the row)", k); return -1; }
            const bool empty = warp_box_empty(b);
            const Span sc = empty ? Span{0, 0} : chunk_span(b.x0, b.x1, C);
            if (!empty && (b.x0 < 0 || b.y0 < 0 || b.x1 > W - 1 || b.y1 > H - 1 || (long long)(b.y1 - b.y0 + 1) * sc.n() * 16 > max_bytes)) { describe("FAILED (box)", k); return -1; }
            for (int Y = tl.ty0; Y < tl.ty0 + tl.rows_out; Y++)
                for (int X = px.lo; X <= px.hi; X++) {
                    const WarpCoord q = persp_coord(w.h, MI_BLUR_RESIZE_BILINEAR, W, H, X, Y);
                    for (int t = 0; t < 4; t++) {
                        const int x = q.x0 + (t & 1), y = q.y0 + (t >> 1);
                        const bool in_image = x >= 0 && x <= W - 1 && y >= 0 && y <= H - 1;
                        if (w.border == MI_BLUR_WARP_CONSTANT && !in_image) continue;          // `fill`: not read
                        const int cx = clamp_int(x, 0, W - 1), cy = clamp_int(y, 0, H - 1);
                        if (empty || cx < b.x0 || cx > b.x1 || cy < b.y0 || cy > b.y1) { describe("FAILED (a tap outside the box of the corners)", k); printf("  pixel %d %d tap %d %d\n", X, Y, x, y); return -1; }
                    }
                    if (empty) continue;
                    const WarpTap wt = warp_tap(b, sc, C, q.x0, q.y0);
                    for (const int off : {wt.off_a, wt.off_b})
                        if (off < 0 || (long long)(off & ~3) + warp_read_bytes(C) > lds) { describe("FAILED (a tap read outside the LDS)", k); printf("  pixel %d %d off %d lds %lld\n", X, Y, off, lds); return -1; }
                    *taps += 2;
                }
        }
    return 1;
}

int main(int argc, char **argv)
{
    unsigned s = 97531;
    auto rnd = [&](int n) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (unsigned)n); };
    const i64 Q = 65536, L = (i64)1 << 32, O = (i64)1 << 48;
    std::vector<Case> cases, walks;
    // random small shapes: affine parts up to 2, shifts around the image, perspective terms up to 1/32 per pixel either way
    while (cases.size() < 300) {
        Case k{1 + rnd(40), 1 + rnd(40), 1 + rnd(5), {1 + rnd(40), 1 + rnd(40), rnd(2), rnd(2), rnd(256), {}}};
        for (int i = 0; i < 6; i++) k.w.h[i] = i % 3 == 2 ? (i64)rnd(120 * 65536) - 40 * Q : (i64)rnd(4 * 65536) - 2 * Q;
        k.w.h[6] = rnd(4096) - 2048; k.w.h[7] = rnd(4096) - 2048; k.w.h[8] = Q;
        if (persp_ok(&k.w, k.W, k.H, k.C)) cases.push_back(k);
    }
    // aligned random shapes for the walk (and the CPU device)
    while (walks.size() < 60) {
        const int C = 1 + rnd(4), unit = C == 3 ? 16 : 16 / C;
        Case k{unit * (1 + rnd(8)), 1 + rnd(90), C, {unit * (1 + rnd(12)), 1 + rnd(90), MI_BLUR_RESIZE_BILINEAR, rnd(2), rnd(256), {}}};
        for (int i = 0; i < 6; i++) k.w.h[i] = i % 3 == 2 ? (i64)rnd(200 * 65536) - 60 * Q : (i64)rnd(3 * 65536) - 3 * Q / 2;
        k.w.h[6] = rnd(1024) - 512; k.w.h[7] = rnd(1024) - 512; k.w.h[8] = Q;
        if (persp_ok(&k.w, k.W, k.H, k.C)) walks.push_back(k);
    }
    // the limit maps of tests/warp_perspective_ref.py on 64 x 64 to 80 x 40 (96 x 40 for 3 channels), 1-4 channels, both modes and borders
    for (int C = 1; C <= 4; C++) {
        const i64 Wo = C == 3 ? 96 : 80;
        const i64 limits[][9] = {{0, 0, 30 * Wo, 0, 0, 20 * Wo, -1, 0, Wo}, {L, 0, 10 * O / 16, 0, L, 5 * O / 16, L, L, O}, {L, 0, 0, 0, L, 0, -L, -L, 95 * L + 39 * L + 1},
                                 {0, 0, O, 0, 0, -O, 0, 0, O}, {L, 0, O, 0, L, O, 0, 0, 1}, {3, 0, -7, 0, 2, 5, 0, 0, 1},
                                 {1, 0, 5 * O / 64, 0, 1, 6 * O / 64 + 12345, 0, 0, O / 64}, {Q, 0, 0, 0, Q, 0, Q / 8, Q / 16, Q},
                                 {-L, -L, -O, -L, -L, -O, L, L, O}, {L, L, O, -L, -L, -O, 0, 0, 1}};     // the last two: every entry at its limit
        for (const auto &h : limits)
            for (int mode = 0; mode < 2; mode++)
                for (int border = 0; border < 2; border++) {
                    Case k{64, 64, C, {(int)Wo, 40, mode, border, 173, {}}};
                    for (int i = 0; i < 9; i++) k.w.h[i] = h[i];
                    (mode == MI_BLUR_RESIZE_BILINEAR ? walks : cases).push_back(k);
                }
    }
    // the extreme shapes
    for (int border = 0; border < 2; border++) {
        walks.push_back(Case{32768, 1, 1, {32768, 1, MI_BLUR_RESIZE_BILINEAR, border, 7, {(i64)1 << 30, 0, 0, 0, (i64)1 << 30, 0, 1 << 14, 0, (i64)1 << 30}}});
        walks.push_back(Case{16, 32768, 1, {16, 32768, MI_BLUR_RESIZE_BILINEAR, border, 7, {(i64)1 << 30, 0, 0, 0, (i64)1 << 30, 0, 0, -(1 << 13), (i64)1 << 30}}});
    }
    if (argc > 1) {
        FILE *fp = fopen(argv[1], "r");
        if (!fp) { printf("FAILED: no case file %s\n", argv[1]); return 1; }
        Case k{};
        i64 h[9];
        while (fscanf(fp, "%d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld", &k.W, &k.H, &k.C, &k.w.out_width, &k.w.out_height, h, h + 1, h + 2, h + 3,
                      h + 4, h + 5, h + 6, h + 7, h + 8) == 14)
            for (int border = 0; border < 2; border++) {
                k.w.mode = MI_BLUR_RESIZE_BILINEAR; k.w.border = border; k.w.fill = 173;
                for (int i = 0; i < 9; i++) k.w.h[i] = h[i];
                walks.push_back(k);
            }
        fclose(fp);
    }
    int ran = 0, walked = 0;
    long long taps = 0;
    for (const Case &k : cases) { if (run_case(k, 1 + rnd(3), 1 + rnd(3), &s)) return 1; ran++; }
    for (const Case &k : walks) {
        if (run_case(k, 1, 1 + rnd(4), &s)) return 1;
        ran++;
        const int r = walk_tiles(k, &taps);
        if (r < 0) return 1;
        walked += r;
    }
    if (walked < (int)walks.size() * 3 / 4) { printf("FAILED: only %d of %zu aligned cases fit the LDS\n", walked, walks.size()); return 1; }
    printf("%d perspective warp cases clean\n", ran);
    printf("%d launches walked tile by tile: %lld taps inside their LDS\n", walked, taps);
    return 0;
}
