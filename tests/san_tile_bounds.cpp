// host-only sanitizer run: the LDS arithmetic of blur_resize_tiled_kernel and blur_warp_tiled_kernel, executed on the CPU.
// The kernels take their footprint and every LDS position from functions of filter.h ("Tile geometry"), and the host
// sizes the dynamic LDS with the same functions.  For each launch of a sweep this walks every tile as the kernel does and
// checks (a) that every staged row and chunk lies inside the input image, (b) that the staged box fits the LDS the host's
// sizing returned, (c) that every position and row the tap functions return, for every output pixel, lies inside the
// staged box (for the warp with the bytes its reads touch behind it, within the slack), and (d) that a launch the sweep
// expects to be admitted is admitted.  UBSan sees any overflow of the coordinate arithmetic on the way.  The warp sweep
// includes the extreme shapes, one-chunk inputs and maps at the header's limits of tests/warp_ref.py (EXTREME,
// narrow_cases(), LIMIT_MAPS) and the two near-2-GiB launches of tests/test_large_shapes_gpu.py; where the output is the
// image near 2^31 bytes (700 M pixels) every tile's box is checked and the taps of three tile rows.
#include "filter.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace mi_blur;
typedef int64_t i64;

static const i64 Q = 65536;
static const int LDS_LIMIT = 65536;                 // the dynamic LDS a launch may ask for without raising the limit
static long launches = 0, tiles = 0, taps = 0, empty_tiles = 0;

#define CHECK(cond, ...) \
    do { if (!(cond)) { printf("FAILED %s (line %d): ", #cond, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// The strips cover the row exactly, in whole units, no tile is empty or wider than the kernel's widest.
static void check_grid(const TileGrid &g, int rows, int unit, int max_cols)
{
    CHECK(g.nstrips >= 1 && g.ntiles_y >= 1 && g.ncols >= unit && g.ncols <= max_cols && g.ncols % unit == 0, "cpr %d rows %d", g.cpr, rows);
    int covered = 0;
    for (int s = 0; s < g.nstrips; s++) {
        const Tile t = tile_at(g, rows, s, 0);
        CHECK(t.x0c == covered && t.nc >= unit && t.nc <= g.ncols && t.nc % unit == 0, "cpr %d strip %d", g.cpr, s);
        covered += t.nc;
    }
    CHECK(covered == g.cpr, "cpr %d covered %d", g.cpr, covered);
    int rows_covered = 0;
    for (int ty = 0; ty < g.ntiles_y; ty++) {
        const Tile t = tile_at(g, rows, 0, ty);
        CHECK(t.ty0 == rows_covered && t.rows_out >= 1 && t.rows_out <= TILE_TH, "rows %d tile row %d", rows, ty);
        rows_covered += t.rows_out;
    }
    CHECK(rows_covered == rows, "rows %d covered %d", rows, rows_covered);
}

// ---------------------------------------------------------------- resize
static void check_resize(int W, int H, int Wo, int Ho, int C)
{
    CHECK(W * C % 16 == 0 && Wo * C % 16 == 0 && Wo >= W && Ho >= H, "not a launch of the tiled kernel");
    const TileGrid g = tile_grid(Wo * C / 16, Ho);
    check_grid(g, Ho, 1, TILE_NCOLS);
    const ResizeTiles t = resize_tiles(g, W, H, Wo, Ho, C);
    CHECK(resize_tiles_fit(t), "W %d H %d Wo %d Ho %d C %d: %d chunks x %d rows", W, H, Wo, Ho, C, t.max_nsc, t.max_nsr);      // (d): every enlargement
    const int v_off = resize_v_off(t);
    const size_t lds = resize_lds_bytes(t);
    CHECK(lds <= (size_t)LDS_LIMIT, "lds %zu", lds);
    launches++;
    for (int ty = 0; ty < g.ntiles_y; ty++)
        for (int s = 0; s < g.nstrips; s++) {
            const Tile tl = tile_at(g, Ho, s, ty);
            const Span sr = resize_stage_rows(H, Ho, tl.ty0, tl.rows_out), sc = resize_stage_chunks(W, Wo, C, tl.x0c, tl.nc);
            const int nsr = sr.n(), nsc = sc.n();
            tiles++;
            CHECK(0 <= sr.lo && sr.lo <= sr.hi && sr.hi < H && 0 <= sc.lo && sc.lo <= sc.hi && sc.hi < W * C / 16, "(a) tile %d,%d", s, ty);
            CHECK(nsr <= t.max_nsr && nsc <= t.max_nsc && RS_XTAB + RS_YTAB + nsr * nsc * 16 <= v_off, "(b) staged box, tile %d,%d", s, ty);
            CHECK((size_t)v_off + (size_t)RS_GROUP * nsc * 64u <= lds, "(b) V rows, tile %d,%d", s, ty);
            CHECK(tl.nc * 16 * 4 <= RS_XTAB && tl.rows_out * 4 <= RS_YTAB, "(b) tables, tile %d,%d", s, ty);
            for (int ob = 0; ob < tl.nc * 16; ob++) {               // the x table, as the kernel fills it
                const int gb = tl.x0c * 16 + ob, X = gb / C, c = gb - X * C;
                const ResizeCoord rc = resize_axis(W, Wo, MI_BLUR_RESIZE_BILINEAR, X);
                const uint32_t e = resize_x_entry(rc, C, c, sc.lo, nsc);
                const int qa = rc.a * C + c - sc.lo * 16, qb = rc.b * C + c - sc.lo * 16;
                CHECK(qa >= 0 && qa < nsc * 16 && qb >= 0 && qb < nsc * 16, "(c) staged byte of X %d", X);
                CHECK(resize_x_pos_a(e) == resize_v_pos(qa, nsc) && resize_x_pos_b(e) == resize_v_pos(qb, nsc) && resize_x_f(e) == (uint32_t)rc.f, "(c) x entry of X %d", X);
                CHECK(resize_x_pos_a(e) < (uint32_t)nsc * 16u && resize_x_pos_b(e) < (uint32_t)nsc * 16u, "(c) V position of X %d", X);
                taps++;
            }
            for (int k = 0; k < tl.rows_out; k++) {                 // the y table
                const ResizeCoord rc = resize_axis(H, Ho, MI_BLUR_RESIZE_BILINEAR, tl.ty0 + k);
                const uint32_t e = resize_y_entry(rc, sr.lo);
                CHECK(resize_y_row_a(e) == (uint32_t)(rc.a - sr.lo) && resize_y_row_b(e) == (uint32_t)(rc.b - sr.lo) && resize_y_f(e) == (uint32_t)rc.f, "(c) y entry of Y %d", tl.ty0 + k);
                CHECK(rc.a >= sr.lo && rc.b >= sr.lo && resize_y_row_a(e) < (uint32_t)nsr && resize_y_row_b(e) < (uint32_t)nsr, "(c) staged row of Y %d", tl.ty0 + k);
            }
        }
}

// kernel_proofs.chunk_cols: cpr rounded to the nearest chunk count that whole pixels of c channels fill
static int chunk_cols(int cpr, int c)
{
    const int a = c == 3 ? 3 : 1, n = (int)std::lround((double)cpr / a) * a;
    return n > a ? n : a;
}

static void sweep_resize()
{
    const int CI[] = {1, 2, 3, 31, 32, 33}, HS[] = {1, 2, 31, 32, 33};         // RESIZE_CI, RESIZE_H of test_kernel_proofs_gpu.py
    for (int c = 1; c <= 4; c++)
        for (int ci : CI) {
            const int a = chunk_cols(ci, c);
            for (int co : {ci, ci + 1, 2 * ci - 1, 2 * ci, 2 * ci + 1, 3 * ci + 1, 97}) {
                const int b = chunk_cols(co, c);
                if (b < a) continue;
                for (int h : HS)
                    for (int ho : {h, h + 1, 2 * h - 1, 2 * h, 2 * h + 1, 32 * h + 1})
                        if (ho >= h) check_resize(a * 16 / c, h, b * 16 / c, ho, c);
            }
        }
    for (int c = 1; c <= 4; c++) check_resize(1920, 1080, 3840, 2160, c);     // the x2 of a video frame
}

// the tiles of the INPUT image of blur_sep_down_tiled_kernel (DOWN_PAIRS x SEP_ROWS of test_kernel_proofs_gpu.py)
static void sweep_sep_down_grid()
{
    for (int c = 1; c <= 4; c++)
        for (int pairs : {1, 2, 3, 15, 16, 17, 32, 33, 49}) {
            if (c == 3) pairs = (int)std::lround(pairs / 3.0) * 3 > 3 ? (int)std::lround(pairs / 3.0) * 3 : 3;
            const int unit = c == 3 ? 6 : 2, max_units = c == 3 ? 4 : TILE_NCOLS / unit;
            for (int rows : {1, 2, 7, 8, 9, 31, 32, 33, 64, 65}) {
                check_grid(tile_grid(2 * pairs, rows, unit, max_units), rows, unit, unit * max_units);
                launches++;
            }
        }
}

// ---------------------------------------------------------------- warp
struct Mat { i64 m[6]; };

static Mat quantise(const double (&v)[6])
{
    Mat q;
    for (int i = 0; i < 6; i++) q.m[i] = (i64)std::floor(v[i] * 65536.0 + 0.5);
    return q;
}
// warp_ref.rotation_m: the OUTPUT -> INPUT matrix of a rotation about (cx, cy)
static Mat rotation_m(double cx, double cy, double deg, double scale = 1.0)
{
    const double r = deg * 3.14159265358979323846 / 180.0, a = scale * std::cos(r), b = scale * std::sin(r);
    const double tx = (1 - a) * cx - b * cy, ty = b * cx + (1 - a) * cy, det = a * a + b * b;
    const double ia = a / det, ib = -b / det, ic = b / det, id = a / det;
    return quantise({ia, ib, -(ia * tx + ib * ty), ic, id, -(ic * tx + id * ty)});
}
static Mat centre_rotation(int w, int h, double deg, double scale = 1.0) { return rotation_m((w - 1) / 2.0, (h - 1) / 2.0, deg, scale); }
static Mat scale_m(int num, int den) { const i64 s = Q * den / num, t = (s - Q) / 2; return {{s, 0, t, 0, s, t}}; }

// Returns whether the launch is admitted; every tile of an admitted launch is checked: its grid position and box, and
// the taps of every pixel (tap_tile_rows: of the pixels of those tile rows only).
static bool check_warp(int W, int H, int Wo, int Ho, int C, const Mat &mat, int border, std::initializer_list<int> tap_tile_rows = {})
{
    const i64 *m = mat.m;
    CHECK(W * C % 16 == 0 && Wo * C % 16 == 0, "not a launch of the tiled kernel");
    const TileGrid g = warp_grid(Wo * C / 16, Ho, C);
    check_grid(g, Ho, warp_unit(C), warp_max_cols(C));
    const i64 max_bytes = warp_tiles_max_bytes(g, m, border, W, H, Ho, C);
    launches++;
    if (max_bytes > WARP_LDS_MAX) return false;
    const i64 lds = max_bytes + WARP_LDS_SLACK;
    CHECK(lds <= LDS_LIMIT, "lds %lld", (long long)lds);
    for (int ty = 0; ty < g.ntiles_y; ty++)
        for (int s = 0; s < g.nstrips; s++) {
            const Tile tl = tile_at(g, Ho, s, ty);
            const Span px = tile_pixels(tl.x0c, tl.nc, C);
            CHECK(px.lo * C == tl.x0c * 16 && (px.hi + 1) * C == (tl.x0c + tl.nc) * 16, "a strip of whole pixels, tile %d,%d", s, ty);
            const WarpBox b = warp_tile_box(m, border, W, H, C, tl.ty0, tl.rows_out, tl.x0c, tl.nc);
            tiles++;
            if (warp_box_empty(b)) {
                CHECK(border == MI_BLUR_WARP_CONSTANT, "an empty box under CLAMP, tile %d,%d", s, ty);
                empty_tiles++;
            }
            Span sc{0, 0};
            int nsr = 0;
            i64 box_bytes = 0;
            if (!warp_box_empty(b)) {
                sc = chunk_span(b.x0, b.x1, C);
                nsr = b.y1 - b.y0 + 1;
                box_bytes = (i64)nsr * sc.n() * 16;
                CHECK(0 <= b.x0 && b.x1 < W && 0 <= b.y0 && b.y1 < H && 0 <= sc.lo && sc.hi < W * C / 16, "(a) tile %d,%d", s, ty);
                CHECK(sc.lo * 16 <= b.x0 * C && (b.x1 + 1) * C <= (sc.hi + 1) * 16, "(a) the chunks hold the box, tile %d,%d", s, ty);
                CHECK(box_bytes <= max_bytes, "(b) tile %d,%d: %lld > %lld", s, ty, (long long)box_bytes, (long long)max_bytes);
                // the offsets the kernel forms in 32 bits: the first staged chunk, the last output byte of the tile
                CHECK((i64)b.y0 * W * C + (i64)sc.lo * 16 <= 0x7fffffffLL && (i64)(tl.ty0 + tl.rows_out) * Wo * C <= 0x7fffffffLL, "an offset over 2^31, tile %d,%d", s, ty);
            }
            if (tap_tile_rows.size() && std::find(tap_tile_rows.begin(), tap_tile_rows.end(), ty) == tap_tile_rows.end()) continue;
            for (int Y = tl.ty0; Y < tl.ty0 + tl.rows_out; Y++)
                for (int X = px.lo; X <= px.hi; X++) {
                    const WarpPos p = warp_position(m, X, Y);
                    const WarpAxis ax = warp_axis(p.sx, MI_BLUR_RESIZE_BILINEAR, W), ay = warp_axis(p.sy, MI_BLUR_RESIZE_BILINEAR, H);
                    const bool in_x[2] = {ax.i0 >= 0 && ax.i0 < W, ax.i0 + 1 >= 0 && ax.i0 + 1 < W}, in_y[2] = {ay.i0 >= 0 && ay.i0 < H, ay.i0 + 1 >= 0 && ay.i0 + 1 < H};
                    if (warp_box_empty(b)) {                        // the kernel writes `fill` and reads nothing: no tap may lie inside the image
                        CHECK(!((in_x[0] || in_x[1]) && (in_y[0] || in_y[1])), "a tap of (%d, %d) inside the image, tile %d,%d empty", X, Y, s, ty);
                        continue;
                    }
                    // the box holds every tap that lies inside the image (CONSTANT) / the clamp into it is the clamp into the image (CLAMP)
                    for (int k = 0; k < 2; k++) {
                        const int x = ax.i0 + k, y = ay.i0 + k;
                        if (border == MI_BLUR_WARP_CLAMP) {
                            CHECK(clamp_int(x, b.x0, b.x1) == clamp_int(x, 0, W - 1) && clamp_int(y, b.y0, b.y1) == clamp_int(y, 0, H - 1), "(c) clamp of (%d, %d)", X, Y);
                        } else {
                            CHECK((!in_x[k] || (x >= b.x0 && x <= b.x1)) && (!in_y[k] || (y >= b.y0 && y <= b.y1)), "(c) tap of (%d, %d) outside the box", X, Y);
                        }
                    }
                    const WarpTap wt = warp_tap(b, sc, C, ax.i0, ay.i0);
                    const int rowb = sc.n() * 16;
                    for (const int off : {wt.off_a, wt.off_b}) {
                        const int row = off / rowb, col = off - row * rowb, npix = wt.one ? 1 : 2, rd = off & ~3;
                        CHECK(off >= 0 && row < nsr && col + npix * C <= rowb, "(c) tap of (%d, %d) at %d", X, Y, off);
                        CHECK(rd + warp_read_bytes(C) >= off + npix * C, "(c) the reads of (%d, %d) miss a tap", X, Y);
                        CHECK(rd + warp_read_bytes(C) <= box_bytes + WARP_LDS_SLACK && box_bytes + WARP_LDS_SLACK <= lds, "(c) the reads of (%d, %d) at %d leave the LDS", X, Y, off);
                        taps++;
                    }
                }
        }
    return true;
}

static void sweep_warp()
{
    unsigned seed = 97531;
    auto rnd = [&](int k) { seed = seed * 1664525u + 1013904223u; return (int)((seed >> 8) % (unsigned)k); };
    const int BORDERS[] = {MI_BLUR_WARP_CLAMP, MI_BLUR_WARP_CONSTANT};
    // TILED_SHAPES of test_warp_gpu.py (H, W, C, Wo, Ho) under maps of its maps(): rotations, scales, a shear, sub-pixel
    // and negative translations, maps that leave the image
    const int shapes[][5] = {{80, 96, 1, 144, 70}, {80, 96, 2, 136, 70}, {80, 96, 3, 144, 70}, {80, 96, 4, 132, 70}};
    for (const auto &sh : shapes) {
        const int H = sh[0], W = sh[1], C = sh[2], Wo = sh[3], Ho = sh[4];
        Mat maps[] = {centre_rotation(W, H, 0), centre_rotation(W, H, 90), centre_rotation(W, H, 180), centre_rotation(W, H, 270), centre_rotation(W, H, 30),
                      centre_rotation(W, H, 45), centre_rotation(W, H, -17.3), centre_rotation(W, H, 30, 1 / 0.67), centre_rotation(W, H, -50, 1 / 1.04),
                      quantise({1.5, 0, -7.25, 0, 1.5, 3.5}), quantise({0.67, 0, 0.3, 0, 0.67, -0.6}), quantise({1.0, 0.5, -20.75, -0.5, 1.0, 30.5}),
                      {{Q, 0, 3 * Q / 8 + 1, 0, Q, -5 * Q / 8 - 1}}, {{Q, 0, -37 * Q + 77, 0, Q, -21 * Q - 5}}, {{Q, 0, (W + 70) * Q, 0, Q, 0}},
                      quantise({0.9, 0.1, -3.0 * W, -0.1, 0.9, -2.5 * H}), rotation_m(0, 0, 20)};
        for (const Mat &m : maps)
            for (int border : BORDERS) {
                CHECK(check_warp(W, H, Wo, Ho, C, m, border), "(d) a map of the admitted region");
                CHECK(check_warp(W, H, W, H, C, m, border), "(d) a map of the admitted region, at the input's size");
            }
    }
    // the matrices of test_the_admitted_region_fits_the_lds: 256 x 192 -> 272 x 200
    {
        Mat mats[] = {centre_rotation(256, 192, 0), centre_rotation(256, 192, 30), centre_rotation(256, 192, 45), centre_rotation(256, 192, 90),
                      centre_rotation(256, 192, -17.3), centre_rotation(256, 192, 135), scale_m(2, 1), scale_m(4, 1), quantise({1.0, 0.5, 0, 0.5, 1.0, 0}),
                      quantise({1.0, -0.5, 9.5, 0.5, 1.0, -3.25}), {{3 * Q / 2, 0, 0, 0, 3 * Q / 2, 0}}, {{0, -3 * Q / 2, 255 * Q, 3 * Q / 2, 0, 0}},
                      {{3 * Q / 4, 3 * Q / 4, 11, -3 * Q / 4, 3 * Q / 4, 100 * Q + 7}}};
        for (const Mat &m : mats)
            for (int c = 1; c <= 4; c++)
                for (int border : BORDERS) CHECK(check_warp(256, 192, 272, 200, c, m, border), "(d) a map of the admitted region");
    }
    // 512 x 256 pixels under one tile: not admitted; the 4x reduction fits
    for (int border : BORDERS) {
        CHECK(!check_warp(512, 512, 64, 64, 1, scale_m(1, 8), border), "an 8x reduction was admitted");
        CHECK(check_warp(512, 512, 128, 128, 1, scale_m(1, 4), border), "(d) the 4x reduction");
    }
    // CONSTANT, translated so that the tiles on the right and at the bottom miss the image
    {
        const long before = empty_tiles;
        for (int c = 1; c <= 4; c++)
            for (int border : BORDERS) CHECK(check_warp(96, 80, 144, 65, c, {{Q, 0, 40 * Q + 123, 0, Q, 45 * Q - 77}}, border), "(d) a translation");
        CHECK(empty_tiles > before, "no tile missed the image");
    }
    // random warps on a 96 x 80 input: any box inside that image fits, so all are admitted
    for (int it = 0; it < 400; it++) {
        const int C = 1 + rnd(4), unit = C == 3 ? 16 : 16 / C;       // pixels of a whole chunk (group of 3 for 3 channels)
        const int Wo = unit * (1 + rnd(160 / unit)), Ho = 1 + rnd(70);
        Mat m;
        for (int i = 0; i < 6; i++) m.m[i] = i % 3 == 2 ? (i64)rnd(300 * 65536) - 100 * Q : (i64)rnd(4 * 65536) - 2 * Q;
        CHECK(check_warp(96, 80, Wo, Ho, C, m, rnd(2)), "(d) a warp of a 30 KB image");
    }
}

// tests/warp_ref.py: EXTREME, narrow_cases(), LIMIT_MAPS, and the near-2-GiB launches of test_large_shapes_gpu.py.  All
// are launches the GPU tests expect on the tiled kernel, under both borders.
static void sweep_warp_extremes()
{
    const int BORDERS[] = {MI_BLUR_WARP_CLAMP, MI_BLUR_WARP_CONSTANT};
    const i64 L = (i64)1 << 26, O = (i64)1 << 46;
    // 32768 pixels along one axis: (H, W, C, Wo, Ho) and the map
    struct { int H, W, C, Wo, Ho; Mat m; } extreme[] = {
        {1, 32768, 1, 32768, 1, {{Q, 0, 3 * Q / 8 + 1, 0, Q, 0}}},
        {2, 32768, 1, 16384, 2, {{2 * Q, 0, Q / 2, 0, Q, Q / 3}}},
        {32768, 16, 1, 16, 32768, centre_rotation(16, 32768, 0.02)},
        {16, 32768, 1, 16, 32768, {{0, -Q, 32767 * Q, Q, 0, 0}}},
        {32768, 16, 1, 32768, 16, {{0, Q, 0, -Q, 0, 32767 * Q}}},
        {3, 16384, 4, 32768, 3, {{Q / 2, 0, -Q / 4, 0, Q, 0}}},
        {2, 32768, 3, 32768, 2, {{Q, 0, -5 * Q / 8, 0, Q, Q / 2}}},
        {2, 32768, 1, 16384, 2, {{2 * Q, 0, 40 * Q + Q / 2, 0, Q, Q / 3}}},          // these two pass 2^31, beyond the right and the bottom edge
        {32768, 16, 1, 16, 32768, {{Q, 0, Q / 3, 0, Q, 40 * Q + Q / 2}}}};
    for (const auto &e : extreme)
        for (int border : BORDERS) CHECK(check_warp(e.W, e.H, e.Wo, e.Ho, e.C, e.m, border), "(d) an extreme shape, H %d W %d", e.H, e.W);
    // inputs of one chunk per row (3 channels: one group of three): the box is the whole row or image
    const int rows[][2] = {{16, 1}, {8, 2}, {16, 3}, {4, 4}};
    for (const auto &r : rows)
        for (int H : {1, 2, 33}) {
            const int W = r[0], C = r[1], Wo = C == 4 ? 132 : 144, Ho = 33;
            const Mat maps[] = {scale_m(4, 1), centre_rotation(W, H, 30), {{Q, 0, -3 * Q / 8, 0, Q, 5 * Q / 8}}, {{Q, 0, (-W - 3) * Q, 0, Q, Q}}};
            for (const Mat &m : maps)
                for (int border : BORDERS) CHECK(check_warp(W, H, Wo, Ho, C, m, border), "(d) a one-chunk input, W %d C %d H %d", W, C, H);
        }
    // maps at the limits of the header and degenerate maps on 64 x 64: the whole image fits, so all are admitted
    const Mat limits[] = {{{L, 0, 0, 0, L, 0}}, {{-L, L, 63 * Q, L, -L, 63 * Q}}, {{L, 0, -79 * L + 5 * Q, 0, L, -39 * L + 7 * Q + 123}}, {{Q, 0, O, 0, Q, O}},
                          {{-Q, 0, -O, 0, -Q, -O}}, {{Q, 0, -O, 0, Q, 3 * Q}}, {{L, L, O, -L, -L, -O}}, {{0, 0, 10 * Q + 777, 0, 0, 20 * Q + 31111}},
                          {{Q, 0, 0, Q, 0, Q / 3}}, {{1, 0, 5 * Q, 0, 1, 6 * Q + 65535}}, {{L, 0, -40 * L + 30 * Q, 0, Q, 0}}, {{Q, 0, 0, L, Q, -20 * L}}};
    for (const Mat &m : limits)
        for (int c = 1; c <= 4; c++)
            for (int border : BORDERS) CHECK(check_warp(64, 64, c == 3 ? 96 : 80, 40, c, m, border), "(d) a map at the limits, m0 %lld m2 %lld", (long long)m.m[0], (long long)m.m[2]);
    // the OUTPUT within 75 kB of 2^31 bytes: every tile's box; the taps of the first tile row, the one at the 2^30-byte
    // offset (output row 13380) and the last
    const int BIG_H = 26757, BIG_W = 26752;
    for (int border : BORDERS)
        CHECK(check_warp(BIG_W, BIG_H / 2 + 1, BIG_W, BIG_H, 3, {{Q, 0, 0, -655, Q / 2, 133 * Q}}, border, {0, 13380 / TILE_TH, (BIG_H - 1) / TILE_TH}), "(d) the output near 2^31 bytes");
    // the INPUT near 2^31 bytes, 64 output rows from its first rows, those at the 2^30-byte offset, its last rows and beyond
    for (int first_row : {0, 13376, BIG_H - 60})
        for (int border : BORDERS)
            CHECK(check_warp(BIG_W, BIG_H, BIG_W, 64, 3, {{Q, 0, 3 * Q / 8 + 1, 0, Q, first_row * Q + 5 * Q / 8}}, border), "(d) the input near 2^31 bytes");
}

int main()
{
    sweep_sep_down_grid();
    sweep_resize();
    sweep_warp();
    sweep_warp_extremes();
    printf("%ld launches, %ld tiles (%ld outside the image), %ld taps inside their LDS\n", launches, tiles, empty_tiles, taps);
    return 0;
}
