// host-only sanitizer run of the remap: (1) the CPU device (cpu_blur_batch with a REMAP filter) against a scalar loop written
// here from the header's text, on random small shapes with random maps, with the four extreme entries (INT32_MIN,
// INT32_MAX, -4097, (n + 1) * 2048 + 1) planted, in exact-size heap buffers so ASan sees any over-read / over-write and
// UBSan any overflow of the coordinate arithmetic; (2) every tile of the mixed, rot30 and wild maps of tests/remap_ref.py
// walked with the kernel's own remap_box() / warp_tap() (filter.h): every LDS byte a staged tile would read must lie
// inside stage_bytes + WARP_LDS_SLACK, and the box a staged tile copies inside the image.
#include "cpu_device.h"
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef long long i64;
using namespace mi_blur;

static i64 floor_shift(i64 v, int s) { return v >= 0 ? v >> s : -((-v + ((i64)1 << s) - 1) >> s); }   // floor(v / 2^s) without shifting a negative

static i64 tap(const uint8_t *img, i64 W, i64 H, int C, int c, int border, int fill, i64 y, i64 x)
{
    if (border == MI_BLUR_WARP_CONSTANT && (x < 0 || x > W - 1 || y < 0 || y > H - 1)) return fill;
    x = x < 0 ? 0 : x > W - 1 ? W - 1 : x;
    y = y < 0 ? 0 : y > H - 1 ? H - 1 : y;
    return img[(y * W + x) * C + c];
}

static int run_case(int W, int H, int C, int n, int nt, const mi_blur_remap &r, const int32_t *map_src, unsigned *seed)
{
    auto rnd = [&](int k) { *seed = *seed * 1664525u + 1013904223u; return (int)((*seed >> 8) % (unsigned)k); };
    const int Wo = r.out_width, Ho = r.out_height;
    const size_t isz = (size_t)W * H * C, osz = (size_t)Wo * Ho * C, msz = (size_t)Wo * Ho * 2;
    uint8_t *in = (uint8_t *)malloc(isz * n), *out = (uint8_t *)malloc(osz * n), *want = (uint8_t *)malloc(osz * n);
    int32_t *map = (int32_t *)malloc(msz * sizeof(int32_t));            // exact size: a read past the last entry shows
    memcpy(map, map_src, msz * sizeof(int32_t));
    for (size_t i = 0; i < isz * n; i++) in[i] = (uint8_t)rnd(256);
    memset(out, 0xA5, osz * n);
    Filter f;
    if (filter_remap(&r, map, &f) != MI_BLUR_OK || !remap_ok(&r, W, H, C)) { printf("REFUSED W%d H%d Wo%d Ho%d\n", W, H, Wo, Ho); return 1; }
    cpu_blur_batch(in, out, W, H, C, f, n, 0, H, nt, 0, 0);
    for (int i = 0; i < n; i++)
        for (int Y = 0; Y < Ho; Y++)
            for (int X = 0; X < Wo; X++) {
                i64 px = map[((size_t)Y * Wo + X) * 2], py = map[((size_t)Y * Wo + X) * 2 + 1];
                px = px < -4096 ? -4096 : px > ((i64)W + 1) * 2048 ? ((i64)W + 1) * 2048 : px;
                py = py < -4096 ? -4096 : py > ((i64)H + 1) * 2048 ? ((i64)H + 1) * 2048 : py;
                for (int c = 0; c < C; c++) {
                    const uint8_t *p = in + i * isz;
                    i64 v;
                    if (r.mode == MI_BLUR_RESIZE_NEAREST) {
                        v = tap(p, W, H, C, c, r.border, r.fill, floor_shift(py + 1024, 11), floor_shift(px + 1024, 11));
                    } else {
                        const i64 x0 = floor_shift(px, 11), y0 = floor_shift(py, 11), fx = px - x0 * 2048, fy = py - y0 * 2048;
                        const i64 top = (2048 - fx) * tap(p, W, H, C, c, r.border, r.fill, y0, x0) + fx * tap(p, W, H, C, c, r.border, r.fill, y0, x0 + 1);
                        const i64 bot = (2048 - fx) * tap(p, W, H, C, c, r.border, r.fill, y0 + 1, x0) + fx * tap(p, W, H, C, c, r.border, r.fill, y0 + 1, x0 + 1);
                        v = ((2048 - fy) * top + fy * bot + (1 << 21)) >> 22;
                    }
                    want[i * osz + ((size_t)Y * Wo + X) * C + c] = (uint8_t)v;
                }
            }
    const int bad = memcmp(out, want, osz * n);
    if (bad) printf("MISMATCH W%d H%d Wo%d Ho%d C%d n%d nt%d mode%d border%d\n", W, H, Wo, Ho, C, n, nt, r.mode, r.border);
    free(in); free(out); free(want); free(map);
    return bad ? 1 : 0;
}

// Every tile of one output image as blur_remap_tiled_kernel would treat it: returns 1 on a tap outside the LDS.
static int walk(const char *name, const std::vector<int32_t> &map, int W, int H, int C, int Wo, int Ho, int border, int stage_bytes, long long *taps, int *staged, int *direct, int *empty)
{
    const TileGrid g = warp_grid(Wo * C / 16, Ho, C);
    const long long lds = (long long)stage_bytes + WARP_LDS_SLACK;
    for (int ty = 0; ty < g.ntiles_y; ty++)
        for (int s = 0; s < g.nstrips; s++) {
            const Tile tl = tile_at(g, Ho, s, ty);
            const WarpBox b = remap_tile_box(map.data(), border, W, H, Wo, C, tl.ty0, tl.rows_out, tl.x0c, tl.nc);
            if (warp_box_empty(b)) { if (border != MI_BLUR_WARP_CONSTANT) { printf("FAILED %s: an empty box under CLAMP\n", name); return 1; } ++*empty; continue; }
            if (b.x0 < 0 || b.y0 < 0 || b.x1 > W - 1 || b.y1 > H - 1 || b.x0 > b.x1 || b.y0 > b.y1) { printf("FAILED %s: box outside the image\n", name); return 1; }
            const Span sc = chunk_span(b.x0, b.x1, C);
            if (sc.lo < 0 || (sc.hi + 1) * 16 > W * C) { printf("FAILED %s: staged chunks outside the row\n", name); return 1; }
            const long long bytes = remap_box_bytes(b, C);
            if (bytes > stage_bytes) { ++*direct; continue; }
            ++*staged;
            const Span px = tile_pixels(tl.x0c, tl.nc, C);
            for (int Y = tl.ty0; Y < tl.ty0 + tl.rows_out; Y++)
                for (int X = px.lo; X <= px.hi; X++) {
                    const int32_t *e = map.data() + ((size_t)Y * Wo + X) * 2;
                    const WarpCoord q = remap_coord(e[0], e[1], MI_BLUR_RESIZE_BILINEAR, W, H);
                    const WarpTap wt = warp_tap(b, sc, C, q.x0, q.y0);
                    for (int off : {wt.off_a, wt.off_b}) {
                        const long long lo = off & ~3, hi = lo + warp_read_bytes(C);       // the bytes warp_taps<C> reads
                        if (off < 0 || hi > lds || off + C > bytes) { printf("FAILED %s: tap at %d of a %lld byte box, LDS %lld\n", name, off, bytes, lds); return 1; }
                        ++*taps;
                    }
                }
        }
    return 0;
}

static void identity(std::vector<int32_t> &m, int Wo, int Ho)
{
    m.resize((size_t)Wo * Ho * 2);
    for (int Y = 0; Y < Ho; Y++)
        for (int X = 0; X < Wo; X++) { m[((size_t)Y * Wo + X) * 2] = X * 2048; m[((size_t)Y * Wo + X) * 2 + 1] = Y * 2048; }
}

int main()
{
    unsigned s = 97531;
    auto rnd = [&](int n) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (unsigned)n); };
    int cases = 0;
    for (int it = 0; it < 300; it++) {
        const int W = 1 + rnd(40), H = 1 + rnd(40), C = 1 + rnd(5), n = 1 + rnd(3), nt = 1 + rnd(3);
        const mi_blur_remap r{1 + rnd(40), 1 + rnd(40), rnd(2), rnd(2), rnd(256), it % 3 == 0 ? 0 : 16 + rnd(65505)};
        std::vector<int32_t> map((size_t)r.out_width * r.out_height * 2);
        for (size_t i = 0; i < map.size(); i += 2) { map[i] = rnd((W + 5) * 2048) - 3 * 2048; map[i + 1] = rnd((H + 5) * 2048) - 3 * 2048; }
        const int32_t ex[4] = {INT32_MIN, INT32_MAX, -4097, (W + 1) * 2048 + 1}, ey[4] = {INT32_MIN, INT32_MAX, -4097, (H + 1) * 2048 + 1};
        for (int k = 0; k < 8; k++) {                       // the extreme entries: in x, in y, in both
            const size_t at = (size_t)rnd((int)(map.size() / 2)) * 2;
            if (k % 3 != 1) map[at] = ex[k % 4];
            if (k % 3 != 0) map[at + 1] = ey[(k + k / 4) % 4];
        }
        if (run_case(W, H, C, n, nt, r, map.data(), &s)) return 1;
        cases++;
    }
    for (int mode = 0; mode < 2; mode++)                    // every entry extreme, on a 1 x 1 and a small image
        for (int border = 0; border < 2; border++)
            for (int shape = 0; shape < 2; shape++) {
                const int W = shape ? 9 : 1, H = shape ? 8 : 1;
                const mi_blur_remap r{4, 4, mode, border, 200, 0};
                const int32_t ex[4] = {INT32_MIN, INT32_MAX, -4097, (W + 1) * 2048 + 1}, ey[4] = {INT32_MIN, INT32_MAX, -4097, (H + 1) * 2048 + 1};
                int32_t map[32];
                for (int i = 0; i < 16; i++) { map[2 * i] = ex[i % 4]; map[2 * i + 1] = ey[i / 4]; }
                if (run_case(W, H, 1 + shape * 2, 2, 2, r, map, &s)) return 1;
                cases++;
            }
    printf("%d random and extreme remap cases clean\n", cases);

    // the tile walk.  mixed: 512 x 512 x 1 -> 128 x 64, the identity left, an 8x reduction right (tests/remap_ref.py)
    long long taps = 0;
    int staged = 0, direct = 0, empty = 0;
    std::vector<int32_t> m;
    identity(m, 128, 64);
    for (int Y = 0; Y < 64; Y++)
        for (int X = 64; X < 128; X++) { m[((size_t)Y * 128 + X) * 2] = (X - 64) * 8 * 2048; m[((size_t)Y * 128 + X) * 2 + 1] *= 8; }
    for (int border = 0; border < 2; border++)
        if (walk("mixed", m, 512, 512, 1, 128, 64, border, 65520, &taps, &staged, &direct, &empty)) return 1;
    if (!staged || !direct) { printf("FAILED mixed: staged %d direct %d\n", staged, direct); return 1; }
    // rot30 (in double here: the walk does not depend on the last bit) and wild, on the GPU tests' shapes, every stage_bytes the tests use and the limits
    const int shapes[4][3] = {{1, 144, 70}, {2, 136, 70}, {3, 144, 70}, {4, 132, 70}};
    const int stages[4] = {16, 4096, 32752, 65520};
    for (const auto &sh : shapes) {
        const int C = sh[0], Wo = sh[1], Ho = sh[2], W = 96, H = 80;
        std::vector<int32_t> rot((size_t)Wo * Ho * 2), wild((size_t)Wo * Ho * 2);
        const double cs = std::cos(30.0 * 3.14159265358979323846 / 180.0), sn = std::sin(30.0 * 3.14159265358979323846 / 180.0), cx = (W - 1) / 2.0, cy = (H - 1) / 2.0;
        for (int Y = 0; Y < Ho; Y++)
            for (int X = 0; X < Wo; X++) {
                const size_t at = ((size_t)Y * Wo + X) * 2;
                rot[at] = (int32_t)std::floor((cs * (X - cx) - sn * (Y - cy) + cx) * 2048.0 + 0.5);
                rot[at + 1] = (int32_t)std::floor((sn * (X - cx) + cs * (Y - cy) + cy) * 2048.0 + 0.5);
                wild[at] = rnd((W + 5) * 2048 + 1) - 3 * 2048;
                wild[at + 1] = rnd((H + 5) * 2048 + 1) - 3 * 2048;
            }
        wild[0] = INT32_MIN; wild[1] = INT32_MAX; wild[wild.size() - 2] = INT32_MAX; wild[wild.size() - 1] = INT32_MIN;
        for (int border = 0; border < 2; border++)
            for (int stage : stages) {
                if (walk("rot30", rot, W, H, C, Wo, Ho, border, stage, &taps, &staged, &direct, &empty)) return 1;
                if (walk("wild", wild, W, H, C, Wo, Ho, border, stage, &taps, &staged, &direct, &empty)) return 1;
            }
    }
    printf("%lld taps inside their LDS (%d staged, %d direct, %d empty tiles)\n", taps, staged, direct, empty);
    return 0;
}
