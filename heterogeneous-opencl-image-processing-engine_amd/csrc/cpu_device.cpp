// cpu_device.cpp — the engine's host-thread device and host-side helpers.
//
// The reference runs the same OpenCL kernel on a CL_DEVICE_TYPE_CPU device
// (heterogeneous_blur.c:170-176,507).  ROCm's OpenCL has no CPU device, so the
// `cpu` / `both` modes run this native implementation instead: same arithmetic
// (integer form of gaussian_kernel.cl:19-72, see blur_kernels.hip header), rows
// processed separably with an edge-replicated scratch row so the inner loops are
// branch-free and auto-vectorise.  This is a DEVICE THE CALLER ASKS FOR BY NAME
// (MI_BLUR_DEVICE_CPU), never a fallback for a missing GPU, and it shares no code
// with oracle/ (which is test infrastructure).
#include "cpu_device.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace mi_blur {

int hardware_threads()
{
    unsigned n = std::thread::hardware_concurrency();
    return n ? (int)n : 1;
}

// Persistent worker pool: a batch of 10-35 small images is ~1 ms of work, less than spawning a thread per core.
// Workers are created on first use (up to the hardware thread count) and reused by every parallel_for; callers
// are serialised (one parallel_for at a time), which is what a single CPU device wants anyway.
namespace {
class Pool {
public:
    static Pool &get() { static Pool p; return p; }
    // run fn(worker_index) on n_workers threads (including the caller); returns when all are done
    void run(int n_workers, const std::function<void(int)> &fn)
    {
        if (n_workers <= 1) { fn(0); return; }
        std::lock_guard<std::mutex> call(call_m_);
        grow(n_workers - 1);
        // Spinning pays only while batches follow each other closely (a stream: one every ~100 us); a caller that does something
        // long between two uses of the pool — builds a batch on one thread, say — should find the helpers asleep, not burning
        // the cores (and the cgroup's CPU quota) it is working on.  The gap since the previous use decides.
        const auto now = std::chrono::steady_clock::now();
        const double gap_us = std::chrono::duration<double, std::micro>(now - last_done_).count();
        // OFF by default (MI_BLUR_POOL_SPIN=<pause count> turns it on): measured, it is worth +30 % to a caller that does nothing
        // but feed the pool on an idle 8-vCPU VM, nothing on the 256-thread GPU hosts (a sleeping worker is woken fast enough
        // there: 71-95 us per 35-image batch on 16 threads either way), and it costs 4x inside the hosts on the small VM, where
        // the spinners take the cores the batch-building threads need
        static const int spin_max = [] { const char *e = getenv("MI_BLUR_POOL_SPIN"); const int v = e ? atoi(e) : -1; return v >= 0 ? v : 0; }();
        spin_budget_.store(gap_us < 250.0 ? spin_max : 0, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lk(m_);
            fn_ = &fn; active_ = n_workers - 1; pending_ = n_workers - 1; gen_++;
            pending_hint_.store(pending_, std::memory_order_release);
            gen_hint_.store(gen_, std::memory_order_release);
        }
        cv_.notify_all();
        fn(0);
        // the helpers finish within microseconds of the caller: look before sleeping
        for (int i = 0; i < 4000 && pending_hint_.load(std::memory_order_acquire) != 0; i++) cpu_relax();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this] { return pending_ == 0; });
        fn_ = nullptr;
        last_done_ = std::chrono::steady_clock::now();
    }
    ~Pool()
    {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; gen_++; gen_hint_.store(gen_, std::memory_order_release); }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }

private:
    void grow(int n)
    {
        while ((int)th_.size() < n) {
            const int id = (int)th_.size() + 1;
            th_.emplace_back([this, id] { loop(id); });
        }
    }
    void loop(int id)
    {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(int)> *fn = nullptr;
            // a stream of batches wakes the pool every ~100 us: a worker that has just finished spins that long for the next
            // generation before it goes to sleep on the condition variable (a sleeping worker costs the batch ~30-50 us)
            for (int i = 0, n = spin_budget_.load(std::memory_order_relaxed); i < n && gen_hint_.load(std::memory_order_acquire) == seen; i++) cpu_relax();
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                if (id <= active_) fn = fn_;
            }
            if (fn) {
                (*fn)(id);
                std::lock_guard<std::mutex> lk(m_);
                pending_hint_.store(pending_ - 1, std::memory_order_release);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    static void cpu_relax()
    {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
    std::atomic<int> spin_budget_{0};
    std::chrono::steady_clock::time_point last_done_{};
    std::atomic<unsigned long long> gen_hint_{0};
    std::atomic<int> pending_hint_{0};
    std::mutex call_m_, m_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    const std::function<void(int)> *fn_ = nullptr;
    unsigned long long gen_ = 0;
    int active_ = 0, pending_ = 0;
    bool stop_ = false;
};
}  // namespace

// Rows [y_begin, y_end) of one image / band of H rows.
void cpu_blur_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, int R, int y_begin, int y_end,
                   int out_row_shift)
{
    const int pitch = W * C, pad = R * C;
    std::vector<uint16_t> scratch((size_t)pitch + 2 * pad);
    uint16_t *v = scratch.data() + pad;               // v[-pad .. pitch+pad)
    for (int y = y_begin; y < y_end; y++) {
        // vertical pass: v[b] = sum_k taps[k] * in[clamp(y+k)][b]   (<= 4080)
        const uint8_t *rows[5];
        for (int k = -R; k <= R; k++) rows[k + R] = in + (size_t)std::min(std::max(y + k, 0), H - 1) * pitch;
        if (R == 1) {
            const uint8_t *a = rows[0], *b = rows[1], *c = rows[2];
            for (int i = 0; i < pitch; i++) v[i] = (uint16_t)(a[i] + 2 * b[i] + c[i]);
        } else {
            const uint8_t *a = rows[0], *b = rows[1], *c = rows[2], *d = rows[3], *e = rows[4];
            for (int i = 0; i < pitch; i++) v[i] = (uint16_t)(a[i] + e[i] + 4 * (b[i] + d[i]) + 6 * c[i]);
        }
        // clamp-to-edge in x == replicate the first/last pixel's channels outward
        for (int k = 1; k <= pad; k++) {
            v[-k] = v[((-k % C) + C) % C];
            v[pitch + k - 1] = v[pitch - C + ((k - 1) % C)];
        }
        // horizontal pass on the 16-bit sums, one truncating shift (gaussian_kernel.cl:70)
        uint8_t *o = out + (size_t)(y - out_row_shift) * pitch;
        if (R == 1) {
            for (int i = 0; i < pitch; i++) o[i] = (uint8_t)((v[i - C] + 2 * v[i] + v[i + C]) >> 4);
        } else {
            for (int i = 0; i < pitch; i++)
                o[i] = (uint8_t)((v[i - 2 * C] + v[i + 2 * C] + 4 * (v[i - C] + v[i + C]) + 6 * v[i]) >> 8);
        }
    }
}

// The same two passes at runtime taps: vertical sums <= 255 * 256 (16 bits), horizontal sums < 2^24 in 32 bits, one
// truncating shift.  R = 1 | 2 with the binomial taps is what cpu_blur_rows computes.
void cpu_blur_rows_sep(const uint8_t *in, uint8_t *out, int W, int H, int C, const SepTaps &k, int y_begin, int y_end,
                       int out_row_shift)
{
    const int pitch = W * C, pad = k.rx * C, nj = 2 * k.ry + 1;
    std::vector<uint16_t> scratch((size_t)pitch + 2 * pad);
    uint16_t *v = scratch.data() + pad;               // v[-pad .. pitch+pad)
    std::vector<uint32_t> acc((size_t)pitch);
    const uint8_t *rows[2 * SEP_MAX_R + 1];
    uint16_t wy[2 * SEP_MAX_R + 1], wx[2 * SEP_MAX_R + 1];
    for (int j = 0; j < nj; j++) wy[j] = (uint16_t)k.wy[SEP_MAX_R - k.ry + j];
    for (int i = 0; i <= 2 * k.rx; i++) wx[i] = (uint16_t)k.wx[SEP_MAX_R - k.rx + i];
    for (int y = y_begin; y < y_end; y++) {
        for (int j = 0; j < nj; j++) rows[j] = in + (size_t)std::min(std::max(y + j - k.ry, 0), H - 1) * pitch;
        {
            const uint8_t *a = rows[0];
            const uint16_t w0 = wy[0];
            for (int b = 0; b < pitch; b++) v[b] = (uint16_t)(w0 * a[b]);
        }
        for (int j = 1; j < nj; j++) {
            const uint8_t *a = rows[j];
            const uint16_t w = wy[j];
            if (w) for (int b = 0; b < pitch; b++) v[b] = (uint16_t)(v[b] + w * a[b]);
        }
        for (int q = 1; q <= pad; q++) {
            v[-q] = v[((-q % C) + C) % C];
            v[pitch + q - 1] = v[pitch - C + ((q - 1) % C)];
        }
        uint32_t *s = acc.data();
        {
            const uint16_t *a = v - pad;
            const uint32_t w0 = wx[0];
            for (int b = 0; b < pitch; b++) s[b] = w0 * a[b];
        }
        for (int i = 1; i <= 2 * k.rx; i++) {
            const uint16_t *a = v + (i - k.rx) * C;
            const uint32_t w = wx[i];
            if (w) for (int b = 0; b < pitch; b++) s[b] += w * a[b];
        }
        uint8_t *o = out + (size_t)(y - out_row_shift) * pitch;
        for (int b = 0; b < pitch; b++) o[b] = (uint8_t)(s[b] >> k.shift);
    }
}

// Huang's running median: per output row and channel one 256-bin histogram of the (2R+1)^2 window, slid along the row
// (one column of 2R+1 values out, one in), with the current median m and lt = #{window values < m} kept up to date, so
// a pixel costs O(R) plus the few steps m moves.  Exact: m is the smallest value with lt + hist[m] > k.
void cpu_median_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, int R, int y_begin, int y_end, int out_row_shift)
{
    const int pitch = W * C, D = 2 * R + 1, k = (D * D - 1) / 2;
    const uint8_t *rows[2 * 7 + 1];
    int hist[256];
    for (int y = y_begin; y < y_end; y++) {
        for (int j = 0; j < D; j++) rows[j] = in + (size_t)std::min(std::max(y + j - R, 0), H - 1) * pitch;
        uint8_t *o = out + (size_t)(y - out_row_shift) * pitch;
        for (int c = 0; c < C; c++) {
            std::fill(hist, hist + 256, 0);
            for (int i = -R; i <= R; i++) {
                const int xo = std::min(std::max(i, 0), W - 1) * C + c;
                for (int j = 0; j < D; j++) hist[rows[j][xo]]++;
            }
            int m = 0, lt = 0;
            for (int x = 0; x < W; x++) {
                if (x > 0) {
                    const int xr = std::min(std::max(x - R - 1, 0), W - 1) * C + c;   // column leaving the window
                    const int xa = std::min(x + R, W - 1) * C + c;                      // column entering it
                    for (int j = 0; j < D; j++) {
                        const int vr = rows[j][xr], va = rows[j][xa];
                        hist[vr]--; if (vr < m) lt--;
                        hist[va]++; if (va < m) lt++;
                    }
                }
                while (lt > k) { m--; lt -= hist[m]; }
                while (lt + hist[m] <= k) { lt += hist[m]; m++; }
                o[x * C + c] = (uint8_t)m;
            }
        }
    }
}

// Window minimum and / or maximum, separably: per output row the extremum of the 2 ry + 1 source rows (clamped to the band)
// into an edge-replicated scratch row, then the extremum of the 2 rx + 1 pixels along it.  Byte loops that vectorise.
void cpu_morph_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, int op, int rx, int ry, int y_begin, int y_end,
                    int out_row_shift)
{
    const int pitch = W * C, pad = rx * C;
    const bool want_lo = op != MI_BLUR_MORPH_DILATE, want_hi = op != MI_BLUR_MORPH_ERODE;
    std::vector<uint8_t> scratch(2 * ((size_t)pitch + 2 * pad) + 2 * (size_t)pitch);
    uint8_t *vlo = scratch.data() + pad, *vhi = vlo + pitch + 2 * pad;   // v[-pad .. pitch+pad)
    uint8_t *hlo = vhi + pitch + pad, *hhi = hlo + pitch;
    for (int y = y_begin; y < y_end; y++) {
        for (int j = -ry; j <= ry; j++) {
            const uint8_t *a = in + (size_t)std::min(std::max(y + j, 0), H - 1) * pitch;
            if (j == -ry) { memcpy(vlo, a, pitch); memcpy(vhi, a, pitch); continue; }
            if (want_lo) for (int b = 0; b < pitch; b++) vlo[b] = std::min(vlo[b], a[b]);
            if (want_hi) for (int b = 0; b < pitch; b++) vhi[b] = std::max(vhi[b], a[b]);
        }
        for (int q = 1; q <= pad; q++) {
            vlo[-q] = vlo[((-q % C) + C) % C]; vlo[pitch + q - 1] = vlo[pitch - C + ((q - 1) % C)];
            vhi[-q] = vhi[((-q % C) + C) % C]; vhi[pitch + q - 1] = vhi[pitch - C + ((q - 1) % C)];
        }
        uint8_t *o = out + (size_t)(y - out_row_shift) * pitch;
        uint8_t *lo = op == MI_BLUR_MORPH_ERODE ? o : hlo, *hi = op == MI_BLUR_MORPH_DILATE ? o : hhi;
        if (want_lo) memcpy(lo, vlo - pad, pitch);
        if (want_hi) memcpy(hi, vhi - pad, pitch);
        for (int i = 1; i <= 2 * rx; i++) {
            const uint8_t *a = vlo + (i - rx) * C, *b2 = vhi + (i - rx) * C;
            if (want_lo) for (int b = 0; b < pitch; b++) lo[b] = std::min(lo[b], a[b]);
            if (want_hi) for (int b = 0; b < pitch; b++) hi[b] = std::max(hi[b], b2[b]);
        }
        if (op == MI_BLUR_MORPH_GRADIENT) for (int b = 0; b < pitch; b++) o[b] = (uint8_t)(hi[b] - lo[b]);
    }
}

// The bilateral filter as include/mi_blur.h defines it: per output byte the taps of the window with a non-zero spatial
// weight, 32-bit unsigned sums (exact: filter_bilateral bounds the spatial sum), one rounding division.
void cpu_bilateral_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int y_begin, int y_end,
                        int out_row_shift)
{
    const int pitch = W * C, r = f.bil_r;
    for (int y = y_begin; y < y_end; y++) {
        uint8_t *o = out + (size_t)(y - out_row_shift) * pitch;
        for (int x = 0; x < W; x++) {
            for (int c = 0; c < C; c++) {
                const unsigned v0 = in[(size_t)y * pitch + (size_t)x * C + c];
                uint32_t num = 0, den = 0;
                for (int j = -r; j <= r; j++) {
                    const uint8_t *row = in + (size_t)std::min(std::max(y + j, 0), H - 1) * pitch + c;
                    const uint8_t *s = f.bil_s + (j + 8) * 17 + 8;
                    for (int i = -r; i <= r; i++) {
                        if (!s[i]) continue;
                        const unsigned v = row[(size_t)std::min(std::max(x + i, 0), W - 1) * C];
                        const uint32_t w = (uint32_t)s[i] * f.bil_range[v > v0 ? v - v0 : v0 - v];
                        den += w; num += w * v;
                    }
                }
                o[(size_t)x * C + c] = (uint8_t)((num + den / 2) / den);
            }
        }
    }
}

// The signed convolution as include/mi_blur.h defines it: per output row an int32 accumulator row; per window row an
// edge-replicated copy of the (clamped) source row, then one multiply-add pass along it per non-zero tap.
void cpu_conv_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int y_begin, int y_end,
                   int out_row_shift)
{
    const int pitch = W * C, rx = f.conv_rx, ry = f.conv_ry, pad = rx * C;
    const bool mag = f.conv_mode == MI_BLUR_CONV_MAG;
    std::vector<uint8_t> rowbuf((size_t)pitch + 2 * pad);
    std::vector<int32_t> accbuf(2 * (size_t)pitch);
    uint8_t *v = rowbuf.data() + pad;                    // v[-pad .. pitch + pad)
    int32_t *acc = accbuf.data(), *acc2 = acc + pitch;
    for (int y = y_begin; y < y_end; y++) {
        std::fill(accbuf.begin(), accbuf.end(), 0);
        for (int j = -ry; j <= ry; j++) {
            memcpy(v, in + (size_t)std::min(std::max(y + j, 0), H - 1) * pitch, pitch);
            for (int q = 1; q <= pad; q++) { v[-q] = v[((-q % C) + C) % C]; v[pitch + q - 1] = v[pitch - C + ((q - 1) % C)]; }
            for (int t = 0; t < (mag ? 2 : 1); t++) {
                const int16_t *k = f.conv_k[t] + (j + 7) * 15 + 7;
                int32_t *a = t ? acc2 : acc;
                for (int i = -rx; i <= rx; i++) {
                    const int32_t w = k[i];
                    if (!w) continue;
                    const uint8_t *s = v + i * C;
                    for (int b = 0; b < pitch; b++) a[b] += w * s[b];
                }
            }
        }
        uint8_t *o = out + (size_t)(y - out_row_shift) * pitch;
        for (int b = 0; b < pitch; b++) {
            int32_t a = f.conv_mode == MI_BLUR_CONV_SAT ? acc[b] : std::abs(acc[b]);
            if (mag) a += std::abs(acc2[b]);
            a = (a + f.conv_bias) >> f.conv_shift;       // arithmetic shift: the floor
            o[b] = (uint8_t)std::min(std::max(a, 0), 255);
        }
    }
}

// Output rows [Y_begin, Y_end) of the decimating separable filter of f (f.taps, f.down_*) on one W x H image: the two
// passes of cpu_blur_rows_sep at runtime taps, the vertical one on the kept rows only, the horizontal one at the kept
// columns only.  out = the decimated image (dense).
void cpu_sep_down_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end)
{
    const SepTaps &k = f.taps;
    const int pitch = W * C, pad = k.rx * C, nj = 2 * k.ry + 1, ni = 2 * k.rx + 1;
    const int sx = f.down_sx, sy = f.down_sy, ox = f.down_ox, oy = f.down_oy;
    const int Wo = down_cols(W, sx, ox), opitch = Wo * C;
    std::vector<uint16_t> scratch((size_t)pitch + 2 * pad);
    uint16_t *v = scratch.data() + pad;               // v[-pad .. pitch+pad)
    uint16_t wy[2 * SEP_MAX_R + 1], wx[2 * SEP_MAX_R + 1];
    for (int j = 0; j < nj; j++) wy[j] = (uint16_t)k.wy[SEP_MAX_R - k.ry + j];
    for (int i = 0; i < ni; i++) wx[i] = (uint16_t)k.wx[SEP_MAX_R - k.rx + i];
    for (int Y = Y_begin; Y < Y_end; Y++) {
        const int y = oy + Y * sy;
        {
            const uint8_t *a = in + (size_t)std::min(std::max(y - k.ry, 0), H - 1) * pitch;
            const uint16_t w0 = wy[0];
            for (int b = 0; b < pitch; b++) v[b] = (uint16_t)(w0 * a[b]);
        }
        for (int j = 1; j < nj; j++) {
            const uint8_t *a = in + (size_t)std::min(std::max(y + j - k.ry, 0), H - 1) * pitch;
            const uint16_t w = wy[j];
            if (w) for (int b = 0; b < pitch; b++) v[b] = (uint16_t)(v[b] + w * a[b]);
        }
        for (int q = 1; q <= pad; q++) {
            v[-q] = v[((-q % C) + C) % C];
            v[pitch + q - 1] = v[pitch - C + ((q - 1) % C)];
        }
        uint8_t *o = out + (size_t)Y * opitch;
        for (int X = 0; X < Wo; X++) {
            const uint16_t *a = v + (ox + X * sx - k.rx) * C;
            for (int c = 0; c < C; c++) {
                uint32_t s = 0;
                for (int i = 0; i < ni; i++) s += (uint32_t)wx[i] * a[i * C + c];
                o[X * C + c] = (uint8_t)(s >> k.shift);
            }
        }
    }
}

// Output rows [Y_begin, Y_end) of the resize of f (f.out_w, f.out_h, f.sample_mode) on one W x H image; out = the resized image (dense).
// xtab: resize_axis of every output column (resize_xtable: built once per call, shared by the threads).  BILINEAR blends
// the two input rows at the two input columns with bilinear_blend() (filter.h); NEAREST copies pixels.
void cpu_resize_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end, const ResizeCoord *xtab)
{
    const int Wo = f.out_w, Ho = f.out_h;
    const size_t pitch = (size_t)W * C, opitch = (size_t)Wo * C;
    for (int Y = Y_begin; Y < Y_end; Y++) {
        const ResizeCoord cy = resize_axis(H, Ho, f.sample_mode, Y);
        const uint8_t *ra = in + (size_t)cy.a * pitch, *rb = in + (size_t)cy.b * pitch;
        uint8_t *o = out + (size_t)Y * opitch;
        if (f.sample_mode == MI_BLUR_RESIZE_NEAREST) {
            for (int X = 0; X < Wo; X++)
                for (int c = 0; c < C; c++) o[(size_t)X * C + c] = ra[(size_t)xtab[X].a * C + c];
            continue;
        }
        for (int X = 0; X < Wo; X++) {
            const size_t xa = (size_t)xtab[X].a * C, xb = (size_t)xtab[X].b * C;
            for (int c = 0; c < C; c++)
                o[(size_t)X * C + c] = (uint8_t)bilinear_blend(ra[xa + c], ra[xb + c], rb[xa + c], rb[xb + c], (unsigned)xtab[X].f, (unsigned)cy.f);
        }
    }
}

// Output rows [Y_begin, Y_end) of the area resize of f (f.out_w, f.out_h) on one W x H image; out = the resized image (dense).
// Separable: the vertical sums V[q] = sum_j wy(Y, j) * in[j][q] of a whole input row of bytes (at most 255 H < 2^23), then
// per output byte S = sum_i wx(X, i) * V[i * C + c] in 64 bits and the one rounding of area_round() (filter.h): the
// arithmetic of blur_area_tiled_kernel.  xtab, ytab: area_xtable / area_ytable, built once per call, shared by the threads.
void cpu_area_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end, const AreaAxis *xtab, const AreaAxis *ytab)
{
    const int Wo = f.out_w, Ho = f.out_h;
    const size_t pitch = (size_t)W * C, opitch = (size_t)Wo * C;
    const int64_t D = (int64_t)W * H;
    const double rden = area_rden(W, H);
    std::vector<uint32_t> V(pitch);
    for (int Y = Y_begin; Y < Y_end; Y++) {
        const AreaAxis ay = ytab[Y];
        for (int j = ay.i_lo; j <= ay.i_hi; j++) {
            const uint8_t *r = in + (size_t)j * pitch;
            const uint32_t w = area_weight(ay, Ho, j);
            if (j == ay.i_lo) for (size_t q = 0; q < pitch; q++) V[q] = w * r[q];
            else for (size_t q = 0; q < pitch; q++) V[q] += w * r[q];
        }
        uint8_t *o = out + (size_t)Y * opitch;
        for (int X = 0; X < Wo; X++) {
            const AreaAxis ax = xtab[X];
            for (int c = 0; c < C; c++) {
                const uint32_t *v = V.data() + (size_t)ax.i_lo * C + c;
                uint64_t S = (uint64_t)(uint32_t)ax.w_lo * v[0];
                uint32_t mid = 0;                                       // at most 63 taps of less than 2^23
                const int n = ax.i_hi - ax.i_lo;
                for (int k = 1; k < n; k++) mid += v[(size_t)k * C];
                S += (uint64_t)(uint32_t)Wo * mid;
                if (n > 0) S += (uint64_t)(uint32_t)ax.w_hi * v[(size_t)n * C];
                o[(size_t)X * C + c] = (uint8_t)area_round(S, D, rden);
            }
        }
    }
}

// Rows [Y_begin, Y_end) of the colour transform f.color on one image of W pixels x C channels per row; out = the
// transformed image (dense, f.color.co channels).  Every byte through color_channel() (filter.h), the function of the
// GPU's generic kernel.
void cpu_color_rows(const uint8_t *in, uint8_t *out, int W, int C, const Filter &f, int Y_begin, int Y_end)
{
    const ColorSpec &k = f.color;
    const int co = k.co;
    const uint8_t *px = in + (size_t)Y_begin * W * C;
    uint8_t *o = out + (size_t)Y_begin * W * co;
    for (size_t n = (size_t)(Y_end - Y_begin) * W; n > 0; n--, px += C, o += co)
        for (int c = 0; c < co; c++) o[c] = color_channel(k, C, px, c);
}

// Output rows [Y_begin, Y_end) of the affine warp of f (f.warp_*) on one W x H image; out = the warped image (dense).
// Every byte through warp_coord() and warp_sample() (filter.h), the functions of the GPU's generic kernel.
void cpu_warp_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end)
{
    const int Wo = f.out_w;
    const size_t pitch = (size_t)W * C, opitch = (size_t)Wo * C;
    for (int Y = Y_begin; Y < Y_end; Y++) {
        uint8_t *o = out + (size_t)Y * opitch;
        for (int X = 0; X < Wo; X++) {
            const WarpCoord q = warp_coord(f.warp_m, f.sample_mode, W, H, X, Y);
            for (int c = 0; c < C; c++)
                o[(size_t)X * C + c] = (uint8_t)warp_sample(in + c, pitch, C, W, H, f.warp_border, (unsigned)f.warp_fill, q);
        }
    }
}

// The same for the perspective warp of f (f.warp_h): every byte through persp_coord_at() and warp_sample() (filter.h), the
// functions of the GPU's generic kernel; the numerators and the denominator step along a row as the tiled kernel's do.
void cpu_warp_persp_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end)
{
    const int Wo = f.out_w;
    const size_t pitch = (size_t)W * C, opitch = (size_t)Wo * C;
    for (int Y = Y_begin; Y < Y_end; Y++) {
        uint8_t *o = out + (size_t)Y * opitch;
        PerspPos s = persp_position(f.warp_h, 0, Y);
        for (int X = 0; X < Wo; X++) {
            const WarpCoord q = persp_coord_at(s, f.sample_mode, W, H);
            for (int c = 0; c < C; c++)
                o[(size_t)X * C + c] = (uint8_t)warp_sample(in + c, pitch, C, W, H, f.warp_border, (unsigned)f.warp_fill, q);
            s.nx += f.warp_h[0]; s.ny += f.warp_h[3]; s.d += f.warp_h[6];
        }
    }
}

// The same for the remap of f (f.remap_map, host memory here): every byte through remap_coord() and warp_sample() (filter.h),
// the functions of the GPU's generic kernel.
void cpu_remap_rows(const uint8_t *in, uint8_t *out, int W, int H, int C, const Filter &f, int Y_begin, int Y_end)
{
    const int Wo = f.out_w;
    const size_t pitch = (size_t)W * C, opitch = (size_t)Wo * C;
    for (int Y = Y_begin; Y < Y_end; Y++) {
        uint8_t *o = out + (size_t)Y * opitch;
        const int32_t *e = f.remap_map + (size_t)Y * (size_t)Wo * 2;
        for (int X = 0; X < Wo; X++) {
            const WarpCoord q = remap_coord(e[2 * X], e[2 * X + 1], f.sample_mode, W, H);
            for (int c = 0; c < C; c++)
                o[(size_t)X * C + c] = (uint8_t)warp_sample(in + c, pitch, C, W, H, f.warp_border, (unsigned)f.warp_fill, q);
        }
    }
}

// Empty for any filter but a resize.
std::vector<ResizeCoord> resize_xtable(int W, const Filter &f)
{
    if (f.kind != FilterKind::RESIZE) return {};
    std::vector<ResizeCoord> t((size_t)f.out_w);
    for (int X = 0; X < f.out_w; X++) t[(size_t)X] = resize_axis(W, f.out_w, f.sample_mode, X);
    return t;
}

// Empty for any filter but an area resize.
std::vector<AreaAxis> area_xtable(int W, const Filter &f)
{
    if (f.kind != FilterKind::AREA) return {};
    std::vector<AreaAxis> t((size_t)f.out_w);
    for (int X = 0; X < f.out_w; X++) t[(size_t)X] = area_axis(W, f.out_w, X);
    return t;
}
std::vector<AreaAxis> area_ytable(int H, const Filter &f)
{
    if (f.kind != FilterKind::AREA) return {};
    std::vector<AreaAxis> t((size_t)f.out_h);
    for (int Y = 0; Y < f.out_h; Y++) t[(size_t)Y] = area_axis(H, f.out_h, Y);
    return t;
}

// n_images bands of band_rows rows; output rows [y0,y1) of each.  Threads take whole
// images when there are enough of them, else row slices of each image.  A whole_image_only filter (filter.h): y0 = 0,
// y1 = band_rows; the output blocks are the filter's own output images and the row slices are cut in output rows.
void cpu_blur_batch(const uint8_t *in, uint8_t *out, int W, int band_rows, int C, const Filter &f, int n_images,
                    int y0, int y1, int n_threads, size_t in_stride, size_t out_stride)
{
    if (n_images <= 0) return;
    if (n_threads <= 0) n_threads = hardware_threads();
    if (in_stride == 0) in_stride = (size_t)W * C * band_rows;
    const OutShape o = out_shape(f, W, band_rows, C, y0, y1);
    if (whole_image_only(f)) { y0 = 0; y1 = o.rows; }           // from here on: output rows
    if (out_stride == 0) out_stride = (size_t)o.width * o.channels * o.rows;
    const std::vector<ResizeCoord> xtab = resize_xtable(W, f);
    const std::vector<AreaAxis> area_x = area_xtable(W, f), area_y = area_ytable(band_rows, f);
    const int rows = y1 - y0;
    // work items: (image, row slice)
    // enough items for the threads to end together: a batch of 35 images on 16 threads is three rounds of whole images with the
    // last one half empty; cut into row slices (of at least 16 rows) until there are ~4 items per thread
    static const int per_thread = [] { const char *e = getenv("MI_BLUR_POOL_ITEMS"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= 64 ? v : 4; }();
    int slices = 1;
    if (n_images < per_thread * n_threads)
        slices = std::max(1, std::min(std::max(1, rows / 16), (per_thread * n_threads + n_images - 1) / n_images));
    const long long items = (long long)n_images * slices;
    std::atomic<long long> next{0};
    auto worker = [&]() {
        for (;;) {
            const long long it = next.fetch_add(1, std::memory_order_relaxed);
            if (it >= items) break;
            const int img = (int)(it / slices), s = (int)(it % slices);
            const int ys = y0 + (int)((long long)rows * s / slices), ye = y0 + (int)((long long)rows * (s + 1) / slices);
            const uint8_t *src = in + img * in_stride;
            uint8_t *dst = out + img * out_stride;
            switch (f.kind) {                                   // no default label: a kind without a case is a -Wswitch warning
            case FilterKind::BOX: cpu_blur_rows(src, dst, W, band_rows, C, f.radius, ys, ye, y0); break;
            case FilterKind::SEP: cpu_blur_rows_sep(src, dst, W, band_rows, C, f.taps, ys, ye, y0); break;
            case FilterKind::MEDIAN: cpu_median_rows(src, dst, W, band_rows, C, f.radius, ys, ye, y0); break;
            case FilterKind::MORPH: cpu_morph_rows(src, dst, W, band_rows, C, f.morph_op, f.morph_rx, f.morph_ry, ys, ye, y0); break;
            case FilterKind::BILATERAL: cpu_bilateral_rows(src, dst, W, band_rows, C, f, ys, ye, y0); break;
            case FilterKind::CONV: cpu_conv_rows(src, dst, W, band_rows, C, f, ys, ye, y0); break;
            case FilterKind::SEP_DOWN: cpu_sep_down_rows(src, dst, W, band_rows, C, f, ys, ye); break;
            case FilterKind::RESIZE: cpu_resize_rows(src, dst, W, band_rows, C, f, ys, ye, xtab.data()); break;
            case FilterKind::WARP: cpu_warp_rows(src, dst, W, band_rows, C, f, ys, ye); break;
            case FilterKind::WARP_PERSP: cpu_warp_persp_rows(src, dst, W, band_rows, C, f, ys, ye); break;
            case FilterKind::REMAP: cpu_remap_rows(src, dst, W, band_rows, C, f, ys, ye); break;
            case FilterKind::AREA: cpu_area_rows(src, dst, W, band_rows, C, f, ys, ye, area_x.data(), area_y.data()); break;
            case FilterKind::COLOR: cpu_color_rows(src, dst, W, C, f, ys, ye); break;
            }
        }
    };
    const int nt = (int)std::min<long long>(n_threads, items);
    Pool::get().run(nt, [&](int) { worker(); });
}

// The histogram family works on the flat run of an image's W * H pixels: items are (image, slice of pixels), at least
// 4096 pixels a slice and about four items per thread.
namespace {
template <typename F>
void for_pixel_slices(size_t pixels, int n_images, int n_threads, F &&body)
{
    if (n_threads <= 0) n_threads = hardware_threads();
    int slices = 1;
    if (n_images < 4 * n_threads)
        slices = (int)std::max<size_t>(1, std::min<size_t>(pixels / 4096, (size_t)(4 * n_threads + n_images - 1) / (size_t)n_images));
    const long long items = (long long)n_images * slices;
    std::atomic<long long> next{0};
    Pool::get().run((int)std::min<long long>(n_threads, items), [&](int) {
        for (;;) {
            const long long it = next.fetch_add(1, std::memory_order_relaxed);
            if (it >= items) break;
            const int img = (int)(it / slices), s = (int)(it % slices);
            body(img, pixels * (size_t)s / (size_t)slices, pixels * (size_t)(s + 1) / (size_t)slices);
        }
    });
}
}  // namespace

// hist[i][c][v] = the pixels of image i whose channel c holds v: every slice counts on its own and adds its non-zero
// counters to the image's with atomic adds (integer adds commute: the result does not depend on the threads).
void cpu_hist(const uint8_t *in, uint32_t *hist, int W, int H, int C, int n_images, int n_threads)
{
    if (n_images <= 0) return;
    const size_t pixels = (size_t)W * H;
    memset(hist, 0, (size_t)n_images * C * MI_BLUR_HIST_BINS * sizeof(uint32_t));
    for_pixel_slices(pixels, n_images, n_threads, [&](int img, size_t p0, size_t p1) {
        uint32_t local[MI_BLUR_COLOR_MAX_CHANNELS * MI_BLUR_HIST_BINS] = {};
        const uint8_t *px = in + ((size_t)img * pixels + p0) * C;
        for (size_t n = p1 - p0; n > 0; n--, px += C)
            for (int c = 0; c < C; c++) local[c * MI_BLUR_HIST_BINS + px[c]]++;
        uint32_t *dst = hist + (size_t)img * C * MI_BLUR_HIST_BINS;
        for (int i = 0; i < C * MI_BLUR_HIST_BINS; i++)
            if (local[i]) __atomic_fetch_add(dst + i, local[i], __ATOMIC_RELAXED);
    });
}

// out[i][p][c] = tables[i][c][in[i][p][c]].
void cpu_tables(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const uint8_t *tables, int n_threads)
{
    if (n_images <= 0) return;
    const size_t pixels = (size_t)W * H;
    for_pixel_slices(pixels, n_images, n_threads, [&](int img, size_t p0, size_t p1) {
        const uint8_t *tab = tables + (size_t)img * C * MI_BLUR_HIST_BINS;
        const uint8_t *px = in + ((size_t)img * pixels + p0) * C;
        uint8_t *o = out + ((size_t)img * pixels + p0) * C;
        for (size_t n = p1 - p0; n > 0; n--, px += C, o += C)
            for (int c = 0; c < C; c++) o[c] = tab[c * MI_BLUR_HIST_BINS + px[c]];
    });
}

// Histogram -> tables (tone_tables(), filter.h) -> look-up; work = the histograms, then the tables.
void cpu_tone(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_tone &t, void *work, int n_threads)
{
    if (n_images <= 0) return;
    uint32_t *hist = static_cast<uint32_t *>(work);
    uint8_t *tables = reinterpret_cast<uint8_t *>(hist + (size_t)n_images * C * MI_BLUR_HIST_BINS);
    cpu_hist(in, hist, W, H, C, n_images, n_threads);
    for (int i = 0; i < n_images; i++)
        tone_tables(t, hist + (size_t)i * C * MI_BLUR_HIST_BINS, C, tables + (size_t)i * C * MI_BLUR_HIST_BINS);
    cpu_tables(in, out, W, H, C, n_images, tables, n_threads);
}

// out[i][p][c] = arith_byte(a, b, m) of the operands' bytes; a plane operand has one byte per pixel, a shared one a
// single image.  Slices of pixels as above; the operation is a constant inside each loop.
namespace {
template <int OP>
void arith_slices(const uint8_t *a, const uint8_t *b, const uint8_t *m, uint8_t *out, size_t pixels, int C, int n_images, const mi_blur_arith &k, int n_threads)
{
    const size_t bc = k.b_plane ? 1 : (size_t)C, mc = k.m_plane ? 1 : (size_t)C;
    for_pixel_slices(pixels, n_images, n_threads, [&](int img, size_t p0, size_t p1) {
        const uint8_t *pa = a + ((size_t)img * pixels + p0) * C;
        const uint8_t *pb = b + ((k.b_shared ? 0 : (size_t)img * pixels) + p0) * bc;
        const uint8_t *pm = OP == MI_BLUR_ARITH_LERP ? m + ((k.m_shared ? 0 : (size_t)img * pixels) + p0) * mc : nullptr;
        uint8_t *o = out + ((size_t)img * pixels + p0) * C;
        for (size_t n = p1 - p0; n > 0; n--, pa += C, pb += bc, o += C) {
            for (int c = 0; c < C; c++) {
                const int vm = OP == MI_BLUR_ARITH_LERP ? pm[k.m_plane ? 0 : c] : 0;
                o[c] = (uint8_t)arith_byte(OP, k.wa, k.wb, k.bias, k.shift, pa[c], pb[k.b_plane ? 0 : c], vm);
            }
            if (OP == MI_BLUR_ARITH_LERP) pm += mc;
        }
    });
}
}  // namespace

void cpu_arith(const uint8_t *a, const uint8_t *b, const uint8_t *m, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_arith &k, int n_threads)
{
    if (n_images <= 0) return;
    const size_t pixels = (size_t)W * H;
    switch (k.op) {
    case MI_BLUR_ARITH_LINEAR: return arith_slices<MI_BLUR_ARITH_LINEAR>(a, b, m, out, pixels, C, n_images, k, n_threads);
    case MI_BLUR_ARITH_ABSDIFF: return arith_slices<MI_BLUR_ARITH_ABSDIFF>(a, b, m, out, pixels, C, n_images, k, n_threads);
    case MI_BLUR_ARITH_MIN: return arith_slices<MI_BLUR_ARITH_MIN>(a, b, m, out, pixels, C, n_images, k, n_threads);
    case MI_BLUR_ARITH_MAX: return arith_slices<MI_BLUR_ARITH_MAX>(a, b, m, out, pixels, C, n_images, k, n_threads);
    case MI_BLUR_ARITH_MUL: return arith_slices<MI_BLUR_ARITH_MUL>(a, b, m, out, pixels, C, n_images, k, n_threads);
    default: return arith_slices<MI_BLUR_ARITH_LERP>(a, b, m, out, pixels, C, n_images, k, n_threads);
    }
}

// Integral images: items are (image, band of rows), about four per thread and at least 16 rows a band.
namespace {
template <typename F>
void for_items(long long items, int n_threads, F &&body)
{
    std::atomic<long long> next{0};
    Pool::get().run((int)std::min<long long>(n_threads, items), [&](int) {
        for (;;) {
            const long long it = next.fetch_add(1, std::memory_order_relaxed);
            if (it >= items) break;
            body(it);
        }
    });
}
}  // namespace

// CLAHE.  Items (for_items() above) are (image, tile) for the tables and (image, band of 16 rows) for the look-up.
// A tile's histogram by a walk over its rows, then clahe_table() (filter.h) per transformed channel.
void cpu_clahe_tables(const uint8_t *in, uint32_t *hist, uint8_t *tables, int W, int H, int C, int n_images, const mi_blur_clahe &k, int n_threads)
{
    if (n_images <= 0) return;
    if (n_threads <= 0) n_threads = hardware_threads();
    const int TX = k.tiles_x, TY = k.tiles_y, mask = tone_mask(k.channel_mask, C);
    for_items((long long)n_images * TY * TX, n_threads, [&](long long job) {
        const int img = (int)(job / (TY * TX)), tile = (int)(job % (TY * TX)), ty = tile / TX, tx = tile % TX;
        const int x0 = clahe_edge(W, TX, tx), x1 = clahe_edge(W, TX, tx + 1), y0 = clahe_edge(H, TY, ty), y1 = clahe_edge(H, TY, ty + 1);
        uint32_t *h = hist + (size_t)job * C * MI_BLUR_HIST_BINS;
        uint8_t *lut = tables + (size_t)job * C * MI_BLUR_HIST_BINS;
        memset(h, 0, (size_t)C * MI_BLUR_HIST_BINS * sizeof(uint32_t));
        for (int y = y0; y < y1; y++) {
            const uint8_t *px = in + (((size_t)img * H + y) * W + x0) * C;
            for (int x = x0; x < x1; x++, px += C)
                for (int c = 0; c < C; c++) h[c * MI_BLUR_HIST_BINS + px[c]]++;
        }
        const uint32_t A = (uint32_t)(x1 - x0) * (uint32_t)(y1 - y0);
        for (int c = 0; c < C; c++) {
            if ((mask >> c) & 1) clahe_table(h + c * MI_BLUR_HIST_BINS, A, k.clip_q8, lut + c * MI_BLUR_HIST_BINS);
            else for (int v = 0; v < MI_BLUR_HIST_BINS; v++) lut[c * MI_BLUR_HIST_BINS + v] = (uint8_t)v;
        }
    });
}

// out = bilinear_blend() of the four tables' bytes; the columns' (t0, t1, frac) are worked out once.
void cpu_clahe_apply(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_clahe &k, const uint8_t *tables, int n_threads)
{
    if (n_images <= 0) return;
    if (n_threads <= 0) n_threads = hardware_threads();
    const int TX = k.tiles_x, TY = k.tiles_y, BAND = 16, bands = (H + BAND - 1) / BAND;
    struct Col { int t0, t1, f; };
    std::vector<Col> cols((size_t)W);
    for (int x = 0; x < W; x++) clahe_axis(W, TX, x, cols[x].t0, cols[x].t1, cols[x].f);
    const size_t tile = (size_t)C * MI_BLUR_HIST_BINS;
    for_items((long long)n_images * bands, n_threads, [&](long long it) {
        const int img = (int)(it / bands), band = (int)(it % bands);
        const uint8_t *tab = tables + (size_t)img * TY * TX * tile;
        for (int y = band * BAND; y < std::min(H, (band + 1) * BAND); y++) {
            int ty0, ty1, fy;
            clahe_axis(H, TY, y, ty0, ty1, fy);
            const uint8_t *r0 = tab + (size_t)ty0 * TX * tile, *r1 = tab + (size_t)ty1 * TX * tile;
            const uint8_t *px = in + ((size_t)img * H + y) * W * C;
            uint8_t *o = out + ((size_t)img * H + y) * W * C;
            for (int x = 0; x < W; x++, px += C, o += C) {
                const size_t a = cols[x].t0 * tile, b = cols[x].t1 * tile;
                for (int c = 0; c < C; c++) {
                    const size_t e = (size_t)c * MI_BLUR_HIST_BINS + px[c];
                    o[c] = (uint8_t)bilinear_blend(r0[a + e], r0[b + e], r1[a + e], r1[b + e], (unsigned)cols[x].f, (unsigned)fy);
                }
            }
        }
    });
}

void cpu_clahe(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_clahe &k, void *work, int n_threads)
{
    if (n_images <= 0) return;
    uint32_t *hist = static_cast<uint32_t *>(work);
    uint8_t *tables = reinterpret_cast<uint8_t *>(hist + clahe_tables_of(n_images, k, C) * MI_BLUR_HIST_BINS);
    cpu_clahe_tables(in, hist, tables, W, H, C, n_images, k, n_threads);
    cpu_clahe_apply(in, out, W, H, C, n_images, k, tables, n_threads);
}

bool cpu_integral(const uint8_t *in, uint32_t *sum, uint32_t *sqsum, int W, int H, int C, int n_images, int n_threads)
{
    if (n_images <= 0) return true;
    if (n_threads <= 0) n_threads = hardware_threads();
    const size_t row_e = (size_t)W * C;
    const int want = std::max(1, std::min(std::max(1, H / 16), (4 * n_threads + n_images - 1) / n_images));
    const int band = (H + want - 1) / want, nb = (H + band - 1) / band;
    uint32_t *const tab[2] = {sum ? sum : sqsum, sum ? sqsum : nullptr};
    const bool squares[2] = {!sum, true};
    const int nt = tab[1] ? 2 : 1;
    // carry[image][band][table][W * C]: first the column sums of the band, then S (or Q) of the row above the band
    std::vector<uint32_t> carry;
    try { carry.assign((size_t)n_images * nb * nt * row_e, 0u); } catch (...) { return false; }
    const long long items = (long long)n_images * nb;
    for_items(items, n_threads, [&](long long it) {
        const int img = (int)(it / nb), b = (int)(it % nb);
        if (b == nb - 1) return;                                            // nothing lies below the last band
        uint32_t *c0 = carry.data() + (size_t)it * nt * row_e;
        const uint8_t *src = in + ((size_t)img * H + (size_t)b * band) * row_e;
        for (int y = 0; y < band; y++, src += row_e)
            for (int k = 0; k < nt; k++) {
                uint32_t *c = c0 + k * row_e;
                if (squares[k]) for (size_t e = 0; e < row_e; e++) c[e] += (uint32_t)src[e] * src[e];
                else for (size_t e = 0; e < row_e; e++) c[e] += src[e];
            }
    });
    // the exclusive prefix over an image's bands, then along the row: the table's row above each band
    for_items((long long)n_images * nt, n_threads, [&](long long it) {
        const int img = (int)(it / nt), k = (int)(it % nt);
        std::vector<uint32_t> run(row_e, 0u);
        for (int b = 0; b < nb; b++) {
            uint32_t *c = carry.data() + (((size_t)img * nb + b) * nt + k) * row_e;
            uint32_t along[MI_BLUR_COLOR_MAX_CHANNELS] = {0, 0, 0, 0};
            for (size_t e = 0; e < row_e; e++) {
                const uint32_t below = c[e];
                along[e % C] += run[e];
                c[e] = along[e % C];
                run[e] += below;
            }
        }
    });
    for_items(items, n_threads, [&](long long it) {
        const int img = (int)(it / nb), b = (int)(it % nb);
        const int y0 = b * band, y1 = std::min(H, y0 + band);
        const uint8_t *src = in + ((size_t)img * H + y0) * row_e;
        for (int k = 0; k < nt; k++) {
            uint32_t *above = carry.data() + ((size_t)it * nt + k) * row_e;
            uint32_t *dst = tab[k] + ((size_t)img * H + y0) * row_e;
            const uint8_t *s = src;
            for (int y = y0; y < y1; y++, s += row_e, dst += row_e) {
                uint32_t along[MI_BLUR_COLOR_MAX_CHANNELS] = {0, 0, 0, 0};
                for (size_t e = 0; e < row_e; e++) {
                    const uint32_t v = s[e];
                    along[e % C] += squares[k] ? v * v : v;
                    dst[e] = above[e] += along[e % C];
                }
            }
        }
    });
    return true;
}

void cpu_box_from_integral(const uint8_t *in, const uint32_t *sum, const uint32_t *sqsum, uint8_t *out, int W, int H, int C, int n_images,
                           const mi_blur_box &k, int n_threads)
{
    if (n_images <= 0) return;
    if (n_threads <= 0) n_threads = hardware_threads();
    const BoxConst bc = box_const(k);
    const size_t row_e = (size_t)W * C;
    for_items((long long)n_images * H, n_threads, [&](long long row) {
        const long long img = row / H;
        const int y = (int)(row - img * H);
        const uint32_t *S = sum + (size_t)img * H * row_e, *Q = k.op == MI_BLUR_BOX_STDDEV ? sqsum + (size_t)img * H * row_e : nullptr;
        const size_t at = (size_t)row * row_e;
        for (int x = 0; x < W; x++)
            for (int c = 0; c < C; c++) {
                const size_t e = at + (size_t)x * C + c;
                const uint32_t s = box_window(S, W, H, C, x, y, c, k.rx, k.ry), q = Q ? box_window(Q, W, H, C, x, y, c, k.rx, k.ry) : 0u;
                out[e] = (uint8_t)box_byte(k.op, k.offset, k.invert, bc.A, bc.inv_2a, bc.inv_a, s, q, k.op == MI_BLUR_BOX_THRESHOLD ? in[e] : 0);
            }
    });
}

// The distance transform.  The column pass: items are (image, strip of DIST_CPU_STRIP columns and channels), each walks
// its strip down the image and up again.  The row pass: items are (image, band of rows); a row is laid out as the tiled
// kernel lays it out in LDS, one padded plane per channel and the chunks' minima, and searched by the same dist_search().
namespace {
constexpr int DIST_CPU_STRIP = 256;
constexpr int DIST_CPU_CHUNK = 1 << DIST_CHUNK_LOG2;

template <int METRIC>
void dist_row(const uint16_t *plane, const uint16_t *cm, int nch, int W, int C, uint32_t start, const mi_blur_dist &k, uint32_t *table, uint8_t *out)
{
    const size_t wp = (size_t)nch * DIST_CPU_CHUNK;
    for (int c = 0; c < C; c++)
        for (int x = 0; x < W; x++) {
            const uint32_t T = dist_final(dist_search<METRIC, DIST_CPU_CHUNK>(plane + c * wp, cm + (size_t)c * nch, nch, x, start), start);
            if (table) table[(size_t)x * C + c] = T;
            else out[(size_t)x * C + c] = (uint8_t)dist_byte(k.metric, k.byte_op, k.invert, T);
        }
}
}  // namespace

bool cpu_dist(const uint8_t *in, uint32_t *table, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_dist &k, int n_threads)
{
    if (n_images <= 0) return true;
    if (n_threads <= 0) n_threads = hardware_threads();
    const size_t row_e = (size_t)W * C;
    std::vector<uint16_t> g;
    try { g.resize((size_t)n_images * H * row_e); } catch (...) { return false; }
    const uint32_t cap = dist_cap(k.limit);
    const long long strips = ((long long)row_e + DIST_CPU_STRIP - 1) / DIST_CPU_STRIP;
    for_items((long long)n_images * strips, n_threads, [&](long long it) {
        const long long img = it / strips;
        const size_t e0 = (size_t)(it - img * strips) * DIST_CPU_STRIP, e1 = std::min(row_e, e0 + DIST_CPU_STRIP);
        const uint8_t *src = in + (size_t)img * H * row_e;
        uint16_t *dst = g.data() + (size_t)img * H * row_e;
        uint32_t site[DIST_CPU_STRIP];
        for (size_t e = e0; e < e1; e++) site[e - e0] = DIST_G_NONE;
        for (int y = 0; y < H; y++)
            for (size_t e = e0; e < e1; e++) {
                uint32_t &s = site[e - e0];
                if ((src[(size_t)y * row_e + e] != 0) == (k.sites_nonzero != 0)) s = (uint32_t)y;
                dst[(size_t)y * row_e + e] = (uint16_t)(s == DIST_G_NONE ? DIST_G_NONE : (uint32_t)y - s);
            }
        for (size_t e = e0; e < e1; e++) site[e - e0] = DIST_G_NONE;
        for (int y = H - 1; y >= 0; y--)
            for (size_t e = e0; e < e1; e++) {
                uint32_t &s = site[e - e0];
                uint32_t d = dst[(size_t)y * row_e + e];
                if (d == 0) s = (uint32_t)y;
                const uint32_t up = s == DIST_G_NONE ? DIST_G_NONE : s - (uint32_t)y;
                d = up < d ? up : d;
                dst[(size_t)y * row_e + e] = (uint16_t)dist_g_cap(d, cap);
            }
    });
    const int want = std::max(1, std::min(std::max(1, H / 16), (4 * n_threads + n_images - 1) / n_images));
    const int band = (H + want - 1) / want, nb = (H + band - 1) / band;
    const int nch = dist_chunks(W, DIST_CPU_CHUNK);
    const size_t wp = (size_t)nch * DIST_CPU_CHUNK;
    const uint32_t start = dist_start(k.metric, k.limit);
    std::atomic<bool> ok{true};
    for_items((long long)n_images * nb, n_threads, [&](long long it) {
        const int img = (int)(it / nb), b = (int)(it % nb);
        std::vector<uint16_t> plane, cm;
        try { plane.assign((size_t)C * wp, (uint16_t)DIST_G_NONE); cm.resize((size_t)C * nch); } catch (...) { ok = false; return; }
        for (int y = b * band; y < std::min(H, (b + 1) * band); y++) {
            const size_t at = ((size_t)img * H + y) * row_e;
            const uint16_t *row = g.data() + at;
            for (int x = 0; x < W; x++)
                for (int c = 0; c < C; c++) plane[c * wp + x] = row[(size_t)x * C + c];
            for (size_t q = 0; q < (size_t)C * nch; q++) {
                uint32_t m = DIST_G_NONE;
                for (int j = 0; j < DIST_CPU_CHUNK; j++) m = std::min<uint32_t>(m, plane[q * DIST_CPU_CHUNK + j]);
                cm[q] = (uint16_t)m;
            }
            uint32_t *t = table ? table + at : nullptr;
            uint8_t *o = out ? out + at : nullptr;
            switch (k.metric) {
            case MI_BLUR_DIST_L2: dist_row<MI_BLUR_DIST_L2>(plane.data(), cm.data(), nch, W, C, start, k, t, o); break;
            case MI_BLUR_DIST_L1: dist_row<MI_BLUR_DIST_L1>(plane.data(), cm.data(), nch, W, C, start, k, t, o); break;
            default: dist_row<MI_BLUR_DIST_LINF>(plane.data(), cm.data(), nch, W, C, start, k, t, o); break;
            }
        }
    });
    return ok;
}

// Synthetic stream: image i = LCG bytes, seed 0x9E3779B9 ^ i.
void fill_synthetic(uint8_t *host, int W, int H, int C, int first_index, int n_images, int n_threads)
{
    if (n_images <= 0) return;
    if (n_threads <= 0) n_threads = hardware_threads();
    const size_t isz = (size_t)W * H * C;
    std::atomic<int> next{0};
    auto worker = [&]() {
        for (;;) {
            const int i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= n_images) break;
            uint32_t s = 0x9E3779B9u ^ (uint32_t)(first_index + i);
            uint8_t *p = host + (size_t)i * isz;
            for (size_t k = 0; k < isz; k++) {
                s = s * 1664525u + 1013904223u;
                p[k] = (uint8_t)(s >> 24);
            }
        }
    };
    Pool::get().run(std::min(n_threads, n_images), [&](int) { worker(); });
}

// n blocks of `bytes` bytes from src (stride src_stride) to dst (stride dst_stride), split over a few pool threads when
// there is enough to move: the staging copies of a GPU context fed from pageable caller memory.
void copy_blocks(uint8_t *dst, size_t dst_stride, const uint8_t *src, size_t src_stride, size_t bytes, int n, int n_threads)
{
    const size_t total = bytes * (size_t)n;
    if (n_threads <= 1 || total < (1u << 20)) {
        for (int i = 0; i < n; i++) memcpy(dst + (size_t)i * dst_stride, src + (size_t)i * src_stride, bytes);
        return;
    }
    // cut every block into n_threads slices so the split is even whatever n is
    Pool::get().run(n_threads, [&](int t) {
        const size_t b = bytes * (size_t)t / (size_t)n_threads, e = bytes * (size_t)(t + 1) / (size_t)n_threads;
        for (int i = 0; i < n; i++) memcpy(dst + (size_t)i * dst_stride + b, src + (size_t)i * src_stride + b, e - b);
    });
}

// The reference's host loops (heterogeneous_blur.c:125-134 in, split_image_blur.c:40-56 out), over images on pool threads.
void cpu_repack(const uint8_t *src, uint8_t *dst, int W, int H, int C, int n_images, bool p2i, int n_threads)
{
    if (n_images <= 0) return;
    if (n_threads <= 0) n_threads = hardware_threads();
    const size_t plane = (size_t)W * H, isz = plane * C;
    std::atomic<int> next{0};
    Pool::get().run(std::min(n_threads, n_images), [&](int) {
        for (;;) {
            const int i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= n_images) break;
            const uint8_t *s = src + (size_t)i * isz;
            uint8_t *d = dst + (size_t)i * isz;
            for (int c = 0; c < C; c++)
                for (size_t px = 0; px < plane; px++) {
                    if (p2i) d[px * C + c] = s[(size_t)c * plane + px];
                    else d[(size_t)c * plane + px] = s[px * C + c];
                }
        }
    });
}

// ---- template matching and the peak search (include/mi_blur.h, "Template matching and peak search")
void cpu_match(const uint8_t *in, const uint8_t *t, void *out, int W, int H, int C, int n_images, const mi_blur_match &k, int n_threads)
{
    if (n_images <= 0) return;
    if (n_threads <= 0) n_threads = hardware_threads();
    const int Wo = W - k.tw + 1, Ho = H - k.th + 1, tb = k.tw * C;
    const size_t row_e = (size_t)W * C;
    const uint32_t A = (uint32_t)(k.tw * k.th * C);
    for_items((long long)n_images * Ho, n_threads, [&](long long it) {
        const long long img = it / Ho;
        const int y = (int)(it - img * Ho);
        const uint8_t *T = t + (k.t_shared ? 0 : (size_t)img * k.th * tb);
        uint32_t sum_t = 0, sum_tt = 0;
        for (int i = 0; i < k.th * tb; i++) { sum_t += T[i]; sum_tt += (uint32_t)T[i] * T[i]; }
        uint32_t *dst = static_cast<uint32_t *>(out) + ((size_t)img * Ho + y) * Wo;
        for (int x = 0; x < Wo; x++) {
            const uint8_t *a = in + ((size_t)img * H + y) * row_e + (size_t)x * C;
            const uint8_t *tr = T;
            uint32_t at = 0, sq = 0, sad = 0, sa = 0, saa = 0;
            for (int dy = 0; dy < k.th; dy++, a += row_e, tr += tb)
                for (int b = 0; b < tb; b++) {
                    const int av = a[b], tv = tr[b], d = av - tv;
                    at += (uint32_t)(av * tv);
                    sq += (uint32_t)(d * d);
                    sad += (uint32_t)(d < 0 ? -d : d);
                    sa += (uint32_t)av;
                    saa += (uint32_t)(av * av);
                }
            switch (k.method) {
            case MI_BLUR_MATCH_SQDIFF: dst[x] = sq; break;
            case MI_BLUR_MATCH_CCORR: dst[x] = at; break;
            case MI_BLUR_MATCH_SAD: dst[x] = sad; break;
            default: dst[x] = (uint32_t)match_score(k.method, A, at, sa, saa, sum_t, sum_tt); break;
            }
        }
    });
}

void cpu_match_peak(const void *table, int is_signed, int Wo, int Ho, int n_images, int64_t *peaks, int n_threads)
{
    if (n_images <= 0) return;
    if (n_threads <= 0) n_threads = hardware_threads();
    const size_t entries = (size_t)Wo * Ho;
    for_items(n_images, n_threads, [&](long long img) {
        const uint32_t *src = static_cast<const uint32_t *>(table) + (size_t)img * entries;
        const auto value = [&](size_t i) { return is_signed ? (int64_t)(int32_t)src[i] : (int64_t)src[i]; };
        size_t lo = 0, hi = 0;
        for (size_t i = 1; i < entries; i++) {                          // strict comparisons: the first entry keeps a tie
            if (value(i) < value(lo)) lo = i;
            if (value(i) > value(hi)) hi = i;
        }
        int64_t *o = peaks + 6 * (size_t)img;
        o[0] = value(lo); o[1] = (int64_t)(lo % (size_t)Wo); o[2] = (int64_t)(lo / (size_t)Wo);
        o[3] = value(hi); o[4] = (int64_t)(hi % (size_t)Wo); o[5] = (int64_t)(hi / (size_t)Wo);
    });
}

uint64_t fnv1a64(const uint8_t *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

}  // namespace mi_blur
