// table_api.cpp — the part of the C ABI declared in include/mi_blur.h that is not a FilterKind and goes through no
// context: histogram and tone tables, CLAHE, two-image arithmetic, integral images and box filters, the distance
// transform (none has a reference analogue).  Their results are tables, or they take a second image or a work buffer, so
// each family has its own launches (hist_, clahe_, arith_, integral_, dist_kernels.hip) and CPU loops (cpu_device.cpp).
//
// Every export answers in ONE order: all of its arguments (MI_BLUR_ERR_INVALID), then the empty batch (MI_BLUR_OK), then
// the device (MI_BLUR_ERR_NO_DEVICE).  go() is that order; an export is its argument predicate, go() and its launch.
// The blocking mi_blur_run_* forms hand MI_BLUR_DEVICE_CPU to their mi_blur_cpu_run_* first and keep their device memory
// in a DeviceCall.  The forms differ in the alignment they demand: 16 bytes for device tables and work buffers, 4 for host
// ones, 1 for byte outputs.
#include "api_internal.h"
#include "blur_launch.h"
#include "cpu_device.h"

#include <climits>
#include <cmath>
#include <vector>

using namespace mi_blur;

namespace {

// The order of every export: the arguments, the empty batch, a device.  An enqueue export takes any device; a blocking
// export makes the HIP device `device` current, so its empty batch is MI_BLUR_OK on an ordinal that does not exist too.
// GO, which is no status: there is something to launch.
constexpr int GO = 1, ANY_DEVICE = INT_MIN;
int go(bool args_ok, int n_images, int device = ANY_DEVICE)
{
    if (!args_ok) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const int ndev = mi_blur_device_count();
    if (ndev <= 0 || (device != ANY_DEVICE && (device < 0 || device >= ndev))) return MI_BLUR_ERR_NO_DEVICE;
    if (device != ANY_DEVICE) HIP_TRY(hipSetDevice(device));
    return GO;
}

// The device memory of one blocking export, freed when the export returns, whichever way.  The first failed step is
// `status` and every later step does nothing, so an export is a straight line that ends in `return dc.status`; its
// launch goes between put() and get() as `if (!dc.status) dc.status = launch_...`.  The copies are on the null stream:
// get() runs behind the kernels.
struct DeviceCall {
    void *bufs[4] = {};
    int n = 0, status = MI_BLUR_OK;
    ~DeviceCall() { for (int i = 0; i < n; i++) (void)hipFree(bufs[i]); }
    bool ok(hipError_t e)
    {
        if (e != hipSuccess) (void)hipGetLastError();                   // clears the runtime's sticky last error, as HIP_TRY does
        if (e != hipSuccess && !status) status = MI_BLUR_ERR_HIP_BASE - (int)e;
        return !status;
    }
    // A buffer of `bytes` bytes: an input before put(), an output or a work buffer.  nullptr for a buffer that is not
    // wanted (an optional table, the mask of an operation without one) and after a failure.
    template <typename T>
    T *make(size_t bytes, bool wanted = true)
    {
        void *p = nullptr;
        if (!wanted || status || !ok(hipMalloc(&p, bytes ? bytes : 1))) return nullptr;
        bufs[n++] = p;
        return static_cast<T *>(p);
    }
    void put(void *dev, const void *host, size_t bytes) { if (dev && !status) ok(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice)); }
    // To a host pointer that may be null: the caller did not ask for this buffer.
    void get(void *host, const void *dev, size_t bytes) { if (host && !status) ok(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost)); }
};

// The work buffer of a CPU export that takes an optional one: `work`, or `own` grown to `bytes` bytes (4-byte aligned).
// false: no memory.
bool work_or_own(void *&work, std::vector<uint32_t> &own, size_t bytes)
{
    if (work) return true;
    try { own.resize((bytes + 3) / 4); } catch (...) { return false; }
    work = own.data();
    return true;
}

size_t image_bytes(int W, int H, int C, int n_images) { return (size_t)n_images * W * H * C; }
bool aligned_or_null(const void *p, uintptr_t a) { return (uintptr_t)p % a == 0; }      // an optional work buffer
bool aligned_to(const void *p, uintptr_t a) { return p && aligned_or_null(p, a); }

}  // namespace

// ----------------------------------------------------------------------------------
// histogram, tone tables and per-image tables
// ----------------------------------------------------------------------------------
static bool hist_args_ok(const void *in, int W, int H, int C, int n_images) { return in && n_images >= 0 && hist_image_ok(W, H, C); }
static size_t hist_words(int C, int n_images) { return (size_t)n_images * (size_t)C * MI_BLUR_HIST_BINS; }
static bool tables_args_ok(const uint8_t *in, const uint8_t *out, int W, int H, int C, int n_images) { return out && in != out && hist_args_ok(in, W, H, C, n_images); }
static bool tone_args_ok(const uint8_t *in, const uint8_t *out, int W, int H, int C, int n_images, const mi_blur_tone *t)
{
    return tables_args_ok(in, out, W, H, C, n_images) && tone_ok(t, C);
}

extern "C" int mi_blur_enqueue_hist(const uint8_t *d_in, uint32_t *d_hist, int width, int height, int channels, int n_images, void *stream)
{
    if (const int st = go(hist_args_ok(d_in, width, height, channels, n_images) && aligned_to(d_hist, 16), n_images); st != GO) return st;
    return launch_hist(d_in, d_hist, width, height, channels, n_images, (hipStream_t)stream);
}

extern "C" int mi_blur_cpu_run_hist(const uint8_t *in, uint32_t *hist, int width, int height, int channels, int n_images, int n_threads)
{
    if (!hist_args_ok(in, width, height, channels, n_images) || !aligned_to(hist, 4)) return MI_BLUR_ERR_INVALID;
    cpu_hist(in, hist, width, height, channels, n_images, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_tone_tables(const uint32_t *hist, int channels, const mi_blur_tone *t, uint8_t *tables)
{
    if (!hist || !tables || !tone_ok(t, channels)) return MI_BLUR_ERR_INVALID;
    tone_tables(*t, hist, channels, tables);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_enqueue_tables(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                      const uint8_t *d_tables, void *stream)
{
    if (const int st = go(tables_args_ok(d_in, d_out, width, height, channels, n_images) && d_tables, n_images); st != GO) return st;
    return launch_tables(d_in, d_out, width, height, channels, n_images, d_tables, (hipStream_t)stream);
}

extern "C" size_t mi_blur_tone_work_bytes(int channels, int n_images)
{
    if (channels < 1 || channels > MI_BLUR_COLOR_MAX_CHANNELS || n_images < 0) return 0;
    return hist_words(channels, n_images) * (sizeof(uint32_t) + 1);
}

// The three dispatches of mi_blur_enqueue_tone on buffers that are known to be good.
static int enqueue_tone(const uint8_t *d_in, uint8_t *d_out, int W, int H, int C, int n_images, const mi_blur_tone &t, void *d_work, hipStream_t stream)
{
    uint32_t *hist = static_cast<uint32_t *>(d_work);
    uint8_t *tables = reinterpret_cast<uint8_t *>(hist + hist_words(C, n_images));
    if (const int rc = launch_hist(d_in, hist, W, H, C, n_images, stream)) return rc;
    if (const int rc = launch_tone_tables(hist, tables, C, n_images, t, stream)) return rc;
    return launch_tables(d_in, d_out, W, H, C, n_images, tables, stream);
}

extern "C" int mi_blur_enqueue_tone(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                    const mi_blur_tone *t, void *d_work, void *stream)
{
    if (const int st = go(tone_args_ok(d_in, d_out, width, height, channels, n_images, t) && aligned_to(d_work, 16), n_images); st != GO) return st;
    return enqueue_tone(d_in, d_out, width, height, channels, n_images, *t, d_work, (hipStream_t)stream);
}

extern "C" int mi_blur_cpu_run_tables(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                      const uint8_t *tables, int n_threads)
{
    if (!tables_args_ok(in, out, width, height, channels, n_images) || !tables) return MI_BLUR_ERR_INVALID;
    cpu_tables(in, out, width, height, channels, n_images, tables, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_cpu_run_tone(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                    const mi_blur_tone *t, void *work, int n_threads)
{
    if (!tone_args_ok(in, out, width, height, channels, n_images, t) || !aligned_or_null(work, 4)) return MI_BLUR_ERR_INVALID;
    std::vector<uint32_t> own;
    if (!work_or_own(work, own, mi_blur_tone_work_bytes(channels, n_images))) return MI_BLUR_ERR_NOMEM;
    cpu_tone(in, out, width, height, channels, n_images, *t, work, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_run_hist(int device, const uint8_t *host_in, uint32_t *host_hist, int width, int height, int channels, int n_images)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_hist(host_in, host_hist, width, height, channels, n_images, 0);
    if (const int st = go(hist_args_ok(host_in, width, height, channels, n_images) && aligned_to(host_hist, 4), n_images, device); st != GO) return st;
    const size_t in_bytes = image_bytes(width, height, channels, n_images), hist_bytes = hist_words(channels, n_images) * sizeof(uint32_t);
    DeviceCall dc;
    uint8_t *in = dc.make<uint8_t>(in_bytes);
    uint32_t *hist = dc.make<uint32_t>(hist_bytes);
    dc.put(in, host_in, in_bytes);
    if (!dc.status) dc.status = launch_hist(in, hist, width, height, channels, n_images, nullptr);
    dc.get(host_hist, hist, hist_bytes);
    return dc.status;
}

extern "C" int mi_blur_run_tone(int device, const uint8_t *host_in, uint8_t *host_out, void *host_work, int width, int height,
                                int channels, int n_images, const mi_blur_tone *t)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_tone(host_in, host_out, width, height, channels, n_images, t, host_work, 0);
    if (const int st = go(tone_args_ok(host_in, host_out, width, height, channels, n_images, t) && aligned_or_null(host_work, 4), n_images, device); st != GO) return st;
    const size_t bytes = image_bytes(width, height, channels, n_images), work_bytes = mi_blur_tone_work_bytes(channels, n_images);
    DeviceCall dc;
    uint8_t *in = dc.make<uint8_t>(bytes), *out = dc.make<uint8_t>(bytes);
    void *work = dc.make<void>(work_bytes);
    dc.put(in, host_in, bytes);
    if (!dc.status) dc.status = enqueue_tone(in, out, width, height, channels, n_images, *t, work, nullptr);
    dc.get(host_out, out, bytes);
    dc.get(host_work, work, work_bytes);
    return dc.status;
}

// ----------------------------------------------------------------------------------
// CLAHE
// ----------------------------------------------------------------------------------
static bool clahe_args_ok(const uint8_t *in, int W, int H, int C, int n_images, const mi_blur_clahe *k)
{
    return hist_args_ok(in, W, H, C, n_images) && clahe_ok(k, W, H, C);
}
// ... of the forms that write an image too.
static bool clahe_out_args_ok(const uint8_t *in, const uint8_t *out, int W, int H, int C, int n_images, const mi_blur_clahe *k)
{
    return clahe_args_ok(in, W, H, C, n_images, k) && out && in != out;
}
// The tables of a work buffer, behind its histograms.
static uint8_t *clahe_work_tables(void *work, int C, int n_images, const mi_blur_clahe &k)
{
    return reinterpret_cast<uint8_t *>(static_cast<uint32_t *>(work) + clahe_tables_of(n_images, k, C) * MI_BLUR_HIST_BINS);
}

extern "C" int mi_blur_clahe_coord(int size, int tiles, int x, int *t0, int *t1, int *frac)
{
    if (!t0 || !t1 || !frac || size < 1 || size > MI_BLUR_RESIZE_MAX_DIM || tiles < 1 || tiles > MI_BLUR_CLAHE_MAX_TILES || tiles > size ||
        x < 0 || x >= size)
        return MI_BLUR_ERR_INVALID;
    clahe_axis(size, tiles, x, *t0, *t1, *frac);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_clahe_table(const uint32_t hist[256], uint32_t area, int clip_q8, uint8_t lut[256])
{
    if (!hist || !lut || clip_q8 < 0 || clip_q8 > 65536 || area == 0) return MI_BLUR_ERR_INVALID;
    uint64_t sum = 0;
    for (int v = 0; v < MI_BLUR_HIST_BINS; v++) sum += hist[v];
    if (sum != area) return MI_BLUR_ERR_INVALID;
    clahe_table(hist, area, clip_q8, lut);
    return MI_BLUR_OK;
}

extern "C" size_t mi_blur_clahe_work_bytes(int width, int height, int channels, int n_images, const mi_blur_clahe *k)
{
    if (!hist_image_ok(width, height, channels) || n_images < 0 || !clahe_ok(k, width, height, channels)) return 0;
    return clahe_tables_of(n_images, *k, channels) * MI_BLUR_HIST_BINS * (sizeof(uint32_t) + 1);
}

extern "C" int mi_blur_enqueue_clahe_tables(const uint8_t *d_in, int width, int height, int channels, int n_images,
                                            const mi_blur_clahe *k, void *d_work, void *stream)
{
    if (const int st = go(clahe_args_ok(d_in, width, height, channels, n_images, k) && aligned_to(d_work, 16), n_images); st != GO) return st;
    return launch_clahe_tables(d_in, static_cast<uint32_t *>(d_work), clahe_work_tables(d_work, channels, n_images, *k), width, height, channels,
                               n_images, *k, (hipStream_t)stream);
}

extern "C" int mi_blur_enqueue_clahe_apply(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                           const mi_blur_clahe *k, const uint8_t *d_tables, void *stream)
{
    if (const int st = go(clahe_out_args_ok(d_in, d_out, width, height, channels, n_images, k) && d_tables, n_images); st != GO) return st;
    return launch_clahe_apply(d_in, d_out, width, height, channels, n_images, *k, d_tables, (hipStream_t)stream);
}

// The two dispatches of mi_blur_enqueue_clahe on buffers that are known to be good.
static int enqueue_clahe(const uint8_t *d_in, uint8_t *d_out, int W, int H, int C, int n_images, const mi_blur_clahe &k, void *d_work, hipStream_t stream)
{
    uint8_t *tables = clahe_work_tables(d_work, C, n_images, k);
    if (const int rc = launch_clahe_tables(d_in, static_cast<uint32_t *>(d_work), tables, W, H, C, n_images, k, stream)) return rc;
    return launch_clahe_apply(d_in, d_out, W, H, C, n_images, k, tables, stream);
}

extern "C" int mi_blur_enqueue_clahe(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                     const mi_blur_clahe *k, void *d_work, void *stream)
{
    if (const int st = go(clahe_out_args_ok(d_in, d_out, width, height, channels, n_images, k) && aligned_to(d_work, 16), n_images); st != GO) return st;
    return enqueue_clahe(d_in, d_out, width, height, channels, n_images, *k, d_work, (hipStream_t)stream);
}

extern "C" int mi_blur_cpu_run_clahe_tables(const uint8_t *in, int width, int height, int channels, int n_images,
                                            const mi_blur_clahe *k, void *work, int n_threads)
{
    if (!clahe_args_ok(in, width, height, channels, n_images, k) || !aligned_to(work, 4)) return MI_BLUR_ERR_INVALID;
    cpu_clahe_tables(in, static_cast<uint32_t *>(work), clahe_work_tables(work, channels, n_images, *k), width, height, channels, n_images, *k,
                     n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_cpu_run_clahe_apply(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                           const mi_blur_clahe *k, const uint8_t *tables, int n_threads)
{
    if (!clahe_out_args_ok(in, out, width, height, channels, n_images, k) || !tables) return MI_BLUR_ERR_INVALID;
    cpu_clahe_apply(in, out, width, height, channels, n_images, *k, tables, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_cpu_run_clahe(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                     const mi_blur_clahe *k, void *work, int n_threads)
{
    if (!clahe_out_args_ok(in, out, width, height, channels, n_images, k) || !aligned_or_null(work, 4)) return MI_BLUR_ERR_INVALID;
    std::vector<uint32_t> own;
    if (!work_or_own(work, own, mi_blur_clahe_work_bytes(width, height, channels, n_images, k))) return MI_BLUR_ERR_NOMEM;
    cpu_clahe(in, out, width, height, channels, n_images, *k, work, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_run_clahe(int device, const uint8_t *host_in, uint8_t *host_out, void *host_work, int width, int height,
                                 int channels, int n_images, const mi_blur_clahe *k)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_clahe(host_in, host_out, width, height, channels, n_images, k, host_work, 0);
    if (const int st = go(clahe_out_args_ok(host_in, host_out, width, height, channels, n_images, k) && aligned_or_null(host_work, 4), n_images, device); st != GO)
        return st;
    const size_t bytes = image_bytes(width, height, channels, n_images), work_bytes = mi_blur_clahe_work_bytes(width, height, channels, n_images, k);
    DeviceCall dc;
    uint8_t *in = dc.make<uint8_t>(bytes), *out = dc.make<uint8_t>(bytes);
    void *work = dc.make<void>(work_bytes);
    dc.put(in, host_in, bytes);
    if (!dc.status) dc.status = enqueue_clahe(in, out, width, height, channels, n_images, *k, work, nullptr);
    dc.get(host_out, out, bytes);
    dc.get(host_work, work, work_bytes);
    return dc.status;
}

// ----------------------------------------------------------------------------------
// two-image arithmetic.  The arguments: arith_args_ok() (filter.h).
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_arith_preset(int preset, mi_blur_arith *k)
{
    static const struct { int op; int32_t wa, wb, bias; int shift; } PRESETS[] = {
        {MI_BLUR_ARITH_LINEAR, 1, 1, 0, 0},   {MI_BLUR_ARITH_LINEAR, 1, -1, 0, 0}, {MI_BLUR_ARITH_LINEAR, 1, 1, 1, 1},
        {MI_BLUR_ARITH_LINEAR, 1, -1, 128, 0}, {MI_BLUR_ARITH_ABSDIFF, 1, 0, 0, 0}, {MI_BLUR_ARITH_MIN, 0, 0, 0, 0},
        {MI_BLUR_ARITH_MAX, 0, 0, 0, 0},      {MI_BLUR_ARITH_MUL, 257, 0, 32896, 16}, {MI_BLUR_ARITH_MUL, 1, 0, 64, 7},
        {MI_BLUR_ARITH_LERP, 0, 0, 0, 0}};
    if (!k || preset < 0 || preset > MI_BLUR_ARITH_PRESET_LERP) return MI_BLUR_ERR_INVALID;
    *k = mi_blur_arith{PRESETS[preset].op, PRESETS[preset].wa, PRESETS[preset].wb, PRESETS[preset].bias, PRESETS[preset].shift, 0, 0, 0, 0};
    return MI_BLUR_OK;
}

extern "C" int mi_blur_arith_weighted(double alpha, double beta, double gamma, mi_blur_arith *k)
{
    if (!k || !std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(gamma)) return MI_BLUR_ERR_INVALID;
    if (std::fabs(alpha) > 16.0 || std::fabs(beta) > 16.0 || std::fabs(gamma) > 8192.0) return MI_BLUR_ERR_INVALID;
    const auto q12 = [](double v) { return (int32_t)std::floor(v * 4096.0 + 0.5); };
    *k = mi_blur_arith{MI_BLUR_ARITH_LINEAR, q12(alpha), q12(beta), q12(gamma) + 2048, 12, 0, 0, 0, 0};
    return MI_BLUR_OK;
}

extern "C" int mi_blur_arith_value(const mi_blur_arith *k, int a, int b, int m)
{
    if (!arith_ok(k) || a < 0 || a > 255 || b < 0 || b > 255) return -1;
    if (k->op != MI_BLUR_ARITH_LERP) m = 0;
    if (m < 0 || m > 255) return -1;
    return arith_byte(k->op, k->wa, k->wb, k->bias, k->shift, a, b, m);
}

extern "C" int mi_blur_enqueue_arith(const uint8_t *d_a, const uint8_t *d_b, const uint8_t *d_m, uint8_t *d_out, int width, int height,
                                     int channels, int n_images, const mi_blur_arith *k, void *stream)
{
    if (const int st = go(arith_args_ok(d_a, d_b, d_m, d_out, width, height, channels, n_images, k), n_images); st != GO) return st;
    return launch_arith(d_a, d_b, d_m, d_out, width, height, channels, n_images, *k, (hipStream_t)stream);
}

extern "C" int mi_blur_cpu_run_arith(const uint8_t *a, const uint8_t *b, const uint8_t *m, uint8_t *out, int width, int height, int channels,
                                     int n_images, const mi_blur_arith *k, int n_threads)
{
    if (!arith_args_ok(a, b, m, out, width, height, channels, n_images, k)) return MI_BLUR_ERR_INVALID;
    cpu_arith(a, b, m, out, width, height, channels, n_images, *k, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_run_arith(int device, const uint8_t *host_a, const uint8_t *host_b, const uint8_t *host_m, uint8_t *host_out, int width,
                                 int height, int channels, int n_images, const mi_blur_arith *k)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_arith(host_a, host_b, host_m, host_out, width, height, channels, n_images, k, 0);
    if (const int st = go(arith_args_ok(host_a, host_b, host_m, host_out, width, height, channels, n_images, k), n_images, device); st != GO) return st;
    const size_t bytes = (size_t)arith_operand_bytes(width, height, channels, n_images, 0, 0);
    const size_t b_bytes = (size_t)arith_operand_bytes(width, height, channels, n_images, k->b_plane, k->b_shared);      // a shared operand: one image
    const size_t m_bytes = host_m ? (size_t)arith_operand_bytes(width, height, channels, n_images, k->m_plane, k->m_shared) : 0;
    DeviceCall dc;
    uint8_t *a = dc.make<uint8_t>(bytes), *b = dc.make<uint8_t>(b_bytes), *out = dc.make<uint8_t>(bytes);
    dc.put(a, host_a, bytes);
    dc.put(b, host_b, b_bytes);
    uint8_t *m = dc.make<uint8_t>(m_bytes, host_m != nullptr);           // only LERP has a mask
    dc.put(m, host_m, m_bytes);
    if (!dc.status) dc.status = launch_arith(a, b, m, out, width, height, channels, n_images, *k, nullptr);
    dc.get(host_out, out, bytes);
    return dc.status;
}

// ----------------------------------------------------------------------------------
// integral images and the box filters made from them.  The arguments: integral_args_ok(), box_from_args_ok(),
// box_args_ok() (filter.h).
// ----------------------------------------------------------------------------------
static size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
// Bytes of one table inside the work buffer of mi_blur_enqueue_box.
static size_t box_table_bytes(int W, int H, int C, int n_images) { return round16(integral_words(W, H, C, n_images) * sizeof(uint32_t)); }

extern "C" int mi_blur_box_value(const mi_blur_box *k, int A, uint32_t sum, uint32_t sqsum, int a)
{
    if (!box_ok(k) || A != (2 * k->rx + 1) * (2 * k->ry + 1) || sum > 255u * (uint32_t)A) return -1;
    if (k->op == MI_BLUR_BOX_STDDEV) {
        if ((uint64_t)sqsum > 65025ull * (uint64_t)A || (uint64_t)sum * sum > (uint64_t)A * sqsum) return -1;
    } else {
        sqsum = 0;
    }
    if (k->op != MI_BLUR_BOX_THRESHOLD) a = 0;
    if (a < 0 || a > 255) return -1;
    const BoxConst bc = box_const(*k);
    return box_byte(k->op, k->offset, k->invert, bc.A, bc.inv_2a, bc.inv_a, sum, sqsum, a);
}

extern "C" size_t mi_blur_integral_work_bytes(int width, int height, int channels, int n_images, int both)
{
    if (!hist_image_ok(width, height, channels) || n_images < 0) return 0;
    return integral_work_bytes(width, height, channels, n_images, both ? 2 : 1, tunables().integral_band);
}

extern "C" int mi_blur_enqueue_integral(const uint8_t *d_in, uint32_t *d_sum, uint32_t *d_sqsum, int width, int height, int channels, int n_images,
                                        void *d_work, void *stream)
{
    if (const int st = go(integral_args_ok(d_in, d_sum, d_sqsum, width, height, channels, n_images, 16) && aligned_to(d_work, 16), n_images); st != GO) return st;
    return launch_integral(d_in, d_sum, d_sqsum, width, height, channels, n_images, d_work, (hipStream_t)stream);
}

extern "C" int mi_blur_cpu_run_integral(const uint8_t *in, uint32_t *sum, uint32_t *sqsum, int width, int height, int channels, int n_images, int n_threads)
{
    if (!integral_args_ok(in, sum, sqsum, width, height, channels, n_images, 4)) return MI_BLUR_ERR_INVALID;
    return cpu_integral(in, sum, sqsum, width, height, channels, n_images, n_threads) ? MI_BLUR_OK : MI_BLUR_ERR_NOMEM;
}

extern "C" int mi_blur_enqueue_box_from_integral(const uint8_t *d_in, const uint32_t *d_sum, const uint32_t *d_sqsum, uint8_t *d_out, int width,
                                                 int height, int channels, int n_images, const mi_blur_box *k, void *stream)
{
    if (const int st = go(box_from_args_ok(d_in, d_sum, d_sqsum, d_out, width, height, channels, n_images, k), n_images); st != GO) return st;
    return launch_box_from_integral(d_in, d_sum, d_sqsum, d_out, width, height, channels, n_images, *k, (hipStream_t)stream);
}

extern "C" size_t mi_blur_box_work_bytes(int width, int height, int channels, int n_images, const mi_blur_box *k)
{
    if (!box_ok(k) || !hist_image_ok(width, height, channels) || n_images < 0) return 0;
    const int tables = box_tables(*k);
    return tables * box_table_bytes(width, height, channels, n_images) +
           integral_work_bytes(width, height, channels, n_images, tables, tunables().integral_band);
}

// The dispatches of mi_blur_enqueue_box on buffers that are known to be good: work = S [Q] and the integral's own work.
static int enqueue_box(const uint8_t *d_in, uint8_t *d_out, int W, int H, int C, int n_images, const mi_blur_box &k, void *d_work, hipStream_t stream)
{
    const size_t table = box_table_bytes(W, H, C, n_images);
    uint8_t *base = static_cast<uint8_t *>(d_work);
    uint32_t *sum = reinterpret_cast<uint32_t *>(base);
    uint32_t *sqsum = k.op == MI_BLUR_BOX_STDDEV ? reinterpret_cast<uint32_t *>(base + table) : nullptr;
    if (const int rc = launch_integral(d_in, sum, sqsum, W, H, C, n_images, base + box_tables(k) * table, stream)) return rc;
    return launch_box_from_integral(k.op == MI_BLUR_BOX_THRESHOLD ? d_in : nullptr, sum, sqsum, d_out, W, H, C, n_images, k, stream);
}

extern "C" int mi_blur_enqueue_box(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images, const mi_blur_box *k,
                                   void *d_work, void *stream)
{
    if (const int st = go(box_args_ok(d_in, d_out, width, height, channels, n_images, k) && aligned_to(d_work, 16), n_images); st != GO) return st;
    return enqueue_box(d_in, d_out, width, height, channels, n_images, *k, d_work, (hipStream_t)stream);
}

// The one CPU form that answers the empty batch itself, before it makes its tables.
extern "C" int mi_blur_cpu_run_box(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images, const mi_blur_box *k,
                                   int n_threads)
{
    if (!box_args_ok(in, out, width, height, channels, n_images, k)) return MI_BLUR_ERR_INVALID;
    if (n_images == 0) return MI_BLUR_OK;
    const size_t words = integral_words(width, height, channels, n_images);
    std::vector<uint32_t> sum, sqsum;
    try {
        sum.resize(words);
        if (k->op == MI_BLUR_BOX_STDDEV) sqsum.resize(words);
    } catch (...) {
        return MI_BLUR_ERR_NOMEM;
    }
    uint32_t *q = k->op == MI_BLUR_BOX_STDDEV ? sqsum.data() : nullptr;
    if (!cpu_integral(in, sum.data(), q, width, height, channels, n_images, n_threads)) return MI_BLUR_ERR_NOMEM;
    cpu_box_from_integral(in, sum.data(), q, out, width, height, channels, n_images, *k, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_run_integral(int device, const uint8_t *host_in, uint32_t *host_sum, uint32_t *host_sqsum, int width, int height, int channels,
                                    int n_images)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_integral(host_in, host_sum, host_sqsum, width, height, channels, n_images, 0);
    if (const int st = go(integral_args_ok(host_in, host_sum, host_sqsum, width, height, channels, n_images, 4), n_images, device); st != GO) return st;
    const size_t in_bytes = image_bytes(width, height, channels, n_images), table = integral_words(width, height, channels, n_images) * sizeof(uint32_t);
    DeviceCall dc;
    uint8_t *in = dc.make<uint8_t>(in_bytes);
    uint32_t *sum = dc.make<uint32_t>(table, host_sum != nullptr), *sqsum = dc.make<uint32_t>(table, host_sqsum != nullptr);   // only the tables asked for
    void *work = dc.make<void>(mi_blur_integral_work_bytes(width, height, channels, n_images, host_sum && host_sqsum));
    dc.put(in, host_in, in_bytes);
    if (!dc.status) dc.status = launch_integral(in, sum, sqsum, width, height, channels, n_images, work, nullptr);
    dc.get(host_sum, sum, table);
    dc.get(host_sqsum, sqsum, table);
    return dc.status;
}

extern "C" int mi_blur_run_box(int device, const uint8_t *host_in, uint8_t *host_out, int width, int height, int channels, int n_images,
                               const mi_blur_box *k)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_box(host_in, host_out, width, height, channels, n_images, k, 0);
    if (const int st = go(box_args_ok(host_in, host_out, width, height, channels, n_images, k), n_images, device); st != GO) return st;
    const size_t bytes = image_bytes(width, height, channels, n_images);
    DeviceCall dc;
    uint8_t *in = dc.make<uint8_t>(bytes), *out = dc.make<uint8_t>(bytes);
    void *work = dc.make<void>(mi_blur_box_work_bytes(width, height, channels, n_images, k));
    dc.put(in, host_in, bytes);
    if (!dc.status) dc.status = enqueue_box(in, out, width, height, channels, n_images, *k, work, nullptr);
    dc.get(host_out, out, bytes);
    return dc.status;
}

// ----------------------------------------------------------------------------------
// exact distance transform.  The arguments: dist_args_ok() (filter.h).
// ----------------------------------------------------------------------------------
extern "C" int mi_blur_dist_value(const mi_blur_dist *k, uint32_t t)
{
    if (!dist_ok(k, true)) return -1;
    if (t != MI_BLUR_DIST_NONE && (t > dist_max(k->metric) || t >= dist_start(k->metric, k->limit))) return -1;
    return dist_byte(k->metric, k->byte_op, k->invert, t);
}

extern "C" size_t mi_blur_dist_work_bytes(int width, int height, int channels, int n_images, const mi_blur_dist *k)
{
    if (!dist_ok(k, true) || !hist_image_ok(width, height, channels) || n_images < 0) return 0;
    return dist_work_bytes(width, height, channels, n_images, tunables().dist_band);
}

extern "C" int mi_blur_enqueue_dist(const uint8_t *d_in, uint32_t *d_table, int width, int height, int channels, int n_images, const mi_blur_dist *k,
                                    void *d_work, void *stream)
{
    if (const int st = go(dist_args_ok(d_in, d_table, width, height, channels, n_images, k, false, 16) && aligned_to(d_work, 16), n_images); st != GO) return st;
    return launch_dist(d_in, d_table, nullptr, width, height, channels, n_images, *k, d_work, (hipStream_t)stream);
}

extern "C" int mi_blur_enqueue_dist_u8(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images, const mi_blur_dist *k,
                                       void *d_work, void *stream)
{
    if (const int st = go(dist_args_ok(d_in, d_out, width, height, channels, n_images, k, true, 1) && aligned_to(d_work, 16), n_images); st != GO) return st;
    return launch_dist(d_in, nullptr, d_out, width, height, channels, n_images, *k, d_work, (hipStream_t)stream);
}

extern "C" int mi_blur_cpu_run_dist(const uint8_t *in, uint32_t *table, int width, int height, int channels, int n_images, const mi_blur_dist *k,
                                    int n_threads)
{
    if (!dist_args_ok(in, table, width, height, channels, n_images, k, false, 4)) return MI_BLUR_ERR_INVALID;
    return cpu_dist(in, table, nullptr, width, height, channels, n_images, *k, n_threads) ? MI_BLUR_OK : MI_BLUR_ERR_NOMEM;
}

extern "C" int mi_blur_cpu_run_dist_u8(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images, const mi_blur_dist *k,
                                       int n_threads)
{
    if (!dist_args_ok(in, out, width, height, channels, n_images, k, true, 1)) return MI_BLUR_ERR_INVALID;
    return cpu_dist(in, nullptr, out, width, height, channels, n_images, *k, n_threads) ? MI_BLUR_OK : MI_BLUR_ERR_NOMEM;
}

// The blocking forms on a HIP device, the arguments checked: the byte form, or the table (4 bytes an element).
static int run_dist(int device, const uint8_t *host_in, void *host_out, bool bytes, bool args_ok, int W, int H, int C, int n_images, const mi_blur_dist *k)
{
    if (const int st = go(args_ok, n_images, device); st != GO) return st;
    const size_t in_bytes = image_bytes(W, H, C, n_images), out_bytes = in_bytes * (bytes ? 1 : sizeof(uint32_t));
    DeviceCall dc;
    uint8_t *in = dc.make<uint8_t>(in_bytes);
    void *out = dc.make<void>(out_bytes), *work = dc.make<void>(mi_blur_dist_work_bytes(W, H, C, n_images, k));
    dc.put(in, host_in, in_bytes);
    if (!dc.status)
        dc.status = launch_dist(in, bytes ? nullptr : static_cast<uint32_t *>(out), bytes ? static_cast<uint8_t *>(out) : nullptr, W, H, C, n_images, *k,
                                work, nullptr);
    dc.get(host_out, out, out_bytes);
    return dc.status;
}

extern "C" int mi_blur_run_dist(int device, const uint8_t *host_in, uint32_t *host_table, int width, int height, int channels, int n_images,
                                const mi_blur_dist *k)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_dist(host_in, host_table, width, height, channels, n_images, k, 0);
    return run_dist(device, host_in, host_table, false, dist_args_ok(host_in, host_table, width, height, channels, n_images, k, false, 4), width, height,
                    channels, n_images, k);
}

extern "C" int mi_blur_run_dist_u8(int device, const uint8_t *host_in, uint8_t *host_out, int width, int height, int channels, int n_images,
                                   const mi_blur_dist *k)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_dist_u8(host_in, host_out, width, height, channels, n_images, k, 0);
    return run_dist(device, host_in, host_out, true, dist_args_ok(host_in, host_out, width, height, channels, n_images, k, true, 1), width, height,
                    channels, n_images, k);
}

// ----------------------------------------------------------------------------------
// template matching and the peak search.  The arguments: match_args_ok(), match_peak_args_ok() (filter.h).
// ----------------------------------------------------------------------------------
static bool match_sums_ok(uint32_t A, uint32_t s, uint32_t ss)
{
    return (uint64_t)s <= 255ull * A && (uint64_t)ss <= 65025ull * A && (uint64_t)s * s <= (uint64_t)A * ss;
}

extern "C" int32_t mi_blur_match_value(int method, uint32_t A, uint32_t sum_at, uint32_t sum_a, uint32_t sum_aa, uint32_t sum_t, uint32_t sum_tt)
{
    if (!match_is_score(method) || A < 1 || A > MI_BLUR_MATCH_MAX_AREA) return INT32_MIN;
    if (!match_sums_ok(A, sum_a, sum_aa) || !match_sums_ok(A, sum_t, sum_tt)) return INT32_MIN;
    if ((unsigned __int128)sum_at * sum_at > (unsigned __int128)sum_aa * sum_tt) return INT32_MIN;
    return match_score(method, A, sum_at, sum_a, sum_aa, sum_t, sum_tt);
}

extern "C" size_t mi_blur_match_work_bytes(int width, int height, int channels, int n_images, const mi_blur_match *k)
{
    if (!hist_image_ok(width, height, channels) || n_images < 0 || !match_ok(k, width, height, channels)) return 0;
    size_t bytes = round16(match_sums_bytes(*k, n_images)) + round16(match_pad_bytes(*k, channels, n_images));
    if (match_is_score(k->method))
        bytes += match_table_bytes(*k, width, height, n_images) + 2 * box_table_bytes(width, height, channels, n_images) +
                 round16(mi_blur_integral_work_bytes(width, height, channels, n_images, 1));
    return bytes ? bytes : 16;
}

static size_t match_out_bytes(int W, int H, int n_images, const mi_blur_match &k)
{
    return (size_t)n_images * (size_t)(H - k.th + 1) * (size_t)(W - k.tw + 1) * sizeof(uint32_t);
}

extern "C" int mi_blur_enqueue_match(const uint8_t *d_in, const uint8_t *d_t, void *d_out, int width, int height, int channels, int n_images,
                                     const mi_blur_match *k, void *d_work, void *stream)
{
    if (const int st = go(match_args_ok(d_in, d_t, d_out, width, height, channels, n_images, k, 16) && aligned_to(d_work, 16), n_images); st != GO) return st;
    return launch_match(d_in, d_t, d_out, width, height, channels, n_images, *k, d_work, (hipStream_t)stream);
}

extern "C" int mi_blur_cpu_run_match(const uint8_t *in, const uint8_t *t, void *out, int width, int height, int channels, int n_images,
                                     const mi_blur_match *k, int n_threads)
{
    if (!match_args_ok(in, t, out, width, height, channels, n_images, k, 4)) return MI_BLUR_ERR_INVALID;
    cpu_match(in, t, out, width, height, channels, n_images, *k, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_run_match(int device, const uint8_t *host_in, const uint8_t *host_t, void *host_out, int width, int height, int channels,
                                 int n_images, const mi_blur_match *k)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_match(host_in, host_t, host_out, width, height, channels, n_images, k, 0);
    if (const int st = go(match_args_ok(host_in, host_t, host_out, width, height, channels, n_images, k, 4), n_images, device); st != GO) return st;
    const size_t in_bytes = image_bytes(width, height, channels, n_images), out_bytes = match_out_bytes(width, height, n_images, *k);
    const size_t t_bytes = (size_t)match_templates(*k, n_images) * k->th * k->tw * channels;
    DeviceCall dc;
    uint8_t *in = dc.make<uint8_t>(in_bytes), *t = dc.make<uint8_t>(t_bytes);
    void *out = dc.make<void>(out_bytes), *work = dc.make<void>(mi_blur_match_work_bytes(width, height, channels, n_images, k));
    dc.put(in, host_in, in_bytes);
    dc.put(t, host_t, t_bytes);
    if (!dc.status) dc.status = launch_match(in, t, out, width, height, channels, n_images, *k, work, nullptr);
    dc.get(host_out, out, out_bytes);
    return dc.status;
}

extern "C" size_t mi_blur_match_peak_work_bytes(int out_width, int out_height, int n_images)
{
    if (out_width < 1 || out_height < 1 || (long long)out_width * out_height > INT_MAX || n_images < 0) return 0;
    const size_t bytes = (size_t)n_images * MI_BLUR_MATCH_PEAK_PARTS * 2 * sizeof(uint64_t);
    return bytes ? bytes : 16;
}

extern "C" int mi_blur_enqueue_match_peak(const void *d_table, int is_signed, int out_width, int out_height, int n_images, int64_t *d_peaks,
                                          void *d_work, void *stream)
{
    if (const int st = go(match_peak_args_ok(d_table, is_signed, out_width, out_height, n_images, d_peaks, 16, 16) && aligned_to(d_work, 16), n_images); st != GO)
        return st;
    return launch_match_peak(d_table, is_signed, out_width, out_height, n_images, d_peaks, d_work, (hipStream_t)stream);
}

extern "C" int mi_blur_cpu_run_match_peak(const void *table, int is_signed, int out_width, int out_height, int n_images, int64_t *peaks, int n_threads)
{
    if (!match_peak_args_ok(table, is_signed, out_width, out_height, n_images, peaks, 4, 8)) return MI_BLUR_ERR_INVALID;
    cpu_match_peak(table, is_signed, out_width, out_height, n_images, peaks, n_threads);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_run_match_peak(int device, const void *host_table, int is_signed, int out_width, int out_height, int n_images,
                                      int64_t *host_peaks)
{
    if (device == MI_BLUR_DEVICE_CPU) return mi_blur_cpu_run_match_peak(host_table, is_signed, out_width, out_height, n_images, host_peaks, 0);
    if (const int st = go(match_peak_args_ok(host_table, is_signed, out_width, out_height, n_images, host_peaks, 4, 8), n_images, device); st != GO) return st;
    const size_t table_bytes = (size_t)n_images * out_width * out_height * sizeof(uint32_t), peak_bytes = (size_t)n_images * 6 * sizeof(int64_t);
    DeviceCall dc;
    void *table = dc.make<void>(table_bytes), *work = dc.make<void>(mi_blur_match_peak_work_bytes(out_width, out_height, n_images));
    int64_t *peaks = dc.make<int64_t>(peak_bytes);
    dc.put(table, host_table, table_bytes);
    if (!dc.status) dc.status = launch_match_peak(table, is_signed, out_width, out_height, n_images, peaks, work, nullptr);
    dc.get(host_peaks, peaks, peak_bytes);
    return dc.status;
}
