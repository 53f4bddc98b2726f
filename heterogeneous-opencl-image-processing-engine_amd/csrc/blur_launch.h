// blur_launch.h — internal (not part of the C ABI): launch interface between the files that implement the C ABI
// (mi_blur_api.cpp, table_api.cpp, comm_api.cpp) and the gfx950 kernels in the .hip files (what those share among themselves: kernel_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "filter.h"

namespace mi_blur {

struct LaunchDesc {
    const Filter *filter;   // what to apply (filter.h); the caller keeps it alive until launch() returns
    const uint8_t *in;      // device, n_images bands of band_rows rows, laid end to end
    uint8_t *out;           // device, n_images blocks of (y1-y0) rows
    int width, band_rows, channels;
    int n_images;
    int y0, y1;             // output rows [y0,y1) of each band
    long long in_stride, out_stride;  // bytes between consecutive bands / output blocks; 0 = laid end to end.
                            // Non-dense strides are taken by the tiled kernel only (multiples of 16).
    int concurrent;         // hint: how many streams the caller rotates launches like this one over (0/1 = one after another).
                            // Small 3x3 launches that overlap with their like run faster as LDS tiles, alone as the direct kernel.
    int max_blocks;         // > 0: cap the grid of the aligned tiled kernel; its workgroups then loop over the tiles (zero-copy submits)
    int variant;            // mi_blur_variant
    const uint8_t *halo_top, *halo_bottom;   // one band only: rows [0, y0) / [y1, band_rows) are read from here (another shard,
                            // possibly another GPU's memory) instead of from `in`; nullptr = from `in`.  Direct kernel only.
    hipStream_t stream;
    hipEvent_t start, stop; // optional: dispatch start/stop timestamps (hipExtLaunchKernel)
};

// Returns MI_BLUR_OK or a negative mi_blur_status.  Every filter kind but BOX is handed to the launch_* of its family
// below; launch_fused and zc_fill_batch take BOX filters only.
int launch(const LaunchDesc &d);
// The other families, each in the .hip file of its name: the separable kernel of d.filter->taps, the median of
// d.filter->radius, the window minimum / maximum / gradient, the bilateral filter and the signed 2-D convolution of
// d.filter (the last two carry their tables in the kernel arguments).  Each chooses between its fast kernel for rows of
// whole 16-byte chunks, 1-4 channels, aligned buffers and strides (LDS-tiled; the median's register-window kernel, radius
// 1|2 only) and its generic one.  All honour in/out strides, bands [y0, y1) and the 64-bit image offsets of launch();
// ignore max_blocks, concurrent and variant (AUTO); halo_top / halo_bottom: MI_BLUR_ERR_UNSUPPORTED.
int launch_sep(const LaunchDesc &d);
int launch_median(const LaunchDesc &d);
int launch_morph(const LaunchDesc &d);
int launch_bilateral(const LaunchDesc &d);
int launch_conv(const LaunchDesc &d);
// The decimating separable filter (FilterKind::SEP_DOWN, sep_down_kernels.hip): d.in = n_images images of band_rows x width,
// d.out = n_images images of the DECIMATED size (out_stride, when given, is measured against that).  Honours in/out
// strides and 64-bit image offsets like the others; only the whole image: y0 != 0, y1 != band_rows, halo_top / halo_bottom
// are MI_BLUR_ERR_UNSUPPORTED.
int launch_sep_down(const LaunchDesc &d);
// The resize (FilterKind::RESIZE, resize_kernels.hip): d.in = n_images images of band_rows x width, d.out = n_images
// images of out_h x out_w (out_stride, when given, is measured against that, and may exceed in_stride).  The
// contract of launch_sep_down: only the whole image, bands and halo pointers are MI_BLUR_ERR_UNSUPPORTED.
int launch_resize(const LaunchDesc &d);
// The affine warp (FilterKind::WARP, warp_kernels.hip): d.in = n_images images of band_rows x width, d.out = n_images
// images of out_h x out_w.  The contract of launch_resize.
int launch_warp(const LaunchDesc &d);
// The perspective warp (FilterKind::WARP_PERSP, warp_kernels.hip).  The contract of launch_resize.
int launch_warp_persp(const LaunchDesc &d);
// The remap (FilterKind::REMAP, remap_kernels.hip): d.filter->remap_map is DEVICE memory, out_h x out_w int32 pairs, read by
// the kernels of this launch only.  The contract of launch_resize.
int launch_remap(const LaunchDesc &d);
// The area resize (FilterKind::AREA, area_kernels.hip).  The contract of launch_resize.
int launch_area(const LaunchDesc &d);
// The colour transform (FilterKind::COLOR, color_kernels.hip).  The contract of launch_resize; out_stride is measured
// against the image with the OUTPUT's channel count.
int launch_color(const LaunchDesc &d);
// The histogram family (hist_kernels.hip); no Filter and no LaunchDesc: histograms are not images.  Dense images of
// W x H x C (hist_image_ok(), filter.h), n_images of them; every argument is checked (MI_BLUR_ERR_INVALID), an empty
// batch is MI_BLUR_OK.  launch_hist: hist = uint32[n][C][256], 16-byte aligned, zeroed on the stream and then added
// into.  launch_tone_tables: hist -> tables = uint8[n][C][256], by t.  launch_tables: image i through tables[i].
int launch_hist(const uint8_t *in, uint32_t *hist, int W, int H, int C, int n_images, hipStream_t stream);
int launch_tone_tables(const uint32_t *hist, uint8_t *tables, int C, int n_images, const mi_blur_tone &t, hipStream_t stream);
int launch_tables(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const uint8_t *tables, hipStream_t stream);
// The two-image arithmetic (arith_kernels.hip); no Filter and no LaunchDesc either: it has more than one input.  Dense
// images of W x H x C, n_images of them; b and m as *k's plane and shared flags say, m null unless the operation is
// LERP.  Every argument is checked (arith_args_ok(), filter.h: MI_BLUR_ERR_INVALID), an empty batch is MI_BLUR_OK.
int launch_arith(const uint8_t *a, const uint8_t *b, const uint8_t *m, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_arith &k,
                 hipStream_t stream);
// The integral images and the box filters made from them (integral_kernels.hip); no Filter and no LaunchDesc.  Dense
// images of W x H x C, n_images of them; every argument is checked (integral_args_ok(), box_from_args_ok(), filter.h:
// MI_BLUR_ERR_INVALID), an empty batch is MI_BLUR_OK.  launch_integral: sum and / or sqsum = uint32[n][H][W][C], 16-byte
// aligned; work = integral_work_bytes() bytes for the band in force (tunables().integral_band), 16-byte aligned.
// launch_box_from_integral: in only for THRESHOLD, sqsum only for STDDEV.
int launch_integral(const uint8_t *in, uint32_t *sum, uint32_t *sqsum, int W, int H, int C, int n_images, void *work, hipStream_t stream);
int launch_box_from_integral(const uint8_t *in, const uint32_t *sum, const uint32_t *sqsum, uint8_t *out, int W, int H, int C, int n_images,
                             const mi_blur_box &k, hipStream_t stream);
// The distance transform (dist_kernels.hip); no Filter and no LaunchDesc.  Dense images of W x H x C, n_images of them;
// exactly one of table (uint32[n][H][W][C], 16-byte aligned) and out (the byte form, which may be `in`) is given, and k
// is the struct of that call.  Every argument is checked (dist_args_ok(), filter.h: MI_BLUR_ERR_INVALID), an empty batch
// is MI_BLUR_OK.  work = dist_work_bytes() bytes for the band in force (tunables().dist_band), 16-byte aligned.
int launch_dist(const uint8_t *in, uint32_t *table, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_dist &k, void *work, hipStream_t stream);
// CLAHE (clahe_kernels.hip); no Filter and no LaunchDesc.  Dense images of W x H x C, n_images of them; every argument
// is checked (clahe_ok(), hist_image_ok(), filter.h: MI_BLUR_ERR_INVALID), an empty batch is MI_BLUR_OK.
// launch_clahe_tables: hist = uint32[n][TY][TX][C][256], 16-byte aligned, and tables = uint8[n][TY][TX][C][256], both
// overwritten.  launch_clahe_apply: every pixel through the four tables around it; tables at any alignment.
int launch_clahe_tables(const uint8_t *in, uint32_t *hist, uint8_t *tables, int W, int H, int C, int n_images, const mi_blur_clahe &k,
                        hipStream_t stream);
int launch_clahe_apply(const uint8_t *in, uint8_t *out, int W, int H, int C, int n_images, const mi_blur_clahe &k, const uint8_t *tables,
                       hipStream_t stream);
// Template matching and the peak search (match_kernels.hip); no Filter and no LaunchDesc.  Every argument is checked
// (match_args_ok(), match_peak_args_ok(), filter.h: MI_BLUR_ERR_INVALID), an empty batch is MI_BLUR_OK.  launch_match:
// out = 32-bit words [n][Ho][Wo], 16-byte aligned; work = mi_blur_match_work_bytes() bytes, 16-byte aligned.
// launch_match_peak: peaks = int64[n][6] and work = mi_blur_match_peak_work_bytes() bytes, both 16-byte aligned.
int launch_match(const uint8_t *in, const uint8_t *t, void *out, int W, int H, int C, int n_images, const mi_blur_match &k, void *work, hipStream_t stream);
int launch_match_peak(const void *table, int is_signed, int Wo, int Ho, int n_images, int64_t *peaks, void *work, hipStream_t stream);
// Sets what last_kernel() reports for the calling thread.
void set_last_kernel(const char *name);

// Fused stream (blur_fused_kernel): one dispatch over d.n_images images whose blocks are ordered in batches of
// batch_images; every block of batch b adds *waves_per_block (1) to one of count[kb .. kb+k-1], k = *counters_per_batch
// (device, zeroed by the caller) after its stores have drained, so batch b is complete when those k sum to its blocks (geometry outputs:
// a full batch has *tiles_per_batch blocks, the last one what is left of *total_blocks).
// Shapes of the tiled kernel, aligned or ragged, 1-4 channels (MI_BLUR_ERR_UNSUPPORTED otherwise; ragged rows need f.tail_ctr).
// geometry_only: fill the geometry outputs for these knobs and return without launching (the caller decides from them
// whether its counters can keep counting up).  tun: the knob set to use (nullptr = the current one); a caller that asks
// for the geometry first passes the same copy to both calls.
struct Tunables;
struct FusedDesc {
    unsigned *count; int batch_images; unsigned *tiles_per_batch, *waves_per_block, *total_blocks;
    const Tunables *tun; bool geometry_only;
    unsigned *tail_ctr;     // device word, zero between passes: ticket counter of the pass's dynamic tail ("fused_tail"); nullptr = none
    long long count_words;  // how many words `count` holds (0 = at least 8 per batch, the minimum)
    unsigned *counters_per_batch;   // geometry output: counters each batch uses (8 .. 256; count[k * b .. k * b + k - 1] belong to batch b)
    unsigned *tail_tiles;   // geometry output: tiles of the pass's dynamic tail (0 = blur_fused_kernel or an empty tail)
    unsigned *gate;         // device word or nullptr: a pass with a dynamic tail stores `seq` there when "fused_overlap" per mille of
    unsigned seq;           // it is left (one workgroup, once); also the number of the pass among the context's fused passes
};
int launch_fused(const LaunchDesc &d, const FusedDesc &f);
// One wave on `stream` that ends when *gate has reached `want` (signed difference) or after ZC_HARD_TICKS (fused_gate_kernel):
// whatever is queued behind it on that stream starts then.  A hint for WHEN, never a condition for correctness.
int launch_fused_gate(const unsigned *gate, unsigned want, hipStream_t stream);
// Watcher of one fused pass (fused_watch_kernel, one wave on a stream other than the pass's): follows the per-batch counters and keeps
// *host_word (pinned host memory) = (pass_seq << 32) | leading batches complete, so the host reads a batch's completion
// from its own memory instead of copying the counters back.  Ends when all n_batches are complete (or after a hard limit).
int launch_fused_watch(const unsigned *count, unsigned n_batches, unsigned tiles_per_batch, unsigned total_blocks, unsigned per_block,
                       unsigned long long *host_word, unsigned pass_seq, hipStream_t stream, unsigned counters_per_batch);

// Planar (CImg storage: plane c of image i at (i*C + c)*W*H) <-> interleaved repack, layout_kernels.hip.
int launch_planar_to_interleaved(const uint8_t *src, uint8_t *dst, int width, int height, int channels, int n_images, hipStream_t s);
int launch_interleaved_to_planar(const uint8_t *src, uint8_t *dst, int width, int height, int channels, int n_images, hipStream_t s);
// Halo pull: copy `bytes` bytes from each non-null (peer) source into the matching halo destination, one launch.
int launch_halo_pull(const uint8_t *top_src, uint8_t *top_dst, const uint8_t *bottom_src, uint8_t *bottom_dst, size_t bytes, hipStream_t stream);

// ----------------------------------------------------------------------------------------------------------------
// Zero-copy batch server (blur_server_kernel): ONE long-lived dispatch takes batch after batch of pinned host frames from a
// ring of descriptors the host fills, so consecutive batches of a host-fed stream flow through the same workgroups with
// no dispatch boundary between them (a per-batch launch costs the host link ~45 us of a ~200 us batch, profiles/r03_e2e_timeline.md).
//   host -> device: ZcHostCtl::batch[k % ZC_RING] (the tile parameters of batch k), then tail = k + 1
//   device -> host: done[k % ZC_RING] = k + 1 once every output byte of batch k is in host memory
// The grid is n_workers + 1 workgroups: the last one is the POLLER (reads `tail` over the host link, republishes it in
// device memory, decides when the server ends), the others walk the tiles.  A server ALWAYS ends: after `budget` batches,
// after idle_ticks (100 MHz) without a new batch, or when the host sets `quit`; its workers leave once the poller has said
// where the server stops.  The host keeps the next server queued behind the running one on the same stream.
// ----------------------------------------------------------------------------------------------------------------
constexpr unsigned ZC_RING = 64;
constexpr unsigned ZC_PARAM_WORDS = 32;
constexpr unsigned ZC_TRACE_BATCHES = 512;                    // diagnostics: the trace keeps the stamps of a context's first this-many batches
constexpr unsigned long long ZC_HARD_TICKS = 1000000000ull;   // 10 s of the 100 MHz device clock: no wait inside a server outlasts this
struct ZcBatch {
    unsigned params[ZC_PARAM_WORDS];   // TiledParams of the batch, as words
    unsigned tile_first;               // global number of the batch's first tile (tiles are numbered through the batches, mod 2^32)
    unsigned n_tiles;
    unsigned pad[6];
};
struct ZcHostCtl {                     // pinned, device-visible host memory
    unsigned tail;                     // host -> device: descriptors published so far
    unsigned quit;                     // host -> device: leave at the next poll
    unsigned servers_done;             // device -> host: servers that have signalled every batch they took and left
    unsigned error;                    // device -> host: a server's wait ran into its hard limit (ZC_HARD_TICKS) — should never happen
    unsigned pad0[12];
    unsigned done[ZC_RING];            // device -> host: done[k % ZC_RING] = k + 1
    unsigned long long t_begin[ZC_RING], t_end[ZC_RING];   // device clock (100 MHz ticks): batch k taken up / complete
    ZcBatch batch[ZC_RING];
};
struct ZcDevCtl {                      // device memory, zeroed when the server state is created
    unsigned next[2];                  // server `seq` starts at batch next[seq & 1] and leaves next[(seq + 1) & 1]
    unsigned gnext[2];                 // ... and at global tile gnext[seq & 1]
    unsigned start_seq;                // poller -> workers: server (start_seq - 1) has set the ticket counter
    unsigned avail;                    // poller -> workers: batches [.., avail) are published (descriptors in `batch`)
    unsigned stop_seq, stop_at, stop_tile;   // poller -> workers: server (stop_seq - 1) ends before batch stop_at / tile stop_tile
    unsigned ticket;                   // next global tile to hand out
    unsigned pad[6];
    unsigned tiles_done[ZC_RING];      // tiles of the batch in this ring slot whose output is in host memory
    ZcBatch batch[ZC_RING];            // device copies of the descriptors
};
struct ZcGeometry { unsigned threads; size_t lds; int rpg; int channels, radius, ragged; };
// Tile parameters of one batch (d.in/d.out = DEVICE addresses of the pinned buffers) in the server's geometry; *geo is
// filled on the first call (geo->threads == 0) and must match on later ones (MI_BLUR_ERR_UNSUPPORTED otherwise).
int zc_fill_batch(const LaunchDesc &d, ZcGeometry *geo, ZcBatch *b, unsigned *n_tiles);
int zc_launch_server(const ZcGeometry &geo, ZcHostCtl *ctl, ZcDevCtl *dev, unsigned seq, unsigned n_workers, unsigned budget,
                     unsigned idle_ticks, hipStream_t stream, unsigned long long *trace = nullptr, int fixed_share = 0);

// Name of the kernel the calling thread's most recent launch() / launch_fused() chose ("" before the first).
const char *last_kernel();

// True when the LDS-tiled vector kernel can take this shape.
bool tiled_eligible(const void *in, const void *out, int width, int channels);

// Tunables: defaults and their environment variables (MI_BLUR_STAGE=dma|reg, MI_BLUR_RPG=4|8|16, MI_BLUR_XCD=0|1, ...) from
// the KNOBS table below, changeable at run time through mi_blur_set_option.  Process-wide, kept behind a mutex: tunables() returns a coherent COPY and every launch
// works from the one copy it took when it started, so flipping a knob while another thread launches is not a data race
// (that launch sees the old set or the new one, never a mix).
struct Tunables {
    int stage_dma; int rpg; int xcd_remap; int debug_copy; int row_shuffle; int prefer_stream; int stream_bh; int zero_copy; int ragged;
    int fused_release;   // fused stream: 1 = the per-block completion add is release-ordered at agent scope (architectural; slow)
    int experiment;      // 1 = the tiled kernel's OTHER row-pass form (A/B runs; C = 3 only)
    int xcd_run;         // tiled kernel's blockIdx -> tile map: 0/1 = one contiguous eighth of the launch per XCD (default),
                         // r >= 2 = runs of r tiles dealt to the XCDs in turn
    int zero_copy_streams;   // streams the zero-copy submits of a context alternate over (1 = one in-order stream)
    int zero_copy_blocks;    // zero-copy submits: cap on resident workgroups (0 = no cap: one workgroup per tile)
    int stream_updown;   // streaming variant: 1 (default) = odd bands march upwards, so both readers of a band seam come at the same time
    int prefer_direct;   // AUTO and the direct (register-staged, LDS-free) variant: 0 never, 1 (default) where it measured faster
                         // (every 5x5 launch, 3x3 launches up to 128 MiB of output), 2 whenever the shape is eligible
    int direct_bh;       // direct variant: output rows per lane (8; 4 | 12 | 16 instantiated for C = 3 only, A/B runs)
    int debug_xcd_times; // diagnostics: the tiled kernel's workgroups leave start/end times per XCD (mi_blur_debug_xcd_times)
    int fused_window;    // fused stream: batches per window of its blockIdx -> tile map (8: one whole batch per XCD per window)
    int fused_tail;      // fused stream: per mille of a pass's tiles that are handed out dynamically at the end (0 = none)
    int fused_adds_per_word; // fused stream: a batch gets as many completion counters (8 .. 256) as keep the adds per counter and pass under this
    int fused_tail_blocks; // ... by (100 + this) % as many extra workgroups as there are tail tiles (one ticket each; default 100)
    int fused_overlap;   // fused stream: 0 = every pass on one stream; v > 0 = consecutive passes with a dynamic tail alternate over two
                         // streams and a pass starts when its predecessor has v per mille of its tiles left (default 30)
    int zero_copy_server;  // zero-copy submits of aligned shapes go through the batch server (one long-lived dispatch per stream of
                           // batches, blur_server_kernel) instead of one launch per batch: 1 (default) | 0
    int zero_copy_server_min_kb; // batch server: submits whose output is smaller than this many KiB take one launch each instead (default 1280)
    int staged_server;     // submits of PAGEABLE caller memory: 1 (default) = the batch server works on the slot's pinned staging buffers in
                           // place, 0 = DMA copy in, launch on device buffers, DMA copy out
    int zero_copy_workers; // batch server: worker workgroups (default 48: 40-64 measured best, profiles/r03_e2e_timeline.md)
    int zero_copy_idle_us; // batch server: leaves after this long without a new batch (default 300)
    int zero_copy_budget;  // batch server: leaves after this many batches, the queued next one carries on (default 256)
    int zero_copy_tickets; // batch server: 1 (default) = tiles by ticket counter, 0 = fixed share per worker (tile g to worker g mod n; A/B only)
    int resident_place_trials; // mi_blur_resident_alloc: candidate placements of a big pool that are timed before one is kept (default 4; 0/1 = none)
    int zero_copy_spin;    // waiting for a batch of the server: 0 (default) = spin ~20 us, then sleep in 20 us steps; 1 = spin + yield only
    int zero_copy_trace;   // diagnostics: the batch server's workers stamp their phases per batch (mi_blur_debug_zc_trace)
    int zero_copy_debug_base; // test hook: a new batch server starts this many batches (and 7x as many tiles) short of 2^32, so that the
                         // wrap of its batch and tile numbers — 80 minutes into a continuous batch-35 stream — happens at once (0 = off)
    int zero_copy_events; // zero-copy submits: 1 = the dispatch carries start/stop timestamp events (kernel bucket + completion),
                         // 0 = plain launch, completion by stream synchronise (timing experiment: no kernel bucket)
    int integral_band;   // blur_integral_tiled_kernel: rows per band (default INTEGRAL_BAND of filter.h; A/B runs)
    int box_bytes;       // blur_box_tiled_kernel: consecutive output bytes of a row per thread, 4 (default) | 16 (A/B runs)
    int dist_band;       // the distance transform's column pass: rows per band (default DIST_BAND of filter.h; A/B runs)
    int dist_chunk_log2; // blur_dist_tiled_kernel: log2 of the columns per search chunk (default DIST_CHUNK_LOG2 of filter.h; A/B runs)
    int match_tiled;     // 1 (default) = raw match launches go to blur_match_tiled_kernel where it is eligible, 0 = always the generic kernel
};
// Every knob once: its mi_blur_set_option key, its field, what values it takes, its default and the environment variable
// (or nullptr) that may replace the default when the library starts.  FLAG: any value, stored as 0 | 1.  RANGE: lo .. hi.
// ONE_OF: the values whose bit is set in lo (all below 31).  tunables_storage() (blur_kernels.hip) builds the defaults and
// reads the environment from this table — a value it does not accept is ignored — and mi_blur_set_option looks its key up here.
enum class KnobKind { FLAG, RANGE, ONE_OF };
struct Knob { const char *key; int Tunables::*field; KnobKind kind; int lo, hi, def; const char *env; };
constexpr int knob_bits(int a, int b, int c, int d) { return 1 << a | 1 << b | 1 << c | 1 << d; }
static constexpr Knob KNOBS[] = {
    {"stage_dma", &Tunables::stage_dma, KnobKind::FLAG, 0, 1, 1, "MI_BLUR_STAGE"},        // the variable also takes "dma" | "reg"
    {"rows_per_thread", &Tunables::rpg, KnobKind::ONE_OF, knob_bits(0, 4, 8, 16), 0, 0, "MI_BLUR_RPG"},   // 0 = choose per launch
    {"xcd_remap", &Tunables::xcd_remap, KnobKind::FLAG, 0, 1, 1, "MI_BLUR_XCD"},
    {"debug_copy", &Tunables::debug_copy, KnobKind::FLAG, 0, 1, 0, nullptr},              // ablation only (output is NOT a blur)
    {"row_shuffle", &Tunables::row_shuffle, KnobKind::FLAG, 0, 1, 0, nullptr},
    {"prefer_stream", &Tunables::prefer_stream, KnobKind::FLAG, 0, 1, 0, nullptr},
    {"zero_copy", &Tunables::zero_copy, KnobKind::FLAG, 0, 1, 1, nullptr},
    {"ragged_tiled", &Tunables::ragged, KnobKind::FLAG, 0, 1, 1, nullptr},
    {"stream_band_rows", &Tunables::stream_bh, KnobKind::RANGE, 0, 4096, 0, nullptr},     // 0 = choose per launch
    {"fused_release", &Tunables::fused_release, KnobKind::FLAG, 0, 1, 0, nullptr},
    {"experiment", &Tunables::experiment, KnobKind::FLAG, 0, 1, 0, nullptr},
    {"stream_updown", &Tunables::stream_updown, KnobKind::FLAG, 0, 1, 1, nullptr},
    {"zero_copy_streams", &Tunables::zero_copy_streams, KnobKind::RANGE, 1, 8, 4, nullptr},
    {"zero_copy_blocks", &Tunables::zero_copy_blocks, KnobKind::RANGE, 0, 1 << 20, 24, nullptr},
    {"prefer_direct", &Tunables::prefer_direct, KnobKind::RANGE, 0, 2, 1, "MI_BLUR_DIRECT"},
    {"direct_bh", &Tunables::direct_bh, KnobKind::ONE_OF, knob_bits(4, 8, 12, 16), 0, 8, nullptr},
    {"fused_adds_per_word", &Tunables::fused_adds_per_word, KnobKind::RANGE, 4, 4096, 32, nullptr},
    {"fused_tail_blocks", &Tunables::fused_tail_blocks, KnobKind::RANGE, 10, 800, 25, nullptr},
    {"fused_tail", &Tunables::fused_tail, KnobKind::RANGE, 0, 500, 30, "MI_BLUR_FUSED_TAIL"},
    {"fused_overlap", &Tunables::fused_overlap, KnobKind::RANGE, 0, 500, 30, "MI_BLUR_FUSED_OVERLAP"},
    {"fused_window", &Tunables::fused_window, KnobKind::RANGE, 1, 4096, 8, nullptr},
    {"debug_xcd_times", &Tunables::debug_xcd_times, KnobKind::FLAG, 0, 1, 0, nullptr},
    {"zero_copy_events", &Tunables::zero_copy_events, KnobKind::FLAG, 0, 1, 1, nullptr},
    {"zero_copy_server", &Tunables::zero_copy_server, KnobKind::FLAG, 0, 1, 1, nullptr},
    {"staged_server", &Tunables::staged_server, KnobKind::FLAG, 0, 1, 1, "MI_BLUR_STAGED_SERVER"},
    {"zero_copy_server_min_kb", &Tunables::zero_copy_server_min_kb, KnobKind::RANGE, 0, 1 << 20, 1280, nullptr},
    {"zero_copy_trace", &Tunables::zero_copy_trace, KnobKind::FLAG, 0, 1, 0, nullptr},
    {"zero_copy_tickets", &Tunables::zero_copy_tickets, KnobKind::FLAG, 0, 1, 1, nullptr},
    {"zero_copy_spin", &Tunables::zero_copy_spin, KnobKind::FLAG, 0, 1, 0, nullptr},
    {"zero_copy_debug_base", &Tunables::zero_copy_debug_base, KnobKind::RANGE, 0, 1 << 20, 0, nullptr},
    {"resident_place_trials", &Tunables::resident_place_trials, KnobKind::RANGE, 0, 8, 4, "MI_BLUR_PLACE_TRIALS"},
    {"zero_copy_workers", &Tunables::zero_copy_workers, KnobKind::RANGE, 1, 2048, 48, nullptr},
    {"zero_copy_idle_us", &Tunables::zero_copy_idle_us, KnobKind::RANGE, 10, 100000, 300, nullptr},
    {"zero_copy_budget", &Tunables::zero_copy_budget, KnobKind::RANGE, 1, 1 << 20, 256, nullptr},
    {"xcd_run", &Tunables::xcd_run, KnobKind::RANGE, 0, 1 << 20, 0, nullptr},
    {"integral_band", &Tunables::integral_band, KnobKind::RANGE, 1, 256, 16, nullptr},    // the default is INTEGRAL_BAND of filter.h
    {"box_bytes", &Tunables::box_bytes, KnobKind::ONE_OF, knob_bits(4, 16, 4, 16), 0, 4, nullptr},
    {"dist_band", &Tunables::dist_band, KnobKind::RANGE, 1, 256, 32, nullptr},            // the default is DIST_BAND of filter.h
    {"dist_chunk_log2", &Tunables::dist_chunk_log2, KnobKind::RANGE, 3, 5, 4, nullptr},   // the default is DIST_CHUNK_LOG2 of filter.h
    {"match_tiled", &Tunables::match_tiled, KnobKind::FLAG, 0, 1, 1, nullptr},
};
// Stores `value` in the knob's field of t if the knob accepts it; false (t untouched) otherwise.
static inline bool knob_set(const Knob &k, Tunables &t, int value)
{
    switch (k.kind) {
    case KnobKind::FLAG: t.*k.field = value != 0; return true;
    case KnobKind::RANGE: if (value < k.lo || value > k.hi) return false; break;
    case KnobKind::ONE_OF: if (value < 0 || value > 30 || !((k.lo >> value) & 1)) return false; break;
    }
    t.*k.field = value;
    return true;
}

Tunables tunables();
unsigned long long *debug_xcd_buffer();
unsigned debug_xcd_slots();
void set_tunables(const Tunables &t);

}  // namespace mi_blur
