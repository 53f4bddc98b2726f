/*
 * mi_blur.h — C ABI of the MI355X-native image-stream blur engine (libmi_blur.so).
 *
 * The reference (CC834/Heterogeneous-OpenCL-Image-Processing-Engine) has no
 * plugin/FFI surface: its hot path sits behind the OpenCL C API called from two
 * main() functions.  Each entry point below replaces one group of those OpenCL
 * calls; the citation is the reference call site it stands in for (paths are
 * relative to the reference tree).  INTEGRATION.md shows the edit a maintainer
 * makes in heterogeneous_blur.c / split_image_blur.c to bind them.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types; every function returns
 *     MI_BLUR_OK (0) or a negative mi_blur_status / positive passthrough code
 *     (see mi_blur_strerror).  The library never calls exit(): the reference's
 *     cl_error() print-and-exit policy (heterogeneous_blur.c:25-30) stays in the host.
 *   - images are interleaved uint8, row-major, pitch = width*channels, no padding
 *     (gaussian_kernel.cl:60; heterogeneous_blur.c:115,128-135); in != out.
 *   - radius 1 = the reference 3x3 {1,2,1}x{1,2,1}/16 (gaussian_kernel.cl:36-41);
 *     radius 2 = build-defined 5x5 {1,4,6,4,1}x{1,4,6,4,1}/256 (no reference kernel).
 *     Clamp-to-edge (:56-57), truncation (:70).
 *   - a context is single-threaded like a cl_command_queue used from one thread;
 *     different contexts may be driven from different host threads.
 *   - GPU entry points fail with MI_BLUR_ERR_NO_DEVICE when no HIP device is
 *     usable.  There is NO silent CPU fallback: the CPU device exists only when
 *     asked for by name (MI_BLUR_DEVICE_CPU), mirroring the reference's separate
 *     OpenCL CPU device (heterogeneous_blur.c:170-176).
 */
#ifndef MI_BLUR_H
#define MI_BLUR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_BLUR_VERSION 1
#define MI_BLUR_DEVICE_CPU (-1)      /* native host-thread device (reference: CL_DEVICE_TYPE_CPU) */

typedef enum mi_blur_status {
    MI_BLUR_OK = 0,
    MI_BLUR_ERR_INVALID = -1,        /* bad argument (null, non-positive size, radius not 1|2, in==out) */
    MI_BLUR_ERR_NO_DEVICE = -2,      /* no usable HIP device / device index out of range */
    MI_BLUR_ERR_NOMEM = -3,          /* host or device allocation failed */
    MI_BLUR_ERR_STATE = -4,          /* call not valid in the context's current state */
    MI_BLUR_ERR_UNSUPPORTED = -5,    /* e.g. RCCL entry point in a build without RCCL */
    MI_BLUR_ERR_HIP_BASE = -1000,    /* -(1000 + hipError_t) */
    MI_BLUR_ERR_RCCL_BASE = -2000    /* -(2000 + ncclResult_t) */
} mi_blur_status;

/* Kernel variant selector for mi_blur_enqueue_ex (tests force each path). */
typedef enum mi_blur_variant {
    MI_BLUR_VARIANT_AUTO = 0,        /* pitch%16==0 && channels<=4 && aligned pointers: the direct kernel (5x5; small 3x3 launches) or
                                        the LDS-tiled one (big 3x3 launches); other rows of >= 16 B: ragged tiled; 5-8 channels: the tiled
                                        kernel for the 3x3; else generic */
    MI_BLUR_VARIANT_GENERIC = 1,     /* one output byte per thread, any shape */
    MI_BLUR_VARIANT_TILED = 2,       /* LDS halo tile + 16-B vector loads (ragged form for odd pitches; _INVALID if rows < 16 B, C > 8, or
                                        C > 4 with the 5x5) */
    MI_BLUR_VARIANT_STREAM = 3       /* barrier-free: every wave streams its band through a wave-private LDS row ring
                                        (LDS-DMA, counted vmcnt), sliding window of row sums in registers (same eligibility) */,
    MI_BLUR_VARIANT_DIRECT = 4      /* no LDS: rows straight into registers, x-neighbours by DPP wave shifts (same eligibility) */
} mi_blur_variant;

const char *mi_blur_strerror(int status);
int mi_blur_version(void);
/* Which kernel the calling thread's most recent launch went to ("blur_tiled_kernel", "blur_direct_kernel",
 * "blur_fused_kernel", "blur_tiled_loop_kernel", "blur_stream_kernel", "blur_generic_kernel", "blur_sep_tiled_kernel",
 * "blur_sep_generic_kernel", "blur_median_fast_kernel", "blur_median_generic_kernel", "blur_morph_tiled_kernel",
 * "blur_morph_generic_kernel", "blur_bilateral_tiled_kernel", "blur_bilateral_generic_kernel", "blur_conv_tiled_kernel",
 * "blur_conv_generic_kernel", "blur_sep_down_tiled_kernel", "blur_sep_down_generic_kernel",
 * "blur_resize_tiled_kernel", "blur_resize_generic_kernel", "blur_warp_tiled_kernel", "blur_warp_generic_kernel",
 * "blur_warp_persp_tiled_kernel", "blur_warp_persp_generic_kernel", "blur_remap_tiled_kernel",
 * "blur_remap_generic_kernel", "blur_area_tiled_kernel", "blur_area_generic_kernel", "blur_color_tiled_kernel",
 * "blur_color_generic_kernel", "blur_hist_tiled_kernel", "blur_hist_generic_kernel", "blur_tone_table_kernel",
 * "blur_tables_tiled_kernel", "blur_tables_generic_kernel", "blur_arith_flat_kernel", "blur_arith_plane_kernel",
 * "blur_arith_generic_kernel", "blur_integral_tiled_kernel", "blur_integral_generic_kernel", "blur_box_tiled_kernel",
 * "blur_box_generic_kernel", "blur_dist_tiled_kernel", "blur_dist_generic_kernel", "blur_clahe_tables_tiled_kernel",
 * "blur_clahe_tables_generic_kernel", "blur_clahe_apply_tiled_kernel", "blur_clahe_apply_generic_kernel"; "" before the first):
 * reports name the kernel a profiler will show.  Static string, never NULL. */
const char *mi_blur_last_kernel(void);

/* Kernel tuning knobs (A/B benching and tests; defaults are the shipped configuration).  PROCESS-WIDE: a call
 * publishes a new set of knobs that every launch issued afterwards (by any context, any thread) takes a coherent
 * copy of; a launch racing with the call uses the old set or the new one, never a mix.
 *   "stage_dma"        1 = stage LDS tiles with global_load_lds (default), 0 = through VGPRs
 *   "rows_per_thread"  0 (default: chosen per launch from the grid size) | 4 | 8 | 16 output rows per thread
 *   "xcd_remap"        1 = XCD-aware blockIdx->tile map (default), 0 = identity
 *   "xcd_run"          which XCD-aware map: 0 | 1 (default) one contiguous eighth of the launch's tiles per XCD |
 *                      r >= 2 runs of r consecutive tiles dealt to the XCDs in turn
 *   "experiment"       1 = the tiled kernel's other row-pass form (field pairs straight from the raw window for 3x3,
 *                      split-then-shift for 5x5; C = 3 only) — A/B runs
 *   "stream_updown"    streaming variant: 1 (default) = odd bands march upwards (both readers of a band seam come at the
 *                      same time: fewer HBM re-reads), 0 = every band downwards
 *   "row_shuffle"      1 = x-neighbour bytes by DPP wave shifts (LDS only at wave/tile edges), 0 = from LDS (default)
 *   "prefer_stream"    1 = AUTO picks the streaming variant instead of the tiled one (default 0)
 *   "prefer_direct"    AUTO and the direct (LDS-free) variant: 0 never | 1 (default) where it measured faster: every 5x5
 *                      launch and 3x3 launches of up to 128 MiB of output | 2 for every eligible shape
 *   "stream_band_rows" streaming variant: output rows per wave (0 = chosen per launch)
 *   "ragged_tiled"     1 (default) = rows that are not a multiple of 16 bytes / unaligned pointers take the ragged form of the
 *                      tiled kernel; 0 = they take the generic one-byte-per-thread kernel
 *   "zero_copy"        1 (default) = submits whose input AND output are pinned host memory run the kernel on the
 *                      caller's buffers in place (no staging copies); 0 = always H2D -> kernel -> D2H
 *   "zero_copy_server"  1 (default) = zero-copy submits of aligned shapes go through the context's BATCH SERVER: one long-lived
 *                      dispatch (blur_server_kernel) takes batch after batch from a descriptor ring in pinned memory, hands the
 *                      tiles out through one ticket counter that runs through the batches and signals each complete batch
 *                      into host memory — no launch per batch, and no batch waiting for its unluckiest workgroup (+27 % images/s
 *                      end to end at batch 35, profiles/r03_e2e_timeline.md); 0 = one capped launch per batch (the two knobs below)
 *   "zero_copy_workers" 48 (default): the server's worker workgroups (read when a context's server is made)
 *   "zero_copy_idle_us" 300 (default): a server leaves after this long without a new batch (the next submit starts one)
 *   "zero_copy_budget"  256 (default): ... and after this many batches; the next one, already queued behind it, carries on
 *   "zero_copy_tickets" 1 (default) | 0 = a fixed share of tiles per worker (A/B runs: what a per-batch launch does)
 *   "resident_place_trials" 4 (default): see mi_blur_resident_alloc
 *   "zero_copy_spin"    0 (default) = a wait for a batch of the server spins ~20 us, then sleeps in 20 us steps (the core is
 *                      free for the threads that build the next batch); 1 = spin + yield only
 *   "zero_copy_server_min_kb"  1280 (default): in-place submits whose output is smaller than this many KiB take one launch each
 *                       instead of the server — its hand-off costs ~26 us per batch against ~8 us for a launch (a single 256x256
 *                       frame per submit: 126 k against 40 k img/s); 0 = always the server
 *   "staged_server"    1 (default) | 0: submits of PAGEABLE caller memory (the reference's malloc'd batch buffers) are gathered into
 *                       the slot's pinned staging and blurred there in place by the batch server (staging in -> staging out over the
 *                       link, 220 k img/s at batch 35 and 500) instead of a DMA copy each way around a launch (120-158 k).
 *                       MI_BLUR_STAGING_THREADS (default 8) = host threads of the gather / scatter
 *   "zero_copy_trace"   0 (default) | 1 = the server's workers stamp their phases (mi_blur_debug_zc_trace)
 *   "zero_copy_debug_base"  test hook, 0 (default) | n: a context's server starts n batches / 7n tiles short of 2^32, so the
 *                       wrap of its 32-bit batch and tile numbers (80 minutes into a continuous stream) is reached at once
 *   "zero_copy_events"  1 (default) | 0 = per-batch launches carry no timestamp events (timing experiment; no kernel bucket)
 *   "zero_copy_streams" 4 (default): zero-copy submits of a context alternate over this many of its streams (at most n_slots)
 *   "zero_copy_blocks"  24 (default): zero-copy launches of the aligned tiled kernel keep at most this many workgroups
 *                      resident, each looping over tiles (0 = one workgroup per tile).  The host link needs ~100 KB in
 *                      flight; a launch that puts every tile on the chip at once reads everything, then writes
 *                      everything (half duplex).  4 x 24 workgroups, each on its own read/compute/write cycle, keep both
 *                      directions busy: +10-18 % images/s end to end (profiles/r02_e2e.txt)
 *   "fused_window"     8 (default): the fused stream takes its tiles window by window, a window being this many consecutive
 *                      batches dealt over the XCDs (8 = one whole batch per XCD); the batches of a window complete at about
 *                      the same time, windows in stream order.  1 = batch by batch
 *   "fused_tail"       30 (default; MI_BLUR_FUSED_TAIL in the environment): per mille of a fused pass's tiles that are handed out
 *                      by ticket to spare workgroups at the end of the grid instead of being mapped to workgroups, so that an
 *                      XCD that runs ahead takes more of them (passes of >= 8192 tiles; -1.3..1.8 % per pass).  0 = static map
 *   "fused_tail_blocks" 25 (default): spare workgroups beyond the number of tail tiles, per cent
 *   "fused_overlap"    30 (default; MI_BLUR_FUSED_OVERLAP in the environment) | 0 .. 500: consecutive fused passes that take the
 *                      dynamic tail (whole-chunk rows, no watcher, same shape and batch) alternate between the context's first
 *                      stream and a second one, and a pass starts when its predecessor has this many per mille of its tiles
 *                      left to hand out instead of after its last workgroup has ended: the drain of one pass and the ramp of
 *                      the next share the chip.  The predecessor stores its number in a gate word when it gets there; a one-wave
 *                      kernel in front of the next pass waits for that (at most 10 s, then the pass runs anyway).  Outputs,
 *                      counters and what mi_blur_resident_batches_done reports do not depend on it; a pass's own start-to-stop
 *                      time gets longer by about the overlap (profiles/r09_fused_overlap.md).  0 = every pass on one stream
 *   "fused_release"    0 (default) | 1: how a block of the fused stream publishes "my outputs are in memory" — see
 *                      mi_blur_resident_run_fused
 *   "integral_band"    16 (default) | 1 .. 256: rows per band of blur_integral_tiled_kernel (A/B runs; the work buffer's size
 *                      follows it: mi_blur_integral_work_bytes and mi_blur_box_work_bytes answer for the value in force)
 *   "box_bytes"        4 (default) | 16: consecutive output bytes of a row that a thread of blur_box_tiled_kernel owns (A/B
 *                      runs): with 4 a wave's 16-byte loads of a table row are contiguous, with 16 they lie 64 bytes apart
 *   "dist_band"        32 (default) | 1 .. 256: rows per band of the distance transform's column pass (A/B runs; the work
 *                      buffer's size follows it: mi_blur_dist_work_bytes answers for the value in force)
 *   "dist_chunk_log2"  4 (default) | 3 | 5: blur_dist_tiled_kernel keeps one minimum per 2^v columns of a staged row and
 *                      skips a chunk whose minimum cannot beat the best distance so far (A/B runs)
 *   "match_tiled"      1 (default) | 0: SQDIFF, CCORR and SAD launches that blur_match_tiled_kernel can take go to it; 0 sends
 *                      every launch to blur_match_generic_kernel (tests and A/B runs) */
int mi_blur_set_option(const char *key, int value);

/* Number of visible HIP devices (0 is a valid answer: CPU-device contexts still work).
 * Replaces the platform/device scan, heterogeneous_blur.c:142-184. */
int mi_blur_device_count(void);

/* ------------------------------------------------------------------------
 * Kernel level — replaces clSetKernelArg x5 + clEnqueueNDRangeKernel
 * (heterogeneous_blur.c:380-389,525; split_image_blur.c:407-418,533).
 *
 * d_in/d_out are DEVICE pointers on the current HIP device, n_images images laid
 * end to end (image stride = width*height*channels).  One launch blurs the whole
 * batch.  `stream` is a hipStream_t (NULL = default stream).  Asynchronous.
 * ---------------------------------------------------------------------- */
int mi_blur_enqueue(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels,
                    int radius, int n_images, void *stream);

/* Band form (Approach 2, split_image_blur.c:401,414,511-541): the input is a
 * band of `band_rows` rows (clamping happens at the band's own first/last row,
 * exactly as when the reference passes the sub-buffer height as `height`);
 * only output rows [out_row_begin, out_row_end) of the band are produced and
 * are written to d_out starting at d_out[0] (the halo rows the reference
 * computes and then drops at read-back, :526,537, are never computed). */
int mi_blur_enqueue_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                         int radius, int out_row_begin, int out_row_end, void *stream);

/* Full-control form used by the tests: variant selection; n_images bands. */
int mi_blur_enqueue_ex(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                       int radius, int n_images, int out_row_begin, int out_row_end,
                       int variant, void *stream);

/* ------------------------------------------------------------------------
 * Queue level — one context = one device + its in-order stream(s), pinned
 * staging slots, device buffers and event timing.  Replaces context/queue/
 * buffer creation (heterogeneous_blur.c:194-212,341-354), the per-image
 * Write/NDRange/Read triple (:502-533), clFinish (:538-539) and the event
 * bookkeeping (:544-579).
 * ---------------------------------------------------------------------- */
typedef struct mi_blur_ctx mi_blur_ctx;

typedef struct mi_blur_timing {      /* cumulative since create / last reset; mirrors :411-412 */
    double h2d_ms;                   /* transfer IN  (time_*_transfer_in)  */
    double kernel_ms;                /* kernel       (time_*_kernel); zero-copy submits that overlap count the time at
                                        least one of them was executing, not the sum of their durations */
    double d2h_ms;                   /* transfer OUT (time_*_transfer_out) */
    uint64_t bytes_h2d, bytes_d2h;
    uint64_t bytes_alg;              /* algorithmic bytes = 2*W*rows*C per image processed; for a context with
                                        mi_blur_ctx_set_sep_down, mi_blur_ctx_set_resize or mi_blur_ctx_set_warp: input bytes + output bytes, W*H*C + Wo*Ho*C per image */
    uint64_t images;
    uint64_t launches;
} mi_blur_timing;

/* device: HIP ordinal, or MI_BLUR_DEVICE_CPU (n_threads host threads; 0 = all cores, at most 16 — ask for more by number).
 * max_batch: largest n_images of one submit.  n_slots: submits in flight (>=1).  Staged submits: 2-3 lets H2D(n+1),
 * kernel(n) and D2H(n-1) overlap.  In-place (pinned) submits through the batch server: a deeper queue costs the link
 * nothing and keeps the GPU fed while the host builds the next batch — the hosts use 4 (3 in split_image_blur).  Each
 * slot owns one stream and — made by the first submit that needs them, so never for a context whose submits are all in
 * place — a pinned in/out staging pair and a device in/out pair of max_batch images each. */
int mi_blur_create(mi_blur_ctx **out_ctx, int device, int width, int height, int channels,
                   int radius, int max_batch, int n_slots, int n_threads);
void mi_blur_destroy(mi_blur_ctx *ctx);

/* Page-locked, device-visible host memory for stream buffers.  When both buffers of a submit come
 * from here (or are otherwise pinned) the kernel works on them in place over PCIe — the counterpart of
 * CL_MEM_USE_HOST_PTR on the reference's shared-memory iGPU, and the fastest end-to-end form on this
 * platform; the h2d/d2h buckets of such a submit are ~0 and the transfer time is inside kernel_ms.
 * Such submits are batches of the context's batch server (see "zero_copy_server"): the submit publishes a descriptor,
 * mi_blur_wait_oldest / mi_blur_sync spin on the batch's completion word in host memory.
 * With only one side pinned, or "zero_copy" off, submit() DMA-copies straight from/to pinned memory;
 * ordinary (pageable) caller memory is accepted too and goes through the slot's own pinned staging
 * buffers (one extra host memcpy each way). */
void *mi_blur_host_alloc(size_t bytes);
void mi_blur_host_free(void *p);

/* Pin the caller's OWN buffers in place (hipHostRegister): a host that keeps its malloc'd batch buffers
 * (heterogeneous_blur.c:431-432, hoisted out of the batch loop) gets the in-place path of mi_blur_host_alloc memory without
 * changing its allocator.  The range must stay allocated until mi_blur_host_unregister; registering costs ~1 ms per 10 MB,
 * so do it once, not per batch.  Without a GPU both calls succeed and do nothing. */
int mi_blur_host_register(void *p, size_t bytes);
int mi_blur_host_unregister(void *p);

/* NUMA placement of per-GPU host work.  The reference drives both of its devices from one host thread of a one-socket
 * desktop (heterogeneous_blur.c:482-539); an 8-GPU node has two sockets with four GPUs each, and a feeder thread, a
 * batch-building memcpy (:439-442) or a pinned batch buffer on the other socket puts every byte of the stream on the
 * inter-socket link first.  No libnuma involved: hipDeviceGetPCIBusId -> /sys/bus/pci/devices/<bdf>/local_cpulist ->
 * sched_setaffinity.  MI_BLUR_NO_AFFINITY=1 in the environment turns the two binding calls into no-ops.
 *   mi_blur_device_cpulist         the GPU's local CPU list as sysfs spells it ("0-63,128-191") and its NUMA node
 *                                  (-1 if unknown); MI_BLUR_ERR_UNSUPPORTED when sysfs does not say
 *   mi_blur_bind_thread_to_device  restrict the CALLING thread (and threads it starts afterwards) to the GPU's local CPUs
 *                                  that its current mask allows; returns how many CPUs that is, 0 = nothing was changed
 *                                  (disabled, unknown topology, or no allowed CPU on that socket)
 *   mi_blur_host_alloc_on          mi_blur_host_alloc with `device` current and the calling thread on that GPU's socket for
 *                                  the duration of the call: the buffers of GPU g's feeder belong on GPU g's node */
int mi_blur_device_cpulist(int device, char *buf, size_t n, int *numa_node);
int mi_blur_bind_thread_to_device(int device);
void *mi_blur_host_alloc_on(int device, size_t bytes);

/* Asynchronous H2D -> ONE batched launch -> D2H of n_images images from caller
 * memory.  host_in/host_out must stay valid until mi_blur_sync (the reference
 * frees batch_input/batch_output only after clFinish, heterogeneous_blur.c:538,596-597).
 * Blocks only when every slot is still in flight. */
int mi_blur_submit(mi_blur_ctx *ctx, const uint8_t *host_in, uint8_t *host_out, int n_images);

/* Approach 2: host_in points at the first row of a band of band_rows rows that
 * already includes halo_top/halo_bottom halo rows; host_out receives the
 * band_rows-halo_top-halo_bottom interior rows (split_image_blur.c:511-541).
 * band_rows may differ per call but must be <= the context's height. */
int mi_blur_submit_band(mi_blur_ctx *ctx, const uint8_t *host_in, uint8_t *host_out,
                        int band_rows, int halo_top, int halo_bottom);

/* Approach 2 for a whole batch: the SAME band (rows [r, r+band_rows) incl. halos) of n_images
 * images that lie host_image_stride bytes apart in caller memory (the contiguous batch stream
 * of split_image_blur.c:469-480).  host_in points at the band's first row in image 0, host_out
 * at the band's first OUTPUT row in image 0 (same stride).  One 2-D DMA gathers the bands, one
 * launch blurs them, one 2-D DMA scatters the interior rows back — instead of the reference's
 * per-image Write/NDRange/Read on each device (:520-541). */
int mi_blur_submit_bands(mi_blur_ctx *ctx, const uint8_t *host_in, uint8_t *host_out, int n_images,
                         size_t host_image_stride, int band_rows, int halo_top, int halo_bottom);

/* Frames as the reference's loader hands them over — PLANAR, byte (x, y, c) of frame i at (i*C + c)*W*H + y*W + x (CImg
 * storage; the reference interleaves each frame on one host core, heterogeneous_blur.c:125-134, and de-interleaves to
 * save, split_image_blur.c:40-56).  Same contract as mi_blur_submit, with both repacks done by the GPU inside the
 * submit: the repack-in kernel reads the planar frames over the host link (pinned caller memory is read in place) and
 * writes the interleaved batch to HBM, the blur runs HBM -> HBM, and host_out receives interleaved frames
 * (planar_out = 0) or planar ones (planar_out != 0; written straight into pinned caller memory by the repack-out
 * kernel).  h2d_ms / d2h_ms of such a submit are the repack-in / copy-or-repack-out durations. */
int mi_blur_submit_planar(mi_blur_ctx *ctx, const uint8_t *host_planar_in, uint8_t *host_out, int n_images, int planar_out);

/* Block until the OLDEST submit still in flight has finished (its output is in caller memory).
 * Lets a host rotate n_slots batch buffers: refill the oldest while the newer ones run. */
int mi_blur_wait_oldest(mi_blur_ctx *ctx);

/* clFinish + event harvest (heterogeneous_blur.c:538-579).  timing may be NULL. */
int mi_blur_sync(mi_blur_ctx *ctx, mi_blur_timing *timing);
void mi_blur_reset_timing(mi_blur_ctx *ctx);
/* Non-blocking: the buckets of the submits harvested so far (by wait_oldest / sync).  A host that rotates
 * batch buffers reads it after each mi_blur_wait_oldest to get that batch's device times — what the
 * reference prints once per run (heterogeneous_blur.c:541-579) becomes available per batch, which is
 * what continuous CPU/GPU rebalancing needs (`both auto`). */
int mi_blur_get_timing(mi_blur_ctx *ctx, mi_blur_timing *timing);
/* How many of the context's submits so far were blurred in place over the host link: pinned caller buffers (see
 * mi_blur_host_alloc), and pageable ones by way of the slot's pinned staging ("staged_server", default on). */
uint64_t mi_blur_zero_copy_launches(mi_blur_ctx *ctx);

/* ------------------------------------------------------------------------
 * Frame layout on the device.  CImg (the reference's image loader) stores frames
 * PLANAR — byte (x, y, c) of image i at (i*C + c)*W*H + y*W + x — and the
 * reference repacks each frame to the interleaved stream on one host core
 * (heterogeneous_blur.c:125-134; back again to save, split_image_blur.c:40-56).
 * These do the same repack for n_images frames in one HBM pass each way.
 * Buffers are device (or pinned host) memory, distinct, n_images*W*H*C bytes.
 * (No repack at all is needed to BLUR planar frames: a planar stream is a stream
 * of n_images*C one-channel images — mi_blur_enqueue(..., channels = 1, n*C).)
 * ---------------------------------------------------------------------- */
int mi_blur_planar_to_interleaved(const uint8_t *d_planar, uint8_t *d_interleaved, int width, int height,
                                  int channels, int n_images, void *stream);
int mi_blur_interleaved_to_planar(const uint8_t *d_interleaved, uint8_t *d_planar, int width, int height,
                                  int channels, int n_images, void *stream);

/* ------------------------------------------------------------------------
 * Device-resident stream (no reference analogue: the reference re-uploads
 * every image).  The pool holds pool_images images in HBM (in + out).
 * ---------------------------------------------------------------------- */
/* Pools of 128 MiB .. 8 GiB are PLACED: where a pool lands in HBM moves the big launches between two levels ~6 % apart
 * (profiles/r03_placement_channels.txt: same requests per channel, 1.5x the read DRAM-credit stalls on the slow placements),
 * nothing in the address tells which, and a placement keeps its level while it lives — so "resident_place_trials" (default 4;
 * MI_BLUR_PLACE_TRIALS in the environment; 0/1 = off) candidate inputs and as many candidate outputs are allocated side by
 * side, every (input, output) pair is timed on the context's kernel over the whole pool (after a clock ramp), the fastest
 * pair is kept, the other buffers are freed (~0.15 s, once per pool).  mi_blur_resident_placement reports the pairs'
 * per-launch ms (row-major: input i, output j at i*n + j) and which one was kept. */
int mi_blur_resident_alloc(mi_blur_ctx *ctx, int pool_images);
int mi_blur_resident_placement(mi_blur_ctx *ctx, float *ms, int max_n, int *kept);
/* Fill pool image i with the synthetic LCG image (seed 0x9E3779B9 ^ (first_index+i)). */
int mi_blur_resident_fill_synthetic(mi_blur_ctx *ctx, int first_index);
int mi_blur_resident_upload(mi_blur_ctx *ctx, int pool_index, const uint8_t *host_in, int n_images);
int mi_blur_resident_download(mi_blur_ctx *ctx, int pool_index, uint8_t *host_out, int n_images);
void *mi_blur_resident_in(mi_blur_ctx *ctx);       /* device pointers of the pool */
void *mi_blur_resident_out(mi_blur_ctx *ctx);

/* One pass of the image stream over the resident pool: n_images images taken
 * cyclically from the pool, one launch per `batch` images (the last launch takes
 * the remainder, heterogeneous_blur.c:423-427).  Launches go round-robin over the
 * context's streams.  Every timed_every-th launch of the pass (0 = none, 1 = all)
 * carries the dispatch's own start/stop timestamps (the HIP analogue of
 * clGetEventProfilingInfo); their durations accumulate into the context's
 * kernel_ms and mi_blur_timed_coverage says how many launches/bytes that covers.
 * (Timestamped launches cost the host ~3x an ordinary launch, so a small-batch
 * stream is sampled rather than timed in full.)  Asynchronous; follow with mi_blur_sync. */
int mi_blur_resident_run(mi_blur_ctx *ctx, int n_images, int batch, int timed_every);
void mi_blur_timed_coverage(mi_blur_ctx *ctx, uint64_t *launches, uint64_t *bytes_alg);

/* The same pass as ONE dispatch ("fused stream").  A batch-35 stream issued launch by launch is bound by the
 * GPU's per-dispatch processing (~3.5 us each over 4 hardware queues), not by the kernel; here the kernel walks
 * the batches itself — blocks ordered in windows of 8 batches, in stream order — and every workgroup counts itself into its batch's counter once
 * its outputs are in memory.  The batch stays the unit of COMPLETION (mi_blur_resident_batches_done reads the
 * counters and returns how many leading batches have their outputs ready, without waiting for the dispatch, which
 * may still be running) without being the unit of DISPATCH.  n_images <= pool size (one contiguous run of the pool); 1-4 channels, rows of
 * at least 16 bytes — rows that are a multiple of 16 bytes take the aligned tiles, any other width their ragged form
 * (MI_BLUR_ERR_UNSUPPORTED otherwise).  `timed` is a bit set: 1 = the dispatch carries timestamp events like resident_run;
 * 2 = WATCH this pass: a one-wave kernel on the context's second stream (never the pass's own) follows the counters and keeps "leading batches complete" in
 * pinned host memory, so that mi_blur_resident_batches_done is a read of the caller's own memory (tens of ns, no HIP call)
 * instead of a counter read-back (~18 us) — for hosts that consume batch by batch while the pass runs.
 * Asynchronous; follow with mi_blur_sync.
 *
 * Ordering of "counted" against "readable".  Default ("fused_release" 0): outputs are stored write-through
 * (global_store ... sc1), every wave drains its stores (s_waitcnt vmcnt(0)), the block meets at a barrier and one lane
 * adds to the counter with a relaxed agent-scope atomic.  That a batch's outputs are in memory once its count is
 * visible is MEASURED behaviour of gfx950 / ROCm 7.2 (MI355X_MICROARCH.md, cross-XCD hand-off table), not an
 * architectural guarantee of the memory model; tests/test_gpu_parity.py checks it mid-dispatch.  "fused_release" 1
 * makes the add a release at agent scope — the architectural form, ~6x slower per pass (an L2 write-back per block). */
int mi_blur_resident_run_fused(mi_blur_ctx *ctx, int n_images, int batch, int timed);
/* >= 0: how many LEADING batches of the latest fused pass are complete.  NEGATIVE: a mi_blur_status — the counters
 * could not be read (failed copy, faulted device); a polling loop must stop on it, it will not recover by itself. */
int mi_blur_resident_batches_done(mi_blur_ctx *ctx);
/* Copy out outputs of batches already reported done, without waiting for the dispatch that is still producing the
 * later ones (mi_blur_resident_download waits for the whole device). */
int mi_blur_resident_peek(mi_blur_ctx *ctx, int pool_index, uint8_t *host_out, int n_images);

/* ------------------------------------------------------------------------
 * CPU device kernel, exposed for the hosts' `cpu` mode and for timing the
 * host-core path beside the GPU (BASELINE.json config 0).  Scalar per-pixel
 * integer form of gaussian_kernel.cl:19-72, n_threads host threads over images
 * (over row bands when n_images < n_threads).  Synchronous.
 * ---------------------------------------------------------------------- */
int mi_blur_cpu_run(const uint8_t *in, uint8_t *out, int width, int height, int channels,
                    int radius, int n_images, int n_threads);

/* ------------------------------------------------------------------------
 * Separable integer kernels of any radius up to 16 (Gaussian of any sigma, anisotropic included; no reference
 * analogue).  Per axis: radius rx / ry in 0..16, non-negative taps wx[2rx+1] / wy[2ry+1] summing to 2^bx / 2^by,
 * 0 <= bx, by <= 8 (unused tap slots are ignored).  Clamp-to-edge, exact integer arithmetic, one truncating shift:
 *   out[y][x][c] = ( sum_j wy[j] * sum_i wx[i] * in[clamp(y+j-ry)][clamp(x+i-rx)][c] ) >> (bx + by)
 * so wx = wy = {1,2,1} (2 + 2) is exactly the radius-1 kernel above and {1,4,6,4,1} (4 + 4) exactly radius 2.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_SEP_MAX_RADIUS 16
typedef struct mi_blur_sep_kernel {
    int rx, ry, bx, by;
    uint16_t wx[2 * MI_BLUR_SEP_MAX_RADIUS + 1], wy[2 * MI_BLUR_SEP_MAX_RADIUS + 1];
} mi_blur_sep_kernel;

/* Integer Gaussian taps.  r = radius, or ceil(3 sigma) clamped to [1,16] when radius is 0; w_i = exp(-i^2/(2 sigma^2))
 * (double), t_i = floor(w_i * 2^bits / sum w + 0.5), the centre tap absorbs 2^bits - sum t, outer tap pairs that are both 0
 * are dropped.  taps receives 2*r'+1 values, *radius_out the effective radius r'.  bits 0..8 (8 is the usual choice).
 * MI_BLUR_ERR_INVALID: sigma <= 0, radius outside 0..16, bits outside 0..8, or a centre tap that is not positive. */
int mi_blur_gauss_taps(double sigma, int radius, int bits, uint16_t *taps, int *radius_out);
/* Both axes: sigma_y <= 0 means sigma_y = sigma_x; radius (0 = automatic) applies to each axis, each trimmed on its own. */
int mi_blur_sep_kernel_gauss(double sigma_x, double sigma_y, int radius, int bits, mi_blur_sep_kernel *k);

/* mi_blur_enqueue / mi_blur_enqueue_band with a separable kernel (same buffers, same band semantics; asynchronous).
 * Rows of whole 16-byte chunks at 16-byte aligned addresses with 1-4 channels take the LDS-tiled two-pass kernel
 * (blur_sep_tiled_kernel), every other shape the one-byte-per-thread kernel (blur_sep_generic_kernel). */
int mi_blur_enqueue_sep(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                        const mi_blur_sep_kernel *k, void *stream);
int mi_blur_enqueue_sep_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                             int out_row_begin, int out_row_end, const mi_blur_sep_kernel *k, void *stream);
/* mi_blur_cpu_run with a separable kernel. */
int mi_blur_cpu_run_sep(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                        const mi_blur_sep_kernel *k, int n_threads);
/* Give a context a separable kernel in place of the radius it was created with.  Only before its first submit
 * (MI_BLUR_ERR_STATE after).  Every submit form then uses it (mi_blur_submit, _band, _bands, _planar; pinned or pageable
 * memory; GPU or CPU device); such submits never go through the batch server (one launch per submit instead), and
 * the resident runs (mi_blur_resident_run, _run_fused) return MI_BLUR_ERR_UNSUPPORTED.  The context keeps a copy. */
int mi_blur_ctx_set_kernel(mi_blur_ctx *ctx, const mi_blur_sep_kernel *k);

/* ------------------------------------------------------------------------
 * Decimating separable filter: low-pass and subsample in one pass (pyramid level, area downscale; no reference
 * analogue).  Let F be the separable filter of mi_blur_enqueue_sep for the taps k on the whole W x H image (clamp-to-edge,
 * exact integers, one truncating shift).  A decimation keeps column ox + X*sx and row oy + Y*sy of it:
 *   Wo = (W - ox + sx - 1) / sx        Ho = (H - oy + sy - 1) / sy
 *   out[Y][X][c] = F(in)[oy + Y*sy][ox + X*sx][c]        0 <= X < Wo, 0 <= Y < Ho
 * The output is interleaved and dense: its pitch is Wo*C and images lie Wo*Ho*C bytes apart.  It is byte-identical to
 * "filter, then subsample", and the GPU and the CPU device agree byte for byte; only the kept outputs are computed.
 * Valid: 1 <= sx, sy <= MI_BLUR_DECIMATE_MAX, 0 <= ox < sx, 0 <= oy < sy, ox < W and oy < H (the output is never empty);
 * k has the rules of mi_blur_sep_kernel.  sx = sy = 1 gives exactly the bytes of mi_blur_enqueue_sep.
 * This is NOT OpenCV's pyrDown bit for bit: edges clamp here instead of reflecting, and the shift truncates instead of
 * rounding.  The taps and the sampling grid of MI_BLUR_DOWN_PYR are pyrDown's.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_DECIMATE_MAX 4
typedef struct mi_blur_decimation { int sx, sy, ox, oy; } mi_blur_decimation;   /* keep column ox + X*sx, row oy + Y*sy */

/* Wo and Ho of a width x height image under *d.  MI_BLUR_ERR_INVALID: a null pointer, width or height <= 0, or a
 * decimation that is not valid for that size. */
int mi_blur_decimated_size(int width, int height, const mi_blur_decimation *d, int *out_width, int *out_height);

typedef enum mi_blur_down_preset_id {
    MI_BLUR_DOWN_PYR = 0,            /* taps {1,4,6,4,1} on both axes, stride 2, offset 0: one pyramid level */
    MI_BLUR_DOWN_AREA2 = 1,          /* taps {0,1,1}, stride 2, offset 0: the mean of each 2x2 block, >> 2 */
    MI_BLUR_DOWN_AREA4 = 2           /* taps {0,0,0,1,1,1,1}, stride 4, offset 0: the mean of each 4x4 block, >> 4 */
} mi_blur_down_preset_id;
int mi_blur_sep_down_preset(int preset, mi_blur_sep_kernel *k, mi_blur_decimation *d);

/* mi_blur_enqueue_sep that writes only the kept outputs: n_images images of width x height in, n_images images of
 * Wo x Ho out (device memory, asynchronous; n_images == 0 is MI_BLUR_OK).  Every argument is checked before a device
 * is asked for: MI_BLUR_ERR_INVALID comes before MI_BLUR_ERR_NO_DEVICE.
 * blur_sep_down_tiled_kernel (LDS tile, vertical pass over the kept rows only, horizontal pass at the kept columns) takes
 * exactly the launches with sx = sy = 2 (either phase on either axis), 1-4 channels, width*channels a multiple of 32 (so
 * input rows and output rows are whole 16-byte chunks) and both pointers 16-byte aligned (and, where a context's in-place
 * submit gives image strides, strides that are multiples of 16; this export's are dense, which they then are); every other launch goes to
 * blur_sep_down_generic_kernel (one output byte per thread).  mi_blur_last_kernel() says which one ran. */
int mi_blur_enqueue_sep_down(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                             const mi_blur_sep_kernel *k, const mi_blur_decimation *d, void *stream);
/* The same on the CPU device's threads (synchronous), computing only kept rows and kept columns. */
int mi_blur_cpu_run_sep_down(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                             const mi_blur_sep_kernel *k, const mi_blur_decimation *d, int n_threads);
/* Give a context (created with the INPUT width, height, channels) the decimating filter, with the rules of
 * mi_blur_ctx_set_kernel: only before the first submit (MI_BLUR_ERR_STATE after); it replaces what another setter set
 * and is replaced by them; the context keeps a copy.  MI_BLUR_ERR_INVALID also when *d is not valid for the context's
 * size.  mi_blur_submit then writes n_images * Wo*Ho*C bytes to host_out: pageable caller memory, or pinned memory on
 * both sides (in place, one launch per submit, never the batch server), on the GPU or the CPU device.  There are no
 * band forms (a band's phase would depend on where it starts in the image): mi_blur_submit_band, _bands, _planar and
 * both resident runs return MI_BLUR_ERR_UNSUPPORTED for such a context. */
int mi_blur_ctx_set_sep_down(mi_blur_ctx *ctx, const mi_blur_sep_kernel *k, const mi_blur_decimation *d);

/* ------------------------------------------------------------------------
 * Image resize: exact fixed-point bilinear and nearest, any output size (no reference analogue).  The definition is
 * exact integers; the GPU, the CPU device and a numpy restatement agree byte for byte.
 *
 * One axis with n_in input samples and n_out output samples uses pixel centres aligned (half-pixel mapping).  For
 * output index X:
 *   num = (2*X + 1) * n_in - n_out          den = 2 * n_out
 *   i0  = floor(num / den)                  (floor towards minus infinity; i0 >= -1)
 *   rem = num - i0 * den                    (0 <= rem < den)
 *   f   = (rem * 2048 + n_out) / den        (0 .. 2048: the fraction rounded to 11 bits)
 *   a   = clamp(i0, 0, n_in - 1)            b = clamp(i0 + 1, 0, n_in - 1)
 *
 * MI_BLUR_RESIZE_BILINEAR, with (xa, xb, fx) from the x axis and (ya, yb, fy) from the y axis, per channel:
 *   s   = (2048-fy) * ((2048-fx) * in[ya][xa] + fx * in[ya][xb])
 *       +       fy  * ((2048-fx) * in[yb][xa] + fx * in[yb][xb])
 *   out = (s + (1 << 21)) >> 22
 * s is at most 255 * 2^22 and the row blends at most 255 * 2^11, so everything fits in 32 bits unsigned.  The order of
 * the two passes cannot change the value.  n_out == n_in gives rem = 0, so the launch is an identity.  A constant image
 * stays constant.  The result differs from real-valued bilinear by less than 0.5 + 2*255/4096 ~ 0.63, so it is never
 * more than 1 from the exact value rounded half up.
 *
 * MI_BLUR_RESIZE_NEAREST: i = ((2*X + 1) * n_in) / den.  This is the input pixel whose cell contains the output
 * pixel's centre.  It is always in range, so it needs no clamp.
 *
 * Valid: 1 <= out_width, out_height; width, height, out_width, out_height each <= MI_BLUR_RESIZE_MAX_DIM = 32768, so
 * num and rem * 2048 stay inside 32 bits; the per-image byte limits of a launch (W*C <= INT_MAX/2, W*C*H <= INT_MAX)
 * apply to both the input image and the output image.  Any ratio is valid.
 * This is NOT OpenCV's INTER_LINEAR bit for bit: the grid and the 11 fraction bits are the same, but the rounding is a
 * single final one.  A reduction by more than 2x aliases (bilinear reads 2 x 2 input pixels whatever the ratio):
 * mi_blur_enqueue_sep_down's area_down / pyr_down presets should come first for such reductions, or the reduction
 * be an area resize (mi_blur_enqueue_area, below), which is anti-aliased at every ratio.
 * The output is interleaved and dense: its pitch is Wo*C and images lie Wo*Ho*C bytes apart.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_RESIZE_MAX_DIM 32768
typedef enum mi_blur_resize_mode { MI_BLUR_RESIZE_NEAREST = 0, MI_BLUR_RESIZE_BILINEAR = 1 } mi_blur_resize_mode;
typedef struct mi_blur_resize { int out_width, out_height, mode; } mi_blur_resize;

/* (a, b, f) of one axis for output index X, through the same function the kernels and the CPU device use; NEAREST
 * gives i, i, 0.  MI_BLUR_ERR_INVALID: a null pointer, n_in or n_out outside 1..MI_BLUR_RESIZE_MAX_DIM, an unknown mode,
 * X outside [0, n_out). */
int mi_blur_resize_coord(int n_in, int n_out, int mode, int X, int *i0, int *i1, int *frac);

/* n_images images of width x height in, n_images images of r->out_width x r->out_height out (device memory,
 * asynchronous; n_images == 0 is MI_BLUR_OK; image offsets are 64-bit).  Every argument is checked before a device is
 * asked for: MI_BLUR_ERR_INVALID comes before MI_BLUR_ERR_NO_DEVICE.
 * blur_resize_tiled_kernel (LDS tile of the input footprint, index tables in LDS, vertical blend, horizontal gather)
 * takes exactly the launches with BILINEAR mode, 1-4 channels, out_width >= width and out_height >= height
 * (enlargement or equality on both axes), width*channels and out_width*channels multiples of 16 (input and output
 * rows are whole 16-byte chunks) and both pointers 16-byte aligned (and, where a context's in-place submit gives image
 * strides, strides that are multiples of 16; this export's are dense, which they then are); every other launch (NEAREST,
 * any reduction, 5+ channels, odd rows or pointers) goes to blur_resize_generic_kernel (one output byte per thread).
 * mi_blur_last_kernel() says which one ran. */
int mi_blur_enqueue_resize(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                           const mi_blur_resize *r, void *stream);
/* The same on the CPU device's threads (synchronous). */
int mi_blur_cpu_run_resize(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                           const mi_blur_resize *r, int n_threads);
/* Give a context (created with the INPUT width, height, channels) the resize, with the rules of
 * mi_blur_ctx_set_sep_down: only before the first submit (MI_BLUR_ERR_STATE after); it replaces what another setter set
 * and is replaced by them; the context keeps a copy.  MI_BLUR_ERR_INVALID also when *r is not valid for the context's
 * size.  mi_blur_submit then writes n_images * Wo*Ho*C bytes to host_out, which may be MORE than it reads: pageable
 * caller memory, or pinned memory on both sides (in place, one launch per submit, never the batch server), on the GPU
 * or the CPU device.  mi_blur_submit_band, _bands, _planar and both resident runs return MI_BLUR_ERR_UNSUPPORTED for
 * such a context. */
int mi_blur_ctx_set_resize(mi_blur_ctx *ctx, const mi_blur_resize *r);

/* ------------------------------------------------------------------------
 * Area resize: exact box-average resize to any output size, reductions up to 64x per axis (no reference analogue).
 * The anti-aliased reduction: every output pixel is the average of the input area under it, input pixels that it covers
 * partly counted by their share.  The definition is a ratio of integers with a single rounding; the GPU, the CPU device
 * and a numpy restatement agree byte for byte.
 *
 * One axis with n_in input and n_out output samples, measured in units where an input pixel is n_out long and an output
 * pixel n_in long (both images are then n_in * n_out long).  Output X covers [X*n_in, (X+1)*n_in), input i covers
 * [i*n_out, (i+1)*n_out):
 *   i_lo = floor(X*n_in / n_out)              i_hi = floor(((X+1)*n_in - 1) / n_out)
 *   w(X,i) = min((X+1)*n_in, (i+1)*n_out) - max(X*n_in, i*n_out)     for i_lo <= i <= i_hi, else 0
 * Every w in the range is positive; sum_i w(X,i) = n_in and sum_X w(X,i) = n_out; the taps between the first and the
 * last all weigh n_out, only those two are partial; there are at most ceil(n_in/n_out) + 1 taps; nothing clamps, the
 * taps always lie inside the image.
 *
 * With (wx, wy) from the two axes and D = W*H, per channel:
 *   S   = sum_j wy(Y,j) * sum_i wx(X,i) * in[j][i][c]          (<= 255 * D < 2^38: 64 bits)
 *   out = floor((2*S + D) / (2*D))                             (one rounding, half up)
 * The order of the two passes cannot change S.  Equal sizes are the identity; a constant image stays constant; an integer
 * reduction by k is the mean of every k x k block rounded half up (at k = 2 that is (sum + 2) >> 2: never below the
 * MI_BLUR_DOWN_AREA2 preset, which truncates, and at most 1 above it); an integer enlargement by k replicates pixels.  The
 * result is within 0.5 of the real-valued box average.
 * The definition holds at any ratio, so enlarging is valid; there it is NOT OpenCV's INTER_AREA, which switches to
 * bilinear when enlarging.  On reductions it is not OpenCV's bit for bit either: OpenCV weighs in float.
 *
 * Valid: out_width, out_height, width, height in 1..MI_BLUR_RESIZE_MAX_DIM (so X*n_in <= 2^30: one axis stays in 32
 * bits); the resize's per-image byte limits on both images; width <= MI_BLUR_AREA_MAX_RATIO * out_width and height <=
 * MI_BLUR_AREA_MAX_RATIO * out_height.  The cap on the ratio is a condition of the definition's use here, not a tuning
 * number: it bounds the taps one thread of the byte-per-thread kernel walks at 65 x 65 (without it a 1 x 1 output of a
 * 2 GiB image would be two billion serial loads in one thread) and the input under one output chunk at 66 chunks, so the
 * tiled kernel needs no rule about what fits.  A larger reduction is two calls.
 * The output is interleaved and dense: its pitch is Wo*C and images lie Wo*Ho*C bytes apart.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_AREA_MAX_RATIO 64
typedef struct mi_blur_area { int out_width, out_height; } mi_blur_area;

/* The first and the last tap of output index X on one axis and their weights, through the same function the kernels
 * and the CPU device use.  *w_hi = 0 when *i_hi == *i_lo (one tap: *w_lo is then n_in); every tap between the two
 * weighs n_out.  MI_BLUR_ERR_INVALID: a null pointer, n_in or n_out outside 1..MI_BLUR_RESIZE_MAX_DIM, X outside
 * [0, n_out).  (The ratio is not looked at: the axis is defined at any.) */
int mi_blur_area_coord(int n_in, int n_out, int X, int *i_lo, int *i_hi, int *w_lo, int *w_hi);

/* n_images images of width x height in, n_images images of r->out_width x r->out_height out (device memory,
 * asynchronous; n_images == 0 is MI_BLUR_OK; image offsets are 64-bit).  Every argument is checked before a device is
 * asked for: MI_BLUR_ERR_INVALID comes before MI_BLUR_ERR_NO_DEVICE.
 * blur_area_tiled_kernel (every input byte read once, coalesced; vertical sums in registers, handed to the horizontal
 * pass through LDS; nothing staged) takes exactly the launches with 1-4 channels, out_width <= width and out_height <=
 * height (reduction or equality on both axes), width*channels and out_width*channels multiples of 16 (input and output
 * rows are whole 16-byte chunks) and both pointers 16-byte aligned (and, where a context's in-place submit gives image
 * strides, strides that are multiples of 16; this export's are dense, which they then are); every other launch (any
 * enlargement, 5+ channels, odd rows or pointers) goes to blur_area_generic_kernel (one output byte per thread).
 * mi_blur_last_kernel() says which one ran. */
int mi_blur_enqueue_area(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                         const mi_blur_area *r, void *stream);
/* The same on the CPU device's threads (synchronous). */
int mi_blur_cpu_run_area(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                         const mi_blur_area *r, int n_threads);
/* Give a context (created with the INPUT width, height, channels) the area resize, with the rules of
 * mi_blur_ctx_set_resize: only before the first submit (MI_BLUR_ERR_STATE after); it replaces what another setter set
 * and is replaced by them; the context keeps a copy.  MI_BLUR_ERR_INVALID also when *r is not valid for the context's
 * size.  mi_blur_submit then writes n_images * Wo*Ho*C bytes to host_out: pageable caller memory, or pinned memory on
 * both sides (in place, one launch per submit, never the batch server), on the GPU or the CPU device.
 * mi_blur_submit_band, _bands, _planar and both resident runs return MI_BLUR_ERR_UNSUPPORTED for such a context. */
int mi_blur_ctx_set_area(mi_blur_ctx *ctx, const mi_blur_area *r);

/* ------------------------------------------------------------------------
 * Colour transform: an exact channel matrix and an optional lookup table, 1-4 channels in, 1-4 channels out (no reference
 * analogue): grey conversion, BGR <-> RGB, YCbCr, dropping or adding alpha, and gamma, threshold, invert or levels
 * through a table.  The one filter that mixes channels, and the one whose output has another channel count than its
 * input.  The definition is exact integers; the GPU, the CPU device and a numpy restatement agree byte for byte.
 * Pointwise: an output pixel depends on the input pixel at the same (x, y) only.
 *
 * For an input pixel in[0..C-1] and each o < Co = out_channels:
 *   acc    = bias[o] + sum_{i < C} m[o][i] * in[i]          (int32)
 *   v      = clamp(acc >> shift, 0, 255)                    (arithmetic shift: floors)
 *   out[o] = lut_on ? lut[o][v] : v
 *
 * Valid: 1 <= out_channels <= 4; 0 <= shift <= 16; lut_on 0 or 1; for every row o < out_channels
 * sum_{i<4} |m[o][i]| <= 2^18 and |bias[o]| <= 2^26.  Then |acc| < 255 * 2^18 + 2^26 < 2^27: every weight fits a signed
 * 24-bit operand and 32-bit sums are exact.  Rows >= out_channels are not read.  Columns >= C are not used by the
 * arithmetic but count in the row sum: the struct is validated before C is known.  The input has 1..4 channels (C > 4 is
 * MI_BLUR_ERR_INVALID, checked where C is known), and the image obeys the resize's per-image byte limits, on the input
 * with C and on the output with Co.
 * The output is interleaved and dense: its pitch is W*Co and images lie W*H*Co bytes apart.  The image size does not change.
 *
 * Presets (mi_blur_color_preset), with Q = 65536, R = 32768 and q(x) = floor(x * 65536 + 0.5) of the JFIF constants
 * 0.299, 0.587, 0.114, 0.168736, 0.331264, 0.5, 0.418688, 0.081312, 1.402, 0.344136, 0.714136, 1.772; lut_on = 0:
 *   RGB2GRAY   Co 1, shift 16: {19595, 38470, 7471}; bias R        (BT.601 luma; the weights sum to Q)
 *   BGR2GRAY   Co 1, shift 16: {7471, 38470, 19595}; bias R
 *   GRAY2RGB   Co 3, shift 0:  every row {1}
 *   RGB2BGR    Co 3, shift 0:  the permutation 2, 1, 0
 *   RGBA2BGRA  Co 4, shift 0:  the permutation 2, 1, 0, 3
 *   RGBA2RGB   Co 3, shift 0:  the identity on 0..2
 *   RGB2RGBA   Co 4, shift 0:  the identity on 0..2; row 3 all zero, bias 255
 *   RGB2YCBCR  Co 3, shift 16 (JFIF, full range): Y {19595, 38470, 7471}; R   Cb {-11058, -21710, 32768}; 128 Q + R
 *              Cr {32768, -27439, -5329}; 128 Q + R
 *   YCBCR2RGB  Co 3, shift 16: R {Q, 0, 91881}; R - 128 * 91881   G {Q, -22553, -46802}; R + 128 * (22553 + 46802)
 *              B {Q, 116130, 0}; R - 128 * 116130
 * The presets do not fix C: RGB2GRAY on a 4-channel image ignores alpha (column 3 is 0).
 * Properties (checked over all 2^24 colours): grey (v, v, v) gives v under RGB2GRAY and (v, 128, 128) under RGB2YCBCR,
 * and YCBCR2RGB of that gives (v, v, v) back, for every v; the Y of RGB2YCBCR equals RGB2GRAY; the clamp is live in the
 * forward direction (pure blue gives Cb = 256 before it); YCBCR2RGB(RGB2YCBCR(p)) differs from p by at most 1 in every
 * channel.
 * This is NOT claimed to be OpenCV's cvtColor bit for bit: OpenCV's fixed-point widths differ between versions.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_COLOR_MAX_CHANNELS 4
typedef struct mi_blur_color {
    int out_channels;            /* Co in 1..4 */
    int shift;                   /* 0..16 */
    int32_t m[4][4];             /* m[o][i]: weight of input channel i in output channel o */
    int32_t bias[4];             /* added before the shift */
    int lut_on;                  /* 0 | 1 */
    uint8_t lut[4][256];         /* lut[o][v], read only when lut_on */
} mi_blur_color;
typedef enum mi_blur_color_preset_id {
    MI_BLUR_COLOR_RGB2GRAY = 0, MI_BLUR_COLOR_BGR2GRAY = 1, MI_BLUR_COLOR_GRAY2RGB = 2, MI_BLUR_COLOR_RGB2BGR = 3,
    MI_BLUR_COLOR_RGBA2BGRA = 4, MI_BLUR_COLOR_RGBA2RGB = 5, MI_BLUR_COLOR_RGB2RGBA = 6, MI_BLUR_COLOR_RGB2YCBCR = 7,
    MI_BLUR_COLOR_YCBCR2RGB = 8
} mi_blur_color_preset_id;

/* Fill *k with a preset of the table above.  MI_BLUR_ERR_INVALID: an unknown id, a null k. */
int mi_blur_color_preset(int preset, mi_blur_color *k);
/* Fill *k with the identity matrix on `channels` (1..4) channels: shift 0, Co = channels, lut_on = 0.  The base of a pure
 * table look-up (OpenCV's LUT), invert and the like: set lut_on and fill lut[o] for o < channels. */
int mi_blur_color_identity(int channels, mi_blur_color *k);
/* One 256-entry table (host only).  gamma: lut[v] = floor(255 * pow(v / 255.0, gamma) + 0.5), in double; gamma <= 0 or not
 * finite is MI_BLUR_ERR_INVALID.  threshold: lut[v] = v > t ? hi : lo (OpenCV's THRESH_BINARY with two output levels); t in
 * -1..255, lo and hi in 0..255.  A null table is MI_BLUR_ERR_INVALID. */
int mi_blur_color_lut_gamma(double gamma, uint8_t lut[256]);
int mi_blur_color_lut_threshold(int t, int lo, int hi, uint8_t lut[256]);

/* n_images images of width x height x channels in, n_images images of width x height x k->out_channels out (device
 * memory, asynchronous; n_images == 0 is MI_BLUR_OK; image offsets are 64-bit).  Every argument is checked before a
 * device is asked for: MI_BLUR_ERR_INVALID comes before MI_BLUR_ERR_NO_DEVICE.  *k travels in the kernel arguments
 * (about 1.1 KiB with the tables): nothing is allocated, and *k may change as soon as the call returns.
 * blur_color_tiled_kernel takes exactly the launches with width*height a multiple of 16 and both pointers 16-byte aligned
 * (and, where a context's in-place submit gives image strides, strides that are multiples of 16).  The rule is FLAT,
 * unlike the other tiled kernels': rows need not be whole 16-byte chunks, because a pointwise filter on dense images
 * works on the run of width*height pixels, of which 16 are exactly C input chunks and Co output chunks.  One thread
 * owns such a group of 16 pixels (C loads and Co stores of 16 bytes), one workgroup 256 consecutive groups of one image;
 * the kernel is instantiated on (C, Co, lut_on), 32 forms, with the table in LDS where there is one.  Every other launch
 * goes to blur_color_generic_kernel (one output pixel per thread).  mi_blur_last_kernel() says which one ran. */
int mi_blur_enqueue_color(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                          const mi_blur_color *k, void *stream);
/* The same on the CPU device's threads (synchronous). */
int mi_blur_cpu_run_color(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                          const mi_blur_color *k, int n_threads);
/* Give a context (created with the INPUT width, height, channels) the colour transform, with the rules of
 * mi_blur_ctx_set_area: only before the first submit (MI_BLUR_ERR_STATE after); it replaces what another setter set
 * and is replaced by them; the context keeps a copy.  MI_BLUR_ERR_INVALID also when *k is not valid for the context's
 * image.  mi_blur_submit then writes n_images * W*H*Co bytes to host_out: pageable caller memory, or pinned memory on
 * both sides (in place, one launch per submit, never the batch server), on the GPU or the CPU device; bytes_alg counts
 * W*H*(C+Co) per image.  mi_blur_submit_band, _bands, _planar and both resident runs return MI_BLUR_ERR_UNSUPPORTED for
 * such a context: a band of another channel count has no place in those forms. */
int mi_blur_ctx_set_color(mi_blur_ctx *ctx, const mi_blur_color *k);

/* ------------------------------------------------------------------------
 * Histogram, and tone tables made from it: equalisation, min-max and percentile stretch, with one table per image and
 * channel (no reference analogue).  The first operation here that measures an image instead of mapping it.  Counts are
 * integers and the tables are integer ratios rounded once, so the GPU, the CPU device and a numpy / Python-integer
 * restatement agree exactly, whatever the order of the adds.  Not a filter of a context: histograms are not images, so
 * none of this goes through contexts, slots or the batch server.
 *
 * Images are interleaved and dense, 1..4 channels (MI_BLUR_COLOR_MAX_CHANNELS), within the resize's per-image byte
 * limits (width, height <= MI_BLUR_RESIZE_MAX_DIM; width*channels <= INT_MAX/2; width*height*channels <= INT_MAX), so
 * every count fits uint32_t.  n_images == 0 is MI_BLUR_OK and launches nothing.  Image offsets are 64-bit.
 *
 * Histogram: hist[i][c][v] = the number of pixels of image i whose channel c holds v; uint32[n_images][channels][256].
 *
 * Tone table of ONE image from its histogram uint32[channels][256], by *t (mi_blur_tone):
 *   The channels that are transformed are those whose bit is set in channel_mask; 0 means all of them.  Every other
 *   channel gets the identity table (lut[v] = v).
 *   joint == 0: every transformed channel gets the table of its own histogram h(v) = hist[c][v].
 *   joint == 1: every transformed channel gets the SAME table, of h(v) = the sum of hist[c][v] over the transformed
 *   channels (64-bit).
 *   N = sum_v h(v);  c(v) = sum_{u <= v} h(u), c(-1) = 0.  N == 0 (an all-zero histogram, which no image has) gives the
 *   identity.
 *   MI_BLUR_TONE_EQUALIZE:  m = the first v with h(v) > 0;  D = N - h(m).
 *     D == 0 (one grey level): the identity.  Otherwise lut[v] = 0 for v < m, and
 *     lut[v] = floor((510 * (c(v) - h(m)) + D) / (2 * D)) for v >= m.
 *     This is OpenCV's equalizeHist formula as an exact ratio rounded once, half up; it is NOT claimed to be OpenCV's
 *     bytes, which come from a multiplication by a float scale.
 *   MI_BLUR_TONE_STRETCH:  k_lo = floor(N * clip_lo / 65536), lo = the smallest v with c(v) > k_lo;
 *     k_hi = floor(N * clip_hi / 65536), hi = the largest v with N - c(v - 1) > k_hi.
 *     lo <= hi always: at most k_lo pixels lie below lo, at most k_hi above hi, and k_lo + k_hi < N.
 *     lo == hi: the identity.  Otherwise lut[v] = 0 for v <= lo, 255 for v >= hi, and
 *     lut[v] = floor((510 * (v - lo) + (hi - lo)) / (2 * (hi - lo))) between them.  Clips of 0: min-max normalisation.
 *   Everything stays below 2^49 in 64 bits (N <= 2^33 for four summed channels).
 * Valid *t: mode EQUALIZE or STRETCH; clip_lo, clip_hi in 0..32767 (Q16 shares of the pixels), both 0 with EQUALIZE;
 * joint 0 or 1; channel_mask without bits at or above `channels`.  Anything else is MI_BLUR_ERR_INVALID, the output
 * untouched.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_HIST_BINS 256
typedef enum { MI_BLUR_TONE_EQUALIZE = 0, MI_BLUR_TONE_STRETCH = 1 } mi_blur_tone_mode;
typedef struct mi_blur_tone {
    int mode;               /* mi_blur_tone_mode */
    int clip_lo, clip_hi;   /* STRETCH: share of the pixels clipped at each end, Q16, 0..32767 each; EQUALIZE: must be 0 */
    int joint;              /* 0: every channel its own table | 1: one table from the SUM of the masked channels' histograms */
    int channel_mask;       /* bit c = channel c is transformed; others get the identity table (copied); 0 = all channels */
} mi_blur_tone;

/* The histograms of n_images images (device memory, asynchronous).  d_hist: uint32[n_images][channels][256], 16-byte
 * aligned, OVERWRITTEN: the caller need not zero it (the call zeroes it on `stream`, then the kernel adds into it).
 * MI_BLUR_ERR_INVALID (before MI_BLUR_ERR_NO_DEVICE): a null pointer, channels outside 1..4, a size outside the limits
 * above, n_images < 0, d_hist not 16-byte aligned.
 * blur_hist_tiled_kernel takes exactly the launches with width*height a multiple of 16 and d_in 16-byte aligned (the
 * colour transform's flat rule): a workgroup owns a run of 512 consecutive groups of 16 pixels of one image (an image of
 * more than 256 runs has 256 workgroups, each taking every 256th run), reads them in 16-byte chunks, counts in LDS (one
 * set of channels x 256 counters per wave, 32-bit) and adds its non-zero counters to d_hist with atomic adds.  Every
 * other launch goes to blur_hist_generic_kernel (one byte per thread and step).
 * mi_blur_last_kernel() says which one ran. */
int mi_blur_enqueue_hist(const uint8_t *d_in, uint32_t *d_hist, int width, int height, int channels, int n_images, void *stream);
/* The same on the CPU device's threads (synchronous); hist in host memory, 4-byte aligned, overwritten. */
int mi_blur_cpu_run_hist(const uint8_t *in, uint32_t *hist, int width, int height, int channels, int n_images, int n_threads);

/* The tables of ONE image (host only): hist uint32[channels][256] -> tables uint8[channels][256], by the definition
 * above.  MI_BLUR_ERR_INVALID: a null pointer, channels outside 1..4, an invalid *t. */
int mi_blur_tone_tables(const uint32_t *hist, int channels, const mi_blur_tone *t, uint8_t *tables);

/* Every image through its OWN tables (device memory, asynchronous): out[i][p][c] = d_tables[i][c][in[i][p][c]].
 * d_tables: uint8[n_images][channels][256] in device memory, any alignment; read by the kernel of this launch only.
 * d_in == d_out is MI_BLUR_ERR_INVALID, as are the argument errors of mi_blur_enqueue_hist.
 * blur_tables_tiled_kernel takes the launches with width*height a multiple of 16 and d_in and d_out 16-byte aligned
 * (an image's tables go to LDS once per workgroup; a thread owns groups of 16 pixels: C loads of 16 bytes, byte
 * look-ups in LDS, C stores); every other launch goes to blur_tables_generic_kernel. */
int mi_blur_enqueue_tables(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                           const uint8_t *d_tables, void *stream);
/* Bytes of the work buffer of mi_blur_enqueue_tone: n_images*channels*256*4 for the histograms, then
 * n_images*channels*256 for the tables.  0 for channels outside 1..4 or n_images < 0. */
size_t mi_blur_tone_work_bytes(int channels, int n_images);
/* Histogram -> tables -> apply as one call: three dispatches on `stream` (mi_blur_enqueue_hist, blur_tone_table_kernel:
 * one workgroup per table, a prefix sum over the bins and the arithmetic of mi_blur_tone_tables; mi_blur_enqueue_tables),
 * no host round trip.  d_work (device memory, 16-byte aligned, mi_blur_tone_work_bytes() bytes) holds the histograms,
 * then the tables, in the layouts above; both are valid for the caller to read once the stream has drained.
 * MI_BLUR_ERR_INVALID also for an invalid *t, a null or misaligned d_work, d_in == d_out. */
int mi_blur_enqueue_tone(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                         const mi_blur_tone *t, void *d_work, void *stream);
/* The same two on the CPU device's threads (synchronous).  work: host memory laid out as d_work, 4-byte aligned, or
 * NULL (the call then allocates its own and drops it). */
int mi_blur_cpu_run_tables(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                           const uint8_t *tables, int n_threads);
int mi_blur_cpu_run_tone(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                         const mi_blur_tone *t, void *work /* may be NULL */, int n_threads);
/* Blocking, host memory in and out: allocate on `device` (a HIP ordinal), copy in, enqueue, copy out, free.
 * device == MI_BLUR_DEVICE_CPU calls the cpu_run forms with all threads.  MI_BLUR_ERR_NO_DEVICE where there is no such
 * device, after the argument checks.  host_work: as `work` above (receives the histograms and the tables), or NULL. */
int mi_blur_run_hist(int device, const uint8_t *host_in, uint32_t *host_hist, int width, int height, int channels, int n_images);
int mi_blur_run_tone(int device, const uint8_t *host_in, uint8_t *host_out, void *host_work /* may be NULL */,
                     int width, int height, int channels, int n_images, const mi_blur_tone *t);

/* ------------------------------------------------------------------------
 * CLAHE: tile-wise adaptive equalisation with a clip limit (no reference analogue).  The image is cut into a grid of
 * tiles, every tile gets its own table from its own clipped histogram, and every pixel goes through the tables of the
 * four tiles around it, blended by its position.  The first operation here that gives two regions of one image
 * different tables.  Integers only, rounded once (11 fraction bits per axis, one final rounding), so the GPU, the CPU
 * device and a numpy / Python-integer restatement agree byte for byte.  Not a filter of a context.
 *
 * Images: interleaved, dense, 1..4 channels, within the histogram family's limits.  Image offsets are 64-bit.
 * n_images == 0 is MI_BLUR_OK and launches nothing.
 *
 * Valid *k (mi_blur_clahe) for an image of width x height: tiles_x, tiles_y in 1..MI_BLUR_CLAHE_MAX_TILES with
 * tiles_x <= width and tiles_y <= height; clip_q8 in 0..65536; channel_mask without bits at or above `channels`.
 * Anything else is MI_BLUR_ERR_INVALID, the output untouched.
 *
 * Tile geometry.  On an axis of S pixels and T tiles, tile t covers the pixels [b_t, b_(t+1)) with b_t = floor(t*S/T);
 * T <= S makes every tile non-empty.  A tile's area A is its own pixel count.  There is NO padding: OpenCV reflect-pads
 * the image to a multiple of the grid and gives every tile the same area; here the tiles differ by up to one row and one
 * column and the image is never extended.
 *
 * Tile table, per (image, tile, transformed channel), from the tile's histogram h:
 *   1. clip_q8 == 0: h' = h (plain adaptive equalisation).
 *   2. Otherwise clip = max(1, floor(clip_q8 * A / 65536)) (clip_q8 = OpenCV's clipLimit in Q8; its clip is
 *      clipLimit * A / 256), excess = sum_v max(h(v) - clip, 0),
 *        h'(v) = min(h(v), clip) + floor(excess / 256),  residual = excess mod 256,
 *      and if residual > 0: step = max(floor(256 / residual), 1), and h'(v) += 1 for every v with v mod step == 0 and
 *      v / step < residual.  This is OpenCV's single redistribution pass in closed form.  sum_v h'(v) = A.  Bins may
 *      exceed clip afterwards; that is part of the definition.
 *   3. c(v) = sum_{u <= v} h'(u);  lut[v] = floor((510 * c(v) + A) / (2 * A)): 255 * c(v) / A rounded once, half up,
 *      in 64 bits.
 * A channel that is not transformed gets the identity table.  The histograms of ALL channels are counted.
 *
 * Position, per axis (mi_blur_clahe_coord): with p = 2x + 1 and m_t = b_t + b_(t+1) (the tile centres in half-pixels),
 *   p <= m_0, or tiles == 1:   (t0, t1, frac) = (0, 0, 0);
 *   p >= m_(T-1):              (T-1, T-1, 0);
 *   otherwise t0 = the largest t with m_t <= p, t1 = t0 + 1, frac = floor((p - m_t0) * 2048 / (m_t1 - m_t0)), 0..2047.
 *
 * Blend.  With (tx0, tx1, fx) and (ty0, ty1, fy) of the pixel and Lij = lut[tile (ty_i, tx_j)][c][in]:
 *   out = ((2048-fx)*(2048-fy)*L00 + fx*(2048-fy)*L01 + (2048-fx)*fy*L10 + fx*fy*L11 + 2^21) >> 22
 * which stays below 2^31; the weights sum to 2^22, so equal tables give the table's value exactly.
 *
 * The results are NOT claimed to be OpenCV's bytes: OpenCV uses float weights and a float scale, and padded tiles.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_CLAHE_MAX_TILES 64
typedef struct mi_blur_clahe {
    int tiles_x, tiles_y;   /* 1..MI_BLUR_CLAHE_MAX_TILES (64) each; tiles_x <= width, tiles_y <= height */
    int clip_q8;            /* OpenCV's clipLimit in Q8, 0..65536; 0 = no clipping (plain AHE) */
    int channel_mask;       /* as mi_blur_tone: bit c = channel c is transformed, others are copied; 0 = all */
} mi_blur_clahe;

/* (t0, t1, frac) of pixel x on an axis of `size` pixels and `tiles` tiles (host only).  MI_BLUR_ERR_INVALID: a null
 * pointer, size outside 1..MI_BLUR_RESIZE_MAX_DIM, tiles outside 1..min(MI_BLUR_CLAHE_MAX_TILES, size), x outside
 * 0..size-1. */
int mi_blur_clahe_coord(int size, int tiles, int x, int *t0, int *t1, int *frac);
/* One tile table from one histogram (host only), by steps 1 to 3 above.  MI_BLUR_ERR_INVALID: a null pointer, clip_q8
 * outside 0..65536, area == 0, or bins that do not sum to area. */
int mi_blur_clahe_table(const uint32_t hist[256], uint32_t area, int clip_q8, uint8_t lut[256]);
/* Bytes of the work buffer: n_images*tiles_y*tiles_x*channels*256*4 for the raw tile histograms
 * uint32[n_images][tiles_y][tiles_x][channels][256], then n_images*tiles_y*tiles_x*channels*256 for the tables
 * uint8[n_images][tiles_y][tiles_x][channels][256].  0 for invalid arguments. */
size_t mi_blur_clahe_work_bytes(int width, int height, int channels, int n_images, const mi_blur_clahe *k);
/* The tile histograms and the tile tables into d_work (device memory, 16-byte aligned, the layout above; asynchronous).
 * Both are valid for the caller to read once the stream has drained.  MI_BLUR_ERR_INVALID (before
 * MI_BLUR_ERR_NO_DEVICE): a null pointer, d_work not 16-byte aligned, the size errors of mi_blur_enqueue_hist, an
 * invalid *k.
 * blur_clahe_tables_tiled_kernel takes exactly the launches with width a multiple of 16 and d_in 16-byte aligned: one
 * workgroup per (image, tile) reads the tile's rows in aligned 16-byte chunks (a chunk that straddles a tile edge is
 * read by both neighbours and masked per pixel), counts in LDS (one set of channels x 256 counters per wave), sums the
 * sets, writes the histogram, clips, redistributes, runs the prefix sum and writes the tables: no global atomic, no
 * zeroing, no wait for another workgroup.  Every other launch goes to blur_clahe_tables_generic_kernel (one byte per
 * thread and step, at most 16384 workgroups that stride over the tiles). */
int mi_blur_enqueue_clahe_tables(const uint8_t *d_in, int width, int height, int channels, int n_images,
                                 const mi_blur_clahe *k, void *d_work, void *stream);
/* Every pixel through the four tables around it.  d_tables: uint8[n_images][tiles_y][tiles_x][channels][256] in device
 * memory, any alignment; ANY tables, not only ones this library made; clip_q8 and channel_mask are checked and not used.
 * MI_BLUR_ERR_INVALID: as above, and d_in == d_out.
 * blur_clahe_apply_tiled_kernel takes exactly the launches with width a multiple of 16, d_in and d_out 16-byte aligned
 * and this LDS rule: cut the row into spans of 256 pixels from pixel 0; a span needs the tile columns from t0 of its
 * first pixel to t1 of its last (mi_blur_clahe_coord); the launch is tiled when (the most columns any span needs) *
 * 2 * channels * 256 <= 32768 bytes.  A workgroup owns up to 32 rows between two tile-row centres and one span, stages
 * those tables and the span's column entries in LDS, and per group of 16 pixels does C loads of 16 bytes, four LDS byte
 * look-ups and one blend per byte, and C stores.  Every other launch goes to blur_clahe_apply_generic_kernel (one byte
 * per thread, the tables read from device memory). */
int mi_blur_enqueue_clahe_apply(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                const mi_blur_clahe *k, const uint8_t *d_tables, void *stream);
/* Both steps on one stream, no host round trip: two dispatches.  d_work as for mi_blur_enqueue_clahe_tables. */
int mi_blur_enqueue_clahe(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                          const mi_blur_clahe *k, void *d_work, void *stream);
/* The same three on the CPU device's threads (synchronous).  work: host memory laid out as d_work, 4-byte aligned; it
 * may be NULL for mi_blur_cpu_run_clahe (the call then allocates its own and drops it). */
int mi_blur_cpu_run_clahe_tables(const uint8_t *in, int width, int height, int channels, int n_images,
                                 const mi_blur_clahe *k, void *work, int n_threads);
int mi_blur_cpu_run_clahe_apply(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                const mi_blur_clahe *k, const uint8_t *tables, int n_threads);
int mi_blur_cpu_run_clahe(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                          const mi_blur_clahe *k, void *work /* may be NULL */, int n_threads);
/* Blocking, host memory in and out, like mi_blur_run_tone.  host_work: receives the histograms and the tables, or NULL. */
int mi_blur_run_clahe(int device, const uint8_t *host_in, uint8_t *host_out, void *host_work /* may be NULL */,
                      int width, int height, int channels, int n_images, const mi_blur_clahe *k);

/* ------------------------------------------------------------------------
 * Two-image arithmetic: add, subtract, absolute difference, weighted sum, min / max, multiply and the blend through a
 * mask (no reference analogue).  The first operation here with more than one image per output image.  Integers only,
 * rounded once, so the GPU, the CPU device and a numpy restatement agree byte for byte.  Like the histogram family it is
 * not a filter of a context (a context has one input stream): nothing here goes through contexts, slots or the batch
 * server.
 *
 * Operands.  A: n_images interleaved dense images of width x height x channels, channels 1..4, within the histogram
 * family's limits (width, height <= MI_BLUR_RESIZE_MAX_DIM; width*channels <= INT_MAX/2; width*height*channels <=
 * INT_MAX).  B: the same width x height with (b_plane ? 1 : channels) channels, (b_shared ? 1 : n_images) images.
 * M, the mask: present only for MI_BLUR_ARITH_LERP; m_plane and m_shared as for B.  Output: n_images images like A's.
 * For output byte (i, p, c) (image, pixel, channel):
 *     a = A[i][p][c],   b = B[b_shared ? 0 : i][p][b_plane ? 0 : c],   m = M[m_shared ? 0 : i][p][m_plane ? 0 : c].
 * A shared operand is the one background, gain image or watermark of a whole batch; a plane operand is a grey mask or
 * weight applied to every channel.  Image offsets are 64-bit.
 *
 * Operations (all int32; >> is arithmetic, so it floors; clamp is to 0..255):
 *   LINEAR   clamp((wa*a + wb*b + bias) >> shift)        |wa|, |wb| <= 2^16; |bias| <= 2^26
 *   ABSDIFF  clamp((wa*|a - b| + bias) >> shift)         wb = 0; |wa| <= 2^16; |bias| <= 2^26
 *   MIN, MAX min(a, b), max(a, b)                        wa, wb, bias, shift all 0
 *   MUL      clamp((wa*a*b + bias) >> shift)             wb = 0; |wa| <= 2^10; |bias| <= 2^26
 *   LERP     floor((2*(a*m + b*(255 - m)) + 255) / 510)  wa, wb, bias, shift all 0; M required
 * shift is 0..16 wherever it is not required to be 0.  Every sum stays below 2^27 and every multiplicand fits a signed
 * 24-bit operand.  LERP is the convex blend with one rounding, half up: m = 255 gives a, m = 0 gives b.  For every
 * t in 0..65025, floor((2t + 255) / 510) == (257*t + 32896) >> 16, which is the form the code uses.
 * The plane and shared flags are 0 or 1; m_plane and m_shared are 0 unless the operation is LERP.  Any other field
 * value is MI_BLUR_ERR_INVALID, the output untouched.
 *
 * Presets (mi_blur_arith_preset; plane and shared flags 0):          op       wa   wb  bias   shift
 *   ADD                                                              LINEAR    1    1     0      0
 *   SUB                                                              LINEAR    1   -1     0      0
 *   AVG       (a + b + 1) >> 1                                       LINEAR    1    1     1      1
 *   DIFF128   the signed difference around grey                      LINEAR    1   -1   128      0
 *   ABSDIFF                                                          ABSDIFF   1    0     0      0
 *   MIN, MAX                                                         MIN, MAX  0    0     0      0
 *   MUL255    a*b/255 rounded once (the identity above)              MUL     257    0 32896     16
 *   MULQ7     a gain image, 128 = unity, saturating                  MUL       1    0    64      7
 *   LERP                                                             LERP      0    0     0      0
 *
 * Aliasing.  d_out == d_a is allowed (the running accumulator).  d_out == d_b is allowed when B has the output's
 * extent: not plane (or channels == 1) and not shared (or n_images <= 1).  Any other overlap of the output's byte
 * range with an operand's range is MI_BLUR_ERR_INVALID, any overlap with M included.  Every implementation reads the
 * bytes a thread owns before it writes them, so the allowed cases are exact.
 * ---------------------------------------------------------------------- */
typedef enum { MI_BLUR_ARITH_LINEAR = 0, MI_BLUR_ARITH_ABSDIFF = 1, MI_BLUR_ARITH_MIN = 2,
               MI_BLUR_ARITH_MAX = 3, MI_BLUR_ARITH_MUL = 4, MI_BLUR_ARITH_LERP = 5 } mi_blur_arith_op;
typedef struct mi_blur_arith {
    int op;                 /* mi_blur_arith_op */
    int32_t wa, wb, bias;   /* see the table above */
    int shift;              /* 0..16, arithmetic (floors) */
    int b_plane, b_shared;  /* 0 | 1 */
    int m_plane, m_shared;  /* LERP only; otherwise must be 0 */
} mi_blur_arith;
typedef enum mi_blur_arith_preset_id {
    MI_BLUR_ARITH_ADD = 0, MI_BLUR_ARITH_SUB = 1, MI_BLUR_ARITH_AVG = 2, MI_BLUR_ARITH_DIFF128 = 3,
    MI_BLUR_ARITH_PRESET_ABSDIFF = 4, MI_BLUR_ARITH_PRESET_MIN = 5, MI_BLUR_ARITH_PRESET_MAX = 6,
    MI_BLUR_ARITH_MUL255 = 7, MI_BLUR_ARITH_MULQ7 = 8, MI_BLUR_ARITH_PRESET_LERP = 9
} mi_blur_arith_preset_id;

/* *k = the preset; MI_BLUR_ERR_INVALID for another id or a null k. */
int mi_blur_arith_preset(int preset, mi_blur_arith *k);
/* OpenCV's addWeighted in Q12: LINEAR with wa = floor(alpha*4096 + 0.5), wb = floor(beta*4096 + 0.5),
 * bias = floor(gamma*4096 + 0.5) + 2048, shift 12.  |alpha|, |beta| <= 16, |gamma| <= 8192; anything else, a
 * non-finite value or a null k is MI_BLUR_ERR_INVALID. */
int mi_blur_arith_weighted(double alpha, double beta, double gamma, mi_blur_arith *k);
/* The definition for one byte (host only): the output byte for operand bytes a, b and m (m is ignored unless the
 * operation is LERP); -1 for an invalid *k or an operand outside 0..255. */
int mi_blur_arith_value(const mi_blur_arith *k, int a, int b, int m);

/* out = A op B on device memory, asynchronous on `stream`.  d_m: the mask, NULL unless the operation is LERP.
 * n_images == 0 is MI_BLUR_OK.  MI_BLUR_ERR_INVALID (every argument is checked before a device is asked for, so before
 * MI_BLUR_ERR_NO_DEVICE): a null d_a, d_b, d_out or k; d_m null with LERP or non-null without it; channels outside
 * 1..4; a size outside the limits; n_images < 0; an invalid *k; an overlap that "Aliasing" above does not allow.  *k is
 * copied into the kernel arguments: it need not outlive the call.
 * Which kernel takes a launch (mi_blur_last_kernel() says which one ran); plane flags with channels == 1 count as 0:
 *   blur_arith_flat_kernel: no plane flag, width*height*channels a multiple of 16, every pointer 16-byte aligned.  The
 *     operation is bytewise, so an image is a flat run of bytes: a thread owns one chunk of 16 bytes (one 16-byte load per
 *     operand, one store), a workgroup a run of 256 consecutive chunks of one image.
 *   blur_arith_plane_kernel: channels 2..4, at least one plane flag, width*height a multiple of 16, every pointer
 *     16-byte aligned.  A thread owns a group of 16 pixels: `channels` chunks of every full operand, one chunk of every
 *     plane operand, `channels` stores.
 *   blur_arith_generic_kernel: everything else, one output byte per thread. */
int mi_blur_enqueue_arith(const uint8_t *d_a, const uint8_t *d_b, const uint8_t *d_m /* NULL unless LERP */, uint8_t *d_out,
                          int width, int height, int channels, int n_images, const mi_blur_arith *k, void *stream);
/* The same on the CPU device's threads (synchronous), host memory. */
int mi_blur_cpu_run_arith(const uint8_t *a, const uint8_t *b, const uint8_t *m /* NULL unless LERP */, uint8_t *out,
                          int width, int height, int channels, int n_images, const mi_blur_arith *k, int n_threads);
/* Blocking, host memory in and out: allocate on `device` (a HIP ordinal), copy in (a shared operand once), enqueue, copy
 * out, free.  device == MI_BLUR_DEVICE_CPU calls the cpu_run form with all threads.  MI_BLUR_ERR_NO_DEVICE where there is
 * no such device, after the argument checks. */
int mi_blur_run_arith(int device, const uint8_t *host_a, const uint8_t *host_b, const uint8_t *host_m /* NULL unless LERP */,
                      uint8_t *host_out, int width, int height, int channels, int n_images, const mi_blur_arith *k);

/* ------------------------------------------------------------------------
 * Integral images, and box filters of any window up to 255 x 255 made from them: the box mean, the local standard
 * deviation and the adaptive threshold (no reference analogue).  The first operation here whose cost does not depend on
 * the window.  Integers only, so the GPU, the CPU device and a numpy / Python-integer restatement agree exactly.  Like
 * the histogram family it is not a filter of a context: an integral image is not an image, and the box filters need a
 * work buffer.
 *
 * Images: n_images interleaved dense images of width x height x channels (W x H x C below), channels 1..4, within the
 * histogram family's limits (width, height <= MI_BLUR_RESIZE_MAX_DIM; width*channels <= INT_MAX/2;
 * width*height*channels <= INT_MAX).  n_images == 0 is MI_BLUR_OK and launches nothing.  Image offsets are 64-bit.
 *
 * Integral image (inclusive, with the image's own shape, so rows keep their alignment):
 *   S[i][y][x][c] = (sum over y' <= y, x' <= x of in[i][y'][x'][c]) mod 2^32,   uint32[n_images][H][W][C];
 *   Q[i][y][x][c] = the same over the squares in^2, also mod 2^32.
 *   An index of -1 on either axis reads as 0.
 * The modulus is part of the definition: any combination of entries with integer coefficients, computed in uint32, is
 * exact whenever its true value is below 2^32.  So images of any allowed size are valid (not only those with
 * W*H*255 < 2^32), and a window of at most 255 x 255 pixels is always exact for S (65025 * 255 < 2^32) and for Q
 * (65025 * 65025 = 4 228 250 625 < 2^32): one 32-bit table serves the squares too.
 *
 * Box window with clamp-to-edge (the border rule of every filter here).  rx, ry in 0..MI_BLUR_BOX_MAX_RADIUS,
 * A = (2 rx + 1)(2 ry + 1);
 *   Sum(X, Y, c)   = sum over |dy| <= ry, |dx| <= rx of in[clamp(Y + dy, 0, H - 1)][clamp(X + dx, 0, W - 1)][c],
 *   SumSq(X, Y, c) = the same over the squares.
 * Per axis, with N the extent, r the radius and F the inclusive prefix along that axis (F(-1) = 0):
 *   a = max(X - r, 0),  b = min(X + r, N - 1),  e0 = max(0, r - X),  e1 = max(0, X + r - (N - 1));
 *   the clamped sum is  F(b) - F(a - 1) + e0 * F(0) + e1 * (F(N - 1) - F(N - 2)).
 * In two dimensions Sum is the outer product of the two five-term forms over S (SumSq: over Q), in uint32: 4 reads in
 * the interior, at most 25 at a corner; terms with coefficient 0 (and reads at index -1) are skipped.  This holds for
 * windows larger than the image.  Every implementation here uses this form.
 *
 * Operations (mi_blur_box.op), per output byte:
 *   MEAN       out = floor((2 Sum + A) / (2 A)): the mean rounded once, half up (the area resize's rounding).
 *   STDDEV     D = A * SumSq - Sum^2 in 64 bits (>= 0, below 2^49); out = the largest s in 0..128 with s == 0 or
 *              (2 s - 1)^2 A^2 <= 4 D: sqrt(D) / A rounded once, half up, decided in integers.
 *   THRESHOLD  the adaptive threshold: with a = in[Y][X][c] and offset in -255..255, out = 255 if A * (a + offset) > Sum,
 *              else 0; invert (0 | 1) swaps the two outputs.  This is "a > mean - offset" with the mean NOT rounded; it is
 *              not claimed to be the bytes of OpenCV's adaptiveThreshold, which rounds the mean first.
 * Fields a mode does not use (offset and invert outside THRESHOLD) must be 0.  An op outside the enum, a radius outside
 * 0..127, an offset outside -255..255, an invert outside 0 | 1 or a non-zero unused field is MI_BLUR_ERR_INVALID, the
 * output untouched.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_BOX_MAX_RADIUS 127
typedef enum { MI_BLUR_BOX_MEAN = 0, MI_BLUR_BOX_STDDEV = 1, MI_BLUR_BOX_THRESHOLD = 2 } mi_blur_box_op;
typedef struct mi_blur_box {
    int op;                 /* mi_blur_box_op */
    int rx, ry;             /* 0..MI_BLUR_BOX_MAX_RADIUS: a window of (2 rx + 1) x (2 ry + 1) pixels */
    int offset;             /* THRESHOLD: -255..255; otherwise must be 0 */
    int invert;             /* THRESHOLD: 0 | 1; otherwise must be 0 */
} mi_blur_box;

/* The definition for one output byte (host only): the byte for a window of A pixels whose sum is `sum` and whose sum of
 * squares is `sqsum` (read only by STDDEV), with centre byte a (read only by THRESHOLD).  -1 for an invalid *k, an A
 * other than (2 rx + 1)(2 ry + 1), sum > 255 A, and where they are read: sqsum > 65025 A, sum^2 > A * sqsum (no window
 * has such sums), a outside 0..255. */
int mi_blur_box_value(const mi_blur_box *k, int A, uint32_t sum, uint32_t sqsum, int a);

/* Bytes of the work buffer of mi_blur_enqueue_integral: the column sums of every band of the "integral_band" rows in
 * force (16 by default), uint32[n_images][ceil(H / band)][both ? 2 : 1][W * C].  0 for an image outside the limits or
 * n_images < 0. */
size_t mi_blur_integral_work_bytes(int width, int height, int channels, int n_images, int both);
/* The integral images of n_images images (device memory, asynchronous on `stream`).  d_sum receives S, d_sqsum Q;
 * either may be NULL, not both; both come from one read of the input.  Each is uint32[n_images][H][W][C], 16-byte
 * aligned, OVERWRITTEN.  d_work: device memory, 16-byte aligned, mi_blur_integral_work_bytes(..., both outputs given)
 * bytes.  MI_BLUR_ERR_INVALID (every argument is checked before a device is asked for, so before
 * MI_BLUR_ERR_NO_DEVICE): a null d_in or d_work, both outputs null, an output or d_work not 16-byte aligned, channels
 * outside 1..4, a size outside the limits, n_images < 0.
 * No workgroup of these kernels ever waits for another: what one band hands the next crosses a dispatch boundary on the
 * stream, through d_work.
 * blur_integral_tiled_kernel takes exactly the launches with W a multiple of 16, W <= 8192 and d_in 16-byte aligned,
 * as three dispatches.  (1) blur_integral_bands_kernel: per band of rows, the column sums of the bytes (and of their
 * squares) to d_work.  (2) blur_integral_band_prefix_kernel: their exclusive prefix over the bands of an image, in
 * place.  (3) blur_integral_tiled_kernel: one workgroup per (image, band) spans the whole row, a thread owns 16 pixels
 * (C loads of 16 bytes); it keeps the running column sums of its pixels in registers, seeded from (2), adds each row of
 * the band to them and takes the horizontal prefix of them for every row: in registers within the thread, across the
 * wave by lane shifts, across the waves through LDS; 4 C stores of 16 bytes per table.  The input is read twice and the
 * tables are written once.
 * Every other launch goes to blur_integral_generic_kernel (one wave per row: the prefix along each row into the
 * tables) followed by blur_integral_generic_cols_kernel (one thread per column and channel walks down the table, in
 * place); d_work is not written.  mi_blur_last_kernel() says which of the two forms ran. */
int mi_blur_enqueue_integral(const uint8_t *d_in, uint32_t *d_sum /* may be NULL */, uint32_t *d_sqsum /* may be NULL */,
                             int width, int height, int channels, int n_images, void *d_work, void *stream);
/* The same on the CPU device's threads (synchronous), host memory; the tables 4-byte aligned; no work buffer (rows in
 * bands across the threads, with the same carry from band to band). */
int mi_blur_cpu_run_integral(const uint8_t *in, uint32_t *sum /* may be NULL */, uint32_t *sqsum /* may be NULL */,
                             int width, int height, int channels, int n_images, int n_threads);

/* The box filter *k from integral images that are already there (device memory, asynchronous): d_sum = S of the input,
 * always; d_sqsum = Q, non-null exactly for STDDEV; d_in = the images, non-null exactly for THRESHOLD (read only at the
 * byte a thread writes, so d_out == d_in is allowed).  MI_BLUR_ERR_INVALID (before MI_BLUR_ERR_NO_DEVICE): a null
 * d_sum, d_out or k; d_sqsum or d_in given or missing against the rule; a table not 16-byte aligned; an invalid *k;
 * the image and n_images as above.
 * blur_box_tiled_kernel takes the launches whose rows are whole 16-byte chunks (W * C a multiple of 16) with d_out (and
 * d_in) 16-byte aligned: a thread owns 4 consecutive output bytes of a row ("box_bytes": 16 in A/B runs), which is 4
 * consecutive dwords at each corner of the window: one 16-byte load per corner, contiguous across a wave.  Where all of
 * its pixels are more than rx columns and ry rows from every border it takes the 4-read form, elsewhere the general form
 * per byte.  The division by A is a float estimate corrected by the exact
 * remainder; STDDEV's root is a double estimate corrected by the exact 64-bit comparison.  Every other launch goes to
 * blur_box_generic_kernel, one output byte per thread. */
int mi_blur_enqueue_box_from_integral(const uint8_t *d_in /* THRESHOLD only */, const uint32_t *d_sum,
                                      const uint32_t *d_sqsum /* STDDEV only */, uint8_t *d_out, int width, int height,
                                      int channels, int n_images, const mi_blur_box *k, void *stream);
/* Bytes of the work buffer of mi_blur_enqueue_box: the tables the mode needs (S; S and Q for STDDEV), each
 * n_images * H * W * C * 4 bytes, then mi_blur_integral_work_bytes() for them.  0 for an invalid *k, an image outside the
 * limits or n_images < 0. */
size_t mi_blur_box_work_bytes(int width, int height, int channels, int n_images, const mi_blur_box *k);
/* The integral images the mode needs and the box filter from them as one call: the dispatches of
 * mi_blur_enqueue_integral and mi_blur_enqueue_box_from_integral on `stream`, no host round trip.  d_work: device
 * memory, 16-byte aligned, mi_blur_box_work_bytes() bytes.  d_out == d_in is allowed.  MI_BLUR_ERR_INVALID: a null or
 * misaligned d_work, a null d_in, d_out or k, an invalid *k, the image and n_images as above. */
int mi_blur_enqueue_box(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                        const mi_blur_box *k, void *d_work, void *stream);
/* The same on the CPU device's threads (synchronous); the call allocates its tables (MI_BLUR_ERR_NOMEM if it cannot). */
int mi_blur_cpu_run_box(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                        const mi_blur_box *k, int n_threads);
/* Blocking, host memory in and out: allocate on `device` (a HIP ordinal), copy in, enqueue, copy out, free.
 * device == MI_BLUR_DEVICE_CPU calls the cpu_run forms with all threads.  MI_BLUR_ERR_NO_DEVICE where there is no such
 * device, after the argument checks. */
int mi_blur_run_integral(int device, const uint8_t *host_in, uint32_t *host_sum /* may be NULL */,
                         uint32_t *host_sqsum /* may be NULL */, int width, int height, int channels, int n_images);
int mi_blur_run_box(int device, const uint8_t *host_in, uint8_t *host_out, int width, int height, int channels, int n_images,
                    const mi_blur_box *k);

/* ------------------------------------------------------------------------
 * Exact distance transform (squared Euclidean, city block, chessboard) and, from it, dilation and erosion of masks by a
 * disc, diamond or square of any radius up to 32767 (OpenCV's distanceTransform; no reference analogue).  Integers only:
 * the GPU, the CPU device and a numpy / brute-force restatement agree word for word.  Like the histogram and integral
 * families it is not a filter of a context: it produces a table and needs a work buffer.
 *
 * Images: n_images interleaved dense images of W x H x C, channels 1..4, within the histogram family's limits.
 * n_images == 0 is MI_BLUR_OK and launches nothing.  Channels are independent, and so are images.
 *
 * Sites: in image i and channel c, pixel (x, y) is a site when in == 0; with sites_nonzero = 1, when in != 0.  Zero is
 * OpenCV's convention.  Only pixels inside the image can be sites: there is no border rule.
 *
 * Table value T(x, y, c), uint32[n_images][H][W][C], over the sites (x', y') of the same image and channel:
 *   MI_BLUR_DIST_L2    min of (x - x')^2 + (y - y')^2: the SQUARED Euclidean distance, at most 2 * 32767^2 < 2^31;
 *   MI_BLUR_DIST_L1    min of |x - x'| + |y - y'|;
 *   MI_BLUR_DIST_LINF  min of max(|x - x'|, |y - y'|).
 * A channel with no site has MI_BLUR_DIST_NONE everywhere.  limit is 0 (none) or 1..MI_BLUR_DIST_MAX_LIMIT: with a limit
 * L, T is exact where the distance is at most L (T <= L^2 for L2, T <= L for the other two) and MI_BLUR_DIST_NONE
 * everywhere else.  The limit is part of the definition; it bounds the search to 2 L + 1 columns.
 *
 * Byte forms, made from T by byte_op:
 *   MI_BLUR_DIST_BYTE    NONE -> 255.  L2: min(255, s) with s the largest integer with s == 0 or (2 s - 1)^2 <= 4 T:
 *                        sqrt(T) rounded once, half up, decided in integers (BOX_STDDEV's convention).  L1, LINF: min(255, T).
 *   MI_BLUR_DIST_WITHIN  needs limit >= 1: 255 where T != NONE, else 0; invert (0 | 1) swaps the two.  With sites_nonzero
 *                        this is the dilation of a mask by the metric's ball of radius limit (a disc, a diamond, a
 *                        square); with zero sites and invert, its erosion.
 * Fields a call does not use must be 0: byte_op and invert in the table calls, invert outside WITHIN.  A value outside
 * its range, a non-zero unused field or WITHIN with limit == 0 is MI_BLUR_ERR_INVALID, the output untouched.
 *
 * Method, everywhere: g(x, y, c) = the distance along the column to the nearest site of that column (or "none"; with a
 * limit, anything above it is "none" too), then T = min over x' of dx^2 + g^2 (L2), dx + g (L1), max(dx, g) (LINF) with
 * dx = |x - x'| and g = g(x', y, c): exact for all three, and a search outwards from dx = 0 may stop as soon as dx alone
 * (dx^2 for L2) reaches the best value so far.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_DIST_MAX_LIMIT 32767
#define MI_BLUR_DIST_NONE 0xFFFFFFFFu
typedef enum { MI_BLUR_DIST_L2 = 0, MI_BLUR_DIST_L1 = 1, MI_BLUR_DIST_LINF = 2 } mi_blur_dist_metric;
typedef enum { MI_BLUR_DIST_BYTE = 0, MI_BLUR_DIST_WITHIN = 1 } mi_blur_dist_byte_op;
typedef struct mi_blur_dist {
    int metric;             /* mi_blur_dist_metric */
    int sites_nonzero;      /* 0: a site is in == 0 (OpenCV) | 1: a site is in != 0 */
    int limit;              /* 0 = none | 1..MI_BLUR_DIST_MAX_LIMIT */
    int byte_op;            /* mi_blur_dist_byte_op; the table calls: must be 0 */
    int invert;             /* WITHIN: 0 | 1; otherwise must be 0 */
} mi_blur_dist;

/* The definition of the byte forms for one table value (host only): the byte for T = t.  -1 for a *k that is invalid for
 * the byte calls, or a t that no image can give under *k: above the metric's maximum (2 * 32767^2, 2 * 32767, 32767) or
 * above the limit (limit^2 for L2), and not MI_BLUR_DIST_NONE. */
int mi_blur_dist_value(const mi_blur_dist *k, uint32_t t);

/* Bytes of the work buffer of the two enqueue calls: g as uint16[n_images][H][W * C] (rounded up to 16 bytes), then per
 * band of the "dist_band" rows in force (32 by default) the first and the last site row of every column,
 * uint16[n_images][ceil(H / band)][2][W * C].  0 for an invalid *k (as mi_blur_dist_value), an image outside the limits
 * or n_images < 0. */
size_t mi_blur_dist_work_bytes(int width, int height, int channels, int n_images, const mi_blur_dist *k);
/* The table T of n_images images (device memory, asynchronous on `stream`): d_table = uint32[n_images][H][W][C], 16-byte
 * aligned, OVERWRITTEN; d_work: device memory, 16-byte aligned, mi_blur_dist_work_bytes() bytes.  MI_BLUR_ERR_INVALID
 * (every argument is checked before a device is asked for, so before MI_BLUR_ERR_NO_DEVICE): a null d_in, d_table, k or
 * d_work, d_table or d_work not 16-byte aligned, an invalid *k (byte_op and invert must be 0), channels outside 1..4, a
 * size outside the limits, n_images < 0.
 * No workgroup of these kernels ever waits for another; the dispatches on the one stream do the ordering.  Every loop has
 * a bound known at launch.  Four dispatches:
 *  (1) blur_dist_bands_kernel: per (image, band of rows, column and channel) the first and the last site row, to d_work.
 *  (2) blur_dist_carry_kernel: per column the walk over the bands of an image, both ways, in place: the last site row
 *      above each band and the first one below it.
 *  (3) blur_dist_cols_kernel: every band sweeps down and up from those carries: g, to d_work.  Threads of (1)-(3) run
 *      along W * C; any shape and alignment.
 *  (4) the row pass.  blur_dist_tiled_kernel takes exactly the launches with W * C a multiple of 8 and at most 24576
 *      (and, for the byte form, d_out 16-byte aligned): a workgroup of 256 threads owns max(1, min(8, 4096 / (W * C)))
 *      whole rows, stages their g in LDS one plane per channel (rows padded with "none" to whole chunks of 16 columns:
 *      at most 34 bytes per 16 elements, 52.4 KiB), keeps the minimum of every chunk next to it, and a thread owns 4
 *      consecutive outputs: per output first the columns nearer than 16, one dx at a time on both sides (with dense
 *      sites the search ends there), then the other chunks outwards, left and right in turn: it stops a side when the
 *      chunk's nearest dx alone cannot beat the best value so far, skips a chunk whose minimum cannot, and reads the 16
 *      entries of the others; one 16-byte store of 4 words (or one 4-byte store of 4 bytes).  Every other launch goes to
 *      blur_dist_generic_kernel: one output per thread (a capped grid that strides), searching g outwards in global
 *      memory, at most W steps.  mi_blur_last_kernel() says which of the two ran. */
int mi_blur_enqueue_dist(const uint8_t *d_in, uint32_t *d_table, int width, int height, int channels, int n_images,
                         const mi_blur_dist *k, void *d_work, void *stream);
/* The byte form *k of the same (byte_op, invert): it goes straight from the row pass, the 32-bit table never reaches
 * memory.  d_out = uint8 of the images' shape, any alignment.  d_out == d_in is allowed (the column pass has consumed the
 * input before the row pass stores); every other overlap of the two is MI_BLUR_ERR_INVALID. */
int mi_blur_enqueue_dist_u8(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                            const mi_blur_dist *k, void *d_work, void *stream);
/* The same on the CPU device's threads (synchronous), host memory; the table 4-byte aligned; the call allocates g
 * (MI_BLUR_ERR_NOMEM if it cannot).  Columns in strips across the threads, then rows. */
int mi_blur_cpu_run_dist(const uint8_t *in, uint32_t *table, int width, int height, int channels, int n_images,
                         const mi_blur_dist *k, int n_threads);
int mi_blur_cpu_run_dist_u8(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                            const mi_blur_dist *k, int n_threads);
/* Blocking, host memory in and out: allocate on `device` (a HIP ordinal), copy in, enqueue, copy out, free.
 * device == MI_BLUR_DEVICE_CPU calls the cpu_run forms with all threads.  MI_BLUR_ERR_NO_DEVICE where there is no such
 * device, after the argument checks. */
int mi_blur_run_dist(int device, const uint8_t *host_in, uint32_t *host_table, int width, int height, int channels,
                     int n_images, const mi_blur_dist *k);
int mi_blur_run_dist_u8(int device, const uint8_t *host_in, uint8_t *host_out, int width, int height, int channels,
                        int n_images, const mi_blur_dist *k);

/* ------------------------------------------------------------------------
 * Template matching and peak search (OpenCV's matchTemplate and minMaxLoc; no reference analogue).  Defined in integers
 * and exact: the GPU, the CPU device and a Python-integer restatement agree word for word.  None of it is claimed to be
 * OpenCV's bytes, which are float.
 *
 * Operands.  Images are uint8[n][H][W][C], within the histogram family's limits, C = 1..4.  The template is
 * uint8[th][tw][C] when t_shared = 1 and uint8[n][th][tw][C] (one per image) when t_shared = 0.  The output has
 * Wo = W - tw + 1 columns and Ho = H - th + 1 rows and ONE entry per position: the channels are summed, as OpenCV does.
 * Every window lies inside the image: there is no border rule.
 *
 * A spec is valid when method is in the enum, 1 <= tw <= min(W, 255), 1 <= th <= min(H, 255), tw * th * C <= 65536
 * and t_shared is 0 or 1.  With A = tw * th * C <= 65536 every raw sum fits uint32: 255^2 * 65536 = 4 261 478 400 < 2^32;
 * the sides stay within 255 because that is where the integral tables S and Q are exact.
 *
 * Raw methods, uint32[n][Ho][Wo].  With a = in[y + dy][x + dx][c] and t = T[dy][dx][c], summed over dy < th, dx < tw
 * and every c:   CCORR = sum a t      SQDIFF = sum (a - t)^2      SAD = sum |a - t|.
 * (The kernels form SQDIFF as sum a^2 + sum t^2 - 2 sum a t in uint32: exact modulo 2^32, and so exact.)
 *
 * Scores, int32[n][Ho][Wo], -16384 .. 16384 (MI_BLUR_MATCH_ONE = 1.0).  With sum_a, sum_aa, sum_at of the window and
 * sum_t, sum_tt of the template:
 *   NCC  (TM_CCORR_NORMED):   N = sum_at,                              D = sum_aa * sum_tt               < 2^64
 *   ZNCC (TM_CCOEFF_NORMED):  N = A sum_at - sum_a sum_t  (|N| < 2^48), D = Da * Dt                      < 2^96
 *                             Da = A sum_aa - sum_a^2, Dt = A sum_tt - sum_t^2, each in [0, 2^48)
 * The score is sign(N) k, k the largest integer in 0..16384 that is 0 or satisfies (2k - 1)^2 D <= 2^30 N^2: that is
 * 2^14 |N| / sqrt(D) rounded once, half away from zero, decided in integers (both sides are below 2^126).  N^2 <= D by
 * Cauchy-Schwarz, so nothing is clamped.  D = 0 (a flat window or a flat template) gives 0.
 *
 * Peak search over a table of 32-bit words [n][Ho][Wo], taken as unsigned or signed: per image int64[6] = min, min_x,
 * min_y, max, max_x, max_y.  Ties go to the FIRST entry in row-major order, for both.
 *
 * Kernels.  blur_match_tiled_kernel takes SQDIFF, CCORR and SAD when the images are 16-byte aligned and a row is whole
 * 16-byte chunks (W * C a multiple of 16); blur_match_generic_kernel takes the rest, and everything when "match_tiled"
 * is 0.  The scores are made of the integral tables, a CCORR launch, the template's sums and an elementwise kernel.
 *
 * Out of scope: FFT matching for templates beyond the area limit, masks, sub-pixel refinement of the peak, a host CLI
 * flag and context filters. */
typedef enum { MI_BLUR_MATCH_SQDIFF = 0, MI_BLUR_MATCH_CCORR = 1, MI_BLUR_MATCH_SAD = 2,
               MI_BLUR_MATCH_NCC = 3, MI_BLUR_MATCH_ZNCC = 4 } mi_blur_match_method;
typedef struct mi_blur_match { int method; int tw, th; int t_shared; } mi_blur_match;
#define MI_BLUR_MATCH_MAX_SIDE 255
#define MI_BLUR_MATCH_MAX_AREA 65536      /* tw * th * C */
#define MI_BLUR_MATCH_ONE 16384           /* a score of 1.0 */

/* The definition of a score, host only: method NCC | ZNCC, A = tw * th * C and the five sums.  INT32_MIN for another
 * method, A outside 1..65536, or sums no window or template can have: sum_a > 255 A, sum_aa > 65025 A,
 * sum_a^2 > A sum_aa, the same three for t, and sum_at^2 > sum_aa sum_tt. */
int32_t mi_blur_match_value(int method, uint32_t A, uint32_t sum_at, uint32_t sum_a, uint32_t sum_aa, uint32_t sum_t,
                            uint32_t sum_tt);

/* Bytes of the work buffer of mi_blur_enqueue_match; 0 for a spec or an image that is not valid.  A raw method: the
 * templates' sums (16 bytes each) and the templates with every row zero-padded to whole 16-byte chunks, which the tiled
 * kernel reads.  A score adds the CCORR table, S and Q and mi_blur_integral_work_bytes(.., both), each rounded to 16. */
size_t mi_blur_match_work_bytes(int width, int height, int channels, int n_images, const mi_blur_match *k);

/* d_out = 32-bit words [n][Ho][Wo], 16-byte aligned, uint32 for a raw method and int32 for a score; d_work = non-null,
 * 16-byte aligned, mi_blur_match_work_bytes bytes.  d_out equal to d_in or d_t is refused.  Everything goes on `stream`
 * with no host round trip: a score issues the integral dispatches, the template's sums, the CCORR launch into the work
 * buffer and the elementwise score kernel.  Statuses in the order of every table export: the arguments
 * (MI_BLUR_ERR_INVALID), the empty batch (MI_BLUR_OK), the device (MI_BLUR_ERR_NO_DEVICE). */
int mi_blur_enqueue_match(const uint8_t *d_in, const uint8_t *d_t, void *d_out, int width, int height, int channels,
                          int n_images, const mi_blur_match *k, void *d_work, void *stream);
/* The CPU device: the definition's loops, rows across n_threads (0 = all); out 4-byte aligned; no work buffer. */
int mi_blur_cpu_run_match(const uint8_t *in, const uint8_t *t, void *out, int width, int height, int channels,
                          int n_images, const mi_blur_match *k, int n_threads);
/* The blocking form on host memory: a HIP ordinal or MI_BLUR_DEVICE_CPU. */
int mi_blur_run_match(int device, const uint8_t *host_in, const uint8_t *host_t, void *host_out, int width, int height,
                      int channels, int n_images, const mi_blur_match *k);

/* Peak search.  out_width x out_height = the table's extent (1.., out_width * out_height <= INT_MAX), is_signed 0 | 1.
 * Two dispatches: MI_BLUR_MATCH_PEAK_PARTS workgroups per image leave keys (value << 32 | index for the minimum,
 * value << 32 | ~index for the maximum, the value biased by 2^31 when signed) in the work buffer, one workgroup per image
 * finishes and decodes; no workgroup waits for another.  d_table and d_work 16-byte aligned; d_peaks = int64[n][6],
 * 16-byte aligned (8 on the host). */
#define MI_BLUR_MATCH_PEAK_PARTS 256
size_t mi_blur_match_peak_work_bytes(int out_width, int out_height, int n_images);
int mi_blur_enqueue_match_peak(const void *d_table, int is_signed, int out_width, int out_height, int n_images,
                               int64_t *d_peaks, void *d_work, void *stream);
int mi_blur_cpu_run_match_peak(const void *table, int is_signed, int out_width, int out_height, int n_images,
                               int64_t *peaks, int n_threads);
int mi_blur_run_match_peak(int device, const void *host_table, int is_signed, int out_width, int out_height,
                           int n_images, int64_t *host_peaks);

/* ------------------------------------------------------------------------
 * Affine warp: exact fixed-point rotate, scale, shear and translate, any output size (no reference analogue).  The
 * definition is exact integers; the GPU, the CPU device and a numpy restatement agree byte for byte.  It reuses the
 * resize's arithmetic: 11 fraction bits, a four-tap blend, one final rounding.
 *
 * Coordinates: pixel (x, y) sits at integer coordinates (x, y), which is OpenCV's warpAffine convention; there is no
 * half-pixel shift.  m is the OUTPUT -> INPUT map in Q16 (MI_BLUR_WARP_Q fraction bits), row-major 2 x 3.  For output
 * pixel (X, Y), in int64:
 *   Sx = m[0]*X + m[1]*Y + m[2]             Sy = m[3]*X + m[4]*Y + m[5]
 *
 * MI_BLUR_RESIZE_BILINEAR:
 *   px = (Sx + 16) >> 5                     (arithmetic shift: floors; the position rounded to 11 fraction bits)
 *   x0 = px >> 11                           fx = px & 2047          py, y0, fy from Sy in the same way
 *   taps T(y0, x0), T(y0, x0+1), T(y0+1, x0), T(y0+1, x0+1); per channel, with the expression of the resize:
 *   s   = (2048-fy) * ((2048-fx) * T(y0,x0) + fx * T(y0,x0+1)) + fy * ((2048-fx) * T(y0+1,x0) + fx * T(y0+1,x0+1))
 *   out = (s + (1 << 21)) >> 22
 * MI_BLUR_RESIZE_NEAREST: xi = (Sx + 32768) >> 16, likewise yi, out = T(yi, xi).
 *
 * Taps: under MI_BLUR_WARP_CLAMP T(y, x) = in[clamp(y, 0, H-1)][clamp(x, 0, W-1)][c].  Under MI_BLUR_WARP_CONSTANT a
 * tap outside [0, W-1] x [0, H-1] is `fill`; each tap is decided on its own (OpenCV's BORDER_CONSTANT).  Channels
 * never mix.
 *
 * Valid: out_width, out_height in 1..MI_BLUR_RESIZE_MAX_DIM; width, height <= MI_BLUR_RESIZE_MAX_DIM; the resize's
 * per-image byte limits on both images; a known mode and border; 0 <= fill <= 255; |m[0]|, |m[1]|, |m[3]|, |m[4]| <= 2^26
 * and |m[2]|, |m[5]| <= 2^46, so |Sx|, |Sy| < 2^47 and x0, y0 fit an int.  An all-zero linear part is valid: it samples
 * one constant position.  Implementations clamp px into [-2*2048, (W+1)*2048] (py likewise with H) before they split
 * it: under either border rule a position out there gives the bytes of the nearest one inside, and 32 bits do from
 * there on.
 *
 * Properties (Q = 1 << 16; all but the last checked in tests/test_warp_host.py):
 *   m = {Q,0,0, 0,Q,0} with the input's size is the identity;
 *   m = {0,-Q,(W-1)*Q, Q,0,0} with an output of H x W (width H, height W) is np.rot90;
 *   integer translations give a shifted copy;
 *   under CLAMP, m = {s,0,t, 0,s,t} with s = Q*num/den and t = (s - Q)/2 gives the bytes of mi_blur_enqueue_resize at
 *   that ratio whenever s and t are integers (x2, x4, /2, /4, /8);
 *   the result differs from real-valued bilinear interpolation at the exact Q16 position by less than
 *   0.5 + 255 * 2^-11 ~ 0.6245 (each axis rounded by at most 2^-12, blend slope at most 255 per axis, one final rounding);
 *   it is NOT OpenCV's INTER_LINEAR bit for bit: OpenCV quantises the position to 5 bits.
 * The output is interleaved and dense: its pitch is out_width*C and images lie out_width*out_height*C bytes apart.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_WARP_Q 16                     /* fraction bits of the matrix */
typedef enum mi_blur_warp_border { MI_BLUR_WARP_CLAMP = 0, MI_BLUR_WARP_CONSTANT = 1 } mi_blur_warp_border;
typedef struct mi_blur_warp {
    int out_width, out_height;                /* 1 .. MI_BLUR_RESIZE_MAX_DIM each */
    int mode;                                 /* MI_BLUR_RESIZE_NEAREST | MI_BLUR_RESIZE_BILINEAR */
    int border;                               /* mi_blur_warp_border */
    int fill;                                 /* 0..255, every channel; CONSTANT only */
    int64_t m[6];                             /* OUTPUT -> INPUT map, Q16, row-major 2 x 3 */
} mi_blur_warp;

/* The UNCLAMPED tap origin (x0, y0) and the fractions (fx, fy) of output pixel (X, Y), through the function the
 * kernels and the CPU device use; NEAREST gives xi, yi, 0, 0.  Only mode and m of *w are read.  MI_BLUR_ERR_INVALID: a
 * null pointer, an unknown mode, m outside its limits, X or Y outside 0..MI_BLUR_RESIZE_MAX_DIM-1. */
int mi_blur_warp_coord(const mi_blur_warp *w, int X, int Y, int *x0, int *y0, int *fx, int *fy);
/* The FORWARD (input -> output) matrix of OpenCV's getRotationMatrix2D: a rotation by angle_deg about (cx, cy) with
 * an isotropic scale; a positive angle is counter-clockwise with y pointing down.  With a = scale*cos, b = scale*sin:
 * fwd = {a, b, (1-a)*cx - b*cy,  -b, a, b*cx + (1-a)*cy}.  MI_BLUR_ERR_INVALID: fwd null or an argument not finite. */
int mi_blur_warp_rotation(double cx, double cy, double angle_deg, double scale, double fwd[6]);
/* Sets w->m from a real 2 x 3 matrix.  inverse == 0: m maps input to output (what getRotationMatrix2D and
 * getAffineTransform give) and is inverted in double; inverse != 0: m already maps output to input.  Either way every
 * entry is quantised q = floor(v*65536 + 0.5) and range-checked.  MI_BLUR_ERR_INVALID (w->m untouched): a null pointer,
 * an entry not finite, a singular matrix (inverse == 0), an entry outside the limits above. */
int mi_blur_warp_set_matrix(mi_blur_warp *w, const double m[6], int inverse);

/* n_images images of width x height in, n_images images of w->out_width x w->out_height out (device memory,
 * asynchronous; n_images == 0 is MI_BLUR_OK; image offsets are 64-bit).  Every argument is checked before a device is
 * asked for: MI_BLUR_ERR_INVALID comes before MI_BLUR_ERR_NO_DEVICE.
 * blur_warp_tiled_kernel: one workgroup = one tile of 32 output rows x at most 4*C output 16-byte chunk columns (64
 * pixels; the chunk columns of a row are cut into ceil(cpr / (4*C)) equal strips, for 3 channels of whole groups of 3
 * chunks = 16 pixels).  It stages the tile's source footprint in LDS: the bounding box of the taps of the tile's four
 * corner pixels with the + 1 tap, clamped into the image (CLAMP) or intersected with it (CONSTANT), widened to whole
 * 16-byte chunks, 16 bytes per staged chunk.  It takes exactly the launches with BILINEAR mode, 1-4 channels,
 * width*channels and out_width*channels multiples of 16, both pointers 16-byte aligned (and image strides that are
 * multiples of 16, which this export's dense ones then are), and whose largest footprint over the tiles of one image
 * is at most 65520 bytes (64 KiB of LDS less 16 bytes that the kernel's 8-byte tap reads may touch behind it).  That admits every launch of that alignment with |m[0]|+|m[1]| <= 3*Q/2 and
 * |m[3]|+|m[4]| <= 3*Q/2 (every rotation, every enlargement, shears up to 0.5: at most 98 rows x 27 chunks); beyond it
 * the exact walk over the tiles decides.  Every other launch (NEAREST, 5+ channels, odd rows or pointers, a larger
 * footprint) goes to blur_warp_generic_kernel (one output byte per thread).  mi_blur_last_kernel() says which ran. */
int mi_blur_enqueue_warp(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                         const mi_blur_warp *w, void *stream);
/* The same on the CPU device's threads (synchronous). */
int mi_blur_cpu_run_warp(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                         const mi_blur_warp *w, int n_threads);
/* Give a context (created with the INPUT width, height, channels) the warp, with the rules of mi_blur_ctx_set_resize:
 * only before the first submit (MI_BLUR_ERR_STATE after); it replaces what another setter set and is replaced by them;
 * the context keeps a copy.  MI_BLUR_ERR_INVALID also when *w is not valid for the context's size.  mi_blur_submit then
 * writes n_images * Wo*Ho*C bytes to host_out: pageable caller memory, or pinned memory on both sides (in place, one
 * launch per submit, never the batch server), on the GPU or the CPU device.  mi_blur_submit_band, _bands, _planar and
 * both resident runs return MI_BLUR_ERR_UNSUPPORTED for such a context. */
int mi_blur_ctx_set_warp(mi_blur_ctx *ctx, const mi_blur_warp *w);

/* ------------------------------------------------------------------------
 * Perspective warp: exact fixed-point homography, any output size (no reference analogue; OpenCV's warpPerspective is
 * the model).  Exact integers again: the GPU, the CPU device and a numpy restatement agree byte for byte.
 *
 * h[9] is the OUTPUT -> INPUT homography, row-major 3 x 3, int64.  The scale is free: h and c*h (c > 0) are the same
 * map.  For output pixel (X, Y), all in int64:
 *   Nx = h0*X + h1*Y + h2      Ny = h3*X + h4*Y + h5      D = h6*X + h7*Y + h8
 *   BILINEAR:  px = floor((Nx*4096 + D) / (2*D))     (= the position Nx/D rounded to 11 fraction bits)
 *              x0 = px >> 11,  fx = px & 2047        (py, y0, fy from Ny likewise)
 *   NEAREST:   xi = floor((2*Nx + D) / (2*D)),  yi likewise
 * Everything else is the affine warp's: the four taps, the blend expression and its one rounding, the CLAMP / CONSTANT
 * border with `fill`, the clamp of px into [-2*2048, (W+1)*2048] (py likewise with H), applied after the division and
 * before the split, channels never mix, dense output.
 *
 * Valid: the sizes, mode, border, fill and byte limits of the affine warp; |h0|,|h1|,|h3|,|h4|,|h6|,|h7| <= 2^32 and
 * |h2|,|h5|,|h8| <= 2^48; D >= 1 at the four corner pixels of the output.  D is linear, so it is then >= 1 at every
 * output pixel; in particular h8 >= 1.  With X, Y < 2^15 this gives |N|, D < 2^49, |N*4096 + 2048*D| < 2^62, 2D < 2^50:
 * signed 64 bits hold every intermediate; a quotient can reach 2^61 before the clamp.  An output whose horizon
 * (D <= 0) crosses it is MI_BLUR_ERR_INVALID, never garbage.
 *
 * Properties (checked in tests/test_warp_perspective_host.py):
 *   h = {s*m0..s*m5, 0, 0, s*65536} gives the bytes of mi_blur_enqueue_warp with the Q16 matrix m, in both modes and
 *   both borders, for any s >= 1 that keeps the limits;
 *   over any rectangle of output pixels the smallest and largest x0 and y0 occur at its four corners (a
 *   linear-fractional function is monotone along every segment where D > 0, and floor is monotone): the tiled kernel
 *   stages the box of a tile's corners;
 *   the result differs from real-valued bilinear interpolation at the exact rational position by less than
 *   0.5 + 255 * 2^-11, the affine warp's bound, for the same reason;
 *   it is NOT OpenCV's INTER_LINEAR bit for bit (5-bit positions there).
 * ---------------------------------------------------------------------- */
typedef struct mi_blur_warp_perspective {
    int out_width, out_height;                /* 1 .. MI_BLUR_RESIZE_MAX_DIM each */
    int mode;                                 /* MI_BLUR_RESIZE_NEAREST | MI_BLUR_RESIZE_BILINEAR */
    int border;                               /* mi_blur_warp_border */
    int fill;                                 /* 0..255, every channel; CONSTANT only */
    int64_t h[9];                             /* OUTPUT -> INPUT homography, row-major 3 x 3, free scale */
} mi_blur_warp_perspective;

/* The UNCLAMPED tap origin (x0, y0; 64 bits: they can reach 2^50) and the fractions (fx, fy) of output pixel (X, Y),
 * through the function the kernels and the CPU device use; NEAREST gives xi, yi, 0, 0.  Only mode and h of *w are read.
 * MI_BLUR_ERR_INVALID: a null pointer, an unknown mode, h outside its limits, X or Y outside
 * 0..MI_BLUR_RESIZE_MAX_DIM-1, D < 1 at (X, Y). */
int mi_blur_warp_perspective_coord(const mi_blur_warp_perspective *w, int X, int Y, int64_t *x0, int64_t *y0, int *fx, int *fy);
/* The FORWARD (input -> output) matrix H, H[8] = 1, that takes the four points src (x0,y0, .. x3,y3) to the four points
 * dst: OpenCV's getPerspectiveTransform.  MI_BLUR_ERR_INVALID: a null pointer, a value not finite, three collinear
 * points on either side (no such matrix, or none with H[8] = 1). */
int mi_blur_warp_perspective_quad(const double src[8], const double dst[8], double H[9]);
/* Sets w->h from a real 3 x 3 matrix, for w's output size.  inverse == 0: H maps input to output (what
 * getPerspectiveTransform gives) and is inverted in double by the adjugate; inverse != 0: H already maps output to
 * input.  Then v = H / H[8]; k = the largest integer in 0..30 with |v_i| * 2^k <= limit_i - 1 for all nine entries
 * (limit 2^32 or 2^48 as above); h_i = floor(v_i * 2^k + 0.5); then the validity check above.  30 fraction bits matter: a
 * perspective term of 5e-4 per pixel is 33 in Q16 (0.7 % off) and 536871 at k = 30.  MI_BLUR_ERR_INVALID (w->h
 * untouched): a null pointer, an entry not finite, a determinant that is 0 or not finite (inverse == 0), H[8] zero or
 * not finite after the inversion, no such k, out_width or out_height outside 1..MI_BLUR_RESIZE_MAX_DIM, D < 1 at a
 * corner pixel of the output (a horizon crosses it). */
int mi_blur_warp_perspective_set_matrix(mi_blur_warp_perspective *w, const double H[9], int inverse);

/* As mi_blur_enqueue_warp, argument for argument and status for status (MI_BLUR_ERR_INVALID before
 * MI_BLUR_ERR_NO_DEVICE).  blur_warp_persp_tiled_kernel has the tiles, the staging and the stores of
 * blur_warp_tiled_kernel; a work item computes Nx, Ny, D once, adds h0, h3, h6 per pixel and divides twice per pixel,
 * exactly (a double-precision estimate corrected by the exact 64-bit remainder).  It takes the launches the affine
 * tiled kernel's rule admits (BILINEAR, 1-4 channels, both rows whole 16-byte chunks, aligned pointers and strides)
 * whose largest tile footprint, found by walking the tiles of one image, is at most 65520 bytes; footprints differ
 * from tile to tile under a projective map.  Every other launch goes to blur_warp_persp_generic_kernel (one output byte
 * per thread) as a whole.  mi_blur_last_kernel() says which ran. */
int mi_blur_enqueue_warp_perspective(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                                     const mi_blur_warp_perspective *w, void *stream);
/* The same on the CPU device's threads (synchronous). */
int mi_blur_cpu_run_warp_perspective(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                                     const mi_blur_warp_perspective *w, int n_threads);
/* Give a context the perspective warp, with the rules of mi_blur_ctx_set_warp: only before the first submit
 * (MI_BLUR_ERR_STATE after); it replaces what another setter set and is replaced by them; the context keeps a copy.
 * mi_blur_submit writes n_images * Wo*Ho*C bytes (pageable, or pinned in place: one launch per submit, never the batch
 * server); bytes_alg counts input + output bytes; mi_blur_submit_band, _bands, _planar and both resident runs return
 * MI_BLUR_ERR_UNSUPPORTED. */
int mi_blur_ctx_set_warp_perspective(mi_blur_ctx *ctx, const mi_blur_warp_perspective *w);

/* ------------------------------------------------------------------------
 * Remap: exact fixed-point sampling through a per-pixel map (no reference analogue; OpenCV's remap is the model): lens
 * undistortion, rectification, fisheye and cylindrical unwrapping, mesh warps, any map computed elsewhere.  Exact integers
 * again: the GPU, the CPU device and a numpy restatement agree byte for byte.
 *
 * map is int32_t[out_height][out_width][2], dense.  Entry (Y, X) is (px, py): the input position of output pixel (X, Y)
 * with MI_BLUR_REMAP_FRAC = 11 fraction bits, px = x * 2048, pixel (x, y) at integer coordinates (the warps' convention and
 * OpenCV's).  One map serves every image of a launch.  EVERY int32 pair is a valid entry, INT32_MIN and INT32_MAX
 * included: the library cannot validate device memory, so nothing is out of range.  Per axis, with n = W or H:
 *   p = min(max(px, -2*2048), (n+1)*2048)          (the clamp of the affine warp, for the same reason: under either border
 *                                                   rule a position out there gives the bytes of the nearest one inside)
 *   BILINEAR:  x0 = p >> 11,  fx = p & 2047        NEAREST:  xi = (p + 1024) >> 11,  f = 0
 * Everything else is the affine warp's: the four taps, the blend expression and its one rounding, the CLAMP / CONSTANT
 * border with `fill`, each tap decided on its own, channels never mix, and the output is interleaved and dense: pitch
 * out_width*C, images out_width*out_height*C bytes apart.
 *
 * Properties (checked in tests/test_remap_host.py):
 *   a map with px = X*2048, py = Y*2048 at the input's size is the identity;
 *   a BILINEAR map built as px = clip(x0*2048 + fx), py likewise, with x0, fx from mi_blur_warp_coord (clip: into the int32
 *   range) gives the bytes of mi_blur_enqueue_warp under both borders, and with mi_blur_warp_perspective_coord those of
 *   mi_blur_enqueue_warp_perspective; so, through the warp, the x2 / x4 / /2 / /4 / /8 CLAMP maps give the resize's bytes;
 *   the result differs from real-valued bilinear interpolation at the map's exact position by less than
 *   0.5 + 255 * 2^-11, the warp's bound; for a map quantised from real numbers (mi_blur_remap_from_float) the bound holds
 *   against the REAL positions, because each axis is then rounded by at most 2^-12;
 *   it is NOT OpenCV's remap bit for bit: OpenCV quantises positions to 5 bits.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_REMAP_FRAC 11                 /* fraction bits of a map entry */
typedef struct mi_blur_remap {
    int out_width, out_height;                /* 1 .. MI_BLUR_RESIZE_MAX_DIM each */
    int mode;                                 /* MI_BLUR_RESIZE_NEAREST | MI_BLUR_RESIZE_BILINEAR */
    int border;                               /* mi_blur_warp_border */
    int fill;                                 /* 0..255, every channel; CONSTANT only */
    int stage_bytes;                          /* 0 = 65520; else 16..65520: the largest tile footprint the tiled kernel stages in LDS */
} mi_blur_remap;
typedef struct mi_blur_remap_tiles {
    int tiled;                                /* 1: the shape is blur_remap_tiled_kernel's (pointers assumed aligned); 0: the rest stays 0 */
    int tiles, staged, direct, empty;         /* tiles of one output image; staged + direct + empty == tiles */
    long long max_box_bytes, max_staged_bytes;/* the largest footprint of any tile, and of any staged tile */
} mi_blur_remap_tiles;

/* The CLAMPED tap origin (x0, y0) and the fractions (fx, fy) of the map entry (px, py) on a W x H image, through the
 * function the kernels and the CPU device use; NEAREST gives xi, yi, 0, 0.  Only r->mode is read.  MI_BLUR_ERR_INVALID: a
 * null pointer, an unknown mode, W or H outside 1..MI_BLUR_RESIZE_MAX_DIM. */
int mi_blur_remap_coord(const mi_blur_remap *r, int W, int H, int32_t px, int32_t py, int *x0, int *y0, int *fx, int *fy);
/* A map from n pairs of real positions (OpenCV's CV_32FC1 map_x, map_y): map[2i] = q(map_x[i]), map[2i+1] = q(map_y[i]),
 * q(v) = floor(v*2048 + 0.5) in double, clamped into [-2^30, 2^30].  MI_BLUR_ERR_INVALID (map untouched): a null
 * pointer, a value that is not finite. */
int mi_blur_remap_from_float(const float *map_x, const float *map_y, size_t n, int32_t *map);
/* The undistortion map of a pinhole camera with radial and tangential distortion: OpenCV's initUndistortRectifyMap with
 * R = I.  K and new_K are {fx, fy, cx, cy} (new_K null: K); dist is {k1, k2, p1, p2, k3}.  Per output pixel (X, Y), all in
 * double, in this order, without contraction into fused multiply-adds:
 *   x = (X - cx') / fx'     y = (Y - cy') / fy'     r2 = x*x + y*y     rad = 1 + k1*r2 + k2*r2*r2 + k3*r2*r2*r2
 *   xd = x*rad + 2*p1*x*y + p2*(r2 + 2*x*x)         yd = y*rad + p1*(r2 + 2*y*y) + 2*p2*x*y
 *   u = fx*xd + cx          v = fy*yd + cy          map[Y][X] = (q(u), q(v)), q as in mi_blur_remap_from_float
 * MI_BLUR_ERR_INVALID: a null pointer (new_K may be), out_width or out_height outside 1..MI_BLUR_RESIZE_MAX_DIM, a
 * parameter that is not finite, fx' or fy' equal to 0 (map untouched in all of these); a position that is not finite
 * (the map is then partly written). */
int mi_blur_remap_undistort(const double K[4], const double dist[5], const double new_K[4], int out_width, int out_height, int32_t *map);
/* A host-only walk of the tiles of one output image of a remap of width x height x channels images through host_map,
 * with the kernel's own box function.  tiles->tiled: whether the launch is eligible for blur_remap_tiled_kernel by shape.
 * If so: how many tiles stage their box in LDS, how many sample directly (box over stage_bytes), how many are empty
 * (CONSTANT, every tap outside), and the largest boxes.  A caller picks stage_bytes with it.  MI_BLUR_ERR_INVALID: a null
 * pointer, *r not valid for the image. */
int mi_blur_remap_plan(const int32_t *host_map, int width, int height, int channels, const mi_blur_remap *r, mi_blur_remap_tiles *tiles);

/* As mi_blur_enqueue_warp, argument for argument and status for status (MI_BLUR_ERR_INVALID before
 * MI_BLUR_ERR_NO_DEVICE; n_images == 0 is MI_BLUR_OK).  d_map: DEVICE memory, out_height*out_width int32 pairs; null,
 * equal to d_out, or not 4-byte aligned is MI_BLUR_ERR_INVALID.
 * blur_remap_tiled_kernel takes the launches of the affine tiled kernel's rule (BILINEAR, 1-4 channels, width*channels
 * and out_width*channels multiples of 16, 16-byte aligned pointers and strides) whose d_map is 16-byte aligned too.  Its
 * tiles are the warp's (32 output rows x 64 pixels).  The host cannot know a tile's footprint, so each workgroup reduces
 * the extrema of its map entries (kept in registers), builds the box [min x0, max x0 + 1] x [min y0, max y0 + 1], clamped
 * into the image (CLAMP) or intersected with it (CONSTANT), and decides for its tile: an empty box stores `fill`; a box
 * of at most stage_bytes (rows x 16-byte chunks x 16) is staged in LDS and sampled as the warp kernel samples; a larger
 * one is sampled straight from global memory.  The launch asks for 64 + stage_bytes + 16 bytes of LDS: the default 65520
 * admits every footprint the affine tiled kernel admits and lets two workgroups share a CU's 160 KiB; a smaller value buys
 * occupancy and sends more tiles down the direct path (mi_blur_remap_plan counts them).  A caller who holds the map on
 * the host should pass the plan's max_box_bytes: the smallest value that still stages every tile.  Measured
 * (profiles/r16_remap.md): 72.7 -> 42.5 us on 4096x4096x1 and 13.9 -> 11.9 us on 1920x1080x3 under a rotation by 30
 * degrees; one of seven measured rows got slower (35 x 256x256x3, 17.4 -> 20.3 us).  Every other launch (NEAREST,
 * 5+ channels, odd rows or pointers, a map 4 or 8 bytes off) goes to blur_remap_generic_kernel (one output byte per
 * thread).  mi_blur_last_kernel() says which ran. */
int mi_blur_enqueue_remap(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                          const mi_blur_remap *r, const int32_t *d_map, void *stream);
/* The same on the CPU device's threads (synchronous); host_map is host memory. */
int mi_blur_cpu_run_remap(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                          const mi_blur_remap *r, const int32_t *host_map, int n_threads);
/* Give a context the remap, with the rules of mi_blur_ctx_set_warp: only before the first submit (MI_BLUR_ERR_STATE
 * after); it replaces what another setter set and is replaced by them.  The context keeps a COPY of *r and of the map:
 * a GPU context allocates device memory and copies synchronously inside the call (MI_BLUR_ERR_NOMEM or a HIP status when
 * that fails), a CPU-device context keeps a host copy; the copy is freed when another setter replaces it and in
 * mi_blur_destroy.  A setter that fails leaves the old filter and the old map in place.  mi_blur_submit writes
 * n_images * Wo*Ho*C bytes (pageable, or pinned in place: one launch per submit, never the batch server); bytes_alg counts
 * input + output bytes, NOT the map's 8 bytes per output pixel; mi_blur_submit_band, _bands, _planar and both resident
 * runs return MI_BLUR_ERR_UNSUPPORTED. */
int mi_blur_ctx_set_remap(mi_blur_ctx *ctx, const mi_blur_remap *r, const int32_t *host_map);

/* ------------------------------------------------------------------------
 * Median blur, windows 3x3 to 15x15 (no reference analogue).  For a radius r in 1..MI_BLUR_MEDIAN_MAX_RADIUS, with
 * clamp-to-edge as everywhere else:
 *   out[y][x][c] = the k-th smallest (0-based, k = ((2r+1)^2 - 1) / 2) of
 *                  { in[clamp(y+j, 0, H-1)][clamp(x+i, 0, W-1)][c] : -r <= i, j <= r }
 * The window count is odd, so the result is one exact byte; the GPU and the CPU device agree byte for byte.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_MEDIAN_MAX_RADIUS 7

/* mi_blur_enqueue / mi_blur_enqueue_band with the median of that radius (same buffers, same band semantics: clamping at
 * the band's own edges, only rows [out_row_begin, out_row_end) written; asynchronous).  Radius 1 and 2 on rows of whole
 * 16-byte chunks at 16-byte aligned addresses with 1-4 channels take blur_median_fast_kernel, every other case
 * blur_median_generic_kernel.  MI_BLUR_ERR_INVALID: radius outside 1..7, null or equal buffers, non-positive sizes. */
int mi_blur_enqueue_median(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int radius,
                           int n_images, void *stream);
int mi_blur_enqueue_median_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels, int radius,
                                int out_row_begin, int out_row_end, void *stream);
/* mi_blur_cpu_run with the median (a sliding per-channel histogram along each row). */
int mi_blur_cpu_run_median(const uint8_t *in, uint8_t *out, int width, int height, int channels, int radius,
                           int n_images, int n_threads);
/* Give a context the median of that radius in place of its blur, with the rules of mi_blur_ctx_set_kernel: only before
 * the first submit (MI_BLUR_ERR_STATE after), every submit form then uses it, never through the batch server, resident
 * runs MI_BLUR_ERR_UNSUPPORTED.  A context holds one filter: mi_blur_ctx_set_kernel and this call each replace what the
 * other set before. */
int mi_blur_ctx_set_median(mi_blur_ctx *ctx, int radius);

/* ------------------------------------------------------------------------
 * Greyscale morphology, windows up to 33x33 (no reference analogue).  For radii rx, ry in 0..MI_BLUR_MORPH_MAX_RADIUS,
 * independent per axis, with clamp-to-edge as everywhere else:
 *   lo[y][x][c] = min { in[clamp(y+j, 0, H-1)][clamp(x+i, 0, W-1)][c] : -rx <= i <= rx, -ry <= j <= ry }
 *   hi[y][x][c] = max { the same set }
 *   MI_BLUR_MORPH_ERODE -> lo     MI_BLUR_MORPH_DILATE -> hi     MI_BLUR_MORPH_GRADIENT -> hi - lo   (0..255, no wrap)
 * Channels never mix.  rx = ry = 0 is valid: ERODE and DILATE copy, GRADIENT writes zeros.  Clamping equals ignoring the
 * pixels outside the image: a clamped coordinate always lands on a pixel that is already in the window, so this is
 * OpenCV's default border for erode / dilate.  Exact: the GPU and the CPU device agree byte for byte.
 * Opening and closing are two calls by the caller (erode then dilate, dilate then erode); a caller that works in bands
 * needs a halo of 2 ry rows for them, ry for each single call.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_MORPH_MAX_RADIUS 16
typedef enum mi_blur_morph_op { MI_BLUR_MORPH_ERODE = 0, MI_BLUR_MORPH_DILATE = 1, MI_BLUR_MORPH_GRADIENT = 2 } mi_blur_morph_op;

/* mi_blur_enqueue / mi_blur_enqueue_band with that window extremum (same buffers, same band semantics: clamping at the
 * band's own edges, only rows [out_row_begin, out_row_end) written; asynchronous; n_images == 0 is MI_BLUR_OK).  Rows of
 * whole 16-byte chunks at 16-byte aligned addresses with 1-4 channels take blur_morph_tiled_kernel at every radius, every
 * other case blur_morph_generic_kernel.  MI_BLUR_ERR_INVALID (before MI_BLUR_ERR_NO_DEVICE): an unknown op, a radius
 * outside 0..16, null or equal buffers, non-positive sizes. */
int mi_blur_enqueue_morph(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int op, int rx, int ry,
                          int n_images, void *stream);
int mi_blur_enqueue_morph_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels, int op, int rx,
                               int ry, int out_row_begin, int out_row_end, void *stream);
/* mi_blur_cpu_run with the window extremum (a vertical and a horizontal pass per row, exact). */
int mi_blur_cpu_run_morph(const uint8_t *in, uint8_t *out, int width, int height, int channels, int op, int rx, int ry,
                          int n_images, int n_threads);
/* Give a context that window extremum in place of its blur, with the rules of mi_blur_ctx_set_median: only before the
 * first submit (MI_BLUR_ERR_STATE after), every submit form then uses it, never through the batch server, resident runs
 * MI_BLUR_ERR_UNSUPPORTED.  A context holds one filter: mi_blur_ctx_set_kernel, mi_blur_ctx_set_median and this call each
 * replace what another set before. */
int mi_blur_ctx_set_morph(mi_blur_ctx *ctx, int op, int rx, int ry);

/* ------------------------------------------------------------------------
 * Bilateral filter, windows 3x3 to 17x17 (no reference analogue): the edge-preserving smoother.  Defined by two integer
 * tables, so it is exact: a spatial table S over the (2r+1) x (2r+1) window, r in 1..MI_BLUR_BILATERAL_MAX_RADIUS, and a
 * range table R over the absolute difference to the centre sample.  Per output byte, with v0 = in[y][x][c] and
 * v = in[clamp(y+j, 0, H-1)][clamp(x+i, 0, W-1)][c] over -r <= i, j <= r (clamp-to-edge as everywhere else):
 *   w   = S[j][i] * R[|v - v0|]
 *   den = sum w          num = sum w * v
 *   out[y][x][c] = (num + den / 2) / den          (unsigned integer division: round half up)
 * Channels never mix: each channel is filtered on its own, like every other filter here.  For colour images this differs
 * from OpenCV's bilateralFilter, which measures the range distance in colour space; for one channel the definition is
 * the same up to the integer tables.  A valid kernel has S[0][0] > 0 and R[0] > 0 (so den >= 1) and sum S <= 65535 (so
 * num + den / 2 < 2^32: 32-bit unsigned sums are exact).  A tap with S = 0 contributes nothing: a table zero-padded to a
 * larger radius gives the same bytes, and an anisotropic or round window is zeros in the table.  The GPU and the CPU
 * device agree byte for byte.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_BILATERAL_MAX_RADIUS 8
typedef struct mi_blur_bilateral {
    int radius;                       /* r in 1..8: window (2r+1) x (2r+1) */
    uint8_t spatial[17 * 17];         /* S[j][i] at spatial[(j + r) * (2r + 1) + (i + r)], -r <= i, j <= r; rest ignored */
    uint8_t range[256];               /* R[d], d = |neighbour - centre| */
} mi_blur_bilateral;

/* Gaussian tables, computed in double: S[j][i] = floor(128 exp(-(i^2 + j^2) / (2 sigma_space^2)) + 0.5),
 * R[d] = floor(255 exp(-d^2 / (2 sigma_range^2)) + 0.5); sigma_space <= 0 means radius / 2.0.  The centre is 128 and R[0]
 * is 255 by construction.  MI_BLUR_ERR_INVALID: sigma_range <= 0, a radius outside 1..8, a null k. */
int mi_blur_bilateral_gauss(double sigma_space, double sigma_range, int radius, mi_blur_bilateral *k);

/* mi_blur_enqueue / mi_blur_enqueue_band with that bilateral filter (same buffers, same band semantics: clamping at the
 * band's own edges, only rows [out_row_begin, out_row_end) written; asynchronous; n_images == 0 is MI_BLUR_OK).  The tables
 * travel in the kernel arguments: nothing is allocated, nothing needs freeing, *k may change as soon as the call returns.
 * Rows of whole 16-byte chunks at 16-byte aligned addresses with 1-4 channels take blur_bilateral_tiled_kernel at every
 * radius, every other case blur_bilateral_generic_kernel.  MI_BLUR_ERR_INVALID (before MI_BLUR_ERR_NO_DEVICE): a null k, a
 * radius outside 1..8, S[0][0] == 0, R[0] == 0, sum S > 65535, null or equal buffers, non-positive sizes. */
int mi_blur_enqueue_bilateral(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                              const mi_blur_bilateral *k, void *stream);
int mi_blur_enqueue_bilateral_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                                   int out_row_begin, int out_row_end, const mi_blur_bilateral *k, void *stream);
/* mi_blur_cpu_run with the bilateral filter (plain integer loops, exact). */
int mi_blur_cpu_run_bilateral(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                              const mi_blur_bilateral *k, int n_threads);
/* Give a context that bilateral filter in place of its blur, with the rules of mi_blur_ctx_set_median: only before the
 * first submit (MI_BLUR_ERR_STATE after), every submit form then uses it, never through the batch server, resident runs
 * MI_BLUR_ERR_UNSUPPORTED.  A context holds one filter: mi_blur_ctx_set_kernel, mi_blur_ctx_set_median,
 * mi_blur_ctx_set_morph and this call each replace what another set before.  The context keeps a copy. */
int mi_blur_ctx_set_bilateral(mi_blur_ctx *ctx, const mi_blur_bilateral *k);

/* ------------------------------------------------------------------------
 * 2-D convolution with signed integer taps, windows up to 15x15 (no reference analogue): derivatives and edge maps (Sobel,
 * Scharr, Laplacian), sharpening, emboss, or any kernel the caller writes down.  Radii rx, ry in
 * 0..MI_BLUR_CONV_MAX_RADIUS, independent per axis; taps K[j][i], -ry <= j <= ry, -rx <= i <= rx, signed 16-bit.
 * This is CORRELATION, not flipped convolution (OpenCV filter2D's convention): K[j][i] multiplies the sample j rows
 * below and i columns to the right.  Clamp-to-edge as everywhere else; channels never mix.  Exact, in integers:
 *   acc  = sum_{j,i} K[j][i]  * in[clamp(y+j, 0, H-1)][clamp(x+i, 0, W-1)][c]          (int32)
 *   acc2 = sum_{j,i} K2[j][i] * in[...]                                                 (MAG only, same radii)
 *   MI_BLUR_CONV_SAT : out = clamp( floor((acc + bias)            / 2^shift), 0, 255)
 *   MI_BLUR_CONV_ABS : out = clamp( floor((|acc| + bias)          / 2^shift), 0, 255)
 *   MI_BLUR_CONV_MAG : out = clamp( floor((|acc| + |acc2| + bias) / 2^shift), 0, 255)
 * bias is added before the shift (floor: towards minus infinity): rounding is bias = 1 << (shift - 1), an output offset of
 * 128 is 128 << shift; with bias = 0 the shift truncates like the blur kernels', so {1,2,1} x {1,2,1} with shift 4 in SAT
 * mode gives the bytes of radius 1.  A kernel is valid when the mode is known, 0 <= shift <= 16, |bias| <= 2^24 and
 * sum |K| <= 65535 (the same for K2 in MAG; k2 is ignored otherwise): then |acc| < 2^24, every intermediate stays below
 * 2^27, and 24-bit multiplies with 32-bit sums are exact.  An all-zero kernel is valid.  A table zero-padded to larger
 * radii gives the same bytes.  The GPU and the CPU device agree byte for byte.
 * ---------------------------------------------------------------------- */
#define MI_BLUR_CONV_MAX_RADIUS 7
typedef enum mi_blur_conv_mode { MI_BLUR_CONV_SAT = 0, MI_BLUR_CONV_ABS = 1, MI_BLUR_CONV_MAG = 2 } mi_blur_conv_mode;
typedef struct mi_blur_conv {
    int rx, ry;                       /* window (2 rx + 1) columns x (2 ry + 1) rows, each radius 0..7 */
    int mode;                         /* mi_blur_conv_mode */
    int shift;                        /* 0..16 */
    int32_t bias;                     /* |bias| <= 2^24, added before the shift */
    int16_t k[15 * 15], k2[15 * 15];  /* K[j][i] at k[(j + ry) * (2 rx + 1) + (i + rx)]; rest ignored; k2: MAG only */
} mi_blur_conv;

/* Ready kernels, 3x3, which the caller may then edit (all shift 0):
 *   SOBEL_X [-1 0 1; -2 0 2; -1 0 1] ABS     SOBEL_Y its transpose, ABS     SOBEL_MAG both, MAG
 *   SCHARR_X [-3 0 3; -10 0 10; -3 0 3] ABS  SCHARR_Y its transpose, ABS    SCHARR_MAG both, MAG
 *   LAPLACIAN4 [0 1 0; 1 -4 1; 0 1 0] ABS    LAPLACIAN8 [1 1 1; 1 -8 1; 1 1 1] ABS
 *   SHARPEN [0 -1 0; -1 5 -1; 0 -1 0] SAT    EMBOSS [-2 -1 0; -1 1 1; 0 1 2] SAT, bias 128 */
typedef enum mi_blur_conv_preset_id {
    MI_BLUR_CONV_SOBEL_X = 0, MI_BLUR_CONV_SOBEL_Y = 1, MI_BLUR_CONV_SOBEL_MAG = 2,
    MI_BLUR_CONV_SCHARR_X = 3, MI_BLUR_CONV_SCHARR_Y = 4, MI_BLUR_CONV_SCHARR_MAG = 5,
    MI_BLUR_CONV_LAPLACIAN4 = 6, MI_BLUR_CONV_LAPLACIAN8 = 7, MI_BLUR_CONV_SHARPEN = 8, MI_BLUR_CONV_EMBOSS = 9
} mi_blur_conv_preset_id;
/* MI_BLUR_ERR_INVALID: an unknown preset, a null k. */
int mi_blur_conv_preset(int preset, mi_blur_conv *k);

/* mi_blur_enqueue / mi_blur_enqueue_band with that convolution (same buffers, same band semantics: clamping at the band's
 * own edges, only rows [out_row_begin, out_row_end) written; asynchronous; n_images == 0 is MI_BLUR_OK).  The tables travel
 * in the kernel arguments: nothing is allocated, *k may change as soon as the call returns.  Rows of whole 16-byte chunks
 * at 16-byte aligned addresses with 1-4 channels take blur_conv_tiled_kernel at every radius pair, every other case
 * blur_conv_generic_kernel.  MI_BLUR_ERR_INVALID (before MI_BLUR_ERR_NO_DEVICE): a null or invalid k, null or equal
 * buffers, non-positive sizes. */
int mi_blur_enqueue_conv(const uint8_t *d_in, uint8_t *d_out, int width, int height, int channels, int n_images,
                         const mi_blur_conv *k, void *stream);
int mi_blur_enqueue_conv_band(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels,
                              int out_row_begin, int out_row_end, const mi_blur_conv *k, void *stream);
/* mi_blur_cpu_run with the convolution (plain integer loops, exact). */
int mi_blur_cpu_run_conv(const uint8_t *in, uint8_t *out, int width, int height, int channels, int n_images,
                         const mi_blur_conv *k, int n_threads);
/* Give a context that convolution in place of its blur, with the rules of mi_blur_ctx_set_bilateral: only before the
 * first submit (MI_BLUR_ERR_STATE after), every submit form then uses it, never through the batch server, resident runs
 * MI_BLUR_ERR_UNSUPPORTED.  It replaces what another setter set before.  The context keeps a copy.  A caller that works
 * in bands needs a halo of ry rows. */
int mi_blur_ctx_set_conv(mi_blur_ctx *ctx, const mi_blur_conv *k);

/* Developer diagnostics.  With mi_blur_set_option("debug_xcd_times", 1) every workgroup of the tiled kernel leaves its
 * start and end time (100 MHz ticks) in a slot of the XCD it ran on; this call waits for the device, returns per XCD the
 * LATEST end and the EARLIEST start seen since the last re-arm, and re-arms the slots when asked (call it once with
 * rearm = 1 before the launches to be examined).  Shows which XCD a launch waits for (profiles/r02_xcd_finish_times.txt). */
int mi_blur_debug_xcd_times(uint64_t end_ticks[8], uint64_t begin_ticks[8], int rearm);

/* The raw stamps behind mi_blur_debug_xcd_times: waits for the device and copies slots [first_slot, first_slot + n_slots) of the
 * 2^20 slots, two words each: (end tick << 4 | XCD) and the start tick of the workgroup of that number, 0 = not written.  A fused
 * pass with a dynamic tail of at most 65536 workgroups writes the region of 65536 slots numbered (its number among the context's
 * fused passes) mod 16, so that up to 16 back-to-back passes can be read together (profiles/r09_fused_overlap.md). */
int mi_blur_debug_xcd_raw(uint64_t *out, size_t first_slot, size_t n_slots);

/* Developer diagnostics of the zero-copy batch server (mi_blur_set_option("zero_copy_trace", 1) before the context's first
 * zero-copy submit): per worker workgroup and batch, for the context's first 512 batches — device clock (100 MHz ticks)
 * when it took its first tile of the batch, how many tiles it took, ticks spent inside tiles, device clock when its last
 * tile of the batch ended, (unused).  Copies out[batch][worker][5] for the first min(max_batches, 512, published) batches
 * and returns how many that is (negative = mi_blur_status).  profiles/r03_e2e_timeline.md is built from it. */
int mi_blur_debug_zc_trace(mi_blur_ctx *ctx, uint64_t *out, int max_batches, int *n_workers, unsigned *batches_published);

/* Synthetic stream generator shared by hosts, bench and tests. */
void mi_blur_fill_synthetic(uint8_t *host, int width, int height, int channels,
                            int first_index, int n_images, int n_threads);
uint64_t mi_blur_fnv1a64(const uint8_t *host, size_t n);

/* ------------------------------------------------------------------------
 * Work distribution helpers — host logic of the two approaches.
 * ---------------------------------------------------------------------- */
/* Approach 1, heterogeneous_blur.c:449-458: mode 0 both / 1 cpu / 2 gpu. */
void mi_blur_a1_partition(int mode, int batch_count, float gpu_ratio, int *n_cpu, int *n_gpu);
/* Image-level sharding over G devices: shard g owns [begin,end). */
void mi_blur_shard_range(long long n_units, int g, int G, long long *begin, long long *end);

typedef struct mi_blur_a2_geometry { /* split_image_blur.c:144-166 with HALO := halo */
    int split_row;
    int cpu_input_rows, cpu_output_rows;
    int gpu_input_rows, gpu_output_rows;
} mi_blur_a2_geometry;
void mi_blur_a2_split(int height, float gpu_ratio, int halo, mi_blur_a2_geometry *g);

typedef struct mi_blur_band {        /* K-way row split of one image over G devices */
    int row_begin, row_end;          /* owned output rows [begin,end) */
    int halo_top, halo_bottom;       /* halo rows needed from neighbour g-1 / g+1 (0 at image edge) */
} mi_blur_band;
void mi_blur_band_of(int height, int radius, int g, int G, mi_blur_band *b);

/* ------------------------------------------------------------------------
 * Approach 2 on resident row shards: halo rows move GPU<->GPU with RCCL
 * send/recv over xGMI (the reference instead re-uploads overlapping slices
 * from the host, split_image_blur.c:516,520,530).
 * One communicator rank per GPU; either one process per GPU
 * (mi_blur_comm_unique_id on rank 0, broadcast the 128 bytes by any means,
 * mi_blur_comm_init_rank everywhere) or all ranks in one process
 * (mi_blur_comm_init_all).
 * ---------------------------------------------------------------------- */
typedef struct mi_blur_comm mi_blur_comm;
#define MI_BLUR_UNIQUE_ID_BYTES 128
int mi_blur_comm_unique_id(uint8_t id[MI_BLUR_UNIQUE_ID_BYTES]);
int mi_blur_comm_init_rank(mi_blur_comm **comm, int n_ranks, int rank, const uint8_t id[MI_BLUR_UNIQUE_ID_BYTES]);
int mi_blur_comm_init_all(mi_blur_comm **comms, int n_devices, const int *devices);
/* Single-process set that moves halo rows with hipMemcpyPeerAsync instead of RCCL (fallback transport; also the
 * only one that accepts several ranks on one device).  Use with mi_blur_halo_exchange_all. */
int mi_blur_comm_init_p2p(mi_blur_comm **comms, int n_devices, const int *devices);
/* The same single-process set with the halo rows PULLED by one small kernel per rank (mi_blur_halo_pull's) instead of pushed
 * with two peer copies; ordering by the same events.  Use with mi_blur_halo_exchange_all. */
int mi_blur_comm_init_pull(mi_blur_comm **comms, int n_devices, const int *devices);
void mi_blur_comm_destroy(mi_blur_comm *comm);
/* What the communicator is, as its transport reports it: *n_ranks / *rank from ncclCommCount / ncclCommUserRank for an
 * RCCL communicator (the numbers a report should quote for "RCCL carried the halos over N ranks"), the construction
 * arguments otherwise; *transport 0 = none (a single rank: both image edges clamp), 1 = RCCL, 2 = peer copies, 3 = pulled by a kernel.
 * Any out pointer may be NULL. */
int mi_blur_comm_info(mi_blur_comm *comm, int *n_ranks, int *rank, int *transport);

/* d_band: this rank's shard laid out as [halo_top rows][owned rows][halo_bottom rows]
 * (halo_* from mi_blur_band_of; absent halos have zero rows).  Sends the first/last
 * `radius` OWNED rows to rank-1 / rank+1 and receives their mirror into the halo
 * rows, in one RCCL group on `stream`.  Asynchronous. */
int mi_blur_halo_exchange(mi_blur_comm *comm, uint8_t *d_band, int width, int channels,
                          int owned_rows, int radius, void *stream);

/* A second way to fill the halo rows, for hosts that can hand device pointers between ranks: each rank PULLS its halo rows
 * out of its neighbours' shards with a small copy kernel that reads the peer's memory directly (over xGMI between GPUs) —
 * no collective library in the step, one ~4 us launch instead of a send/recv pair.  One process per GPU: every rank exports
 * its shard (mi_blur_peer_export: a 64-byte IPC handle of the allocation + the shard's offset inside it), the handles travel
 * by any means (bench.py: an all_gather), each rank opens its neighbours' (mi_blur_peer_open) and from then on calls
 * mi_blur_halo_pull(d_band, top_src, bottom_src, ...) per step with top_src = address of the LAST `radius` owned rows of rank
 * g-1's shard and bottom_src = the FIRST `radius` owned rows of rank g+1's (NULL where there is no neighbour).  A rank may
 * only pull rows its neighbour is not writing at the time: for the repeated blur of one resident image (BASELINE configs[4])
 * the owned rows never change; an iterated blur needs a cross-rank barrier per step (not provided here).
 * mi_blur_peer_close when done, before the owner frees the shard. */
#define MI_BLUR_PEER_HANDLE_BYTES 64
int mi_blur_peer_export(const void *d_ptr, uint8_t handle[MI_BLUR_PEER_HANDLE_BYTES], uint64_t *offset);
int mi_blur_peer_open(const uint8_t handle[MI_BLUR_PEER_HANDLE_BYTES], uint64_t offset, void **d_ptr);
int mi_blur_peer_close(void *d_ptr, uint64_t offset);
int mi_blur_halo_pull(uint8_t *d_band, const uint8_t *top_src, const uint8_t *bottom_src, int width, int channels,
                      int owned_rows, int radius, void *stream);
/* The step as ONE launch: mi_blur_enqueue_band whose kernel reads band rows [0, out_row_begin) from top_src and rows
 * [out_row_end, band_rows) from bottom_src (each laid out as that many rows, e.g. the same peer addresses mi_blur_halo_pull
 * takes when out_row_begin = radius) instead of from d_in — the halo rows of d_in are never read or written, the neighbours'
 * rows cross xGMI inside the blur kernel's own loads.  NULL for a side = that side's rows come from d_in as usual (both NULL =
 * mi_blur_enqueue_band).  Same rule as the pull: the neighbours must not be writing those rows.  Shapes of the direct kernel
 * only (1-4 channels, rows a multiple of 16 bytes, 16-byte aligned pointers; MI_BLUR_ERR_UNSUPPORTED otherwise — use
 * mi_blur_halo_pull + mi_blur_enqueue_band then). */
int mi_blur_enqueue_band_peer(const uint8_t *d_in, uint8_t *d_out, int width, int band_rows, int channels, int radius,
                              int out_row_begin, int out_row_end, const uint8_t *top_src, const uint8_t *bottom_src,
                              void *stream);

/* Single-process form: all n ranks of a mi_blur_comm_init_all set in one RCCL group. */
int mi_blur_halo_exchange_all(mi_blur_comm **comms, int n, uint8_t **d_bands, int width, int channels,
                              const int *owned_rows, int radius, void **streams);

#ifdef __cplusplus
}
#endif
#endif /* MI_BLUR_H */
