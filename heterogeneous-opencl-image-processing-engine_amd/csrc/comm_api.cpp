// comm_api.cpp — the multi-GPU part of the C ABI declared in include/mi_blur.h: communicators (RCCL, lazily
// dlopen'ed, or single-process peer copies), the halo exchange between row shards, peer memory handles.
#include "api_internal.h"
#include "blur_launch.h"

#include <rccl/rccl.h>

#include <dlfcn.h>

#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace mi_blur;

// ----------------------------------------------------------------------------------
// RCCL halo exchange (Approach 2 on resident row shards)
// ----------------------------------------------------------------------------------
namespace {

struct Rccl {
    void *h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    bool ok = false;
};

Rccl &rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        // A process that already holds an RCCL (torch's bundled librccl.so has no soname and is registered under
        // that name) must keep using that one: a second copy would sit on the same HIP runtime.
        for (const char *name : {"librccl.so", "librccl.so.1"}) {
            r.h = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
            if (r.h) break;
        }
        if (!r.h)
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
                r.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
                if (r.h) break;
            }
        if (!r.h) return;
#define MI_SYM(field, sym) r.field = (decltype(r.field))dlsym(r.h, #sym)
        MI_SYM(GetUniqueId, ncclGetUniqueId);
        MI_SYM(CommInitRank, ncclCommInitRank);
        MI_SYM(CommInitAll, ncclCommInitAll);
        MI_SYM(CommDestroy, ncclCommDestroy);
        MI_SYM(CommCount, ncclCommCount);
        MI_SYM(CommUserRank, ncclCommUserRank);
        MI_SYM(Send, ncclSend);
        MI_SYM(Recv, ncclRecv);
        MI_SYM(GroupStart, ncclGroupStart);
        MI_SYM(GroupEnd, ncclGroupEnd);
#undef MI_SYM
        r.ok = r.GetUniqueId && r.CommInitRank && r.CommInitAll && r.CommDestroy && r.Send && r.Recv &&
               r.GroupStart && r.GroupEnd;
    });
    return r;
}

inline int nccl_status(ncclResult_t e) { return e == ncclSuccess ? MI_BLUR_OK : MI_BLUR_ERR_RCCL_BASE - (int)e; }

}  // namespace

struct mi_blur_comm {
    ncclComm_t comm = nullptr;
    int n_ranks = 1, rank = 0, device = -1;
    bool p2p = false;                            // single-process copy transport instead of RCCL
    bool pull = false;                           // ... whose copies are PULLS: one small kernel per rank reads the neighbours' rows
    hipEvent_t ev_prev = nullptr, ev_push = nullptr;
};

static_assert(sizeof(ncclUniqueId) == MI_BLUR_UNIQUE_ID_BYTES, "ncclUniqueId size");

extern "C" int mi_blur_comm_unique_id(uint8_t id[MI_BLUR_UNIQUE_ID_BYTES])
{
    if (!id) return MI_BLUR_ERR_INVALID;
    Rccl &r = rccl();
    if (!r.ok) return MI_BLUR_ERR_UNSUPPORTED;
    ncclUniqueId u;
    int rc = nccl_status(r.GetUniqueId(&u));
    if (rc) return rc;
    memcpy(id, &u, sizeof u);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_comm_init_rank(mi_blur_comm **comm, int n_ranks, int rank,
                                      const uint8_t id[MI_BLUR_UNIQUE_ID_BYTES])
{
    if (!comm || !id || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return MI_BLUR_ERR_INVALID;
    *comm = nullptr;
    mi_blur_comm *c = new (std::nothrow) mi_blur_comm;
    if (!c) return MI_BLUR_ERR_NOMEM;
    c->n_ranks = n_ranks; c->rank = rank;
    if (hipGetDevice(&c->device) != hipSuccess) { (void)hipGetLastError(); delete c; return MI_BLUR_ERR_NO_DEVICE; }
    if (n_ranks > 1) {
        Rccl &r = rccl();
        if (!r.ok) { delete c; return MI_BLUR_ERR_UNSUPPORTED; }
        ncclUniqueId u;
        memcpy(&u, id, sizeof u);
        int rc = nccl_status(r.CommInitRank(&c->comm, n_ranks, u, rank));
        if (rc) { delete c; return rc; }
    }
    *comm = c;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_comm_init_all(mi_blur_comm **comms, int n_devices, const int *devices)
{
    if (!comms || n_devices <= 0) return MI_BLUR_ERR_INVALID;
    std::vector<ncclComm_t> raw(n_devices, nullptr);
    std::vector<int> devs(n_devices);
    for (int i = 0; i < n_devices; i++) devs[i] = devices ? devices[i] : i;
    if (n_devices > 1) {
        Rccl &r = rccl();
        if (!r.ok) return MI_BLUR_ERR_UNSUPPORTED;
        int rc = nccl_status(r.CommInitAll(raw.data(), n_devices, devs.data()));
        if (rc) return rc;
    }
    for (int i = 0; i < n_devices; i++) comms[i] = nullptr;
    for (int i = 0; i < n_devices; i++) {
        mi_blur_comm *c = new (std::nothrow) mi_blur_comm;
        if (!c) {
            // give back everything made so far: the wrappers already built (each destroys its RCCL communicator)
            // and the raw communicators that have no wrapper yet
            for (int j = 0; j < i; j++) { mi_blur_comm_destroy(comms[j]); comms[j] = nullptr; }
            for (int j = i; j < n_devices; j++) if (raw[j]) (void)rccl().CommDestroy(raw[j]);
            return MI_BLUR_ERR_NOMEM;
        }
        c->comm = raw[i]; c->n_ranks = n_devices; c->rank = i; c->device = devs[i];
        comms[i] = c;
    }
    return MI_BLUR_OK;
}

// Single-process communicator set whose halo rows move with hipMemcpyPeerAsync instead of RCCL: the
// fallback when RCCL is unavailable, and what lets the row-shard flow run with several shards per device.
extern "C" int mi_blur_comm_init_p2p(mi_blur_comm **comms, int n_devices, const int *devices)
{
    if (!comms || n_devices <= 0) return MI_BLUR_ERR_INVALID;
    const int ndev = mi_blur_device_count();
    if (ndev <= 0) return MI_BLUR_ERR_NO_DEVICE;
    for (int i = 0; i < n_devices; i++) comms[i] = nullptr;
    // any failure gives back every rank made so far (mi_blur_comm_destroy releases the events a rank already holds)
    auto fail = [&](int rc) {
        for (int j = 0; j < n_devices; j++) { mi_blur_comm_destroy(comms[j]); comms[j] = nullptr; }
        return rc;
    };
    for (int i = 0; i < n_devices; i++) {
        mi_blur_comm *c = new (std::nothrow) mi_blur_comm;
        if (!c) return fail(MI_BLUR_ERR_NOMEM);
        c->n_ranks = n_devices; c->rank = i; c->device = devices ? devices[i] : i; c->p2p = true;
        comms[i] = c;
        if (c->device < 0 || c->device >= ndev) return fail(MI_BLUR_ERR_NO_DEVICE);
        hipError_t e = hipSetDevice(c->device);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_prev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_push, hipEventDisableTiming);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(MI_BLUR_ERR_HIP_BASE - (int)e); }
    }
    for (int i = 0; i + 1 < n_devices; i++) {     // neighbours on different devices: enable direct access both ways (best effort)
        const int a = comms[i]->device, b = comms[i + 1]->device;
        if (a == b) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) { (void)hipSetDevice(a); (void)hipDeviceEnablePeerAccess(b, 0); }
        if (hipDeviceCanAccessPeer(&can, b, a) == hipSuccess && can) { (void)hipSetDevice(b); (void)hipDeviceEnablePeerAccess(a, 0); }
        (void)hipGetLastError();
    }
    return MI_BLUR_OK;
}

// The same single-process set with the halo rows PULLED: every rank runs one small kernel (mi_blur_halo_pull's) that reads its
// neighbours' edge rows through peer access, instead of pushing its own with two hipMemcpyPeerAsync.
extern "C" int mi_blur_comm_init_pull(mi_blur_comm **comms, int n_devices, const int *devices)
{
    const int rc = mi_blur_comm_init_p2p(comms, n_devices, devices);
    if (rc) return rc;
    for (int i = 0; i < n_devices; i++) comms[i]->pull = true;
    return MI_BLUR_OK;
}

// What a communicator IS, as the transport itself reports it: a bench line that says "RCCL carried the halos over N
// ranks" quotes ncclCommCount / ncclCommUserRank, not the number it asked for.
extern "C" int mi_blur_comm_info(mi_blur_comm *c, int *n_ranks, int *rank, int *transport)
{
    if (!c) return MI_BLUR_ERR_INVALID;
    int n = c->n_ranks, r = c->rank, t = c->pull ? 3 : c->p2p ? 2 : (c->comm ? 1 : 0);
    if (c->comm) {
        Rccl &rc = rccl();
        if (!rc.ok || !rc.CommCount || !rc.CommUserRank) return MI_BLUR_ERR_UNSUPPORTED;
        int e = nccl_status(rc.CommCount(c->comm, &n));
        if (!e) e = nccl_status(rc.CommUserRank(c->comm, &r));
        if (e) return e;
    }
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    if (transport) *transport = t;
    return MI_BLUR_OK;
}

extern "C" void mi_blur_comm_destroy(mi_blur_comm *c)
{
    if (!c) return;
    if (c->comm) (void)rccl().CommDestroy(c->comm);
    if (c->ev_prev || c->ev_push) {
        (void)hipSetDevice(c->device);
        if (c->ev_prev) (void)hipEventDestroy(c->ev_prev);
        if (c->ev_push) (void)hipEventDestroy(c->ev_push);
    }
    delete c;
}

static int halo_exchange_calls(Rccl &r, mi_blur_comm *c, uint8_t *d_band, size_t pitch, int owned_rows, int radius,
                               hipStream_t stream)
{
    const int top = c->rank > 0 ? radius : 0;
    const size_t n = pitch * (size_t)radius;
    ncclResult_t e = ncclSuccess;
    if (c->rank > 0) {
        if ((e = r.Send(d_band + (size_t)top * pitch, n, ncclUint8, c->rank - 1, c->comm, stream)) != ncclSuccess) return nccl_status(e);
        if ((e = r.Recv(d_band, n, ncclUint8, c->rank - 1, c->comm, stream)) != ncclSuccess) return nccl_status(e);
    }
    if (c->rank < c->n_ranks - 1) {
        uint8_t *last = d_band + (size_t)(top + owned_rows - radius) * pitch;
        if ((e = r.Send(last, n, ncclUint8, c->rank + 1, c->comm, stream)) != ncclSuccess) return nccl_status(e);
        if ((e = r.Recv(d_band + (size_t)(top + owned_rows) * pitch, n, ncclUint8, c->rank + 1, c->comm, stream)) != ncclSuccess) return nccl_status(e);
    }
    return MI_BLUR_OK;
}

extern "C" int mi_blur_halo_exchange(mi_blur_comm *c, uint8_t *d_band, int width, int channels, int owned_rows,
                                     int radius, void *stream)
{
    if (!c || !d_band || width <= 0 || channels <= 0 || radius < 1 || owned_rows < radius) return MI_BLUR_ERR_INVALID;
    if (c->n_ranks == 1) return MI_BLUR_OK;            // nothing to exchange: both edges clamp
    if (c->p2p) return MI_BLUR_ERR_STATE;              // the copy transport needs every rank: mi_blur_halo_exchange_all
    Rccl &r = rccl();
    if (!r.ok || !c->comm) return MI_BLUR_ERR_UNSUPPORTED;
    int rc = nccl_status(r.GroupStart());
    if (rc) return rc;
    rc = halo_exchange_calls(r, c, d_band, (size_t)width * channels, owned_rows, radius, (hipStream_t)stream);
    int rc2 = nccl_status(r.GroupEnd());
    return rc ? rc : rc2;
}

// ----------------------------------------------------------------------------------
// Halo pull: a rank reads its halo rows straight out of its neighbours' shards (peer memory) with one small kernel.
// ----------------------------------------------------------------------------------
static_assert(sizeof(hipIpcMemHandle_t) == MI_BLUR_PEER_HANDLE_BYTES, "hipIpcMemHandle_t size");

extern "C" int mi_blur_peer_export(const void *d_ptr, uint8_t handle[MI_BLUR_PEER_HANDLE_BYTES], uint64_t *offset)
{
    if (!d_ptr || !handle || !offset) return MI_BLUR_ERR_INVALID;
    if (mi_blur_device_count() <= 0) return MI_BLUR_ERR_NO_DEVICE;
    // the handle names a whole allocation; callers (torch's caching allocator, for one) hand out pieces of bigger ones
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    HIP_TRY(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_ptr));
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, base));
    memcpy(handle, &h, sizeof h);
    *offset = (uint64_t)((const uint8_t *)d_ptr - (const uint8_t *)base);
    return MI_BLUR_OK;
}

extern "C" int mi_blur_peer_open(const uint8_t handle[MI_BLUR_PEER_HANDLE_BYTES], uint64_t offset, void **d_ptr)
{
    if (!handle || !d_ptr) return MI_BLUR_ERR_INVALID;
    *d_ptr = nullptr;
    if (mi_blur_device_count() <= 0) return MI_BLUR_ERR_NO_DEVICE;
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof h);
    void *base = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess));
    *d_ptr = (uint8_t *)base + offset;
    return MI_BLUR_OK;
}

extern "C" int mi_blur_peer_close(void *d_ptr, uint64_t offset)
{
    if (!d_ptr) return MI_BLUR_OK;
    HIP_TRY(hipIpcCloseMemHandle((uint8_t *)d_ptr - offset));
    return MI_BLUR_OK;
}

extern "C" int mi_blur_halo_pull(uint8_t *d_band, const uint8_t *top_src, const uint8_t *bottom_src, int width, int channels,
                                 int owned_rows, int radius, void *stream)
{
    if (!d_band || width <= 0 || channels <= 0 || radius < 1 || owned_rows < radius) return MI_BLUR_ERR_INVALID;
    if (mi_blur_device_count() <= 0) return MI_BLUR_ERR_NO_DEVICE;
    const size_t pitch = (size_t)width * channels, n = pitch * (size_t)radius;
    const size_t top = top_src ? (size_t)radius : 0;                      // layout: [halo_top rows][owned rows][halo_bottom rows]
    return launch_halo_pull(top_src, d_band, bottom_src, d_band + (top + (size_t)owned_rows) * pitch, n, (hipStream_t)stream);
}

// All ranks of a single-process communicator set in ONE RCCL group (one host thread
// driving G GPUs must not block on rank 0's group before enqueuing rank 1's).
extern "C" int mi_blur_halo_exchange_all(mi_blur_comm **comms, int n, uint8_t **d_bands, int width, int channels,
                                         const int *owned_rows, int radius, void **streams)
{
    if (!comms || !d_bands || !owned_rows || n <= 0) return MI_BLUR_ERR_INVALID;
    if (n == 1) return MI_BLUR_OK;
    for (int i = 0; i < n; i++) if (!comms[i] || owned_rows[i] < radius) return MI_BLUR_ERR_INVALID;
    if (comms[0]->p2p) {
        // Same rows, same offsets as the RCCL form; each rank PUSHES its edge rows into its neighbours' halo rows on
        // its own stream.  Ordering by events: a push waits until the neighbour has finished whatever it queued
        // before this call (its previous blur may still read those halo rows); a rank's later work waits for the
        // pushes into its halos.
        const size_t pitch = (size_t)width * channels, nbytes = pitch * (size_t)radius;
        auto st = [&](int i) { return streams ? (hipStream_t)streams[i] : (hipStream_t) nullptr; };
        auto top = [&](int i) { return i > 0 ? radius : 0; };
        for (int i = 0; i < n; i++) {
            HIP_TRY(hipSetDevice(comms[i]->device));
            HIP_TRY(hipEventRecord(comms[i]->ev_prev, st(i)));
        }
        for (int i = 0; i < n; i++) {
            HIP_TRY(hipSetDevice(comms[i]->device));
            if (comms[0]->pull) {
                // PULL: rank i reads the last owned rows of rank i-1 and the first owned rows of rank i+1 into its own halo rows
                // with one kernel on its own stream, once both neighbours have finished what they queued before this call
                // (their owned rows are final).  ev_push(i) = "rank i has read its neighbours' rows": they wait for it below
                // before anything they queue later may overwrite those rows.
                const uint8_t *top_src = nullptr, *bottom_src = nullptr;
                if (i > 0) {
                    HIP_TRY(hipStreamWaitEvent(st(i), comms[i - 1]->ev_prev, 0));
                    top_src = d_bands[i - 1] + (size_t)(top(i - 1) + owned_rows[i - 1] - radius) * pitch;
                }
                if (i < n - 1) {
                    HIP_TRY(hipStreamWaitEvent(st(i), comms[i + 1]->ev_prev, 0));
                    bottom_src = d_bands[i + 1] + (size_t)top(i + 1) * pitch;
                }
                const int rc = launch_halo_pull(top_src, d_bands[i], bottom_src, d_bands[i] + (size_t)(top(i) + owned_rows[i]) * pitch, nbytes, st(i));
                if (rc) return rc;
                HIP_TRY(hipEventRecord(comms[i]->ev_push, st(i)));
                continue;
            }
            if (i > 0) {          // first owned rows -> bottom halo of rank i-1
                HIP_TRY(hipStreamWaitEvent(st(i), comms[i - 1]->ev_prev, 0));
                uint8_t *dst = d_bands[i - 1] + (size_t)(top(i - 1) + owned_rows[i - 1]) * pitch;
                HIP_TRY(hipMemcpyPeerAsync(dst, comms[i - 1]->device, d_bands[i] + (size_t)top(i) * pitch, comms[i]->device, nbytes, st(i)));
            }
            if (i < n - 1) {      // last owned rows -> top halo of rank i+1
                HIP_TRY(hipStreamWaitEvent(st(i), comms[i + 1]->ev_prev, 0));
                const uint8_t *src = d_bands[i] + (size_t)(top(i) + owned_rows[i] - radius) * pitch;
                HIP_TRY(hipMemcpyPeerAsync(d_bands[i + 1], comms[i + 1]->device, src, comms[i]->device, nbytes, st(i)));
            }
            HIP_TRY(hipEventRecord(comms[i]->ev_push, st(i)));
        }
        for (int i = 0; i < n; i++) {
            HIP_TRY(hipSetDevice(comms[i]->device));
            if (i > 0) HIP_TRY(hipStreamWaitEvent(st(i), comms[i - 1]->ev_push, 0));
            if (i < n - 1) HIP_TRY(hipStreamWaitEvent(st(i), comms[i + 1]->ev_push, 0));
        }
        return MI_BLUR_OK;
    }
    Rccl &r = rccl();
    if (!r.ok) return MI_BLUR_ERR_UNSUPPORTED;
    int rc = nccl_status(r.GroupStart());
    if (rc) return rc;
    for (int i = 0; i < n && !rc; i++) {
        if (hipSetDevice(comms[i]->device) != hipSuccess) { (void)hipGetLastError(); rc = MI_BLUR_ERR_NO_DEVICE; break; }
        rc = halo_exchange_calls(r, comms[i], d_bands[i], (size_t)width * channels, owned_rows[i], radius,
                                 streams ? (hipStream_t)streams[i] : nullptr);
    }
    int rc2 = nccl_status(r.GroupEnd());
    return rc ? rc : rc2;
}
