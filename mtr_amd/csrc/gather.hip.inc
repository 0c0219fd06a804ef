// gather.hip.inc — the ONE exchange of the multi-GPU path (include/mtr_hip.h, "several GPUs in ONE process"): the wire-form record tables of
// every GPU travel device to device to the first GPU over RCCL (xGMI), from there in one copy to pinned host memory, where the host chains and
// prints (reference chaining.cpp; the per-read loop they replace: handle_one_file.c:281-287).  Host code of libmtr_hip.so; included by mtr_abi.hip.
//
// One process, one communicator per GPU (ncclCommInitAll), point-to-point ncclSend / ncclRecv inside ONE group per exchange: a gather of
// variable-length tables has no fixed-size collective, and xGMI is point to point anyway.  librccl.so is bound with dlopen here and nowhere else:
// a single-GPU process never pays for loading it, and libmtr_hip.so has no link-time dependency on it.
//
// RCCL comes up in the BACKGROUND.  [measured, MI355X box, mTR -g 1 on 100 000 reads] loading librccl.so and ncclCommInitAll take 2.2 s - three times
// the whole job (0.71 s) - so mtr_gather_create returns at once and a thread of its own brings the communicators up while the GPUs already work;
// an exchange that finds RCCL not up yet (or not usable at all) moves its tables from every GPU's staging buffer straight to the pinned host buffer
// (one copy per table on the owner's stream, the GPUs' PCIe links side by side) and the job never waits for the library.  mtr_gather_wait_ready
// blocks until RCCL is up for callers that want every exchange on it (tests, the bench's RCCL leg).
#pragma once
#include <dlfcn.h>
#include <atomic>
#include <thread>
#include <rccl/rccl.h>

struct GatherSlot { void *d = nullptr; size_t cap = 0; int64_t bytes = 0; bool busy = false; };
struct GatherRank { int device = 0; hipStream_t stream = nullptr; ncclComm_t comm = nullptr; std::vector<GatherSlot> slots; };
struct mtr_gather {
    int n = 0;
    std::vector<GatherRank> ranks;
    std::mutex mu;                       // the slot tables (mtr_gather_stage runs on every GPU's host thread)
    std::string err;
    void *dl = nullptr;
    void *d_recv = nullptr; size_t recv_cap = 0;      // on the first GPU: where the other GPUs' tables land
    void *h_buf = nullptr; size_t h_cap = 0;          // pinned host memory: what mtr_gather_exchange hands out
    bool self_send = false;              // MTR_GATHER_SELF=1: the first GPU's own tables go through ncclSend / ncclRecv to itself too
    long long n_exchanges = 0, n_exchanges_rccl = 0, bytes_rccl = 0, bytes_local = 0;
    std::thread init_thread;             // dlopen(librccl) + ncclCommInitAll
    std::atomic<int> ready{0};           // 0: RCCL is coming up, 1: up, -1: not usable (rccl_err says why)
    std::string rccl_err;
    double init_seconds = 0;
    std::vector<int> devices;
    // librccl
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
};
#define GATHER_SLOTS_PER_RANK 1024
#define GHIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { g->err = std::string(#call) + ": " + hipGetErrorString(e_); return MTR_ERR_HIP; } } while (0)
#define GNCCL(call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) { g->err = std::string(#call) + ": " + (g->GetErrorString ? g->GetErrorString(r_) : "RCCL error"); return MTR_ERR_HIP; } } while (0)

extern "C" mtr_status mtr_device_count(int32_t *out_count)
{
    if (!out_count) return MTR_ERR_BAD_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { *out_count = 0; return MTR_ERR_NO_DEVICE; }
    *out_count = n;
    return MTR_OK;
}

extern "C" const char *mtr_gather_last_error(const mtr_gather *g) { return g ? g->err.c_str() : "no gather"; }

extern "C" void mtr_gather_destroy(mtr_gather *g)
{
    if (!g) return;
    if (g->ready.load(std::memory_order_acquire) == 0) {
        // RCCL is still coming up (a job shorter than the library's start-up): its thread keeps using *g, so the object is left to the process's
        // end and nobody waits 2 s for a library the job no longer needs.  The caller should leave through _exit (mtr_gather_get_stats [5] == 0
        // says so): tearing the runtime down under a thread inside ncclCommInitAll is not safe.
        if (g->init_thread.joinable()) g->init_thread.detach();
        return;
    }
    if (g->init_thread.joinable()) g->init_thread.join();
    for (auto &r : g->ranks) {
        (void)hipSetDevice(r.device);
        if (r.stream) (void)hipStreamSynchronize(r.stream);
        if (r.comm && g->CommDestroy) (void)g->CommDestroy(r.comm);
        for (auto &s : r.slots) if (s.d) (void)hipFree(s.d);
        if (r.stream) (void)hipStreamDestroy(r.stream);
    }
    if (!g->ranks.empty()) (void)hipSetDevice(g->ranks[0].device);
    if (g->d_recv) (void)hipFree(g->d_recv);
    if (g->h_buf) (void)hipHostFree(g->h_buf);
    // (librccl stays mapped: unloading it at exit races with its own teardown, like the HIP code object of this library)
    delete g;
}

extern "C" mtr_status mtr_gather_create(int32_t n_ranks, const int32_t *devices, mtr_gather **out)
{
    if (!out) return MTR_ERR_BAD_ARG;
    *out = nullptr;
    if (n_ranks <= 0 || n_ranks > 64 || !devices) return MTR_ERR_BAD_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MTR_ERR_NO_DEVICE;
    mtr_gather *g = new (std::nothrow) mtr_gather();
    if (!g) return MTR_ERR_OOM;
    *out = g;                            // (handed out even on failure: the caller reads the reason, then destroys it)
    g->n = n_ranks;
    g->ranks.resize((size_t)n_ranks);
    const char *self = getenv("MTR_GATHER_SELF");
    g->self_send = self && atoi(self) != 0;
    g->devices.assign(devices, devices + n_ranks);
    for (int r = 0; r < n_ranks; r++) {
        if (devices[r] < 0 || devices[r] >= ndev) { g->err = "device " + std::to_string(devices[r]) + " of rank " + std::to_string(r) + " does not exist"; return MTR_ERR_NO_DEVICE; }
        g->ranks[(size_t)r].device = devices[r];
    }
    // RCCL in the background: the library (hundreds of MB of code objects) and the communicators
    g->init_thread = std::thread([g]() {
        const auto t0 = std::chrono::steady_clock::now();
        auto fail = [&](const std::string &why) { g->rccl_err = why; g->ready.store(-1, std::memory_order_release); };
        for (int r = 0; r < g->n; r++) for (int q = 0; q < r; q++) if (g->devices[(size_t)q] == g->devices[(size_t)r])
            return fail("device " + std::to_string(g->devices[(size_t)r]) + " is given to two ranks: RCCL takes a device once per communicator");
        const char *names[] = { getenv("MTR_RCCL_LIB"), "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so" };
        for (const char *nm : names) { if (nm && *nm && !g->dl) g->dl = dlopen(nm, RTLD_NOW | RTLD_LOCAL); }
        if (!g->dl) { const char *de = dlerror(); return fail(std::string("librccl.so could not be loaded: ") + (de ? de : "?")); }
#define GBIND(field, name) do { *(void **)(&g->field) = dlsym(g->dl, name); if (!g->field) return fail(std::string("librccl.so does not export ") + name); } while (0)
        GBIND(GetErrorString, "ncclGetErrorString"); GBIND(CommInitAll, "ncclCommInitAll"); GBIND(CommDestroy, "ncclCommDestroy");
        GBIND(GroupStart, "ncclGroupStart"); GBIND(GroupEnd, "ncclGroupEnd"); GBIND(Send, "ncclSend"); GBIND(Recv, "ncclRecv");
#undef GBIND
        std::vector<ncclComm_t> comms((size_t)g->n);
        const ncclResult_t rc = g->CommInitAll(comms.data(), g->n, g->devices.data());
        if (rc != ncclSuccess) return fail(std::string("ncclCommInitAll: ") + g->GetErrorString(rc));
        for (int r = 0; r < g->n; r++) g->ranks[(size_t)r].comm = comms[(size_t)r];
        g->init_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        g->ready.store(1, std::memory_order_release);
    });
    return MTR_OK;
}

extern "C" mtr_status mtr_gather_wait_ready(mtr_gather *g)
{
    if (!g) return MTR_ERR_BAD_ARG;
    if (g->init_thread.joinable()) g->init_thread.join();
    if (g->ready.load(std::memory_order_acquire) == 1) return MTR_OK;
    g->err = g->rccl_err.empty() ? "RCCL is not up" : g->rccl_err;
    return MTR_ERR_NO_DEVICE;
}

// out[0] exchanges that went over RCCL, [1] exchanges that went straight to the host (RCCL not up yet / not usable), [2] bytes over RCCL, [3] bytes
// copied straight to the host, [4] milliseconds RCCL took to come up (0 while it has not), [5] 1 = up, 0 = coming up, -1 = not usable
extern "C" mtr_status mtr_gather_get_stats(const mtr_gather *g, int64_t *out, int32_t n)
{
    if (!g || !out) return MTR_ERR_BAD_ARG;
    const int64_t v[6] = { g->n_exchanges_rccl, g->n_exchanges - g->n_exchanges_rccl, g->bytes_rccl, g->bytes_local, (int64_t)(g->init_seconds * 1e3), g->ready.load() };
    for (int i = 0; i < n && i < 6; i++) out[i] = v[i];
    return MTR_OK;
}

// wire_form of mtr_abi.hip: the finished batch of `ctx` -> a staging buffer on the same device
extern "C" mtr_status mtr_gather_stage(mtr_gather *g, int32_t rank, mtr_ctx *ctx, int32_t *counts_host, int64_t *out_total_records,
                                       int64_t *out_bytes, int32_t *out_ticket)
{
    if (!g || !ctx || !counts_host || !out_total_records || !out_bytes || !out_ticket || rank < 0 || rank >= g->n) return MTR_ERR_BAD_ARG;
    if (ctx->device != g->ranks[(size_t)rank].device) { ctx->err = "the context lives on device " + std::to_string(ctx->device) + ", rank " + std::to_string(rank) + " of the gather on " + std::to_string(g->ranks[(size_t)rank].device); return MTR_ERR_BAD_ARG; }
    { mtr_status r = results_ready(ctx, false); if (r != MTR_OK) return r; }
    HIPCHK(hipSetDevice(ctx->device));
    GatherRank &gr = g->ranks[(size_t)rank];
    int slot = -1;
    auto release = [&]() { std::lock_guard<std::mutex> lk(g->mu); gr.slots[(size_t)slot].busy = false; };
    // a free slot of this rank that is large enough, else the smallest free one grown, else a new one
    auto take_slot = [&](int64_t bytes, uint8_t **out) {
        void *old = nullptr;
        {
            std::lock_guard<std::mutex> lk(g->mu);
            for (size_t i = 0; i < gr.slots.size(); i++) if (!gr.slots[i].busy && gr.slots[i].cap >= (size_t)bytes && (slot < 0 || gr.slots[i].cap < gr.slots[(size_t)slot].cap)) slot = (int)i;
            if (slot < 0) for (size_t i = 0; i < gr.slots.size(); i++) if (!gr.slots[i].busy) { slot = (int)i; break; }
            if (slot < 0) {
                if (gr.slots.size() >= GATHER_SLOTS_PER_RANK) { ctx->err = "too many staged tables wait for an exchange"; return MTR_ERR_OVERFLOW; }
                gr.slots.emplace_back(); slot = (int)gr.slots.size() - 1;
            }
            gr.slots[(size_t)slot].busy = true; gr.slots[(size_t)slot].bytes = bytes;
            if (gr.slots[(size_t)slot].cap < (size_t)bytes) { old = gr.slots[(size_t)slot].d; gr.slots[(size_t)slot].d = nullptr; gr.slots[(size_t)slot].cap = 0; }
        }
        if (old) (void)hipFree(old);
        void *d = nullptr; size_t cap = 0;
        { std::lock_guard<std::mutex> lk(g->mu); d = gr.slots[(size_t)slot].d; cap = gr.slots[(size_t)slot].cap; }
        if (cap < (size_t)bytes || !d) {
            const size_t want = std::max<size_t>((size_t)bytes * 5 / 4, (size_t)1 << 20);
            if (hipMalloc(&d, want) != hipSuccess) { ctx->err = "cannot allocate a staging buffer of " + std::to_string(want) + " bytes"; return MTR_ERR_OOM; }
            std::lock_guard<std::mutex> lk(g->mu);
            gr.slots[(size_t)slot].d = d; gr.slots[(size_t)slot].cap = want;
        }
        *out = (uint8_t *)d;
        return MTR_OK;
    };
    const mtr_status st = wire_form(ctx, ctx->n_reads, counts_host, out_total_records, out_bytes, take_slot);
    if (st != MTR_OK) { if (slot >= 0) release(); return st; }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { release(); ctx->err = "the wire form could not be staged"; return MTR_ERR_HIP; }
    *out_ticket = rank * GATHER_SLOTS_PER_RANK + slot;
    return MTR_OK;
}

extern "C" mtr_status mtr_gather_exchange(mtr_gather *g, int32_t n_tickets, const int32_t *tickets, const uint8_t **out_ptrs, int64_t *out_bytes)
{
    if (!g || n_tickets < 0 || (n_tickets > 0 && (!tickets || !out_ptrs || !out_bytes))) return MTR_ERR_BAD_ARG;
    if (n_tickets == 0) return MTR_OK;
    struct Item { int rank, slot; void *d; int64_t bytes; size_t off; bool via_rccl; };
    std::vector<Item> items((size_t)n_tickets);
    size_t total = 0, total_rccl = 0;
    const bool rccl_up = g->ready.load(std::memory_order_acquire) == 1;      // not up (yet): every table goes straight from its GPU to the host
    {
        std::lock_guard<std::mutex> lk(g->mu);
        for (int i = 0; i < n_tickets; i++) {
            const int rank = tickets[i] / GATHER_SLOTS_PER_RANK, slot = tickets[i] % GATHER_SLOTS_PER_RANK;
            if (tickets[i] < 0 || rank >= g->n || slot >= (int)g->ranks[(size_t)rank].slots.size() || !g->ranks[(size_t)rank].slots[(size_t)slot].busy) { g->err = "ticket " + std::to_string(tickets[i]) + " names no staged table"; return MTR_ERR_BAD_ARG; }
            const GatherSlot &s = g->ranks[(size_t)rank].slots[(size_t)slot];
            items[(size_t)i] = Item{ rank, slot, s.d, s.bytes, 0, rccl_up && (rank != 0 || g->self_send) };
        }
    }
    // layout of the host buffer: first the tables that come over RCCL (one contiguous piece on the first GPU, one copy to the host), then the others
    for (auto &it : items) if (it.via_rccl) { it.off = total_rccl; total_rccl += ((size_t)it.bytes + 255) & ~(size_t)255; }
    total = total_rccl;
    for (auto &it : items) if (!it.via_rccl) { it.off = total; total += ((size_t)it.bytes + 255) & ~(size_t)255; }
    std::vector<char> used((size_t)g->n, 0);
    for (auto &it : items) if (it.bytes > 0) used[(size_t)it.rank] = 1;
    if (total_rccl > 0) used[0] = 1;
    for (int r = 0; r < g->n; r++) if (used[(size_t)r] && !g->ranks[(size_t)r].stream) {       // the exchange streams, when first needed (the devices are up by then)
        GHIP(hipSetDevice(g->ranks[(size_t)r].device));
        GHIP(hipStreamCreateWithFlags(&g->ranks[(size_t)r].stream, hipStreamNonBlocking));
    }
    GatherRank &r0 = g->ranks[0];
    GHIP(hipSetDevice(r0.device));
    if (g->h_cap < total) {
        if (g->h_buf) (void)hipHostFree(g->h_buf);
        g->h_buf = nullptr; g->h_cap = 0;
        const size_t want = std::max<size_t>(total * 5 / 4, (size_t)4 << 20);
        GHIP(hipHostMalloc(&g->h_buf, want, hipHostMallocPortable));                            // (portable: written by copies of every device)
        g->h_cap = want;
    }
    if (g->recv_cap < total_rccl) {
        if (g->d_recv) (void)hipFree(g->d_recv);
        g->d_recv = nullptr; g->recv_cap = 0;
        const size_t want = std::max<size_t>(total_rccl * 5 / 4, (size_t)4 << 20);
        GHIP(hipMalloc(&g->d_recv, want));
        g->recv_cap = want;
    }
    if (total_rccl > 0) {
        // ONE group: every send of the other GPUs and the matching receives of the first (RCCL pairs them by order per peer)
        GNCCL(g->GroupStart());
        for (auto &it : items) if (it.via_rccl && it.bytes > 0) {
            GatherRank &gr = g->ranks[(size_t)it.rank];
            ncclResult_t a = g->Send(it.d, (size_t)it.bytes, ncclUint8, 0, gr.comm, gr.stream);
            ncclResult_t b = a == ncclSuccess ? g->Recv((uint8_t *)g->d_recv + it.off, (size_t)it.bytes, ncclUint8, it.rank, r0.comm, r0.stream) : a;
            if (b != ncclSuccess) { (void)g->GroupEnd(); g->err = std::string("ncclSend / ncclRecv: ") + g->GetErrorString(b); return MTR_ERR_HIP; }
        }
        GNCCL(g->GroupEnd());
        GHIP(hipSetDevice(r0.device));
        GHIP(hipMemcpyAsync(g->h_buf, g->d_recv, total_rccl, hipMemcpyDeviceToHost, r0.stream));
    }
    for (auto &it : items) if (!it.via_rccl && it.bytes > 0) {             // straight to the host, on the owner's stream: the GPUs' PCIe links side by side
        GatherRank &gr = g->ranks[(size_t)it.rank];
        GHIP(hipSetDevice(gr.device));
        GHIP(hipMemcpyAsync((uint8_t *)g->h_buf + it.off, it.d, (size_t)it.bytes, hipMemcpyDeviceToHost, gr.stream));
    }
    for (int r = 0; r < g->n; r++) if (used[(size_t)r]) {                  // copies done; the senders have let go of their staging buffers
        GHIP(hipSetDevice(g->ranks[(size_t)r].device));
        GHIP(hipStreamSynchronize(g->ranks[(size_t)r].stream));
    }
    GHIP(hipSetDevice(r0.device));
    {
        std::lock_guard<std::mutex> lk(g->mu);
        for (int i = 0; i < n_tickets; i++) {
            const Item &it = items[(size_t)i];
            out_ptrs[i] = (const uint8_t *)g->h_buf + it.off; out_bytes[i] = it.bytes;
            g->ranks[(size_t)it.rank].slots[(size_t)it.slot].busy = false;
            if (it.via_rccl) g->bytes_rccl += it.bytes; else g->bytes_local += it.bytes;
        }
        g->n_exchanges++;
        if (total_rccl > 0) g->n_exchanges_rccl++;
    }
    return MTR_OK;
}
#undef GHIP
#undef GNCCL
