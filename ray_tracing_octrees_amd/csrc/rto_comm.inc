// rto_comm.inc -- the multi-GPU part of the C ABI (included at the end of rto_api.hip): screen-space split of a frame over
// the GPUs of one node + ONE gather per batch of frames over RCCL (xGMI), entirely below the C boundary.
//
// No reference counterpart: the reference is single-GPU (SURVEY.md section 8e); this is what its call sequence
// (453-skeleton/main.cpp:1127-1131, 1357-1363) drives when RayTracerBVH::setDevices(n) is used.
//
// Every rank (= one rto_context = one GPU) holds the whole octree and renders the bands `b % world == rank` (from 4 ranks on:
// rank 0 only gathers and assembles, the others render the bands `b % (world - 1) == rank - 1`) of each
// frame as the 4-byte Lambert term per pixel (rto_render_shade_device's payload); one grouped ncclSend / ncclRecv per
// batch lands all parts on rank 0 -- a direct gather over the 7 point-to-point xGMI links, never a ring -- and rank 0
// finishes the colours while it re-interleaves (k_assemble_shade).  Two streams per rank: renders go to `renderStream`,
// the collective and the assembly to `commStream`; two sets of buffers alternate, so the gather of batch k overlaps the
// render of batch k+1 and nothing ever waits on the host.  Hazards are closed with events:
//   render k   waits for evFree[slot]   (the gather/assembly that last used this slot's buffers, batch k-2)
//   gather k   waits for evRendered[slot]
// librccl is opened with dlopen on first use: processes that never create a communicator never load it, and inside a
// PyTorch process the copy torch already mapped is reused (same SONAME), so one RCCL serves both.
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <memory>
#include <thread>

namespace {

struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
};

RcclApi* rccl() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return &api;
    tried = true;
    const char* names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
    for (const char* n : names) {
        api.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (api.handle) break;
    }
    if (!api.handle) { api.error = std::string("librccl not found: ") + dlerror(); return &api; }
#define RTO_SYM(field, name) api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.handle, name)); if (!api.field) api.error = std::string("librccl lacks ") + name
    RTO_SYM(GetUniqueId, "ncclGetUniqueId"); RTO_SYM(CommInitRank, "ncclCommInitRank"); RTO_SYM(CommInitAll, "ncclCommInitAll");
    RTO_SYM(CommDestroy, "ncclCommDestroy"); RTO_SYM(CommAbort, "ncclCommAbort"); RTO_SYM(CommGetAsyncError, "ncclCommGetAsyncError"); RTO_SYM(GroupStart, "ncclGroupStart"); RTO_SYM(GroupEnd, "ncclGroupEnd");
    RTO_SYM(Send, "ncclSend"); RTO_SYM(Recv, "ncclRecv"); RTO_SYM(GetErrorString, "ncclGetErrorString");
#undef RTO_SYM
    api.CommCount = reinterpret_cast<decltype(api.CommCount)>(dlsym(api.handle, "ncclCommCount"));     // optional: only rto_comm_ranks_seen asks for it
    return &api;
}

}  // namespace

// the kernels' view of a plan's windows
static CropInfo crop_of(const rto_split_plan& plan) {
    CropInfo C;
    C.n = plan.cropped ? plan.n_frames : 0;
    for (int i = 0; i < C.n; i++) { C.x0[i] = plan.win_x0[i]; C.w[i] = plan.win_w[i]; C.off[i] = plan.win_off[i]; }
    return C;
}

// The communicators rto_comm_create_all made live and die together: they are driven by ONE host thread, every batch queues a
// Send / Recv on each of them, so one aborted member leaves its siblings with collectives that can never finish.
struct CommGroup { std::vector<rto_comm*> members; };

struct rto_comm {
    rto_context* ctx = nullptr;
    std::shared_ptr<CommGroup> group;                // rto_comm_create_all only
    ncclComm_t comm = nullptr;
    int world = 1, rank = 0, bandRows = 16;
    int asWorld = 0, asRank = 0;                     // rto_comm_debug_rehearse: split the frame as rank asRank of asWorld GPUs (0: off)
    int splitWorld() const { return asWorld > 0 ? asWorld : world; }
    int splitRank() const { return asWorld > 0 ? asRank : rank; }
    // Who renders what, the windows that travel, every count and offset: rto_split_plan_make (rto_split.inc), the one place
    // they are derived.  From 4 GPUs on, rank 0 only gathers and assembles: writing the assembled RGBA32F frames costs it about
    // as much GPU time as an eighth of the traversal (5.5 vs 6.9 us per 1080p frame), so a rank 0 that also renders an equal
    // share is the slowest rank by that much (rehearsed at 8 GPUs: 12.5 us per frame against 6.9 for the others).
    rto_split_plan plan[2] = {};                        // the plan of the batch in each slot
    hipStream_t renderStream = nullptr, commStream = nullptr;
    hipEvent_t evRendered[2] = { nullptr, nullptr }, evFree[2] = { nullptr, nullptr };
    float* d_local[2] = { nullptr, nullptr };       // [batch][rows of part 0][width] floats (parts are padded to part 0's rows)
    float* d_gathered[2] = { nullptr, nullptr };    // rank 0: [render parts] x that (packed: the plan's windows)
    float* d_pack[2] = { nullptr, nullptr };        // what is sent: the windows of d_local's rows (k_pack_columns)
    size_t capFloats = 0;                           // floats per rank the buffers can hold
    int bufW = 0, bufH = 0, bufParts = 0;
    int lastSlot = 0;
    unsigned long seq = 0;
    bool rehearsalClear = true;                     // rehearsals clear the receive buffer per batch (test scaffolding, not a rank's work)
    bool dead = false;                              // aborted (timeout / asynchronous RCCL error): no further collectives
    bool timing = false;                            // rto_comm_debug_set_timing: four timed events per batch (render start / end, gather start / end)
    hipEvent_t evT[2][4] = { { nullptr, nullptr, nullptr, nullptr }, { nullptr, nullptr, nullptr, nullptr } };
    std::string err;
};

static int comm_fail(rto_comm* m, int code, const std::string& msg) {
    if (m) { m->err = msg; if (m->ctx) m->ctx->err = msg; }
    return code;
}

#define RTO_CHIP(m, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return comm_fail(m, RTO_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define RTO_NCCL(m, call)                                                                      \
    do {                                                                                       \
        ncclResult_t r_ = (call);                                                              \
        if (r_ != ncclSuccess) return comm_fail(m, RTO_E_HIP, std::string(#call) + ": " + rccl()->GetErrorString(r_)); \
    } while (0)

static int comm_init_streams(rto_comm* m) {
    RTO_CHIP(m, hipSetDevice(m->ctx->device));
    RTO_CHIP(m, hipStreamCreateWithFlags(&m->renderStream, hipStreamNonBlocking));
    RTO_CHIP(m, hipStreamCreateWithFlags(&m->commStream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        RTO_CHIP(m, hipEventCreateWithFlags(&m->evRendered[i], hipEventDisableTiming));
        RTO_CHIP(m, hipEventCreateWithFlags(&m->evFree[i], hipEventDisableTiming));
    }
    return RTO_OK;
}

static void comm_free_buffers(rto_comm* m) {
    for (int i = 0; i < 2; i++) {
        (void)hipFree(m->d_local[i]); (void)hipFree(m->d_gathered[i]); (void)hipFree(m->d_pack[i]);
        m->d_local[i] = m->d_gathered[i] = m->d_pack[i] = nullptr;
    }
    m->capFloats = 0; m->bufW = m->bufH = m->bufParts = 0;
}

// buffers for the batch `plan` describes: re-allocated (after draining) when the frame size or the number of parts changes
// or a batch is larger than any before; a smaller batch of the same frames uses the front of what is there.  All or
// nothing: a failed allocation leaves the communicator without buffers (the next submit starts over), never with some.
static int comm_ensure_buffers(rto_comm* m, const rto_split_plan& plan) {
    const size_t need = (size_t)plan.full_floats;
    if (m->bufW == plan.width && m->bufH == plan.height && m->bufParts == plan.render_parts && m->d_local[0] && need <= m->capFloats) return RTO_OK;
    RTO_CHIP(m, hipSetDevice(m->ctx->device));
    RTO_CHIP(m, hipStreamSynchronize(m->renderStream));
    RTO_CHIP(m, hipStreamSynchronize(m->commStream));
    const bool sameFrames = m->bufW == plan.width && m->bufH == plan.height && m->bufParts == plan.render_parts;
    const size_t cap = sameFrames ? std::max(need, m->capFloats) : need;
    comm_free_buffers(m);
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = fallible_malloc(reinterpret_cast<void**>(&m->d_local[i]), std::max<size_t>(cap, 1) * sizeof(float));
        if (e == hipSuccess) e = fallible_malloc(reinterpret_cast<void**>(&m->d_pack[i]), std::max<size_t>(cap, 1) * sizeof(float));
        if (e == hipSuccess && m->rank == 0)
            e = fallible_malloc(reinterpret_cast<void**>(&m->d_gathered[i]), std::max<size_t>(cap, 1) * sizeof(float) * (size_t)plan.render_parts);
    }
    if (e != hipSuccess) {
        comm_free_buffers(m);
        return comm_fail(m, RTO_E_HIP, std::string("rto_comm: buffer allocation: ") + hipGetErrorString(e));
    }
    m->capFloats = cap;
    m->bufW = plan.width; m->bufH = plan.height; m->bufParts = plan.render_parts;
    return RTO_OK;
}

// this rank's part of every frame of the batch into d_local[slot], on renderStream
static int comm_render(rto_comm* m, const rto_frame* frames, int n, int mode, int slot) {
    rto_context* c = m->ctx;
    const rto_split_plan& plan = m->plan[slot];
    RTO_CHIP(m, hipSetDevice(c->device));
    RTO_CHIP(m, hipStreamWaitEvent(m->renderStream, m->evFree[slot], 0));
    if (m->timing) RTO_CHIP(m, hipEventRecord(m->evT[slot][0], m->renderStream));
    const int myPart = rto_split_part_of_rank(&plan, m->splitRank());   // -1: this rank gathers and assembles only
    rto_partition part{ plan.render_parts, std::max(myPart, 0), plan.band_rows };
    const rto_partition* pp = plan.render_parts > 1 ? &part : nullptr;
    const size_t frameFloats = (size_t)plan.frame_floats;
    const bool eventsWere = c->eventsOff;
    c->eventsOff = true;                      // no per-launch event pairs on this pipeline (each costs ~2 us between launches)
    if (myPart < 0) {
        // nothing to render
    } else if (mode == RTO_RESIDENT_OCTREE) {
        // the parts of up to 8 frames per launch: a part's kernel is as long as its deepest tile's chain of node visits
        // (~36 us at config 2 whether the part is a whole frame or an eighth), the parts of a batch walk theirs together
        for (int i0 = 0; i0 < n; i0 += kMaxBatch) {
            const int cnt = std::min(kMaxBatch, n - i0);
            RenderParams P[kMaxBatch];
            float4* outs[kMaxBatch];
            int rc = RTO_OK;
            for (int i = 0; i < cnt && rc == RTO_OK; i++) {
                rc = fill_params(c, &frames[i0 + i], pp, P[i], m->renderStream);
                outs[i] = reinterpret_cast<float4*>(m->d_local[slot] + (size_t)(i0 + i) * frameFloats);
            }
            if (rc == RTO_OK) rc = launch_trace_batch<kModeShade>(c, P, cnt, outs, m->renderStream);
            if (rc != RTO_OK) { c->eventsOff = eventsWere; m->err = c->err; return rc; }
        }
    } else {
        for (int i0 = 0; i0 < n; i0 += kMaxBatch) {
            const int cnt = std::min(kMaxBatch, n - i0);
            float4* outs[kMaxBatch];
            for (int i = 0; i < cnt; i++) outs[i] = reinterpret_cast<float4*>(m->d_local[slot] + (size_t)(i0 + i) * frameFloats);
            const int rc = launch_triangles_batch(c, &frames[i0], cnt, pp, mode == RTO_RESIDENT_TRIANGLES_SHADOW ? 1 : 0, outs, m->renderStream, true);
            if (rc != RTO_OK) { c->eventsOff = eventsWere; m->err = c->err; return rc; }
        }
    }
    c->eventsOff = eventsWere;
    // the packed copy: only the plan's windows travel
    if (plan.cropped && myPart >= 0) {
        hipLaunchKernelGGL(k_pack_columns, dim3(1, (unsigned)std::max(plan.rows_part0, 1), (unsigned)n), dim3(256), 0, m->renderStream,
                           m->d_local[slot], m->d_pack[slot], crop_of(plan), frameFloats, plan.width);
        RTO_CHIP(m, hipGetLastError());
    }
    if (m->timing) RTO_CHIP(m, hipEventRecord(m->evT[slot][1], m->renderStream));
    RTO_CHIP(m, hipEventRecord(m->evRendered[slot], m->renderStream));
    RTO_CHIP(m, hipStreamWaitEvent(m->commStream, m->evRendered[slot], 0));
    if (m->timing) RTO_CHIP(m, hipEventRecord(m->evT[slot][2], m->commStream));      // behind the wait: the gather's own time, not the render's
    return RTO_OK;
}

// the sends / receives of one rank for the batch in `slot`; the caller brackets them with ncclGroupStart / End
static int comm_exchange(rto_comm* m, int slot) {
    RTO_CHIP(m, hipSetDevice(m->ctx->device));
    const rto_split_plan& plan = m->plan[slot];
    const size_t count = (size_t)plan.pack_floats;
    // who sends: every rank that renders (in a rehearsal the one real rank plays splitRank())
    if (rto_split_part_of_rank(&plan, m->splitRank()) >= 0)
        RTO_NCCL(m, rccl()->Send(plan.cropped ? m->d_pack[slot] : m->d_local[slot], count, ncclFloat32, 0, m->comm, m->commStream));
    if (m->rank == 0)
        for (int r = 0; r < m->world; r++) {
            const int part = rto_split_part_of_rank(&plan, m->asWorld > 0 ? m->asRank : r);
            if (part < 0) continue;                                   // the gatherer itself ships nothing
            RTO_NCCL(m, rccl()->Recv(m->d_gathered[slot] + (size_t)part * count, count, ncclFloat32, r, m->comm, m->commStream));
        }
    return RTO_OK;
}

// rank 0: re-interleave + finish the colours of every frame of the batch; every rank: the slot is free again
static int comm_finish(rto_comm* m, const rto_frame* frames, int n, int slot, void* d_frames, size_t strideBytes) {
    RTO_CHIP(m, hipSetDevice(m->ctx->device));
    const rto_split_plan& plan = m->plan[slot];
    if (m->rank == 0) {
        const int bandRows = plan.render_parts > 1 ? plan.band_rows : plan.height;
        // all frames of the batch in one launch (blockIdx.z): they share width / height / split
        if (plan.cropped)
            hipLaunchKernelGGL(k_assemble_shade_crop, dim3(1, (unsigned)plan.height, (unsigned)n), dim3(256), 0,
                               m->commStream, m->d_gathered[slot], static_cast<char*>(d_frames), crop_of(plan), strideBytes, plan.width, plan.height,
                               plan.render_parts, bandRows, (size_t)plan.pack_floats);
        else
            hipLaunchKernelGGL(k_assemble_shade, dim3(1, (unsigned)plan.height, (unsigned)n), dim3(256), 0,
                               m->commStream, m->d_gathered[slot], static_cast<char*>(d_frames), (size_t)plan.frame_floats, strideBytes, plan.width, plan.height,
                               plan.render_parts, bandRows, (size_t)plan.full_floats);
        RTO_CHIP(m, hipGetLastError());
    }
    (void)frames;
    if (m->timing) RTO_CHIP(m, hipEventRecord(m->evT[slot][3], m->commStream));
    RTO_CHIP(m, hipEventRecord(m->evFree[slot], m->commStream));
    return RTO_OK;
}

// plan + buffers of the next batch; returns its slot
static int comm_begin_batch(rto_comm* m, const rto_frame* frames, int n, int* slotOut) {
    rto_split_plan plan;
    const rto_scene_bounds sb = bounds_of(m->ctx);
    if (rto_split_plan_make(&sb, frames, n, m->splitWorld(), m->bandRows, &plan) != RTO_OK)
        return comm_fail(m, RTO_E_INVALID, "rto_comm_submit: the frames of a batch share a positive width and height");
    const int rc = comm_ensure_buffers(m, plan);
    if (rc != RTO_OK) return rc;
    const int slot = (int)(m->seq++ & 1ul);
    m->plan[slot] = plan;
    m->lastSlot = slot;
    if (m->asWorld > 0 && m->rank == 0 && m->rehearsalClear) {     // (timing runs switch the clear off: rto_comm_debug_set_rehearsal_clear)
        // rehearsal: the absent ranks' parts read as shade 0 whatever earlier batches (other windows, other strides) left there
        RTO_CHIP(m, hipStreamWaitEvent(m->commStream, m->evFree[slot], 0));
        RTO_CHIP(m, hipMemsetAsync(m->d_gathered[slot], 0, (size_t)plan.pack_floats * (size_t)plan.render_parts * sizeof(float), m->commStream));
    }
    *slotOut = slot;
    return RTO_OK;
}

static int comm_check_batch(rto_comm* m, const rto_frame* frames, int n, int mode, void* d_frames) {
    if (m->dead) return comm_fail(m, RTO_E_INVALID, "rto_comm_submit: communicator is dead (aborted after a timeout or an RCCL error): destroy it");
    if (!frames || n < 1) return comm_fail(m, RTO_E_INVALID, "rto_comm_submit: empty batch");
    if (mode != RTO_RESIDENT_OCTREE && mode != RTO_RESIDENT_TRIANGLES && mode != RTO_RESIDENT_TRIANGLES_SHADOW)
        return comm_fail(m, RTO_E_INVALID, "rto_comm_submit: mode must be RTO_RESIDENT_OCTREE / _TRIANGLES / _TRIANGLES_SHADOW");
    for (int i = 1; i < n; i++)
        if (frames[i].width != frames[0].width || frames[i].height != frames[0].height)
            return comm_fail(m, RTO_E_INVALID, "rto_comm_submit: the frames of a batch share width and height");
    if (m->rank == 0 && !d_frames) return comm_fail(m, RTO_E_INVALID, "rto_comm_submit: rank 0 needs d_frames");
    return RTO_OK;
}

extern "C" {

int rto_comm_unique_id(void* id) {
    if (!id) return RTO_E_INVALID;
    RcclApi* R = rccl();
    if (!R->error.empty()) return fail(nullptr, RTO_E_UNSUPPORTED, "rto_comm_unique_id: " + R->error);
    static_assert(sizeof(ncclUniqueId) == RTO_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t r = R->GetUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, RTO_E_HIP, std::string("ncclGetUniqueId: ") + R->GetErrorString(r));
    std::memcpy(id, &u, sizeof u);
    return RTO_OK;
}

int rto_comm_create(rto_context* ctx, int world, int rank, const void* id, int band_rows, rto_comm** out) {
    if (!out) return RTO_E_INVALID;
    *out = nullptr;
    if (!ctx || !id) return fail(ctx, RTO_E_INVALID, "rto_comm_create: NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(ctx, RTO_E_INVALID, "rto_comm_create: need 0 <= rank < world");
    if (band_rows <= 0 || band_rows % 8) return fail(ctx, RTO_E_INVALID, "rto_comm_create: band_rows must be a positive multiple of 8");
    RcclApi* R = rccl();
    if (!R->error.empty()) return fail(ctx, RTO_E_UNSUPPORTED, "rto_comm_create: " + R->error);
    rto_comm* m = new rto_comm();
    m->ctx = ctx; m->world = world; m->rank = rank; m->bandRows = band_rows;
    int rc = comm_init_streams(m);
    if (rc == RTO_OK) {
        ncclUniqueId u;
        std::memcpy(&u, id, sizeof u);
        ncclResult_t r = R->CommInitRank(&m->comm, world, u, rank);
        if (r != ncclSuccess) rc = comm_fail(m, RTO_E_HIP, std::string("ncclCommInitRank: ") + R->GetErrorString(r));
    }
    if (rc != RTO_OK) { ctx->err = m->err; rto_comm_destroy(m); return rc; }
    *out = m;
    return RTO_OK;
}

int rto_comm_create_all(rto_context* const* ctxs, int n, int band_rows, rto_comm** out) {
    if (!ctxs || !out || n < 1) return RTO_E_INVALID;
    for (int i = 0; i < n; i++) out[i] = nullptr;
    if (band_rows <= 0 || band_rows % 8) return fail(ctxs[0], RTO_E_INVALID, "rto_comm_create_all: band_rows must be a positive multiple of 8");
    RcclApi* R = rccl();
    if (!R->error.empty()) return fail(ctxs[0], RTO_E_UNSUPPORTED, "rto_comm_create_all: " + R->error);
    std::vector<int> devs((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]) return fail(ctxs[0], RTO_E_INVALID, "rto_comm_create_all: NULL context");
        devs[(size_t)i] = ctxs[i]->device;
        for (int j = 0; j < i; j++)
            if (devs[(size_t)j] == devs[(size_t)i]) return fail(ctxs[0], RTO_E_INVALID, "rto_comm_create_all: one context per GPU");
    }
    std::vector<ncclComm_t> comms((size_t)n);
    ncclResult_t r = R->CommInitAll(comms.data(), n, devs.data());
    if (r != ncclSuccess) return fail(ctxs[0], RTO_E_HIP, std::string("ncclCommInitAll: ") + R->GetErrorString(r));
    auto group = std::make_shared<CommGroup>();
    for (int i = 0; i < n; i++) {
        rto_comm* m = new rto_comm();
        m->ctx = ctxs[i]; m->world = n; m->rank = i; m->bandRows = band_rows; m->comm = comms[(size_t)i];
        m->group = group; group->members.push_back(m);
        out[i] = m;
        const int rc = comm_init_streams(m);
        if (rc != RTO_OK) {
            ctxs[0]->err = m->err;
            for (int j = i + 1; j < n; j++) (void)R->CommDestroy(comms[(size_t)j]);
            for (int j = 0; j <= i; j++) { rto_comm_destroy(out[j]); out[j] = nullptr; }
            return rc;
        }
    }
    return RTO_OK;
}

// Both streams idle within `ms`?  (hipStreamQuery polls: never blocks on a collective that cannot finish.)
static bool comm_streams_idle_within(rto_comm* m, int ms) {
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t streams[2] = { m->renderStream, m->commStream };
    for (hipStream_t s : streams) {
        if (!s) continue;
        for (;;) {
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) return false;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(ms)) return false;
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
    return true;
}

static int comm_kill(rto_comm* m, int code, const std::string& why);

void rto_comm_destroy(rto_comm* m) {
    if (!m) return;
    if (m->ctx) (void)hipSetDevice(m->ctx->device);
    // A healthy communicator drains in microseconds.  One whose streams stay busy holds a collective its peer will never answer
    // (a sibling of an aborted member, a peer process that died): abort it -- that ends its kernels -- instead of waiting for ever.
    constexpr int kDestroyDrainMs = 10000;
    if (m->comm && !m->dead && !comm_streams_idle_within(m, kDestroyDrainMs))
        (void)comm_kill(m, RTO_E_TIMEOUT, "rto_comm_destroy: streams still busy: communicator aborted");
    if (m->renderStream) (void)hipStreamSynchronize(m->renderStream);
    if (m->commStream) (void)hipStreamSynchronize(m->commStream);
    if (m->comm && !m->dead) (void)rccl()->CommDestroy(m->comm);        // a dead communicator was released by ncclCommAbort
    if (m->group) {
        auto& v = m->group->members;
        v.erase(std::remove(v.begin(), v.end(), m), v.end());
    }
    comm_free_buffers(m);
    for (int i = 0; i < 2; i++) { if (m->evRendered[i]) (void)hipEventDestroy(m->evRendered[i]); if (m->evFree[i]) (void)hipEventDestroy(m->evFree[i]); }
    for (int i = 0; i < 2; i++) for (int k = 0; k < 4; k++) if (m->evT[i][k]) (void)hipEventDestroy(m->evT[i][k]);
    if (m->ctx && m->renderStream) (void)rto_forget_stream(m->ctx, m->renderStream);
    if (m->renderStream) (void)hipStreamDestroy(m->renderStream);
    if (m->commStream) (void)hipStreamDestroy(m->commStream);
    delete m;
}

const char* rto_comm_last_error(const rto_comm* m) { return m ? m->err.c_str() : ""; }

int rto_comm_submit(rto_comm* m, const rto_frame* frames, int n, int mode, void* d_frames, size_t frame_stride_bytes) {
    if (!m) return RTO_E_INVALID;
    int rc = comm_check_batch(m, frames, n, mode, d_frames);
    if (rc != RTO_OK) return rc;
    int slot = 0;
    if ((rc = comm_begin_batch(m, frames, n, &slot)) != RTO_OK) return rc;
    if ((rc = comm_render(m, frames, n, mode, slot)) != RTO_OK) return rc;
    RTO_NCCL(m, rccl()->GroupStart());
    rc = comm_exchange(m, slot);
    RTO_NCCL(m, rccl()->GroupEnd());
    if (rc != RTO_OK) return rc;
    return comm_finish(m, frames, n, slot, d_frames, frame_stride_bytes);
}

int rto_comm_submit_all(rto_comm* const* comms, int n_comms, const rto_frame* frames, int n, int mode, void* d_frames, size_t frame_stride_bytes) {
    if (!comms || n_comms < 1 || !comms[0]) return RTO_E_INVALID;
    for (int k = 0; k < n_comms; k++)
        if (!comms[k] || comms[k]->world != n_comms || comms[k]->rank != k) return comm_fail(comms[0], RTO_E_INVALID, "rto_comm_submit_all: pass the handles rto_comm_create_all returned, in order");
    int rc;
    int slot = 0;
    // every member is checked before ANY of them advances its batch counter: a refused batch leaves the group's slots in step
    for (int k = 0; k < n_comms; k++)
        if ((rc = comm_check_batch(comms[k], frames, n, mode, k == 0 ? d_frames : (void*)1)) != RTO_OK) {
            if (k > 0) comms[0]->err = comms[k]->err;
            return rc;
        }
    for (int k = 0; k < n_comms; k++) {
        int sk = 0;
        if ((rc = comm_begin_batch(comms[k], frames, n, &sk)) != RTO_OK) return rc;
        if (k == 0) slot = sk;
        else if (sk != slot) return comm_fail(comms[0], RTO_E_INVALID, "rto_comm_submit_all: the communicators of a group are driven together");
    }
    for (int k = 0; k < n_comms; k++)
        if ((rc = comm_render(comms[k], frames, n, mode, slot)) != RTO_OK) return rc;       // every GPU starts rendering before any collective is issued
    RTO_NCCL(comms[0], rccl()->GroupStart());
    for (int k = 0; k < n_comms && rc == RTO_OK; k++) rc = comm_exchange(comms[k], slot);
    RTO_NCCL(comms[0], rccl()->GroupEnd());
    if (rc != RTO_OK) return rc;
    for (int k = 0; k < n_comms; k++)
        if ((rc = comm_finish(comms[k], frames, n, slot, d_frames, frame_stride_bytes)) != RTO_OK) return rc;
    return RTO_OK;
}

// One frame through all ranks of a single-process group into rank 0's RESIDENT framebuffer (the counterpart of
// rto_render_resident: rto_resident_frame / rto_download_resident of rank 0's context then see the assembled frame).
int rto_comm_render_resident_all(rto_comm* const* comms, int n_comms, const rto_frame* frame, int mode) {
    if (!comms || n_comms < 1 || !comms[0] || !frame) return RTO_E_INVALID;
    rto_context* c0 = comms[0]->ctx;
    if (frame->width <= 0 || frame->height <= 0) return comm_fail(comms[0], RTO_E_INVALID, "render: width/height must be positive");
    RTO_CHIP(comms[0], hipSetDevice(c0->device));
    const size_t pixels = (size_t)frame->width * frame->height;
    int rc = ensure_frame(c0, pixels);
    if (rc != RTO_OK) { comms[0]->err = c0->err; return rc; }
    if ((rc = rto_comm_submit_all(comms, n_comms, frame, 1, mode, c0->d_frame, pixels * sizeof(float4))) != RTO_OK) return rc;
    // order the context's own stream (what rto_download_resident waits on) behind the assembly
    RTO_CHIP(comms[0], hipSetDevice(c0->device));
    const hipEvent_t ev1 = c0->timer.borrow_stop();
    RTO_CHIP(comms[0], hipEventRecord(ev1, comms[0]->commStream));
    RTO_CHIP(comms[0], hipStreamWaitEvent(c0->stream, ev1, 0));
    c0->residentW = frame->width; c0->residentH = frame->height;
    return RTO_OK;
}

// Rehearsal of an N-GPU split on fewer GPUs: this (one-rank) communicator renders, ships and assembles as rank `as_rank` of
// `as_world` GPUs -- every per-rank cost of the split except the other GPUs' traffic.  The assembled frames hold this rank's
// bands only (the others read as shade 0).  as_world = 0 switches it off.
int rto_comm_debug_rehearse(rto_comm* m, int as_world, int as_rank) {
    if (!m) return RTO_E_INVALID;
    if (as_world < 0 || (as_world > 0 && (as_rank < 0 || as_rank >= as_world))) return comm_fail(m, RTO_E_INVALID, "rto_comm_debug_rehearse: need 0 <= as_rank < as_world");
    if (m->world != 1) return comm_fail(m, RTO_E_UNSUPPORTED, "rto_comm_debug_rehearse: one-rank communicators only");
    RTO_CHIP(m, hipSetDevice(m->ctx->device));
    RTO_CHIP(m, hipStreamSynchronize(m->renderStream));
    RTO_CHIP(m, hipStreamSynchronize(m->commStream));
    comm_free_buffers(m);
    m->asWorld = as_world; m->asRank = as_world > 0 ? as_rank : 0;
    return RTO_OK;
}

// Rehearsal only: the per-batch clear of the absent ranks' part of the receive buffer on / off (timing runs: bench.py --rehearse-world).
int rto_comm_debug_set_rehearsal_clear(rto_comm* m, int enabled) {
    if (!m) return RTO_E_INVALID;
    m->rehearsalClear = enabled != 0;
    return RTO_OK;
}

// Bench aid: timed events around the render and around the gather (+ assembly on rank 0) of every batch from now on.
int rto_comm_debug_set_timing(rto_comm* m, int enabled) {
    if (!m) return RTO_E_INVALID;
    if (enabled && !m->evT[0][0]) {
        RTO_CHIP(m, hipSetDevice(m->ctx->device));
        for (int i = 0; i < 2; i++) for (int k = 0; k < 4; k++) RTO_CHIP(m, hipEventCreate(&m->evT[i][k]));
    }
    m->timing = enabled != 0;
    return RTO_OK;
}

// GPU milliseconds of the batch submitted last, after its flush: ms[0] = this rank's render (+ pack), ms[1] = its grouped send / recv
// (+ the assembly on rank 0), measured from the moment the rendered parts were ready.
int rto_comm_debug_last_timing(rto_comm* m, float ms[2]) {
    if (!m || !ms) return RTO_E_INVALID;
    if (!m->timing || !m->evT[0][0] || m->seq == 0) return comm_fail(m, RTO_E_INVALID, "rto_comm_debug_last_timing: switch timing on and submit a batch first");
    RTO_CHIP(m, hipSetDevice(m->ctx->device));
    const int slot = m->lastSlot;
    RTO_CHIP(m, hipEventSynchronize(m->evT[slot][3]));
    RTO_CHIP(m, hipEventElapsedTime(&ms[0], m->evT[slot][0], m->evT[slot][1]));
    RTO_CHIP(m, hipEventElapsedTime(&ms[1], m->evT[slot][2], m->evT[slot][3]));
    return RTO_OK;
}

// Floats this rank shipped for the batch submitted last (packed: the windows only) and what whole rows would have been.
int rto_comm_debug_last_payload(const rto_comm* m, int64_t* packed_floats, int64_t* full_floats) {
    if (!m) return RTO_E_INVALID;
    const rto_split_plan& plan = m->plan[m->lastSlot];              // the plan of the last submit
    if (packed_floats) *packed_floats = plan.pack_floats;
    if (full_floats) *full_floats = plan.full_floats;
    return RTO_OK;
}

// The communicator is beyond use: abort whatever it still has in flight (ncclCommAbort frees the communicator and lets its kernels
// end), remember why.  Idempotent.
static void comm_abort_one(rto_comm* m) {
    if (m->dead) return;
    m->dead = true;
    if (m->comm && rccl()->CommAbort) (void)rccl()->CommAbort(m->comm);
    m->comm = nullptr;
}

// A member of a rto_comm_create_all group takes the whole group with it: its siblings hold queued Send / Recv against it.
static int comm_kill(rto_comm* m, int code, const std::string& why) {
    if (m->group) {
        for (rto_comm* o : m->group->members)
            if (o != m && !o->dead) { comm_abort_one(o); (void)comm_fail(o, code, "rto_comm: a member of this group was aborted (" + why + ")"); }
    }
    comm_abort_one(m);
    return comm_fail(m, code, why);
}

// an asynchronous error RCCL has noticed on this communicator (a peer that went away, a transport failure) since the last look
static int comm_async_error(rto_comm* m) {
    if (m->dead || !m->comm || !rccl()->CommGetAsyncError) return RTO_OK;
    ncclResult_t st = ncclSuccess;
    const ncclResult_t rc = rccl()->CommGetAsyncError(m->comm, &st);
    if (rc != ncclSuccess) return comm_kill(m, RTO_E_HIP, std::string("ncclCommGetAsyncError: ") + rccl()->GetErrorString(rc));
    if (st != ncclSuccess && st != ncclInProgress) return comm_kill(m, RTO_E_HIP, std::string("rto_comm: asynchronous RCCL error: ") + rccl()->GetErrorString(st));
    return RTO_OK;
}

int rto_comm_flush_timeout(rto_comm* m, int timeout_ms) {
    if (!m) return RTO_E_INVALID;
    if (m->dead) return comm_fail(m, RTO_E_INVALID, "rto_comm_flush: communicator is dead (aborted after a timeout or an RCCL error): destroy it");
    RTO_CHIP(m, hipSetDevice(m->ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t streams[2] = { m->renderStream, m->commStream };
    for (hipStream_t s : streams) {
        for (unsigned spins = 0;; spins++) {
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) return comm_kill(m, RTO_E_HIP, std::string("rto_comm_flush: ") + hipGetErrorString(e));
            if ((spins & 63u) == 63u) {                      // every few dozen polls: RCCL's own error state, the clock
                const int rcAsync = comm_async_error(m);
                if (rcAsync != RTO_OK) return rcAsync;
                if (timeout_ms > 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms))
                    return comm_kill(m, RTO_E_TIMEOUT, "rto_comm_flush_timeout: the batch did not complete within " + std::to_string(timeout_ms) +
                                                      " ms (a peer that never sent?): communicator aborted");
            }
            if (spins > 256u) std::this_thread::sleep_for(std::chrono::microseconds(50));      // a long wait: stop burning the core
        }
    }
    return comm_async_error(m);
}

int rto_comm_flush(rto_comm* m) { return rto_comm_flush_timeout(m, 0); }

int rto_comm_is_dead(const rto_comm* m) { return (m && m->dead) ? 1 : 0; }

// ncclCommCount of the live communicator: the number of ranks RCCL itself says take part (a bench line's proof that N ranks ran).
int rto_comm_ranks_seen(const rto_comm* m, int* ranks) {
    if (!m || !ranks) return RTO_E_INVALID;
    *ranks = 0;
    if (m->dead || !m->comm) return comm_fail(const_cast<rto_comm*>(m), RTO_E_INVALID, "rto_comm_ranks_seen: communicator is dead");
    if (!rccl()->CommCount) return comm_fail(const_cast<rto_comm*>(m), RTO_E_UNSUPPORTED, "rto_comm_ranks_seen: librccl lacks ncclCommCount");
    int n = 0;
    RTO_NCCL(const_cast<rto_comm*>(m), rccl()->CommCount(m->comm, &n));
    *ranks = n;
    return RTO_OK;
}

int rto_comm_debug_abort(rto_comm* m) {
    if (!m) return RTO_E_INVALID;
    (void)comm_kill(m, RTO_E_TIMEOUT, "rto_comm_debug_abort: communicator aborted on request");
    return RTO_OK;
}

void* rto_comm_stream(rto_comm* m) { return m ? (void*)m->commStream : nullptr; }

}  // extern "C"
