// Device groups: the prove path and a single MSM point-sharded over the GPUs of one node (BASELINE.json
// configs[4]; north_star: "a single large MSM shards its base points across the 8 GPUs of one node with an RCCL all-reduce of
// partial bucket sums over xGMI").  The reference has one call, groth16.Prove at /root/reference/mt.go:496, and no notion of
// devices; this is what its Go caller binds to spread that one call over several MI355X.
//
//   partitioning   pk points are static: mi_pk_load_sharded cuts the WIRES into `world` contiguous ranges (and the N - 1 pairs
//                  of the Z MSM likewise); rank r keeps the A / B1 / B2 / K points of its wires and its slice of pk.G1.Z
//                  resident (tables included), so a proof moves no point over any link.  Per proof every rank receives its slice
//                  of W from the host, the lead rank runs computeH (NTT = replicas only) and hands each rank its
//                  slice of h device-to-device.
//   exchange       EC addition is not an ncclRedOp, so the "all-reduce of partial bucket sums" is byte-typed:
//                  mode 0 (SURVEY 8e option i)  every rank finishes its Pippenger locally and contributes ONE partial sum per
//                         MSM (128 / 256 B XYZZ); combine = world point additions (the partials of all five MSMs travel in ONE
//                         all-gather together with every rank's status).
//                  mode 1 (option ii, the north_star's wording)  every rank stops at its BUCKET sums; rank r owns the keys
//                         [r K / world, (r+1) K / world) and receives that slice from every other rank -- a reduce-scatter written
//                         as grouped ncclSend / ncclRecv, one hop on the full xGMI mesh, all 7 links at once -- adds the slices
//                         (k_msm_sum_slices), runs the bucket reduce on its slice only, and the per-rank results are combined as
//                         in mode 0 (Horner over the windows is linear, so combining after it is the same sum).
//   transport      1  RCCL (ncclCommInitAll in one process, ncclCommInitRank for one rank per process).
//                  2  same-process copies (hipMemcpyPeerAsync / device-to-device): a single-process group that names a device twice
//                     (the 1-GPU rehearsal of the tests) cannot have an RCCL communicator.
//                  3  host-staged: one rank per process, the processes meet in a POSIX shared-memory segment named after the group
//                     id; slices travel device -> segment -> device through per-(source, destination) chunk rings, small values
//                     (status words, partial sums) through an all-gather area.  For ranks that cannot have an RCCL communicator
//                     between them -- two processes on ONE device (how a 1-GPU box rehearses the one-rank-per-process flow: RCCL
//                     refuses two ranks per device, the bookkeeping does not care) or a box without a working RCCL fabric.  Every
//                     wait has a deadline (MI_GROUP_TIMEOUT_MS, default 60 s): a peer that died is an error, not a hang.
//   failures       with one rank per process every entry point is a collective, and a rank that returned early from a local failure
//                  would leave its peers waiting in the next exchange.  So every phase that can fail locally (argument checks,
//                  workspaces, uploads, enqueues) is followed by an AGREEMENT -- an all-gather of the ranks' status words -- before
//                  the next exchange starts, and the last all-gather (the partial sums) carries the status too: either every rank
//                  enters an exchange or every rank returns an error (its own, or "another rank failed") and its MSM slots are drained.
#include "prove_internal.h"
#include "msm_curve_ops.h"
#include "ntt_cross.h"
#include <rccl/rccl.h>
#include "group_link.h"   // transport 3: the shared-memory segment, its rings and its all-gather area (host code only)
#include <cstdlib>
#include <future>

// Everything one LOCAL rank owns.  The events, one enum: seven "ready" events of computeH over the ranks -- a transfer waits for the ONE
// kernel that produced what it moves, not for whatever else has been enqueued on the context's stream since: that is what lets the
// next vector's arithmetic run under this vector's transfer -- and the six hand-over events of the exchanges.
enum { E_IN, E_DA, E_DB, E_DC, E_FA, E_FB, E_MID,          // computeH: inputs, cross-rank steps of a / b / c, coset transforms of a / b, middle kernel
       E_C0, E_C1,                                         // computeH: the context's stream -> the exchange stream (last coefficient) and back
       E_PEER_IN, E_PEER_OUT,                              // transport 2: the stream-level barriers on entry to and exit from a batch
       E_DONE, E_H, E_COUNT };                             // slice sums -> an MSM's stream; the h slice has arrived (recorded by its receiver)
enum { H_A, H_B, H_C, H_Y0, H_Y1, H_COUNT };               // computeH over the ranks: the slice vectors of a, b, c and the two exchange vectors
struct GroupRank {
    int dev = 0; mi_ctx *ctx = nullptr;
    ncclComm_t comm = nullptr;     // transport 1: this rank's RCCL communicator
    hipStream_t xs = nullptr;      // the exchange stream (sends, receives, slice sums)
    hipEvent_t ev[E_COUNT] = {};
    DevBuf recv;                   // bucket slices received from the other ranks
    DevBuf stage;                  // small staging area for the all-gathers (transport 1)
    // computeH over the ranks (compute_h_sharded): the vectors of H_*, the h slice with one slot in front (the previous rank's last
    // coefficient: the Z cut of a sharded key starts one element early) and the cross-rank tables
    DevBuf hv[H_COUNT], hh;
    CrossNttTables xt;
};
struct mi_group {
    int world = 0;                 // ranks in the group
    int rank0 = 0;                 // global rank of the first local rank
    int transport = 0;             // 1 = RCCL, 2 = same-process copies, 3 = host-staged (shared memory)
    std::vector<GroupRank> rk;     // the LOCAL ranks, complete at creation (threads of a call hold references into it)
    ShmLink shm;                   // transport 3
    std::vector<void *> pinned;    // transport 3: the ring regions pinned for the device (hipHostRegister): this rank's row and column
    bool sharded_h = false;        // mi_group_set_sharded_compute_h: mi_groth16_prove_sharded runs computeH over all ranks
    uint32_t lead_share = 0xffffffffu;   // permille of an even wire share that rank 0 -- which also runs computeH -- takes (mi_group_set_lead_share; all ones = automatic)
    int timeout_ms = 60000;        // how long a rank waits for its peers without anything completing (MI_GROUP_TIMEOUT_MS; both transports)
    bool nonblocking = false;      // transport 1, one rank per process: the communicator is non-blocking and every wait on it is a deadline poll
    std::string err;
    bool broken = false;           // a transport call failed half-way: rings / communicator are in an unknown state, every later call is refused
    std::atomic<bool> busy{false};   // calls on one group must not overlap: an entry point that finds it set returns MI_EINVAL (GroupCall)
    int n_local() const { return (int)rk.size(); }
    bool local(int r) const { return r >= rank0 && r < rank0 + n_local(); }
    u32 log_w() const { u32 lw = 0; while ((1 << lw) < world) lw++; return lw; }
    // computeH over the ranks at N = 2^log_n: a rank's slice has M = 2^log_m elements, a block of an all-to-all cnt = M / world of them
    struct HCut { u32 log_w, log_m; size_t M, cnt; };
    HCut h_cut(u32 log_n) const { const u32 lw = log_w(), lm = log_n - lw; return {lw, lm, (size_t)1 << lm, ((size_t)1 << lm) >> lw}; }
};
// The first LOCAL failure of a call: noted, carried through every exchange the peers are already in, returned afterwards.
struct Carried {
    int32_t rc = MI_OK; std::string text;
    void note(int32_t r, const std::string &msg) { if (r != MI_OK && rc == MI_OK) { rc = r; text = msg; } }
    bool ok() const { return rc == MI_OK; }
    int32_t leave(mi_group *g) const { if (!ok()) g->err = text; return rc; }   // the call's return: the failure with its text, or MI_OK
};
struct mi_pk_sharded {
    std::vector<mi_pk *> part;     // one per local rank
    u32 log_n = 0;
    u64 nb_wires = 0;
    bool uniform = false;          // every local part chose the same MSM plan per group (needed by mode 1)
    uint32_t lead_share = 1000;    // the wire cut this key was loaded with (permille, resolved): a prove under another cut is refused
};

#define G_FAIL(g, code, msg) do { (g)->err = (msg); return (code); } while (0)
#define G_HIP(g, call) do { hipError_t e__ = mi_fault_hit() ? hipErrorUnknown : (call); if (e__ != hipSuccess) { (g)->err = std::string(#call) + ": " + hipGetErrorString(e__); \
                            return e__ == hipErrorOutOfMemory ? MI_ENOMEM : MI_EHIP; } } while (0)
#define G_CTX(g, i, expr) do { int32_t rc__ = (expr); if (rc__ != MI_OK) { (g)->err = mi_last_error((g)->rk[i].ctx); return rc__; } } while (0)

// Entry-point guard: the group's exchange streams, receive buffers and per-rank contexts serve ONE call at a time.  A second call that
// arrives while one is running is refused (MI_EINVAL, the running call's error text is left alone) instead of corrupting the ranks' receive buffers.
struct GroupCall {
    mi_group *g; bool ok;
    explicit GroupCall(mi_group *g_) : g(g_), ok(g_ && !g_->busy.exchange(true, std::memory_order_acquire)) {}
    ~GroupCall() { if (ok) g->busy.store(false, std::memory_order_release); }
};
#define G_ENTER(g) GroupCall call__(g); if (!call__.ok) return MI_EINVAL; \
                   if ((g)->broken) G_FAIL(g, MI_EHIP, "group: an earlier exchange failed half-way; destroy the group and create a new one")

static void range_of(u64 total, int world, int r, u64 &lo, u64 &hi) { lo = total * (u64)r / (u64)world; hi = total * (u64)(r + 1) / (u64)world; }
// The WIRE cut of a sharded key.  Rank 0 (the lead) also runs computeH, which no other rank can help with (NTT = replicas only, SURVEY
// 8e), and the other ranks cannot start their Z MSMs before h exists: giving the lead a smaller share of the wire MSMs shortens the
// proof's critical path (the projection).  share = permille of the even share: the lead takes share / 1000 of
// nb_wires / world wires, the other ranks split the rest evenly; 1000 = the even cut of range_of, bit for bit.  The N - 1 pairs of the
// Z MSM stay cut evenly (Z starts on every rank at the same moment, when h arrives).
// Automatic: 1000 * max(0, 1 - rho (world - 1)) with rho = computeH time / wire-MSM time = 1/2 (measured at N = 2^26 on one MI355X
// with the WHIR witness mix: 60 of 115 ms) -- 1000 for one rank, 500 for two, 0 from three ranks on.
static uint32_t lead_share_of(const mi_group *g) {
    if (g->lead_share <= 1000) return g->lead_share;
    const int w = g->world;
    return w <= 1 ? 1000u : w == 2 ? 500u : 0u;
}
static void wire_range_of(u64 nb_wires, int world, int r, uint32_t share, u64 &lo, u64 &hi) {
    if (share >= 1000 || world <= 1) { range_of(nb_wires, world, r, lo, hi); return; }
    const u64 lead_n = nb_wires * share / (1000ull * (u64)world), rest = nb_wires - lead_n;
    if (r == 0) { lo = 0; hi = lead_n; return; }
    u64 a, b;
    range_of(rest, world - 1, r - 1, a, b);
    lo = lead_n + a; hi = lead_n + b;
}

// ---------------------------------------------------------------- transport 3: the link (group_link.h) on this group
static int32_t link_status(mi_group *g, const LinkStatus &s) {   // what the link reports becomes the group's text and flag
    if (!s.text.empty()) g->err = s.text;
    if (s.broken) g->broken = true;
    return s.code;
}
static int32_t shm_attach(mi_group *g, const uint8_t id[128]) {
    uint64_t chunk = (uint64_t)1 << 20;
    if (const char *e = getenv("MI_GROUP_SHM_CHUNK_KB")) { const long v = atol(e); if (v >= 4 && v <= (1 << 16)) chunk = (uint64_t)v << 10; }
    ShmLink &L = g->shm;
    MI_TRY(link_status(g, L.attach(shm_name_of(id), g->rank0, g->world, g->timeout_ms, chunk, 4)));
    // The rings THIS rank sources (row `rank`, contiguous) or sinks (column `rank`) as pinned memory: copies to and from them run at the
    // bus rate and do not stage a second time (best effort).  Registering pins -- and therefore allocates -- every page it covers: the
    // whole area would be W * W rings for every rank (256 MB at W = 8, 16 GB at 64), these are 2 W - 1.
    const size_t W = (size_t)g->world, rank = (size_t)g->rank0;
    auto reg = [&](size_t first_ring, size_t n_rings) {
        void *p = L.data + first_ring * L.ring_bytes();
        if (hipHostRegister(p, n_rings * L.ring_bytes(), hipHostRegisterDefault) == hipSuccess) g->pinned.push_back(p);
        else (void)hipGetLastError();
    };
    reg(rank * W, W);
    for (size_t s = 0; s < W; s++) if (s != rank) reg(s * W + rank, 1);
    return MI_OK;
}
static void shm_detach(mi_group *g) {
    for (void *p : g->pinned) (void)hipHostUnregister(p);
    g->pinned.clear();
    g->shm.detach();
}

// ---------------------------------------------------------------- transport 1 with one rank per process: deadlines
// The communicator of a per-rank group is NON-BLOCKING (ncclCommInitRankConfig, blocking = 0): no RCCL call may hold this thread for
// longer than it takes to queue work, and every wait -- for the communicator to come up, for a group of sends / receives to be
// issued, for the exchange stream to drain -- is a poll of ncclCommGetAsyncError / hipStreamQuery against MI_GROUP_TIMEOUT_MS.  When
// the deadline passes (a peer's process ended, a link went down) or RCCL reports an asynchronous error, the communicator is ABORTED
// (ncclCommAbort: its kernels leave the stream), the group is marked broken and the call returns an error: a timeout, not a hang.
// Single-process groups (ncclCommInitAll) keep blocking communicators: all their ranks live and die with this process.
static inline bool nccl_ok(ncclResult_t r) { return r == ncclSuccess || r == ncclInProgress; }
static int32_t nccl_abort_all(mi_group *g, const std::string &msg) {
    for (GroupRank &k : g->rk) if (k.comm) { (void)ncclCommAbort(k.comm); k.comm = nullptr; }
    g->broken = true;
    G_FAIL(g, MI_EHIP, msg);
}
// waits until communicator i has left the "in progress" state (the last non-blocking call on it has been carried out)
static int32_t nccl_settle(mi_group *g, int i, const char *what) {
    if (!g->nonblocking) return MI_OK;
    const Deadline dl(g->timeout_ms);
    unsigned spins = 0;
    for (;;) {
        ncclResult_t st = ncclSuccess;
        const ncclResult_t r = ncclCommGetAsyncError(g->rk[i].comm, &st);
        if (r != ncclSuccess) return nccl_abort_all(g, std::string("group: ncclCommGetAsyncError failed ") + what + ": " + ncclGetErrorString(r));
        if (st == ncclSuccess) return MI_OK;
        if (st != ncclInProgress) return nccl_abort_all(g, std::string("group: RCCL reported an asynchronous error ") + what + ": " + ncclGetErrorString(st));
        if (dl.passed()) return nccl_abort_all(g, std::string("group: RCCL did not finish ") + what + " (timeout; did a peer's process end?)");
        shm_pause(spins);
    }
}
// waits for stream s of local rank i to drain, watching the communicator meanwhile
static int32_t nccl_wait_stream(mi_group *g, int i, hipStream_t s, const char *what) {
    if (!g->nonblocking) { G_HIP(g, hipStreamSynchronize(s)); return MI_OK; }
    const Deadline dl(g->timeout_ms);
    unsigned spins = 0;
    bool injected = mi_fault_hit();   // ONE count per wait: the call number an injected failure fires at does not depend on how often this loop polls
    for (;;) {
        const hipError_t q = injected ? hipErrorUnknown : hipStreamQuery(s);
        if (q == hipSuccess) return MI_OK;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); return nccl_abort_all(g, std::string("group: the exchange stream failed ") + what + ": " + hipGetErrorString(q)); }
        ncclResult_t st = ncclSuccess;
        if (ncclCommGetAsyncError(g->rk[i].comm, &st) != ncclSuccess || (st != ncclSuccess && st != ncclInProgress))
            return nccl_abort_all(g, std::string("group: RCCL reported an asynchronous error ") + what + ": " + ncclGetErrorString(st));
        if (dl.passed()) return nccl_abort_all(g, std::string("group: the exchange did not complete ") + what + " (timeout; did a peer's process end?)");
        shm_pause(spins);
    }
}

// ---------------------------------------------------------------- point-to-point batches
// transport 3: the link's progress loop over this rank's exchange stream; a chunk is complete in its slot / on the device when its copy returns
static int32_t run_xfers_shm(mi_group *g, const std::vector<Xfer> &list) {
    hipStream_t xs = g->rk[0].xs;
    (void)hipSetDevice(g->rk[0].dev);
    G_HIP(g, hipStreamSynchronize(xs));   // what this rank sends is complete; what it receives into is no longer read
    auto copy = [&](void *dst, const void *src, size_t nb, hipMemcpyKind kind) -> int32_t {
        G_HIP(g, hipMemcpyAsync(dst, src, nb, kind, xs));
        G_HIP(g, hipStreamSynchronize(xs));
        return MI_OK;
    };
    return link_status(g, g->shm.run_xfers(list, [&](void *slot, const void *src, size_t nb) { return copy(slot, src, nb, hipMemcpyDeviceToHost); },
                                           [&](void *dst, const void *slot, size_t nb) { return copy(dst, slot, nb, hipMemcpyHostToDevice); }));
}
// Runs the batch on the ranks' exchange streams.  Afterwards rk[i].xs is ordered after every transfer rank i sends or receives.
// A failure inside a batch leaves the transport in an unknown state (some ranks may be waiting in it): the group is marked broken.
static int32_t run_xfers_impl(mi_group *g, const std::vector<Xfer> &xs_list) {
    const MiRange range_fn("mi.group.exchange");
    if (g->transport == 3) return run_xfers_shm(g, xs_list);
    if (g->transport == 1) {
        // every ncclGroupStart is closed by its ncclGroupEnd whatever happens in between (an open group would swallow this thread's next
        // RCCL calls); the first failure is reported after the group has been closed
        ncclResult_t bad = ncclSuccess;
        const char *where = "";
        ncclResult_t r = ncclGroupStart();
        if (!nccl_ok(r)) { g->err = std::string("ncclGroupStart: ") + ncclGetErrorString(r); return MI_EHIP; }
        for (const Xfer &x : xs_list) {
            if (!x.bytes || bad != ncclSuccess) continue;
            if (g->local(x.src)) {
                const GroupRank &k = g->rk[x.src - g->rank0];
                (void)hipSetDevice(k.dev);
                r = mi_fault_hit() ? ncclInternalError : ncclSend(x.sp, x.bytes, ncclUint8, x.dst, k.comm, k.xs);
                if (!nccl_ok(r)) { bad = r; where = "ncclSend"; continue; }
            }
            if (g->local(x.dst)) {
                const GroupRank &k = g->rk[x.dst - g->rank0];
                (void)hipSetDevice(k.dev);
                r = ncclRecv(x.dp, x.bytes, ncclUint8, x.src, k.comm, k.xs);
                if (!nccl_ok(r)) { bad = r; where = "ncclRecv"; }
            }
        }
        r = ncclGroupEnd();
        if (bad == ncclSuccess && !nccl_ok(r)) { bad = r; where = "ncclGroupEnd"; }
        if (bad != ncclSuccess) {
            const std::string msg = std::string("group: ") + where + ": " + ncclGetErrorString(bad);
            if (g->nonblocking) return nccl_abort_all(g, msg);   // part of the batch may be queued: the communicator cannot be used again
            G_FAIL(g, MI_EHIP, msg);
        }
        if (g->nonblocking) {
            // one rank per process: the batch is issued AND complete (or the group is broken) before anything else is built on it -- a peer
            // that ended mid-exchange surfaces here, within the deadline, not in some later synchronisation without one
            MI_TRY(nccl_settle(g, 0, "while issuing an exchange"));
            MI_TRY(nccl_wait_stream(g, 0, g->rk[0].xs, "in an exchange"));
        }
        return MI_OK;
    }
    // same process, no communicator (a device named twice): peer copies on the source's stream, then every stream waits for all.
    // A copy is issued by its SOURCE into the destination's buffer, so the sources must first wait for whatever the destinations
    // still do with those buffers (the slice sums of the previous exchange): a stream-level barrier on entry as well.
    auto barrier = [&](int ev) -> int32_t {   // every exchange stream waits for what every other one has been given so far
        for (GroupRank &k : g->rk) { (void)hipSetDevice(k.dev); G_HIP(g, hipEventRecord(k.ev[ev], k.xs)); }
        for (GroupRank &k : g->rk) {
            (void)hipSetDevice(k.dev);
            for (GroupRank &o : g->rk) if (&o != &k) G_HIP(g, hipStreamWaitEvent(k.xs, o.ev[ev], 0));
        }
        return MI_OK;
    };
    MI_TRY(barrier(E_PEER_IN));
    for (const Xfer &x : xs_list) {
        if (!x.bytes) continue;
        if (!g->local(x.src) || !g->local(x.dst)) G_FAIL(g, MI_EINVAL, "group: peer-copy transport reached a remote rank");
        const GroupRank &s = g->rk[x.src - g->rank0], &d = g->rk[x.dst - g->rank0];
        (void)hipSetDevice(s.dev);
        if (s.dev == d.dev) G_HIP(g, hipMemcpyAsync(x.dp, x.sp, x.bytes, hipMemcpyDeviceToDevice, s.xs));
        else G_HIP(g, hipMemcpyPeerAsync(x.dp, d.dev, x.sp, s.dev, x.bytes, s.xs));
    }
    return barrier(E_PEER_OUT);
}
static int32_t run_xfers(mi_group *g, const std::vector<Xfer> &xs_list) {
    const int32_t rc = run_xfers_impl(g, xs_list);
    if (rc != MI_OK && g->n_local() != g->world) {   // the peers may be inside the exchange this rank just left
        g->broken = true;
        if (g->transport == 3) g->shm.poison();
    }
    return rc;
}

// ---------------------------------------------------------------- all-gather of small host values, agreement
// local: n_local x bytes (this process's ranks, in order); all: world x bytes in rank order.  Single process: a copy.  One rank
// per process: ncclAllGather(ncclUint8) through a staging area (transport 1) or the shared segment (transport 3).
static int32_t group_allgather(mi_group *g, const void *local, size_t bytes, void *all) {
    const MiRange range_fn("mi.group.allgather");
    // (a per-rank RCCL group of ONE rank goes through its communicator all the same: that is how a 1-GPU box runs the polled path)
    if (g->n_local() == g->world && !g->nonblocking) { std::memcpy(all, local, bytes * (size_t)g->world); return MI_OK; }
    if (g->n_local() != 1) G_FAIL(g, MI_EINVAL, "group: a process holds either all ranks or exactly one");
    int32_t rc;
    if (g->transport == 3) rc = link_status(g, g->shm.allgather(local, bytes, all));
    else if (g->transport != 1 || !g->rk[0].comm) G_FAIL(g, MI_EINVAL, "group: no transport between the processes of this group");
    else rc = [&]() -> int32_t {
        GroupRank &k = g->rk[0];
        (void)hipSetDevice(k.dev);
        G_CTX(g, 0, mi_reserve(k.ctx, k.stage, bytes * (size_t)(g->world + 1)));
        char *st = (char *)k.stage.p;
        hipStream_t s = k.xs;
        G_HIP(g, hipMemcpyAsync(st, local, bytes, hipMemcpyHostToDevice, s));
        const ncclResult_t r = mi_fault_hit() ? ncclInternalError : ncclAllGather(st, st + bytes, bytes, ncclUint8, k.comm, s);
        if (!nccl_ok(r)) {
            const std::string msg = std::string("group: ncclAllGather: ") + ncclGetErrorString(r);
            if (g->nonblocking) return nccl_abort_all(g, msg);
            G_FAIL(g, MI_EHIP, msg);
        }
        MI_TRY(nccl_settle(g, 0, "while issuing an all-gather"));
        G_HIP(g, hipMemcpyAsync(all, st + bytes, bytes * (size_t)g->world, hipMemcpyDeviceToHost, s));
        MI_TRY(nccl_wait_stream(g, 0, s, "in an all-gather"));
        return MI_OK;
    }();
    if (rc != MI_OK) g->broken = true;   // some ranks may have got through, others not: nothing collective can follow
    return rc;
}
// Every local rank contributes the call's carried status and a payload (mine[local rank]) in ONE all-gather: either every rank of the
// group returns MI_OK with all `world` payloads, or every rank returns an error -- a rank that failed its own, the others
// "group: rank r failed <phase> (status n)<tail>".
template <class P>
static int32_t group_gather(mi_group *g, const Carried &st, const std::vector<P> &mine, const char *phase, const char *tail, std::vector<P> &all) {
    struct Slot { int32_t rc; uint32_t pad[3]; P p; };
    static_assert(sizeof(Slot) <= SHM_AG_MAX, "a gathered payload must fit the link's all-gather area");
    std::vector<Slot> in(mine.size()), out((size_t)g->world);
    for (size_t i = 0; i < in.size(); i++) { std::memset((void *)&in[i], 0, sizeof(Slot)); in[i].rc = st.rc; std::memcpy((void *)&in[i].p, (const void *)&mine[i], sizeof(P)); }
    MI_TRY(group_allgather(g, in.data(), sizeof(Slot), out.data()));
    all.resize(out.size());
    for (int r = 0; r < g->world; r++) {
        if (out[r].rc != MI_OK) {
            if (!st.ok()) return st.leave(g);
            g->err = std::string("group: rank ") + std::to_string(r) + " failed " + phase + " (status " + std::to_string(out[r].rc) + ")" + tail;
            return out[r].rc;
        }
        std::memcpy((void *)&all[r], (const void *)&out[r].p, sizeof(P));
    }
    return MI_OK;
}
// What every rank says before the group enters an exchange: its status (st: the first failure among this process's ranks) and up to ten
// values that must be EQUAL on all ranks (bucket layouts of an exchange).  Every rank of the group returns MI_OK or every rank returns an
// error: the failing rank its own, the others "another rank failed".
static int32_t group_agree(mi_group *g, const Carried &st, const char *phase, const uint64_t *check = nullptr, uint32_t check_n = 0) {
    struct Checks { uint32_t n; uint64_t v[10]; } c;
    std::memset(&c, 0, sizeof c);
    c.n = check_n;
    for (uint32_t k = 0; k < check_n && k < 10; k++) c.v[k] = check[k];
    std::vector<Checks> all;
    MI_TRY(group_gather(g, st, std::vector<Checks>((size_t)g->n_local(), c), phase, "; nothing was exchanged", all));
    for (int r = 1; r < g->world; r++)
        if (all[r].n != all[0].n || std::memcmp(all[r].v, all[0].v, sizeof c.v) != 0)
            G_FAIL(g, MI_EINVAL, std::string("group: the ranks disagree on the shape of the exchange ") + phase);
    return MI_OK;
}
// Group-wide minimum and maximum of one 64-bit value per local rank (plans every rank must agree on: table budgets, window widths).
static int32_t group_min_max(mi_group *g, const std::vector<u64> &local, u64 *mn, u64 *mx) {
    std::vector<u64> all((size_t)g->world, 0);
    MI_TRY(group_allgather(g, local.data(), 8, all.data()));
    *mn = ~(u64)0; *mx = 0;
    for (u64 v : all) { if (v < *mn) *mn = v; if (v > *mx) *mx = v; }
    return MI_OK;
}

// ---------------------------------------------------------------- lifecycle
// The local ranks on devices devs[0..n): every rank's context first, then every rank's exchange stream and all the events it will ever
// record (the order matters: context, stream, context, stream moved a sharded proof at 2^22 by half a millisecond, up in mode 0 and
// down in mode 1, profiles/group_ranks.txt).  A rank is in g->rk from the moment it has a context, so that
// mi_group_destroy releases whatever a failure half-way left.
static int32_t ranks_open(mi_group *g, const int *devs, int n) {
    for (int i = 0; i < n; i++) {
        GroupRank k;
        MI_TRY(mi_init(k.dev = devs[i], &k.ctx));
        g->rk.push_back(k);
    }
    for (GroupRank &k : g->rk) {
        (void)hipSetDevice(k.dev);
        G_HIP(g, hipStreamCreateWithFlags(&k.xs, hipStreamNonBlocking));
        for (hipEvent_t &e : k.ev) G_HIP(g, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return MI_OK;
}
static void rank_release(GroupRank &k, bool broken) {   // everything but the context
    (void)hipSetDevice(k.dev);
    (void)hipStreamSynchronize(k.ctx->stream);
    if (k.xs) { (void)hipStreamSynchronize(k.xs); (void)hipStreamDestroy(k.xs); }
    // (a broken group's communicator was aborted where it broke; one that is merely unused is destroyed -- on a non-blocking
    //  communicator neither call holds this thread)
    if (k.comm) (void)(broken ? ncclCommAbort(k.comm) : ncclCommDestroy(k.comm));
    for (hipEvent_t e : k.ev) if (e) (void)hipEventDestroy(e);
    for (DevBuf *b : {&k.hv[H_A], &k.hv[H_B], &k.hv[H_C], &k.hv[H_Y0], &k.hv[H_Y1], &k.hh, &k.recv, &k.stage}) if (b->p) (void)hipFree(b->p);
    mi_cross_tables_free(&k.xt);
}

extern "C" {

int32_t mi_group_destroy(mi_group *g) {
    if (!g) return MI_EINVAL;
    for (GroupRank &k : g->rk) rank_release(k, g->broken);
    shm_detach(g);
    for (GroupRank &k : g->rk) { (void)hipSetDevice(k.dev); mi_shutdown(k.ctx); }
    delete g;
    return MI_OK;
}

// One process, n_dev contexts (SURVEY 8b's mi_init(dev_ids, n_dev, ...)): what a Go caller uses.
int32_t mi_group_create(const int *dev_ids, int n_dev, mi_group **out) {
    if (!dev_ids || !out || n_dev < 1 || n_dev > 64) return MI_EINVAL;
    *out = nullptr;
    mi_group *g = new (std::nothrow) mi_group();
    if (!g) return MI_ENOMEM;
    g->world = n_dev; g->rank0 = 0;
    bool distinct = true;
    for (int i = 0; i < n_dev; i++) for (int j = 0; j < i; j++) if (dev_ids[i] == dev_ids[j]) distinct = false;
    g->transport = distinct ? 1 : 2;
    int32_t rc = ranks_open(g, dev_ids, n_dev);
    if (rc == MI_OK && distinct) {
        // full-mesh xGMI: let every device map every other one (peer copies of the h slices; RCCL does its own set-up)
        for (int i = 0; i < n_dev; i++) for (int j = 0; j < n_dev; j++) if (i != j) {
            (void)hipSetDevice(dev_ids[i]);
            hipError_t e = hipDeviceEnablePeerAccess(dev_ids[j], 0);
            if (e != hipSuccess) (void)hipGetLastError();   // already enabled, or no direct link: hipMemcpyPeerAsync still works (staged)
        }
        std::vector<ncclComm_t> comms((size_t)n_dev, nullptr);
        if (ncclCommInitAll(comms.data(), n_dev, dev_ids) != ncclSuccess) rc = MI_EHIP;
        else for (int i = 0; i < n_dev; i++) g->rk[i].comm = comms[i];
    }
    if (rc != MI_OK) { mi_group_destroy(g); return rc; }
    *out = g;
    return MI_OK;
}

// One rank per process (torch.distributed.run, MPI): rank 0 makes the id, the caller's own channel distributes its 128 bytes.
int32_t mi_group_unique_id(uint8_t id[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    if (!id) return MI_EINVAL;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return MI_EHIP;
    std::memcpy(id, &u, 128);
    return MI_OK;
}
int32_t mi_group_create_rank_ex(int device_id, int rank, int world, const uint8_t id[128], int transport, mi_group **out) {
    if (!id || !out || world < 1 || rank < 0 || rank >= world || (transport != MI_GROUP_TRANSPORT_RCCL && transport != MI_GROUP_TRANSPORT_HOST)) return MI_EINVAL;
    *out = nullptr;
    mi_group *g = new (std::nothrow) mi_group();
    if (!g) return MI_ENOMEM;
    g->world = world; g->rank0 = rank; g->transport = transport;
    if (const char *e = getenv("MI_GROUP_TIMEOUT_MS")) { const int v = atoi(e); if (v > 0) g->timeout_ms = v; }
    int32_t rc = ranks_open(g, &device_id, 1);
    if (rc == MI_OK && transport == MI_GROUP_TRANSPORT_RCCL) {
        ncclUniqueId u;
        std::memcpy(&u, id, 128);
        (void)hipSetDevice(device_id);
        ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
        cfg.blocking = 0;   // (see "transport 1 with one rank per process: deadlines")
        g->nonblocking = true;
        const ncclResult_t r = ncclCommInitRankConfig(&g->rk[0].comm, world, u, rank, &cfg);
        if (!nccl_ok(r) || !g->rk[0].comm) { g->rk[0].comm = nullptr; g->err = std::string("ncclCommInitRankConfig: ") + ncclGetErrorString(r); rc = MI_EHIP; }
        else rc = nccl_settle(g, 0, "while the communicator was coming up (every rank of the group must call mi_group_create_rank)");
    }
    if (rc == MI_OK && transport == MI_GROUP_TRANSPORT_HOST) { (void)hipSetDevice(device_id); rc = shm_attach(g, id); }
    if (rc != MI_OK) { mi_group_destroy(g); return rc; }
    *out = g;
    return MI_OK;
}
int32_t mi_group_create_rank(int device_id, int rank, int world, const uint8_t id[128], mi_group **out) {
    return mi_group_create_rank_ex(device_id, rank, world, id, MI_GROUP_TRANSPORT_RCCL, out);
}
int32_t mi_group_set_lead_share(mi_group *g, uint32_t permille) {
    if (!g || (permille > 1000 && permille != MI_LEAD_SHARE_AUTO)) return MI_EINVAL;
    G_ENTER(g);
    g->lead_share = permille;
    return MI_OK;
}
int32_t mi_group_wire_range(const mi_group *g, uint64_t nb_wires, int rank, uint64_t *lo, uint64_t *hi) {
    if (!g || !lo || !hi || rank < 0 || rank >= g->world) return MI_EINVAL;
    u64 a, b;
    wire_range_of(nb_wires, g->world, rank, lead_share_of(g), a, b);
    *lo = a; *hi = b;
    return MI_OK;
}
int32_t mi_group_world(const mi_group *g) { return g ? g->world : 0; }
int32_t mi_group_rank(const mi_group *g) { return g ? g->rank0 : -1; }
int32_t mi_group_local(const mi_group *g) { return g ? g->n_local() : 0; }
mi_ctx *mi_group_ctx(mi_group *g, int local_rank) { return g && local_rank >= 0 && local_rank < g->n_local() ? g->rk[local_rank].ctx : nullptr; }
const char *mi_group_last_error(mi_group *g) { return g ? g->err.c_str() : "null group"; }
// 1 = RCCL communicator, 2 = copies inside this process (a device named twice), 3 = host-staged through shared memory
int32_t mi_group_transport(const mi_group *g) { return !g ? 0 : g->transport; }
// What the communicator ITSELF says about the group (observed, not derived from the arguments of mi_group_create_rank): the number of
// ranks RCCL joined (ncclCommCount of this process's first communicator), 0 when the transport is not RCCL, negative on an RCCL error.
int32_t mi_group_comm_ranks(const mi_group *g) {
    if (!g) return MI_EINVAL;
    if (g->transport != MI_GROUP_TRANSPORT_RCCL || g->rk.empty() || !g->rk[0].comm) return 0;
    int n = 0;
    return ncclCommCount(g->rk[0].comm, &n) == ncclSuccess ? n : MI_EHIP;
}
// PCI bus id ("0000:c1:00.0") of the device local rank `local_rank` runs on, as the HIP runtime reports it: what tells two ranks on two
// GPUs from two ranks on one.
int32_t mi_group_device_pci(const mi_group *g, int local_rank, char out[32]) {
    if (!g || !out || local_rank < 0 || local_rank >= g->n_local()) return MI_EINVAL;
    out[0] = 0;
    return hipDeviceGetPCIBusId(out, 32, g->rk[local_rank].dev) == hipSuccess ? MI_OK : MI_EHIP;
}

// Every local rank sends a distinct pattern of `bytes` bytes to every rank of the group (itself included) and checks what it
// received: the transport (RCCL grouped send / recv, peer copies, or the shared-memory rings) in isolation, then the all-gather of
// host values the agreements and the partial-sum combine use.  All ranks of the group call it together.
int32_t mi_group_exchange_selftest(mi_group *g, size_t bytes) {
    if (!g || !bytes || bytes > ((size_t)1 << 28)) return MI_EINVAL;
    G_ENTER(g);
    const int nl = g->n_local(), W = g->world;
    std::vector<void *> sbuf(nl, nullptr), rbuf(nl, nullptr);
    std::vector<Xfer> list;
    auto pat = [](int src, int dst, size_t k) { return (unsigned char)(17 * src + 101 * dst + 3 * k + (k >> 8)); };
    auto prepare = [&]() -> int32_t {
        for (int i = 0; i < nl; i++) {
            hipStream_t xs = g->rk[i].xs;
            (void)hipSetDevice(g->rk[i].dev);
            G_HIP(g, hipMalloc(&sbuf[i], bytes * W)); G_HIP(g, hipMalloc(&rbuf[i], bytes * W));
            std::vector<unsigned char> h(bytes * W);
            for (int d = 0; d < W; d++) for (size_t k = 0; k < bytes; k++) h[d * bytes + k] = pat(g->rank0 + i, d, k);
            G_HIP(g, hipMemcpyAsync(sbuf[i], h.data(), h.size(), hipMemcpyHostToDevice, xs));
            G_HIP(g, hipMemsetAsync(rbuf[i], 0, bytes * W, xs));
            G_HIP(g, hipStreamSynchronize(xs));
        }
        return MI_OK;
    };
    auto verify = [&]() -> int32_t {
        for (int i = 0; i < nl; i++) {
            (void)hipSetDevice(g->rk[i].dev);
            std::vector<unsigned char> h(bytes * W);
            G_HIP(g, hipMemcpyAsync(h.data(), rbuf[i], h.size(), hipMemcpyDeviceToHost, g->rk[i].xs));
            G_HIP(g, hipStreamSynchronize(g->rk[i].xs));
            for (int s = 0; s < W; s++) for (size_t k = 0; k < bytes; k++)
                if (h[s * bytes + k] != pat(s, g->rank0 + i, k)) G_FAIL(g, MI_EHIP, "group: exchange self-test received wrong bytes");
        }
        return MI_OK;
    };
    auto body = [&]() -> int32_t {
        Carried st, seen;
        st.note(prepare(), g->err);
        MI_TRY(group_agree(g, st, "while preparing the self-test"));   // a rank without buffers must not leave the others in the exchange
        for (int s = 0; s < W; s++) for (int d = 0; d < W; d++) {
            Xfer x{s, d, nullptr, nullptr, bytes};
            if (g->local(s)) x.sp = (char *)sbuf[s - g->rank0] + (size_t)d * bytes;
            if (g->local(d)) x.dp = (char *)rbuf[d - g->rank0] + (size_t)s * bytes;
            list.push_back(x);
        }
        MI_TRY(run_xfers(g, list));
        seen.note(verify(), g->err);
        // the all-gather of host values: every rank contributes (rank, 3 rank + 1) and must read that back from everyone
        std::vector<u64> mine(2 * (size_t)nl), all(2 * (size_t)W);
        for (int i = 0; i < nl; i++) { mine[2 * i] = (u64)(g->rank0 + i); mine[2 * i + 1] = 3 * (u64)(g->rank0 + i) + 1; }
        MI_TRY(group_allgather(g, mine.data(), 16, all.data()));
        for (int r = 0; r < W; r++)
            if (all[2 * r] != (u64)r || all[2 * r + 1] != 3 * (u64)r + 1) seen.note(MI_EHIP, "group: all-gather self-test received wrong values");
        return group_agree(g, seen, "in the transport self-test");
    };
    const int32_t rc = body();
    for (int i = 0; i < nl; i++) { (void)hipSetDevice(g->rk[i].dev); if (sbuf[i]) (void)hipFree(sbuf[i]); if (rbuf[i]) (void)hipFree(rbuf[i]); }
    return rc;
}

}  // extern "C"

// ---------------------------------------------------------------- mode 1: reduce-scatter of the bucket sums of MSM slots
// Every local rank has enqueued the MSMs of `slots` with MI_MSM_DEFER_REDUCE.  prepare (local, may fail): bucket views, receive
// buffer, the layout values the ranks must agree on.  run (after the agreement): ONE batch of the transport for all the slots,
// then per slot the sum of the received slices and the reduce.  Local failures inside run are returned AFTER the rank has taken part
// in the batch (the peers are in it).
struct BucketExchange {
    std::vector<int> slots, curves;
    std::vector<std::vector<MsmBucketView>> v;   // [slot index][local rank]
    std::vector<size_t> off;                     // receive-buffer offset of every slot's region
};
static int32_t exchange_prepare(mi_group *g, BucketExchange &bx, const int *slots, const int *curves, int n_slots, std::vector<uint64_t> &check) {
    const int nl = g->n_local(), W = g->world;
    bx.slots.assign(slots, slots + n_slots); bx.curves.assign(curves, curves + n_slots);
    bx.v.assign(n_slots, std::vector<MsmBucketView>(nl));
    bx.off.assign(n_slots + 1, 0);
    for (int k = 0; k < n_slots; k++) {
        const MsmCurveOps &ops = mi_msm_ops(curves[k]);
        for (int i = 0; i < nl; i++) {
            G_CTX(g, i, mi_msm_bucket_view(g->rk[i].ctx, slots[k], curves[k], &bx.v[k][i]));
            if (!bx.v[k][i].bucket) G_FAIL(g, MI_EINVAL, "group: mode 1 (bucket exchange): a rank has no bucket array for one of the MSMs");
            if (bx.v[k][i].nkeys != bx.v[k][0].nkeys || bx.v[k][i].c != bx.v[k][0].c) G_FAIL(g, MI_EINVAL, "group: the ranks disagree on the bucket layout of an MSM");
        }
        const size_t K = bx.v[k][0].nkeys, own_max = (K + W - 1) / W + 1;
        bx.off[k + 1] = bx.off[k] + (size_t)(W > 1 ? W - 1 : 1) * own_max * ops.xyzz_bytes;
        check.push_back(((uint64_t)K << 8) | bx.v[k][0].c);
    }
    for (int i = 0; i < nl; i++) {
        (void)hipSetDevice(g->rk[i].dev);
        // the previous batch's slice sums still read the buffer on the exchange stream: growing it (hipFree) synchronises the device, reusing it is ordered by that stream
        G_CTX(g, i, mi_reserve(g->rk[i].ctx, g->rk[i].recv, bx.off[n_slots] + 256));
    }
    return MI_OK;
}
static int32_t exchange_run(mi_group *g, const BucketExchange &bx, int first, int count) {
    const int nl = g->n_local(), W = g->world;
    Carried st;
    for (int i = 0; i < nl; i++) {
        (void)hipSetDevice(g->rk[i].dev);
        for (int k = first; k < first + count; k++) {
            const hipError_t e = hipStreamWaitEvent(g->rk[i].xs, bx.v[k][i].ready, 0);
            if (e != hipSuccess) st.note(MI_EHIP, std::string("hipStreamWaitEvent (bucket sums ready): ") + hipGetErrorString(e));
        }
    }
    std::vector<Xfer> list;
    for (int k = first; k < first + count; k++) {
        const size_t K = bx.v[k][0].nkeys, B = mi_msm_ops(bx.curves[k]).xyzz_bytes;
        for (int s = 0; s < W; s++) for (int d = 0; d < W; d++) {
            if (s == d) continue;
            u64 lo, hi;
            range_of(K, W, d, lo, hi);
            Xfer x{s, d, nullptr, nullptr, (size_t)(hi - lo) * B};
            if (g->local(s)) x.sp = (const char *)bx.v[k][s - g->rank0].bucket + lo * B;
            if (g->local(d)) x.dp = (char *)g->rk[d - g->rank0].recv.p + bx.off[k] + (size_t)(s < d ? s : s - 1) * (hi - lo) * B;
            list.push_back(x);
        }
    }
    MI_TRY(run_xfers(g, list));   // a transport failure: the group is broken, nothing below matters
    for (int i = 0; i < nl; i++) {
        GroupRank &rk = g->rk[i];
        (void)hipSetDevice(rk.dev);
        for (int k = first; k < first + count; k++) {
            const MsmCurveOps &ops = mi_msm_ops(bx.curves[k]);
            const size_t K = bx.v[k][0].nkeys, B = ops.xyzz_bytes;
            const auto post = [&]() -> int32_t {
                u64 lo, hi;
                range_of(K, W, g->rank0 + i, lo, hi);
                char *bk = (char *)bx.v[k][i].bucket;
                ops.sum_slices(rk.xs, bk + lo * B, (const char *)rk.recv.p + bx.off[k], (u32)(W - 1), (u32)(hi - lo));
                G_HIP(g, hipGetLastError());
                // keys of other owners: their sums live there now; here they read as infinity for the reduce
                if (lo) G_HIP(g, hipMemsetAsync(bk, 0, lo * B, rk.xs));
                if (hi < K) G_HIP(g, hipMemsetAsync(bk + hi * B, 0, (K - hi) * B, rk.xs));
                G_HIP(g, hipEventRecord(rk.ev[E_DONE], rk.xs));
                G_HIP(g, hipStreamWaitEvent(bx.v[k][i].stream, rk.ev[E_DONE], 0));
                G_CTX(g, i, mi_msm_reduce_enqueue(rk.ctx, bx.slots[k], bx.curves[k]));
                return MI_OK;
            };
            st.note(post(), g->err);
        }
    }
    return st.leave(g);
}

// Whatever a failed call left on a context's MSM slots is collected (a deferred slot runs its reduce over its local buckets first), so
// that the next call finds every slot idle.  Errors here change nothing any more.
static void drain_slots(mi_group *g, const int *slots, const int *curves, int n) {
    for (GroupRank &rk : g->rk) {
        (void)hipSetDevice(rk.dev);
        G1X t1; G2X t2;
        for (int k = 0; k < n; k++) {
            (void)mi_msm_reduce_enqueue(rk.ctx, slots[k], curves[k]);
            (void)mi_msm_finish(rk.ctx, slots[k], curves[k], curves[k] == 1 ? (void *)&t1 : (void *)&t2);
        }
        (void)hipStreamSynchronize(rk.ctx->stream);
        (void)hipStreamSynchronize(rk.xs);
    }
}

template <class F, class JacT>
static void write_jac(const XYZZ<F> &r, JacT *out) {
    Jac<F> j;
    if (r.is_inf()) j = Jac<F>{F::one(), F::one(), F::zero()};
    else { Affine<F> a = xyzz_to_affine(r); j = Jac<F>{a.x, a.y, F::one()}; }
    std::memcpy(out, &j, sizeof(j));
}
// runs fn(i) for every local rank, rank 0 on this thread and the others on threads of their own (an MSM enqueue waits once on the
// host for its sort's largest bucket, msm.hip: one after the other, rank i + 1 would not even start its sort before rank i's has
// counted); notes the first failure in rank order with its context's text
template <class Fn>
static void for_each_local_rank(mi_group *g, Carried &st, Fn fn) {
    const int nl = g->n_local();
    std::vector<int32_t> rcs((size_t)nl, MI_OK);
    auto guarded = [&](int i) { try { (void)hipSetDevice(g->rk[i].dev); rcs[i] = fn(i); } catch (...) { rcs[i] = MI_ENOMEM; } };
    std::vector<std::thread> th;
    for (int i = 1; i < nl; i++) {
        try { th.emplace_back(guarded, i); } catch (...) { guarded(i); }   // no thread to be had: in line
    }
    guarded(0);
    for (auto &t : th) t.join();
    (void)hipSetDevice(g->rk[0].dev);
    for (int i = 0; i < nl; i++) st.note(rcs[i], mi_last_error(g->rk[i].ctx));
}

// One MSM whose (point, scalar) pairs are already spread over the local ranks' devices.
template <class F, class JacT>
static int32_t msm_sharded_dev(mi_group *g, int curve, const void *const *pts_dev, const void *const *sc_dev, const size_t *n_local, size_t n_total,
                               uint32_t flags, uint32_t mode, JacT *out) {
    if (!g || !pts_dev || !sc_dev || !n_local || !out || (flags & ~1u) || mode > 1) return MI_EINVAL;
    const int nl = g->n_local();
    // every rank must cut its scalars into the same windows: width from the largest share, not from the local count
    const u32 c = mi_msm_auto_c((n_total + g->world - 1) / g->world);
    const uint32_t df = mode == 1 ? MI_MSM_DEFER_REDUCE : 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int slots[1] = {MSM_SLOT_A}, curves[1] = {curve};
    Carried st;
    for_each_local_rank(g, st, [&](int i) -> int32_t {
        mi_ctx *ctx = g->rk[i].ctx;
        std::memset(&ctx->stats, 0, sizeof(ctx->stats));
        MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_T0], ctx->stream));
        return mi_msm_enqueue(ctx, MSM_SLOT_A, -1, curve, pts_dev[i], sc_dev[i], n_local[i], flags | df, ctx->ev[EV_T0], curve == 1, 0, 0, c);
    });
    BucketExchange bx;
    std::vector<uint64_t> check{(uint64_t)n_total, (uint64_t)mode, (uint64_t)flags};
    if (mode == 1 && st.ok()) st.note(exchange_prepare(g, bx, slots, curves, 1, check), g->err);
    int32_t rc = group_agree(g, st, "while enqueueing its share of the MSM", check.data(), (uint32_t)check.size());
    if (rc == MI_OK && mode == 1) { const int32_t r = exchange_run(g, bx, 0, 1); if (g->broken) rc = r; else st.note(r, g->err); }
    // the partial sums and the status of every rank in ONE all-gather: all ranks return the sum, or all return an error
    std::vector<XYZZ<F>> mine((size_t)nl), all;
    if (rc == MI_OK) {
        for (int i = 0; i < nl; i++) {
            (void)hipSetDevice(g->rk[i].dev);
            std::memset((void *)&mine[i], 0, sizeof mine[i]);
            if (st.ok()) st.note(mi_msm_finish(g->rk[i].ctx, MSM_SLOT_A, curve, &mine[i]), mi_last_error(g->rk[i].ctx));
        }
        rc = group_gather(g, st, mine, "in its share of the MSM", "", all);
    }
    if (rc != MI_OK) { const std::string keep = g->err; drain_slots(g, slots, curves, 1); g->err = keep; return rc; }
    XYZZ<F> total = XYZZ<F>::inf();
    for (const XYZZ<F> &p : all) xyzz_add(total, p);
    write_jac<F>(total, out);
    g->rk[0].ctx->stats.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MI_OK;
}

// Host arrays, one process: cut into contiguous slices, upload slice r to rank r, run the sharded MSM.
template <class F, class AffT, class JacT>
static int32_t msm_sharded_host(mi_group *g, int curve, const AffT *pts, const mi_fr *scalars, size_t n, uint32_t flags, uint32_t mode, JacT *out) {
    if (!g || !out || ((!pts || !scalars) && n)) return MI_EINVAL;
    if (g->n_local() != g->world) G_FAIL(g, MI_EINVAL, "group: host-array entry points need all ranks in this process");
    const int nl = g->n_local();
    std::vector<const void *> pp(nl), ss(nl);
    std::vector<size_t> nn(nl);
    for (int i = 0; i < nl; i++) {
        u64 lo, hi;
        range_of(n, g->world, i, lo, hi);
        (void)hipSetDevice(g->rk[i].dev);
        mi_ctx *ctx = g->rk[i].ctx;
        G_CTX(g, i, mi_reserve(ctx, ctx->ws[WS_HOST_IO0], (hi - lo) * sizeof(AffT) + 64));
        G_CTX(g, i, mi_reserve(ctx, ctx->ws[WS_HOST_IO1], (hi - lo) * sizeof(mi_fr) + 64));
        if (hi > lo) {
            G_HIP(g, hipMemcpyAsync(ctx->ws[WS_HOST_IO0].p, pts + lo, (hi - lo) * sizeof(AffT), hipMemcpyHostToDevice, ctx->stream));
            G_HIP(g, hipMemcpyAsync(ctx->ws[WS_HOST_IO1].p, scalars + lo, (hi - lo) * sizeof(mi_fr), hipMemcpyHostToDevice, ctx->stream));
        }
        pp[i] = ctx->ws[WS_HOST_IO0].p; ss[i] = ctx->ws[WS_HOST_IO1].p; nn[i] = hi - lo;
    }
    return msm_sharded_dev<F>(g, curve, pp.data(), ss.data(), nn.data(), n, flags, mode, out);
}

extern "C" {

int32_t mi_msm_g1_sharded_dev(mi_group *g, const mi_g1_affine *const *pts_dev, const mi_fr *const *scalars_dev, const size_t *n_local, size_t n_total,
                              uint32_t flags, uint32_t mode, mi_g1_jac *out) {
    G_ENTER(g);
    return msm_sharded_dev<Fp>(g, 1, (const void *const *)pts_dev, (const void *const *)scalars_dev, n_local, n_total, flags, mode, out);
}
int32_t mi_msm_g2_sharded_dev(mi_group *g, const mi_g2_affine *const *pts_dev, const mi_fr *const *scalars_dev, const size_t *n_local, size_t n_total,
                              uint32_t flags, uint32_t mode, mi_g2_jac *out) {
    G_ENTER(g);
    return msm_sharded_dev<Fp2>(g, 2, (const void *const *)pts_dev, (const void *const *)scalars_dev, n_local, n_total, flags, mode, out);
}
int32_t mi_msm_g1_sharded(mi_group *g, const mi_g1_affine *pts, const mi_fr *scalars, size_t n, uint32_t flags, uint32_t mode, mi_g1_jac *out) {
    G_ENTER(g);
    return msm_sharded_host<Fp>(g, 1, pts, scalars, n, flags, mode, out);
}
int32_t mi_msm_g2_sharded(mi_group *g, const mi_g2_affine *pts, const mi_fr *scalars, size_t n, uint32_t flags, uint32_t mode, mi_g2_jac *out) {
    G_ENTER(g);
    return msm_sharded_host<Fp2>(g, 2, pts, scalars, n, flags, mode, out);
}

// ---------------------------------------------------------------- computeH over the ranks of the group (csrc/ntt_cross.hip has the maths)
// Data: rank r holds the natural-order slice [r M, (r + 1) M) of a, b (and c) in its hv[H_A], [H_B], [H_C], M = N / world.  Result: the
// coefficients of h in gnark's bit-reversed order, slice r on rank r, in its hh + 1 (slot 0 = the previous rank's last coefficient,
// fetched by one more batch: the Z pairs of a sharded key are cut over N - 1, so every slice but the first starts one element early).
// Six transforms as on one device (h = den FFT^-1_coset(ca cb) - den FFT^-1(c)); each is a local size-M transform and one cross-rank
// step between two all-to-alls over the group's transport -- 9 batches of (world - 1) / world of a slice per rank: the pair between
// the coset transforms of a, b and the last transform cancels.
// Local failures are CARRIED THROUGH every batch (the peers are in them) and returned at the end; a transport failure breaks the group.
static bool sharded_h_possible(const mi_group *g, u32 log_n) {
    const int W = g->world;
    if (W < 2 || W > 16 || (W & (W - 1))) return false;
    return log_n >= 2 * g->log_w() && log_n <= 28;
}
// Everything compute_h_sharded allocates -- the cross-rank tables, the two exchange vectors, the h slice -- for ONE local rank.
// Called in the LOCAL phase of the callers, before the group agrees to proceed: an allocation that fails here is an MI_ENOMEM
// every rank returns with the group intact, not a null pointer under kernels and transfers the peers are already waiting for.
static int32_t compute_h_sharded_prepare(mi_group *g, int i, u32 log_n) {
    const mi_group::HCut cut = g->h_cut(log_n);
    GroupRank &k = g->rk[i];
    MI_TRY(mi_cross_tables_build(k.ctx, log_n, cut.log_w, (u32)(g->rank0 + i), &k.xt));
    MI_TRY(mi_reserve(k.ctx, k.hv[H_Y0], cut.M * sizeof(Fr)));
    MI_TRY(mi_reserve(k.ctx, k.hv[H_Y1], cut.M * sizeof(Fr)));
    return mi_reserve(k.ctx, k.hh, (cut.M + 1) * sizeof(Fr));
}
static bool compute_h_sharded_prepared(const GroupRank &k) { return k.hv[H_Y0].p && k.hv[H_Y1].p && k.hh.p && k.xt.s_fwd && k.xt.s_inv; }
// One batch between two stream hand-overs: the exchange stream of every local rank picks up behind event `after` of its context's
// stream, the batch runs, and with `back` the context's stream picks up behind the batch.  A hand-over that fails is a LOCAL failure:
// noted, and the rank still takes part in the batch.  Returns the transport's status.
static int32_t run_batch_behind(mi_group *g, const std::vector<Xfer> &list, int after, bool back, Carried &st) {
    for (GroupRank &k : g->rk) {
        (void)hipSetDevice(k.dev);
        if (hipStreamWaitEvent(k.xs, k.ev[after], 0) != hipSuccess) st.note(MI_EHIP, "sharded computeH: stream hand-over failed");
    }
    MI_TRY(run_xfers(g, list));
    for (GroupRank &k : g->rk) {
        if (!back) break;
        (void)hipSetDevice(k.dev);
        if (hipEventRecord(k.ev[E_C1], k.xs) != hipSuccess || hipStreamWaitEvent(k.ctx->stream, k.ev[E_C1], 0) != hipSuccess) st.note(MI_EHIP, "sharded computeH: stream hand-over failed");
    }
    return MI_OK;
}
static int32_t compute_h_sharded(mi_group *g, u32 log_n, bool derive_c) {
    const MiRange range_fn("mi.group.computeH.enqueue");
    const int W = g->world;
    const mi_group::HCut cut = g->h_cut(log_n);
    const u32 log_m = cut.log_m;
    const size_t M = cut.M, row = cut.cnt * sizeof(Fr);
    Carried st;
    auto each = [&](const std::function<int32_t(GroupRank &, mi_ctx *)> &fn) {
        for (GroupRank &k : g->rk) { (void)hipSetDevice(k.dev); st.note(fn(k, k.ctx), mi_last_error(k.ctx)); }
    };
    // the callers prepared every local rank and the GROUP agreed on the outcome: nothing is allocated from here on.  (A caller that skipped
    // that would have kernels and transfers run on null buffers: refused before anything is enqueued.)
    for (const GroupRank &k : g->rk) if (!compute_h_sharded_prepared(k)) { g->err = "sharded computeH: buffers were not prepared before the agreement"; return MI_EINVAL; }
    auto mark = [&](int ev, const char *what = "sharded computeH: hipEventRecord failed") {
        for (GroupRank &k : g->rk) { (void)hipSetDevice(k.dev); if (hipEventRecord(k.ev[ev], k.ctx->stream) != hipSuccess) st.note(MI_EHIP, what); }
    };
    // all-to-all: block d of the source rank's buffer -> block s of rank d's buffer (the same rule in both directions); the exchange
    // streams pick up behind event `after` of their context's stream and hand back to it when the batch is done
    auto a2a = [&](int from, int to, int after) -> int32_t {
        std::vector<Xfer> list;
        for (int s = 0; s < W; s++) for (int d = 0; d < W; d++) {
            Xfer x{s, d, nullptr, nullptr, row};
            if (g->local(s)) x.sp = (const char *)g->rk[s - g->rank0].hv[from].p + (size_t)d * row;
            if (g->local(d)) x.dp = (char *)g->rk[d - g->rank0].hv[to].p + (size_t)s * row;
            list.push_back(x);
        }
        return run_batch_behind(g, list, after, true, st);
    };
    // the pieces of a transform (csrc/ntt_cross.hip header): cross-rank step of FFTInverse on the columns in Y; local size-M FFTInverse;
    // coset factor + local size-M FFT (DIT) of a coefficient slice
    auto cross_inv = [&](int Y, bool den_scale) { each([&](GroupRank &k, mi_ctx *c) { return mi_cross_dft(c, c->stream, k.hv[Y].p, k.xt, 0, den_scale); }); };
    auto local_inv = [&](int X) { each([&](GroupRank &k, mi_ctx *c) { return mi_ntt_dev_impl(c, (mi_fr *)k.hv[X].p, log_m, MI_NTT_INVERSE); }); };
    auto local_fwd = [&](int X) {
        each([&](GroupRank &k, mi_ctx *c) -> int32_t {
            MI_TRY(mi_cross_mul(c, c->stream, k.hv[X].p, k.hv[X].p, k.xt.s_fwd, nullptr, M));
            return mi_ntt_dev_impl(c, (mi_fr *)k.hv[X].p, log_m, MI_NTT_DIT);
        });
    };
    // The six transforms, interleaved so that a batch of the transport moves one vector while the kernels of another run (a batch
    // blocks this thread until it is complete -- the transports' deadline rule -- so what should overlap it is enqueued BEFORE it):
    //   FFTInverse(a), (b), (c) = [rows -> columns] cross-rank step [columns -> rows] local transform;  FFT_coset(a), (b) = factor, local
    //   transform [rows -> columns];  then the middle kernel (cross-rank steps of a and b, product, cross-rank step of the last
    //   FFTInverse: the all-to-all pair in between cancels)  [columns -> rows]  local transform.   9 batches.
    if (derive_c) each([&](GroupRank &k, mi_ctx *c) { return mi_cross_mul(c, c->stream, k.hv[H_C].p, k.hv[H_A].p, k.hv[H_B].p, nullptr, M); });
    mark(E_IN);
    MI_TRY(a2a(H_A, H_Y0, E_IN));
    cross_inv(H_Y0, false); mark(E_DA);
    MI_TRY(a2a(H_B, H_Y1, E_IN));               // under a's cross-rank step
    cross_inv(H_Y1, false); mark(E_DB);
    MI_TRY(a2a(H_Y0, H_A, E_DA));               // under b's cross-rank step
    local_inv(H_A); local_fwd(H_A); mark(E_FA);
    MI_TRY(a2a(H_C, H_Y0, E_IN));               // under a's two local transforms
    cross_inv(H_Y0, true); mark(E_DC);          // den * coefficients of c
    MI_TRY(a2a(H_Y1, H_B, E_DB));
    local_inv(H_B); local_fwd(H_B); mark(E_FB);
    MI_TRY(a2a(H_Y0, H_C, E_DC));               // under b's two local transforms
    local_inv(H_C);
    MI_TRY(a2a(H_A, H_Y0, E_FA));               // under c's local transform
    MI_TRY(a2a(H_B, H_Y1, E_FB));
    each([&](GroupRank &k, mi_ctx *c) { return mi_cross_mid(c, c->stream, k.hv[H_Y0].p, k.hv[H_Y1].p, k.xt); });
    mark(E_MID);
    MI_TRY(a2a(H_Y0, H_A, E_MID));
    local_inv(H_A);
    // h = den g^-k (.) - den c_k, into the h slice behind its front slot
    each([&](GroupRank &k, mi_ctx *c) { return mi_cross_mul(c, c->stream, (char *)k.hh.p + sizeof(Fr), k.hv[H_A].p, k.xt.s_inv, k.hv[H_C].p, M); });
    std::vector<Xfer> last;   // every rank's last coefficient -> the front slot of the next rank
    for (int r = 0; r + 1 < W; r++) {
        Xfer x{r, r + 1, nullptr, nullptr, sizeof(Fr)};
        if (g->local(r)) x.sp = (const char *)g->rk[r - g->rank0].hh.p + M * sizeof(Fr);
        if (g->local(r + 1)) x.dp = g->rk[r + 1 - g->rank0].hh.p;
        last.push_back(x);
    }
    mark(E_C0, "sharded computeH: stream hand-over failed");
    MI_TRY(run_batch_behind(g, last, E_C0, true, st));
    return st.leave(g);
}
// fills hv[which] of local rank i with its slice of a vector of n_valid elements: rows [r M, (r + 1) M), zero beyond n_valid.
// src: host (whole vector) or device (THIS rank's slice, i.e. the elements [r M, min((r + 1) M, n_valid)))
static int32_t load_h_slice(mi_group *g, int i, int which, u32 log_m, const mi_fr *src, bool host_whole, size_t n_valid, hipStream_t st) {
    mi_ctx *c = g->rk[i].ctx;
    const size_t M = (size_t)1 << log_m, lo = (size_t)(g->rank0 + i) * M;
    const size_t have = n_valid > lo ? (n_valid - lo < M ? n_valid - lo : M) : 0;
    MI_TRY(mi_reserve(c, g->rk[i].hv[which], M * sizeof(Fr)));
    char *dst = (char *)g->rk[i].hv[which].p;
    if (have) {
        if (!src) MI_FAIL(c, MI_EINVAL, "sharded computeH: null input vector");
        if (host_whole) MI_CHECK_HIP(c, hipMemcpyAsync(dst, src + lo, have * sizeof(Fr), hipMemcpyHostToDevice, st));
        else MI_CHECK_HIP(c, hipMemcpyAsync(dst, src, have * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    }
    if (have < M) MI_CHECK_HIP(c, hipMemsetAsync(dst + have * sizeof(Fr), 0, (M - have) * sizeof(Fr), st));
    return MI_OK;
}

extern "C" {
int32_t mi_group_set_sharded_compute_h(mi_group *g, uint32_t on) {
    if (!g || on > 1) return MI_EINVAL;
    G_ENTER(g);
    g->sharded_h = on != 0;
    return MI_OK;
}
// computeH alone over the ranks: every local rank passes ITS slices (device pointers; c_sl == NULL: c = a o b) and receives its slice
// of h (M elements of gnark's bit-reversed order).  A collective: all ranks call it together.
int32_t mi_compute_h_sharded_dev(mi_group *g, uint32_t log_n, const mi_fr *const *a_sl, const mi_fr *const *b_sl, const mi_fr *const *c_sl,
                                 size_t n_constraints, mi_fr *const *h_sl) {
    if (!g || !a_sl || !b_sl || !h_sl) return MI_EINVAL;
    G_ENTER(g);
    Carried st;
    if (!sharded_h_possible(g, log_n) || n_constraints > ((size_t)1 << log_n)) st.note(MI_EINVAL, "sharded computeH: needs 2, 4, 8 or 16 ranks, N >= ranks^2 and n_constraints <= N");
    const u32 log_m = log_n - g->log_w();   // (meaningless where the shape was refused: nothing below uses it then)
    for (int i = 0; i < g->n_local() && st.ok(); i++) {
        (void)hipSetDevice(g->rk[i].dev);
        mi_ctx *c = g->rk[i].ctx;
        int32_t rc = load_h_slice(g, i, H_A, log_m, a_sl[i], false, n_constraints, c->stream);
        if (rc == MI_OK) rc = load_h_slice(g, i, H_B, log_m, b_sl[i], false, n_constraints, c->stream);
        if (rc == MI_OK) rc = c_sl ? load_h_slice(g, i, H_C, log_m, c_sl[i], false, n_constraints, c->stream) : mi_reserve(c, g->rk[i].hv[H_C], sizeof(Fr) << log_m);
        if (rc == MI_OK) rc = compute_h_sharded_prepare(g, i, log_n);   // every buffer of the collective exists BEFORE the ranks agree to enter it
        st.note(rc, mi_last_error(c));
    }
    const uint64_t check[3] = {log_n, (uint64_t)n_constraints, c_sl ? 1u : 0u};
    MI_TRY(group_agree(g, st, "while loading its slices for computeH", check, 3));
    const int32_t rc = compute_h_sharded(g, log_n, c_sl == nullptr);
    if (g->broken) return rc;
    st.note(rc, g->err);
    for (int i = 0; i < g->n_local() && st.ok(); i++) {
        (void)hipSetDevice(g->rk[i].dev);
        mi_ctx *c = g->rk[i].ctx;
        hipError_t e = hipMemcpyAsync(h_sl[i], (const char *)g->rk[i].hh.p + sizeof(Fr), sizeof(Fr) << log_m, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) st.note(MI_EHIP, std::string("sharded computeH: copying h out failed: ") + hipGetErrorString(e));
    }
    return group_agree(g, st, "in the sharded computeH");
}
}  // extern "C"

// ---------------------------------------------------------------- sharded proving key
static void pk_sharded_release(mi_group *g, mi_pk_sharded *spk) {
    for (size_t i = 0; i < spk->part.size(); i++) if (spk->part[i]) { (void)hipSetDevice(g->rk[i].dev); mi_pk_free(g->rk[i].ctx, spk->part[i]); }
    delete spk;
}
int32_t mi_pk_sharded_free(mi_group *g, mi_pk_sharded *spk) {
    if (!g || !spk) return MI_EINVAL;
    GroupCall call__(g);
    if (!call__.ok) return MI_EINVAL;   // (a broken group still frees its keys)
    pk_sharded_release(g, spk);
    return MI_OK;
}

}  // extern "C"

// Splits pk.G1.{A,B,K,Z} and pk.G2.B into `world` contiguous slices (by wire; Z by index) and makes slice r resident on rank r.
//   host arrays    descs = ONE whole-key descriptor (what mi_pk_load takes); every process of a multi-process group passes it.
//   device arrays  descs = one descriptor per LOCAL rank: header and masks of the WHOLE key (host), point arrays = that rank's
//                  slices already on that rank's device (counts = points of the slice), adopted by reference as mi_pk_load_dev does.
static int32_t pk_load_sharded_impl(mi_group *g, const mi_pk_desc *descs, bool device_points, mi_pk_sharded **out) {
    if (!g || !descs || !out) return MI_EINVAL;
    *out = nullptr;
    const mi_pk_desc *d = descs;
    const int nl = g->n_local(), W = g->world;
    {   // the header every process passes must be acceptable AND the same everywhere before anything collective starts
        Carried st;
        if (d->log_n > 28 || !d->infinity_a || !d->infinity_b || d->nb_public > d->nb_wires) st.note(MI_EINVAL, "pk: bad header");
        if (st.ok() && device_points) for (int i = 1; i < nl; i++)
            if (descs[i].log_n != d->log_n || descs[i].nb_wires != d->nb_wires || descs[i].nb_public != d->nb_public || !descs[i].infinity_a || !descs[i].infinity_b)
                st.note(MI_EINVAL, "pk: the per-rank descriptors disagree on the key's header");
        const uint64_t check[4] = {d->log_n, d->nb_wires, d->nb_public, lead_share_of(g)};   // (the lead's wire share must be the same on every rank)
        MI_TRY(group_agree(g, st, "while checking the key's header", check, 4));
    }
    const u64 N = (u64)1 << d->log_n;
    mi_pk_sharded *spk = new (std::nothrow) mi_pk_sharded();
    if (!spk) return MI_ENOMEM;
    spk->part.assign(nl, nullptr); spk->log_n = d->log_n; spk->nb_wires = d->nb_wires;
    // window widths of the generic path that all parts share (mode 1 needs equal bucket layouts): from the LARGEST part of each MSM
    // (a rank WITHOUT pairs of some MSM -- the lead with a wire share of 0, a tiny key -- still takes part in mode 1: an empty deferred MSM
    //  leaves a zeroed bucket array of the agreed shape, msm.hip mi_msm_enqueue)
    const uint32_t share = lead_share_of(g);
    spk->lead_share = share;
    u64 largest[3] = {0, 0, 0};   // pairs of A+K, B, Z
    for (int r = 0; r < W; r++) {
        u64 lo, hi, zlo, zhi, nb = 0;
        wire_range_of(d->nb_wires, W, r, share, lo, hi); range_of(N - 1, W, r, zlo, zhi);
        for (u64 j = lo; j < hi; j++) nb += d->infinity_b[j] ? 0 : 1;
        const u64 part[3] = {hi - lo, nb, zhi - zlo};
        for (int k = 0; k < 3; k++) largest[k] = std::max(largest[k], part[k]);
    }
    // ONE fixed-base plan for all parts (mode 1 exchanges buckets, so the parts must cut their scalars alike; and a part just under the
    // 2^20-point threshold next to one just over it would otherwise pick different paths): mi_pk_load's rule (fixed_base_plan) for the LARGEST part
    // and the tightest device OF THE WHOLE GROUP (the budgets are all-gathered), handed to every part.  Knobs the caller set are kept.
    auto fail = [&](int32_t rc) { pk_sharded_release(g, spk); return rc; };
    std::vector<u64> budgets(nl, 0);
    for (int i = 0; i < nl; i++) {
        (void)hipSetDevice(g->rk[i].dev);
        size_t fr = 0, tot = 0, sharers = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
        for (const GroupRank &o : g->rk) sharers += o.dev == g->rk[i].dev ? 1 : 0;
        budgets[i] = fr / 3 / sharers;
    }
    u64 bmin = 0, bmax = 0, smin = 0, smax = 0;
    int32_t rc = group_min_max(g, budgets, &bmin, &bmax);
    if (rc != MI_OK) return fail(rc);
    const u32 automatic[3] = {0, 0, 0};
    const FixedBasePlan plan = fixed_base_plan(automatic, bmin, largest[KEY_AK], largest[KEY_B], largest[KEY_Z]);
    Carried loaded;
    for_each_local_rank(g, loaded, [&](int i) {   // uploads (and table builds) of the parts run side by side, one host thread per device
        ShardRange sr;
        wire_range_of(d->nb_wires, W, g->rank0 + i, share, sr.w_lo, sr.w_hi); range_of(N - 1, W, g->rank0 + i, sr.z_lo, sr.z_hi);
        return mi_pk_load_range(g->rk[i].ctx, device_points ? &descs[i] : d, &spk->part[i], device_points, &sr, &plan);
    });
    // every process reaches the agreement below even when a local part failed (a collective that only some ranks enter would hang)
    const int32_t first_bad = loaded.leave(g);
    // all parts on the same plan?  (a part whose tables could not be allocated after all fell back to the generic path by itself)
    std::vector<u64> sig(nl, 0);
    for (int i = 0; i < nl; i++) {
        mi_pk *p = spk->part[i];
        for (int k = 0; p && k < 3; k++) p->group[k].gen_c = p->group[k].c ? 0 : mi_msm_auto_c(largest[k]);
        sig[i] = p ? ((u64)1 << 32 | (u64)p->group[KEY_AK].c << 16 | (u64)p->group[KEY_B].c << 8 | (u64)p->group[KEY_Z].c) : 0;   // 0 = this part failed to load
    }
    rc = group_min_max(g, sig, &smin, &smax);
    if (first_bad != MI_OK) return fail(first_bad);
    if (rc != MI_OK) return fail(rc);
    if (smin == 0) { g->err = "pk: another rank of the group failed to load its part"; return fail(MI_EHIP); }
    spk->uniform = smin == smax;
    *out = spk;
    return MI_OK;
}

// One proof over the ranks of the group (groth16.Prove, mt.go:496).  Inputs either in host memory (host = true: W is the WHOLE wire
// vector, a process reads only the ranges of its local ranks; a, b, c are read by the process that holds rank 0) or already on the
// devices (W_dev[i] = the wire range of local rank i on its device; a, b, c on rank 0's device).  c == null on the lead: c = a o b,
// formed on the device (mi_groth16_prove).
// mode 0: per-rank partial sums (option i); mode 1: bucket reduce-scatter before the reduce (option ii).
// Phases: [local: checks, workspaces, uploads, wire MSMs, computeH + Z on the lead] AGREE [h slices over the transport] [local: the other
// ranks' Z MSMs; mode 1: bucket views] (mode 1: AGREE [bucket slices of A, B1, B2, K] [bucket slices of Z]) [local: collect] ALL-GATHER
// of every rank's status and five partial sums.
// abc_sl (may be null): per LOCAL rank device pointers to its rows of a, b, c (abc_sl[2] == null: c = a o b): computeH runs over the ranks
// (compute_h_sharded); so it does for host arrays when the group asks for it (mi_group_set_sharded_compute_h) and the shape allows.
struct ShardedProve {   // the arguments of one call, what follows from them, and the call's carried status
    mi_group *g; mi_pk_sharded *spk; bool host; const mi_fr *W_host; const mi_fr *const *W_dev; size_t n_wires;
    const mi_fr *a, *b, *c; size_t n_constraints; const mi_fr *r_m, *s_m; uint32_t mode; const mi_fr *const *const *abc_sl;
    bool lead_here = false, use_sh = false, defer = false;   // global rank 0 (it runs computeH and owns a, b, c) is here; computeH runs over the ranks; mode 1
    size_t N = 0, cb = 0;
    std::chrono::steady_clock::time_point t_begin;
    Carried st;
};
static const int PROVE_SLOTS[5] = {MSM_SLOT_A, MSM_SLOT_B1, MSM_SLOT_B2, MSM_SLOT_K, MSM_SLOT_Z}, PROVE_CURVES[5] = {1, 1, 2, 1, 1};   // the same order on every rank

// ---- local phase 1.  Nothing returns from here on without the group having agreed on it (a process that left alone would leave
//      the others waiting in the next exchange): failures are noted and carried to the agreement.
static void prove_check_and_reserve(ShardedProve &p) {
    mi_group *g = p.g; Carried &st = p.st;
    const bool use_sh = p.use_sh, lead_here = p.lead_here;
    if (!p.r_m || !p.s_m || p.mode > 1 || (p.host ? (!p.W_host && p.n_wires) : !p.W_dev)) st.note(MI_EINVAL, "prove: null argument or unknown mode");
    if (p.abc_sl && !use_sh) st.note(MI_EINVAL, "prove: row slices of a, b, c need computeH over the ranks: 2, 4, 8 or 16 ranks and N >= ranks^2");
    if (p.abc_sl && (!p.abc_sl[0] || !p.abc_sl[1])) st.note(MI_EINVAL, "prove: null slice arrays");
    if (!p.abc_sl && (lead_here || use_sh) && (!p.a || !p.b) && p.n_constraints)
        st.note(MI_EINVAL, use_sh ? "prove: with computeH over the ranks every process passes a and b" : "prove: the process that holds rank 0 must pass a and b");
    if (use_sh && p.n_constraints > p.N) st.note(MI_EINVAL, "prove: witness size does not match the proving key");
    if (p.n_wires != p.spk->nb_wires || (lead_here && p.n_constraints > p.N)) st.note(MI_EINVAL, "prove: witness size does not match the proving key");
    if (p.mode == 1 && !p.spk->uniform) st.note(MI_EINVAL, "group: mode 1 needs every part of the key to use the same MSM plan");
    // (mi_group_wire_range answers with the group's CURRENT share: a caller of the _dev entry points would cut W unlike the key's parts)
    if (lead_share_of(g) != p.spk->lead_share) st.note(MI_EINVAL, "group: the lead's wire share (mi_group_set_lead_share) changed since this key was loaded: reload the key");
    // workspaces, each on its own device: W slice (+ a, b, c on the lead) for host inputs; h (whole on the lead, a slice elsewhere)
    for (int i = 0; i < g->n_local() && st.ok(); i++) {
        (void)hipSetDevice(g->rk[i].dev);
        mi_ctx *ctx = g->rk[i].ctx;
        mi_pk *pk = p.spk->part[i];
        const bool lead = g->rank0 + i == 0;
        std::memset(&ctx->stats, 0, sizeof(ctx->stats));
        int32_t rc = MI_OK;
        if (p.host) rc = mi_reserve(ctx, ctx->ws[WS_PROVE_IN], pk->nb_wires * sizeof(mi_fr) + (lead && !use_sh ? 3 * p.cb : 0) + 128);
        if (rc == MI_OK && !use_sh) rc = mi_reserve(ctx, ctx->ws[WS_H], (lead ? p.N : pk->n_z_msm + 1) * sizeof(Fr));
        st.note(rc, mi_last_error(ctx));
    }
}
// Local rank i: its slice of W, its wire MSMs; the lead also a, b, c, computeH and its own Z MSM.  One host thread per rank:
// enqueueing the wire MSMs waits once for the count pass of their sorts (msm.hip, MI_MSM_EXACT_SIZE)
static int32_t prove_rank_local(const ShardedProve &p, int i) {
    mi_group *g = p.g;
    mi_ctx *ctx = g->rk[i].ctx; mi_pk *pk = p.spk->part[i];
    hipEvent_t *ev = ctx->ev;
    const bool lead = g->rank0 + i == 0, host = p.host;
    const size_t wb = pk->nb_wires * sizeof(mi_fr), cb = p.cb;
    const mi_fr *Wd = host ? (const mi_fr *)ctx->ws[WS_PROVE_IN].p : p.W_dev[i];
    if (!Wd && wb) MI_FAIL(ctx, MI_EINVAL, "prove: null wire slice");
    // host inputs: pageable copies on the context's copy stream (which carries nothing else), ordered by synchronising it on this
    // thread -- no event between two of them (prove.hip, pool.hip: a marker slows every copy behind it)
    const auto t_up = std::chrono::steady_clock::now();
    hipStream_t cps = nullptr;
    if (host) MI_TRY(mi_copy_stream(ctx, &cps));
    if (host && wb) {
        MI_CHECK_HIP(ctx, hipMemcpyAsync((void *)Wd, p.W_host + pk->wire_lo, wb, hipMemcpyHostToDevice, cps));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(cps));
    }
    MI_CHECK_HIP(ctx, hipEventRecord(ev[EV_W_READY], ctx->stream));
    MI_TRY(mi_prove_enqueue_wire_msms(ctx, pk, Wd, ev[EV_W_READY], p.defer));
    if (p.use_sh) {   // this rank's rows of a, b (, c) into the group's slice vectors; computeH itself is a collective and follows the agreement
        const mi_fr *const *const *abc_sl = p.abc_sl;
        const u32 log_m = pk->log_n - g->log_w();
        MI_CHECK_HIP(ctx, hipEventRecord(ev[EV_PROVE_BEGIN], ctx->stream));
        for (int which = 0; which < 3; which++) {
            const mi_fr *src = abc_sl ? (abc_sl[which] ? abc_sl[which][i] : nullptr) : (which == 0 ? p.a : which == 1 ? p.b : p.c);
            const bool given = abc_sl ? abc_sl[which] != nullptr : src != nullptr;
            if (which == H_C && !given) { MI_TRY(mi_reserve(ctx, g->rk[i].hv[H_C], sizeof(Fr) << log_m)); continue; }
            MI_TRY(load_h_slice(g, i, which, log_m, src, !abc_sl, p.n_constraints, abc_sl ? ctx->stream : cps));
        }
        if (!abc_sl) MI_CHECK_HIP(ctx, hipStreamSynchronize(cps));   // (grown buffers: hipFree inside mi_reserve has synchronised already)
        return compute_h_sharded_prepare(g, i, pk->log_n);   // the collective's own buffers too: a failure is agreed on below, before any rank enters it
    }
    if (!lead) return MI_OK;
    // lead: a, b, c arrive while the wire MSMs run; computeH; its own slice of h feeds its Z MSM straight away
    const mi_fr *da = p.a, *db = p.b, *dc = p.c;
    if (host) {
        char *base = (char *)ctx->ws[WS_PROVE_IN].p;
        da = (mi_fr *)(base + wb); db = (mi_fr *)(base + wb + cb); dc = p.c ? (mi_fr *)(base + wb + 2 * cb) : nullptr;
        if (cb) {
            MI_CHECK_HIP(ctx, hipMemcpyAsync((void *)da, p.a, cb, hipMemcpyHostToDevice, cps));
            MI_CHECK_HIP(ctx, hipMemcpyAsync((void *)db, p.b, cb, hipMemcpyHostToDevice, cps));
            if (p.c) MI_CHECK_HIP(ctx, hipMemcpyAsync((void *)dc, p.c, cb, hipMemcpyHostToDevice, cps));
            MI_CHECK_HIP(ctx, hipStreamSynchronize(cps));
        }
        ctx->stats.h2d_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_up).count();
    }
    MI_CHECK_HIP(ctx, hipEventRecord(ev[EV_PROVE_BEGIN], ctx->stream));
    Fr *h = (Fr *)ctx->ws[WS_H].p;
    MI_TRY(mi_compute_h_dev_impl(ctx, pk->log_n, da, db, dc, p.n_constraints, (mi_fr *)h));
    MI_CHECK_HIP(ctx, hipEventRecord(ev[EV_H_READY], ctx->stream));
    return mi_prove_enqueue_z_msm(ctx, pk, (const mi_fr *)(h + pk->z_lo), ev[EV_H_READY], p.defer);
}
// ---- h, first form: computeH over all ranks; every rank's h slice is born where its Z pairs live (front slot = the previous rank's
// last coefficient).  This and the two phases below return MI_OK or what ends the call: a transport failure, a failed agreement.
static int32_t prove_h_over_ranks(ShardedProve &p) {
    mi_group *g = p.g;
    const bool derive_c = p.abc_sl ? p.abc_sl[2] == nullptr : p.c == nullptr;
    const int32_t rc = compute_h_sharded(g, p.spk->log_n, derive_c);
    if (g->broken) return rc;
    p.st.note(rc, g->err);
    if (p.st.ok()) for_each_local_rank(g, p.st, [&](int i) -> int32_t {
        mi_ctx *ctx = g->rk[i].ctx;
        MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_H_READY], ctx->stream));
        const Fr *hz = (const Fr *)g->rk[i].hh.p + (g->rank0 + i == 0 ? 1 : 0);
        return mi_prove_enqueue_z_msm(ctx, p.spk->part[i], (const mi_fr *)hz, ctx->ev[EV_H_READY], p.defer);
    });
    return MI_OK;
}
// ---- h, second form: rank 0 hands every other rank its slice device to device, as one batch of the group's transport (grouped ncclSend /
// ncclRecv, same-process copies or the shared-memory rings) on the exchange streams; the events that order the Z MSMs behind it are recorded
// by each RECEIVER on its own stream (an event is recorded only on a stream of the device it was created on)
static int32_t prove_h_from_lead(ShardedProve &p) {
    mi_group *g = p.g;
    std::vector<Xfer> list;
    for (int j = 1; j < g->world; j++) {
        u64 zlo, zhi;
        range_of(p.N - 1, g->world, j, zlo, zhi);
        Xfer x{0, j, nullptr, nullptr, (size_t)(zhi - zlo) * sizeof(Fr)};
        if (g->local(0)) x.sp = (const char *)g->rk[0 - g->rank0].ctx->ws[WS_H].p + zlo * sizeof(Fr);
        if (g->local(j)) x.dp = g->rk[j - g->rank0].ctx->ws[WS_H].p;
        list.push_back(x);
    }
    if (p.lead_here) {
        (void)hipSetDevice(g->rk[0].dev);
        const hipError_t e = hipStreamWaitEvent(g->rk[0].xs, g->rk[0].ctx->ev[EV_H_READY], 0);
        if (e != hipSuccess) p.st.note(MI_EHIP, std::string("hipStreamWaitEvent (h ready): ") + hipGetErrorString(e));   // (still takes part in the batch)
    }
    MI_TRY(run_xfers(g, list));   // transport failure: the group is broken
    if (p.st.ok()) for_each_local_rank(g, p.st, [&](int i) -> int32_t {
        if (g->rank0 + i == 0) return MI_OK;
        GroupRank &k = g->rk[i];
        MI_CHECK_HIP(k.ctx, hipEventRecord(k.ev[E_H], k.xs));
        return mi_prove_enqueue_z_msm(k.ctx, p.spk->part[i], (const mi_fr *)k.ctx->ws[WS_H].p, k.ev[E_H], p.defer);
    });
    return MI_OK;
}
// ---- mode 1: the wire MSMs' slices go first (one batch), Z's -- the last to have its bucket sums -- second: their reduces then run under
// Z's accumulation.  No local failure point lies between the agreement and the end of the second batch that a rank does not carry
// THROUGH both batches.
static int32_t prove_bucket_exchange(ShardedProve &p) {
    mi_group *g = p.g;
    BucketExchange bx;
    std::vector<uint64_t> check;
    if (p.st.ok()) p.st.note(exchange_prepare(g, bx, PROVE_SLOTS, PROVE_CURVES, 5, check), g->err);
    MI_TRY(group_agree(g, p.st, "before the exchange of the bucket sums", check.data(), (uint32_t)check.size()));
    static const int batches[2][2] = {{0, 4}, {4, 1}};   // {first slot, count}
    for (const auto &b : batches) {
        const int32_t rc = exchange_run(g, bx, b[0], b[1]);
        if (g->broken) return rc;
        p.st.note(rc, g->err);
    }
    return MI_OK;
}
// ---- collect: this process's partial results of the five MSMs, then ONE all-gather of (status, five partial sums) per rank: every
// process ends with the same five sums, or every process returns an error.  Then the assembly of the proof and the call's statistics.
static int32_t prove_collect(ShardedProve &p, mi_proof_out *out, mi_stats *stats) {
    mi_group *g = p.g;
    ProofAssembler as;
    if (p.st.ok()) as.start(p.spk->part[0], p.r_m, p.s_m);
    struct Sums { G1X a, b1, k, z; G2X b2; };
    std::vector<Sums> mine((size_t)g->n_local()), all;
    for (int i = 0; i < g->n_local(); i++) {
        GroupRank &rk = g->rk[i];
        (void)hipSetDevice(rk.dev);
        std::memset((void *)&mine[i], 0, sizeof(Sums));
        if (!p.st.ok()) continue;
        mi_ctx *ctx = rk.ctx;
        int32_t rc = mi_msm_finish(ctx, MSM_SLOT_A, 1, &mine[i].a);
        if (rc == MI_OK) rc = mi_msm_finish(ctx, MSM_SLOT_B1, 1, &mine[i].b1);
        if (rc == MI_OK) rc = mi_msm_finish(ctx, MSM_SLOT_K, 1, &mine[i].k);
        if (rc == MI_OK) rc = mi_msm_finish(ctx, MSM_SLOT_B2, 2, &mine[i].b2);
        if (rc == MI_OK) rc = mi_msm_finish(ctx, MSM_SLOT_Z, 1, &mine[i].z);
        if (rc == MI_OK && (hipStreamSynchronize(ctx->stream) != hipSuccess || hipStreamSynchronize(rk.xs) != hipSuccess)) { mi_set_err(ctx, "prove: stream synchronisation failed"); rc = MI_EHIP; }
        p.st.note(rc, mi_last_error(ctx));
    }
    MI_TRY(group_gather(g, p.st, mine, "in its part of the proof", "", all));
    G1X sum_a = G1X::inf(), sum_b1 = G1X::inf(), sum_k = G1X::inf(), sum_z = G1X::inf();
    G2X sum_b2 = G2X::inf();
    for (const Sums &s : all) { xyzz_add(sum_a, s.a); xyzz_add(sum_b1, s.b1); xyzz_add(sum_k, s.k); xyzz_add(sum_z, s.z); xyzz_add(sum_b2, s.b2); }
    const auto t_gpu_done = std::chrono::steady_clock::now();
    as.have_a_b1(sum_a, sum_b1);
    as.finish(sum_k, sum_b2, sum_z, out);
    const auto t_end = std::chrono::steady_clock::now();
    (void)hipSetDevice(g->rk[0].dev);
    mi_ctx *c0 = g->rk[0].ctx;
    mi_stats &st = c0->stats;
    auto ms = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) { return std::chrono::duration<float, std::milli>(y - x).count(); };
    // (statistics are best effort: past the last all-gather nothing may fail on one rank alone)
    if ((p.lead_here || p.use_sh) && hipEventElapsedTime(&st.compute_h_ms, c0->ev[EV_PROVE_BEGIN], c0->ev[EV_H_READY]) != hipSuccess) { (void)hipGetLastError(); st.compute_h_ms = 0; }
    st.assemble_ms = ms(t_gpu_done, t_end);
    st.total_ms = ms(p.t_begin, t_end);
    if (stats) *stats = st;
    return MI_OK;
}
static int32_t prove_sharded(ShardedProve p, mi_proof_out *out, mi_stats *stats) {
    const MiRange range_fn("mi.group.prove");
    mi_group *g = p.g;
    if (!p.spk || !out) return MI_EINVAL;
    const int nl = g->n_local(), W = g->world;
    if ((nl != W && nl != 1) || (int)p.spk->part.size() != nl) G_FAIL(g, MI_EINVAL, "group: a process holds either all ranks or exactly one");
    p.t_begin = std::chrono::steady_clock::now();
    p.lead_here = g->rank0 == 0; p.defer = p.mode == 1;
    p.N = (size_t)1 << p.spk->log_n; p.cb = p.n_constraints * sizeof(mi_fr);
    p.use_sh = (p.abc_sl != nullptr || (p.host && g->sharded_h)) && sharded_h_possible(g, p.spk->log_n);
    prove_check_and_reserve(p);
    if (p.st.ok()) for_each_local_rank(g, p.st, [&](int i) { return prove_rank_local(p, i); });
    // (without computeH over the ranks n_constraints is the lead's alone)
    const uint64_t check[5] = {(uint64_t)p.n_wires, (uint64_t)p.mode, (uint64_t)p.spk->log_n, p.use_sh ? 1u : 0u, p.use_sh ? (uint64_t)p.n_constraints : 0u};
    int32_t rc = group_agree(g, p.st, "before computeH / the exchange of the h slices", check, 5);
    if (rc == MI_OK) rc = p.use_sh ? prove_h_over_ranks(p) : W > 1 ? prove_h_from_lead(p) : MI_OK;
    if (rc == MI_OK && p.defer) rc = prove_bucket_exchange(p);
    if (rc == MI_OK) rc = prove_collect(p, out, stats);
    if (rc != MI_OK) { const std::string keep = g->err; drain_slots(g, PROVE_SLOTS, PROVE_CURVES, 5); g->err = keep; }
    return rc;
}

extern "C" {

int32_t mi_pk_load_sharded(mi_group *g, const mi_pk_desc *d, mi_pk_sharded **out) {
    G_ENTER(g);
    return pk_load_sharded_impl(g, d, false, out);
}
int32_t mi_pk_load_sharded_dev(mi_group *g, const mi_pk_desc *slice_descs, mi_pk_sharded **out) {
    G_ENTER(g);
    return pk_load_sharded_impl(g, slice_descs, true, out);
}
int32_t mi_groth16_prove_sharded(mi_group *g, mi_pk_sharded *spk, const mi_fr *W, size_t n_wires, const mi_fr *a, const mi_fr *b, const mi_fr *c,
                                 size_t n_constraints, const mi_fr *r_m, const mi_fr *s_m, uint32_t mode, mi_proof_out *out, mi_stats *stats) {
    G_ENTER(g);
    return prove_sharded({g, spk, true, W, nullptr, n_wires, a, b, c, n_constraints, r_m, s_m, mode, nullptr}, out, stats);
}
int32_t mi_groth16_prove_sharded_slices_dev(mi_group *g, mi_pk_sharded *spk, const mi_fr *const *W_dev, size_t n_wires, const mi_fr *const *a_sl,
                                            const mi_fr *const *b_sl, const mi_fr *const *c_sl, size_t n_constraints, const mi_fr *r_m, const mi_fr *s_m,
                                            uint32_t mode, mi_proof_out *out, mi_stats *stats) {
    G_ENTER(g);
    const mi_fr *const *abc[3] = {a_sl, b_sl, c_sl};
    return prove_sharded({g, spk, false, nullptr, W_dev, n_wires, nullptr, nullptr, nullptr, n_constraints, r_m, s_m, mode, abc}, out, stats);
}
int32_t mi_groth16_prove_sharded_dev(mi_group *g, mi_pk_sharded *spk, const mi_fr *const *W_dev, size_t n_wires, const mi_fr *a_dev, const mi_fr *b_dev,
                                     const mi_fr *c_dev, size_t n_constraints, const mi_fr *r_m, const mi_fr *s_m, uint32_t mode, mi_proof_out *out,
                                     mi_stats *stats) {
    G_ENTER(g);
    return prove_sharded({g, spk, false, nullptr, W_dev, n_wires, a_dev, b_dev, c_dev, n_constraints, r_m, s_m, mode, nullptr}, out, stats);
}

}  // extern "C"
