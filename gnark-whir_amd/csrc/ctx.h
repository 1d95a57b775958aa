// Library-internal context shared by the HIP translation units (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <string>
#include <vector>
#include <cstdio>
#include "../../include/mi355x_groth16.h"
#include "../../include/mi355x_groth16_group.h"
#include "../../include/mi355x_whir_ingest.h"
#include "../../include/mi355x_groth16_debug.h"
#include "../../include/mi355x_groth16_setup.h"
#include "../../include/mi355x_groth16_r1cs.h"
#include "../../include/mi355x_groth16_keyfile.h"
#include "../../include/mi355x_groth16_phase2.h"
#include "../../include/mi355x_groth16_phase2_check.h"
#include "../../include/mi355x_groth16_phase1.h"
#include "../../include/mi355x_groth16_keyaudit.h"

struct DevBuf {             // growable device scratch owned by the ctx (no hipMalloc in the hot path
    void *p = nullptr;      // after warm-up: buffers only ever grow)
    size_t cap = 0;
};

// mi_ctx::ws[]: every workspace slot in use, its owner and the stream its work runs on ("main" = ctx->stream).  A new user takes a
// free number here; two phases that can be in flight together never share a slot.
enum {
    WS_H_B = 0,            // ntt.hip computeH: b's transform                                            main
    WS_H_C = 1,            // ntt.hip computeH: c's transform                                            main
    WS_HOST_IO0 = 2,       // host entry points of ntt.hip / msm.hip / group.hip: vector or points       main
    WS_HOST_IO1 = 3,       // the same: computeH's a, b, c / the MSM's scalars                           main
    WS_FB_SUMS = 4,        // fixed_base.hip: the XYZZ sums before their conversion                      main
    WS_FB_INV = 5,         // fixed_base.hip: running products of the batched inversion                  main
    WS_R1CS_A = 6,         // r1cs.hip: A W of an evaluation into workspace                              main
    WS_R1CS_B = 7,         // r1cs.hip: B W                                                              main
    WS_R1CS_C = 8,         // r1cs.hip: C W                                                              main
    WS_R1CS_PARTIAL = 9,   // r1cs.hip: partials of the long rows' pieces                                main
    WS_R1CS_CHECK = 10,    // r1cs.hip check: the counters, then one sum per long row                    main
    WS_R1CS_W = 11,        // r1cs.hip: W of the host entry point                                        main
    WS_SCAN = 12,          // setup.hip: block sums of the shared u32 scan (scan_u32.cuh)                main
    WS_VERIFY = 13,        // verify.hip: scalars, pairs, Miller values, flags and verdicts of a batch           main
    WS_H = 14,             // prove.hip / group.hip: h, computeH's result and the Z MSM's scalars        main, read by msm[MSM_SLOT_Z].stream
    WS_VERIFY_BYTES = 15,  // verify_bytes.hip: proof bytes, lists, decoded points, flags, hashes of a batch           main
    WS_PROVE_IN = 16,      // prove.hip / group.hip: W (+ a, b, c) of a prove over host inputs           filled on copy_stream
    WS_B_WIRES = 17,       // prove.hip: W gathered to the wires that own a pk.G1.B point                msm[MSM_SLOT_B1].stream
    WS_VERIFY_LOCATE = 18, // verify_locate.hip: the per-proof values, their trees and a round's nodes   main
    WS_POK_VALUES = 19,    // prove.hip ProveKnowledge: the committed values                             msm[MSM_SLOT_POK].stream
    WS_FB_TABLE = 20,      // fixed_base.hip: the window table of the base                               main
    WS_FB_SCALARS = 21,    // fixed_base.hip host entry point: the scalars                               main
    WS_FB_OUT = 22,        // fixed_base.hip host entry point: the points                                main
    WS_RPRIME = 23,        // msm.hip device entry point: the points in the R' packed form               main
    WS_COUNT = 24
};
// mi_ctx::ev[]: every event of the context in use, what it marks and the stream that records it ("main" = ctx->stream).
enum {
    EV_T0 = 0,             // timing pair of the NTT, utility and MSM entry points: before the work (the MSM's wait event)     main
    EV_T1 = 1,             // the same: after it                                                             main, msm[MSM_SLOT_A].stream
    EV_W_READY = 2,        // group.hip: this rank's slice of W is on the device -- what its wire MSMs wait for                  main
    EV_H_READY = 3,        // prove: h is ready -- what the Z MSM and the held wire accumulations wait for; compute_h_ms ends   main
    EV_PROVE_BEGIN = 11,   // prove.hip: the head of the proof, and "W is ready" where W is a device input; group.hip: before the
                           // lead's computeH / the slices of computeH over the ranks.  compute_h_ms begins                    main
    EV_R1CS_BEGIN = 12,    // r1cs.hip: before the launches of the last R1CS evaluation                                         main
    EV_R1CS_END = 13,      // r1cs.hip: after them                                                                              main
    EV_COUNT = 24          // the others are free
};

// mi_ctx::msm[]: who runs on which slot.  The values are fixed: the stream plan (msm.hip: K borrows B1's stream, Z has its own
// priority) and the per-slot statistics depend on them.
enum {
    MSM_SLOT_A = 0,        // prove: pk.G1.A over W; its sort serves K.  Also the one slot of the plain MSM entry points
    MSM_SLOT_B1 = 1,       // prove: pk.G1.B over the gathered wires; its sort serves B2
    MSM_SLOT_B2 = 2,       // prove: pk.G2.B (G2)
    MSM_SLOT_K = 3,        // prove: pk.G1.K over W, on B1's stream
    MSM_SLOT_Z = 4,        // prove: pk.G1.Z over h; the one slot whose sort may take its count from computeH's last launch (mi_ctx::zhook)
    MSM_SLOT_POK = 5,      // pool.hip / prove.hip: ProveKnowledge of a BSB22 commitment, beside a proof's five
    MI_MSM_SLOTS = 6
};
#define MI_ZHOOK_SLOT MSM_SLOT_Z
// MsmSlot::ev[]: all recorded on the slot's stream by msm.hip
enum {
    MSM_EV_SORT_DONE = 0,  // the sort stage is enqueued: what an MSM that borrows this slot's sort waits for
    MSM_EV_L1_BEGIN = 1,   // before the level-1 accumulate launch (timed slots)
    MSM_EV_L1_END = 2,     // after it
    MSM_EV_JOB_BEGIN = 3,  // before the whole job
    MSM_EV_JOB_END = 4,    // after it (the result is in pinned host memory)
    MSM_EV_BUCKETS = 5,    // the bucket sums are ready (deferred reduce, group.hip's exchange)
    MSM_EV_MAX_LANDED = 6, // the fullest bucket's size has landed in host memory (exact level count, msm.hip)
    MSM_EV_COUNT = 7
};
enum { B_DIGITS, B_H, B_S, B_SORTED, B_LEVELS, B_PART0, B_PART1, B_BUCKET, B_SCAN, B_WIN, B_PVAL, B_C1, B_CHUNKS, B_ITEMTAB, B_MAX, B_BA_NODES, B_BA_PREFIX, B_BA_TOT, B_COUNT_ };   // MsmSlot::buf[]: the slot's device workspaces (msm.hip)
// MsmSlot::host_wsum, pinned host memory: the window sums the last sum tree (or a copy) stores, then words that kernels of the slot's SORT store (k_scan_final)
struct MsmHostWords {
    unsigned char wsum[128][256];             // <= 128 XYZZ window sums, packed from byte 0: 128 B each (G1) or 256 B (G2)
    uint32_t entries, pad0_[3];               // sorted entries = non-zero digits (the key scan's total)
    uint32_t exact_total, pad1_[3];           // the count pass's total, fetched before the workspaces are sized (MI_MSM_EXACT_SIZE)
    uint32_t max_bucket, pad2_[7];            // entries of the fullest bucket; lands with ev[MSM_EV_MAX_LANDED]
};
static_assert(offsetof(MsmHostWords, entries) == sizeof(MsmHostWords::wsum) && offsetof(MsmHostWords, exact_total) == offsetof(MsmHostWords, entries) + 16 &&
              offsetof(MsmHostWords, max_bucket) == offsetof(MsmHostWords, entries) + 32 && sizeof(MsmHostWords) == 128 * 256 + 64, "the words lie where the kernels store them");
struct MsmSlot {            // one in-flight MSM (msm.hip): own stream, events, workspaces, pinned result
    hipStream_t stream = nullptr;
    hipEvent_t ev[MSM_EV_COUNT]{};
    bool max_pending = false;       // this slot's sort has a "largest bucket" word on its way to the host (ev[MSM_EV_MAX_LANDED])
    uint32_t max_key_count = 0;     // entries of the fullest bucket of this slot's sort, once fetched
    DevBuf buf[B_COUNT_];
    MsmHostWords *host_wsum = nullptr;
    uint32_t n = 0, c = 0, G = 0;
    uint64_t entries_cap = 0;   // entries the sort of this slot is sized for: windows * n, or the counted number (MI_MSM_EXACT_SIZE)
    uint64_t stat_pairs = 0;    // (point, scalar) pairs this MSM really has (A and K run over per-wire expanded arrays with holes)
    uint32_t nwin_keys = 0;     // windows in the key space: ceil(256/c) for the generic MSM, 1 for the fixed-base one
    uint32_t nwin_digits = 0;   // digits per scalar = ceil(256/c)
    bool active = false, timed = false;
    bool deferred = false;      // accumulate stage done up to the bucket sums, reduce not yet enqueued (MI_MSM_DEFER_REDUCE)
    uint32_t tail_seg = 0;      // buckets per bucket-reduce thread
    const uint32_t *entries_src = nullptr;   // HOST word holding the number of sorted entries (stats): in the pinned memory of the slot that owns the sort
    // Set by the caller before mi_msm_enqueue, consumed by it: called on the enqueueing thread right before the bucket accumulation is
    // enqueued (after the sort); blocks until the event it returns HAS BEEN RECORDED and the slot's stream then waits for that event
    // (null result = no wait).  prove.hip holds the wire MSMs' accumulations back until computeH is done this way.
    const std::function<hipEvent_t()> *accum_gate = nullptr;
};

struct mi_ctx {
    int dev = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t copy_stream = nullptr;   // host-pointer inputs of mi_groth16_prove: pageable copies run on a stream that carries nothing else
                                         // (no event between two of them: a marker takes the copies behind it off the runtime's fast path)
    std::string err;
    std::mutex err_m;          // a prove enqueues its MSM groups from helper threads (prove.hip): failures there report through mi_set_err
    mi_stats stats{};
    mi_setup_stats setup_stats{};   // last mi_groth16_setup[_exponents] call (setup.hip)
    mi_phase2_stats phase2_stats{};   // last mi_phase2_init call (phase2.hip)
    mi_srs_check_stats srs_check_stats{}, phase2_verify_stats{};   // last mi_srs_check_powers / mi_phase2_verify_adopt call (phase2_check.hip)
    mi_key_audit_stats key_audit_stats{};   // last mi_key_audit call (keyaudit.hip)
    mi_key_audit_sums key_audit_sums{};     // and the two sides of its relations (mi_debug_key_audit_sums)
    mi_phase1_stats phase1_stats{};   // last contribution of a phase-1 state / mi_debug_scale_powers_dev (phase1.hip)
    uint32_t scale_powers_window = 5, scale_powers_chunk = 0;   // knobs "scale_powers_window" (0 = the bit-by-bit yardstick, 2..5) and "scale_powers_chunk" (0 = the default)
    mi_keyfile_stats keyfile_stats{};   // last mi_pk_load_stream / mi_pk_write_dev call (keyfile.hip)
    mi_r1cs_stats r1cs_stats{};     // last evaluation of a resident R1CS on this context (r1cs.hip); eval_ms is read from ev[EV_R1CS_BEGIN], ev[EV_R1CS_END] on request
    bool r1cs_timed = false;
    hipEvent_t ev[EV_COUNT]{};
    // scratch
    alignas(16) unsigned char ntt_state[384];  // NttState (ntt.hip): root tables + plan knobs
    alignas(16) unsigned char msm_knobs[128];   // MsmKnobs (msm.hip)
    DevBuf ws[WS_COUNT];
    MsmSlot msm[MI_MSM_SLOTS];          // MSM / prove workspaces, see msm.hip / prove.hip
    int cu_count = 256;
    int prio_scheme = 0;      // MI_PRIO_*: how the context's streams rank (api.hip, msm.hip)
    uint32_t fixed_knob[3] = {0, 0, 0};  // prove's fixed-base tables for A+K / B / Z: 0 = automatic, 1 = never, 17..22 = forced (prove.hip)
    // The Z MSM's digit count riding in computeH's LAST launch ("the count pass of Z could ride in computeH's last store"):
    // prove.hip arms it right before that launch (mi_msm_z_count_arm: the sort's shape and its count matrix C1), ntt.hip's fused last
    // kernel counts every h coefficient it stores -- its contiguous tile IS a slice (or two) of the sort -- and sets `done`; the Z sort
    // (msm2_sort_enqueue) then skips its own count pass: h is read once less.  Disarmed again as soon as the launch is enqueued.
    // Behind the knob "z_count_fused" (on by default: throughput equal, a single proof slightly shorter).
    // (only slot MSM_SLOT_Z -- prove's Z MSM -- ever looks at it, and the thread that arms it is the one that enqueues that slot)
    std::atomic<uint64_t> generic_sorts_two_pass{0}, generic_sorts_one_pass{0};   // generic MSM sorts by kind (msm.hip msm_sort_enqueue)
    std::atomic<uint64_t> dense_item_sorts{0};   // accumulations whose item size the dense-sort rule chose (msm.hip; helper threads enqueue too)
    uint64_t z_count_fused_launches = 0;   // computeH last launches that carried the count (mi_debug_get_counter: the tests' proof that the path ran)
    struct ZCountHook { bool armed = false, done = false; int slot = -1; uint32_t n = 0, c = 0; alignas(8) unsigned char shape[64]; uint32_t *C1 = nullptr; const void *h = nullptr; /* the vector whose digits were counted */ } zhook;
    uint32_t locate_round_nodes = 0;     // mi_groth16_verify_locate's node budget per round: 0 = MI_LOCATE_ROUND_NODES (mi_debug_set_locate_round_nodes)
    uint32_t verify_ksum = 1;            // knob "verify_ksum": 1 = the per-proof bodies stage a batch through the key's window table (ksum.hip), 0 = one MSM per proof
    uint32_t verify_ksum_min_batch = 8;  // knob "verify_ksum_min_batch": the proofs from which they do (MI_VERIFY_KSUM_MIN_BATCH, verify_internal.h: not faster at n = 1)
    uint64_t verify_ksum_batches = 0, verify_ksum_launches = 0;   // batches staged that way and the kernel launches of their stages (mi_debug_get_counter)
    uint32_t hold_accum = 0;             // prove: 1 = the wire MSMs' bucket accumulations wait for computeH (mi_debug_set_prove_schedule; measured: no gain)
};

static_assert(sizeof(mi_ctx::ws) == WS_COUNT * sizeof(DevBuf) && WS_RPRIME == WS_COUNT - 1, "WS_* names every slot of mi_ctx::ws up to its end");
static_assert(EV_R1CS_END < EV_COUNT && sizeof(mi_ctx::ev) == EV_COUNT * sizeof(hipEvent_t), "EV_* index mi_ctx::ev");
static_assert(MSM_SLOT_POK == MI_MSM_SLOTS - 1 && sizeof(mi_ctx::msm) == MI_MSM_SLOTS * sizeof(MsmSlot) && MSM_EV_MAX_LANDED == MSM_EV_COUNT - 1 &&
              sizeof(MsmSlot::buf) == B_COUNT_ * sizeof(DevBuf), "MSM_SLOT_* name every slot of mi_ctx::msm, MSM_EV_* every event of a slot, B_* every workspace");

// Fault injection for the error-path tests (mi_debug_inject_hip_failure, api.hip): the n-th MI_CHECK_HIP from now reports
// hipErrorUnknown INSTEAD of running its call.  Disabled (<= 0) it costs one relaxed atomic load per checked call.
#include <atomic>
extern std::atomic<int> mi_fault_countdown;
static inline bool mi_fault_hit() {
    if (mi_fault_countdown.load(std::memory_order_relaxed) <= 0) return false;
    return mi_fault_countdown.fetch_sub(1, std::memory_order_relaxed) == 1;
}
static inline void mi_set_err(struct mi_ctx *ctx, const std::string &msg);
#define MI_CHECK_HIP(ctx, call)                                                                       \
    do {                                                                                              \
        hipError_t e__ = mi_fault_hit() ? hipErrorUnknown : (call);                                   \
        if (e__ != hipSuccess) {                                                                      \
            /* a failed allocation also leaves itself as the thread's last error: clear it, or the next   \
               launch check (hipGetLastError) reports this out-of-memory as its own failure */            \
            if (e__ == hipErrorOutOfMemory) (void)hipGetLastError();                                  \
            mi_set_err((ctx), std::string(#call) + ": " + hipGetErrorString(e__));                    \
            return e__ == hipErrorOutOfMemory ? MI_ENOMEM : MI_EHIP;                                  \
        }                                                                                             \
    } while (0)
#define MI_FAIL(ctx, code, msg)                                                                       \
    do {                                                                                              \
        mi_set_err((ctx), (msg));                                                                     \
        return (code);                                                                                \
    } while (0)
#define MI_TRY(expr)                                                                                  \
    do {                                                                                              \
        int32_t rc__ = (expr);                                                                        \
        if (rc__ != MI_OK) return rc__;                                                               \
    } while (0)

// A helper thread that works on a context beside the thread that owns the call (the prover pool's ProveKnowledge enqueue, pool.hip)
// records its failures in a string of its own: set for the duration of its work, it replaces ctx->err for THIS thread, so the two
// threads never write one std::string and each failure reaches the job with the message of the thread that met it.
// roctx ranges around the host-side phases of a call (mi_debug_set_trace_ranges; off by default: one relaxed load per site).  rocprofv3
// --marker-trace shows them beside the kernel trace.  api.hip loads the roctx library on first use; nothing links against it.
extern std::atomic<int> mi_ranges_on;
void mi_range_push(const char *name);
void mi_range_pop();
struct MiRange {
    bool on;
    explicit MiRange(const char *name) : on(mi_ranges_on.load(std::memory_order_relaxed) != 0) { if (on) mi_range_push(name); }
    ~MiRange() { if (on) mi_range_pop(); }
    MiRange(const MiRange &) = delete;
    MiRange &operator=(const MiRange &) = delete;
};
extern thread_local std::string *mi_err_sink;
static inline void mi_set_err(struct mi_ctx *ctx, const std::string &msg) {
    if (mi_err_sink) { *mi_err_sink = msg; return; }
    std::lock_guard<std::mutex> lk(ctx->err_m);
    ctx->err = msg;
}

// grow-only scratch
static inline int32_t mi_reserve(mi_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return MI_OK;
    if (b.p) { MI_CHECK_HIP(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    size_t want = bytes + bytes / 8 + 256;
    MI_CHECK_HIP(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return MI_OK;
}

// the same for scratch a faster path would like but the slower one does without: false (and no error) when the memory is not there
static inline bool mi_try_reserve(DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return true;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&b.p, want) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return false; }
    b.cap = want;
    return true;
}

// the host's steady clock in milliseconds
static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static inline unsigned mi_blocks_of(uint64_t n, uint32_t per) { return (unsigned)((n + per - 1) / per); }   // workgroups of `per` items over n

// ctx->copy_stream, created on first use (api.hip)
int32_t mi_copy_stream(mi_ctx *ctx, hipStream_t *out);
// internal entry points implemented across translation units
int32_t mi_ntt_dev_impl(mi_ctx *ctx, mi_fr *inout_dev, uint32_t log_n, uint32_t flags);
int32_t mi_compute_h_dev_impl(mi_ctx *ctx, uint32_t log_n, const mi_fr *a, const mi_fr *b, const mi_fr *c,
                              size_t n_constraints, mi_fr *h_out);
// computeH one input vector at a time (ntt.hip): part 0 = a, 1 = b, 2 = c (src = that vector), 3 = the rest (src unused)
// part 2 with src2 != null: c is not given; it is formed as src o src2 (the original a and b) on the way into its transform
int32_t mi_compute_h_part(mi_ctx *ctx, uint32_t log_n, int part, const mi_fr *src, size_t n_constraints, mi_fr *h_out, const mi_fr *src2 = nullptr);
void mi_ntt_state_init(mi_ctx *ctx);
size_t mi_ntt_table_bytes(mi_ctx *ctx);
void mi_ntt_state_free(mi_ctx *ctx);
bool mi_ntt_set_knob(mi_ctx *ctx, const char *name, int64_t value);   // the NTT's share of mi_debug_set_knob: true = name known and value accepted
void mi_ntt_state_trim(mi_ctx *ctx);   // frees every table and marks them unbuilt (mi_ctx_trim)
int32_t mi_msm_state_init(mi_ctx *ctx);   // MI_OK or the first failing HIP call; partial state is freed by mi_msm_state_free
// Stream priority schemes (3 hardware levels; comment in msm.hip).  A context on its own ranks computeH high, the wire MSMs
// normal and Z low.  The contexts of a prover pool are staggered on top of that: the first runs nearly as if alone, the
// others fill what it leaves (28.2-28.4 vs 27.4 proofs/s with three in flight; two staggered contexts reach what three
// equal ones did).
enum { MI_PRIO_SOLO = 0,          // computeH high, A/B1/B2/K normal, Z low
       MI_PRIO_POOL_FIRST = 1,    // computeH high, A/B1/B2/K high,   Z normal
       MI_PRIO_POOL_SECOND = 2,   // computeH normal, A/B1/B2/K normal, Z low
       MI_PRIO_POOL_REST = 3 };   // everything low
void mi_msm_state_free(mi_ctx *ctx);
// Asynchronous MSM on slot `slot` (curve 1 = G1, 2 = G2; device pointers).  sort_slot < 0: sort the scalars
// here; otherwise reuse the sort already enqueued on that slot (same scalars, other bases).  wait_ev (may be
// null) orders the slot's stream after the producer of its inputs.  mi_msm_finish blocks on the slot and
// returns the XYZZ result on the host.
// precomp_c != 0: pts_dev holds the fixed-base window copies [ceil(256/c)][n] built by mi_msm_precompute (msm2_core.cuh).
int32_t mi_msm_enqueue(mi_ctx *ctx, int slot, int sort_slot, int curve, const void *pts_dev, const void *scalars_dev, size_t n,
                       uint32_t flags, hipEvent_t wait_ev, bool timed, uint32_t precomp_c = 0, size_t stat_pairs = 0,
                       uint32_t generic_c = 0 /* window bits of the generic path when the parts of a sharded MSM must agree (0 = from n) */);
// pre[w][i] = 2^(c*w) * base[i] for w < ceil(256/c) (affine), on ctx->stream.  pre must hold ceil(256/c) * n points.
int32_t mi_msm_precompute(mi_ctx *ctx, int curve, const void *base_dev, void *pre_dev, size_t n, uint32_t c);
int32_t mi_msm_finish(mi_ctx *ctx, int slot, int curve, void *out_xyzz_host);
// arms ctx->zhook for the fixed-base MSM that `slot` is about to run over n scalars with c-bit windows (no-op when the knob is off or the
// shape does not fit: the sort then counts by itself, as always)
int32_t mi_msm_z_count_arm(mi_ctx *ctx, int slot, size_t n, uint32_t c);
// Internal flag of mi_msm_enqueue (next to MI_MSM_SCALARS_CANONICAL): stop at the bucket sums.  mi_msm_bucket_view then
// exposes them, mi_msm_reduce_enqueue runs the rest (bucket reduce, window sums, copy to the host) and mi_msm_finish collects.
#define MI_MSM_DEFER_REDUCE 0x100u
// Internal flag: size the entry-indexed workspaces by the COUNTED number of non-zero digits (one synchronisation of the slot's
// stream after the count pass) instead of windows * n.  For scalars that are available when the MSM is enqueued (wire values).
#define MI_MSM_EXACT_SIZE 0x200u
// Internal flag: the points are in the R' = 2^261 packed form (msm_curve_ops.h to_rprime): G1 level 1 runs the 9 x 29-bit kernel.
#define MI_MSM_PTS_RPRIME 0x400u
struct MsmBucketView {
    void *bucket = nullptr;     // XYZZ[nkeys] on the slot's device; null for an empty MSM
    size_t nkeys = 0, xyzz_bytes = 0;
    uint32_t seg = 0, c = 0, nwin = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ready = nullptr; // recorded on `stream` after the last accumulate level
};
int32_t mi_msm_bucket_view(mi_ctx *ctx, int slot, int curve, MsmBucketView *v);
int32_t mi_msm_reduce_enqueue(mi_ctx *ctx, int slot, int curve);
bool mi_msm_limb29_enabled(mi_ctx *ctx);   // the G1 level-1 kernel in 9 x 29-bit limbs is in use (mi_debug_set_msm_limb29)
uint32_t mi_msm_auto_c(size_t n);   // the generic path's window bits for n pairs
const struct MsmCurveOps &mi_msm_ops(int curve);

