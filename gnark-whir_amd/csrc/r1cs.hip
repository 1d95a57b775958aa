// The device-resident R1CS (include/mi355x_groth16_r1cs.h): a = A W, b = B W, c = C W and the constraint check (A W)(B W) = C W.
//
// A row-wise sparse product over Fr: per entry an 8-byte (wire, coefficient) record and a 32-byte gather of W[wire]; at N = 2^23 W is
// 268 MB, far beyond an XCD's L2, so the gathers are served by the Infinity Cache and HBM and what the kernel can do about them is to
// keep many in flight (one row per lane, 64 independent rows per wave) and to fetch nothing it does not need:
//   load   on the host, once per circuit: the checks Setup makes of the same descriptor (mi_r1cs_validate, shared with setup.hip), the
//          coefficient table classified by value -- Montgomery 0, 1, -1, anything else -- with the class carried in the two spare top
//          bits of the entry's wire word (wires are below 2^27), so that an entry with coefficient +-1 adds or subtracts W[wire] without
//          a multiplication and without touching the table, and one with coefficient 0 is skipped: those are the bulk of a real gnark
//          table; and the row-length plan below
//   sum    the split sum of sparse_fr.cuh, by row: row lengths are as skewed as Setup's column lengths -- most rows hold one to four
//          entries, a few linear combinations thousands.  Planned on the host at load time (sparse_cut), not per call: short rows
//          by k_rows_short, the pieces of the long ones by k_row_pieces, their partials by k_row_combine.
// The matrices one call asks for (A and B on the prove path) share each launch (blockIdx.y picks the matrix): three launches per call
// on the context's stream.  The partials live in context workspace (mi_reserve: grow-only, freed by mi_ctx_trim); nothing is allocated
// in steady state.  The handle is read-only after load and shared by every context of its device.
#include "prove_internal.h"
#include "r1cs_internal.h"
#include "sparse_fr.cuh"
#include <algorithm>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

namespace {

constexpr u32 CLS_SHIFT = 30, COL_MASK = (1u << CLS_SHIFT) - 1;   // MI_MSM_MAX_PAIRS = 2^27 wires at most: bits 30, 31 are spare
enum : u32 { CLS_ANY = 0, CLS_ONE = 1, CLS_MINUS_ONE = 2, CLS_ZERO = 3 };
static_assert(MI_MSM_MAX_PAIRS <= (1ull << CLS_SHIFT), "the class bits need the top of the wire word");

struct MatArg {
    const u32 *row_off;
    const uint2 *entries;
    const SparseLong *long_rows;
    const uint2 *pieces;
    Fr *out;        // n_constraints rows; the check: one value per LONG row, in long_rows' order
    Fr *partial;    // one per piece
    u32 n_long, n_pieces;
};
struct EvalArgs { MatArg m[3]; };

// the term of an entry (wire | class << 30, coefficient): nothing, +-W[wire] without a product, or coeffs[coefficient] * W[wire]
struct RowTerm {
    const Fr *W, *coeffs;
    MI_D void operator()(Fr &acc, const uint2 en) const {
        const u32 cls = en.x >> CLS_SHIFT;
        if (cls == CLS_ZERO) return;
        const Fr w = ld_fr(W + (en.x & COL_MASK));
        if (cls == CLS_ONE) acc = acc + w;
        else if (cls == CLS_MINUS_ONE) acc = acc - w;
        else acc = acc + ld_fr(coeffs + en.y) * w;
    }
};

// the wrappers of sparse_fr.cuh's bodies; blockIdx.y = the matrix.  One lane per row, 64 rows in a wave:
__global__ void __launch_bounds__(256) k_rows_short(EvalArgs args, u64 nc, RowTerm term) {
    const u64 row = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nc) return;
    const MatArg &m = args.m[blockIdx.y];
    const u32 lo = m.row_off[row], len = m.row_off[row + 1] - lo;
    if (len > SPARSE_SHORT) return;   // k_row_combine writes it
    st_fr(m.out + row, sparse_sum_short(m.entries, lo, len, term));
}
__global__ void __launch_bounds__(256) k_row_pieces(EvalArgs args, RowTerm term) {
    const MatArg &m = args.m[blockIdx.y];
    sparse_sum_pieces(m.partial, m.pieces, m.n_pieces, m.entries, term);
}
// compact (the check): a long row's sum goes to out[its place among the long rows], not to out[row]
__global__ void __launch_bounds__(256) k_row_combine(EvalArgs args, bool compact) {
    const MatArg &m = args.m[blockIdx.y];
    sparse_combine(m.out, m.long_rows, m.n_long, m.partial, compact);
}
// (M W)[row] inside the check: a short row is summed here, a long one was summed by the two kernels above into out[its index]
MI_D Fr row_value(const MatArg &m, u32 row, const RowTerm &term) {
    const u32 lo = m.row_off[row], len = m.row_off[row + 1] - lo;
    if (len <= SPARSE_SHORT) return sparse_sum_short(m.entries, lo, len, term);
    u32 a = 0, b = m.n_long;   // long_rows is ascending by row and holds this one
    while (b - a > 1) {
        const u32 mid = a + (b - a) / 2;
        if (m.long_rows[mid].index <= row) a = mid; else b = mid;
    }
    return ld_fr(m.out + a);
}
// ctr[0] = rows with (A W)(B W) != C W, ctr[1] = the lowest of them: a wave counts its rows with a ballot, one lane adds
__global__ void __launch_bounds__(256) k_check(EvalArgs args, u64 nc, RowTerm term, unsigned long long *ctr) {
    const u64 row = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (row < nc) {
        const Fr a = row_value(args.m[0], (u32)row, term), b = row_value(args.m[1], (u32)row, term), c = row_value(args.m[2], (u32)row, term);
        bad = !(a * b == c);
    }
    const u64 mask = __ballot(bad);
    if (mask && (threadIdx.x & 63) == (u32)(__ffsll((long long)mask) - 1)) {   // the lowest bad lane holds the wave's lowest bad row
        atomicAdd(&ctr[0], (unsigned long long)__popcll(mask));
        atomicMin(&ctr[1], (unsigned long long)row);
    }
}

// fn(t, lo, hi) over [0, n) on a few host threads when n is large
template <class Fn>
void parallel_ranges(u64 n, Fn fn) {
    const unsigned T = n > (1u << 20) ? 8 : 1;
    if (T == 1) { fn(0u, (u64)0, n); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; t++) th.emplace_back(fn, t, n * t / T, n * (t + 1) / T);
    for (auto &x : th) x.join();
}

int32_t check_matrix(mi_ctx *ctx, const std::string &who, const char *name, const mi_r1cs_matrix &m, const mi_r1cs_desc *d, R1csShape &sh, int k) {
    const std::string nm(name);
    if (!m.row_ptr) MI_FAIL(ctx, MI_EINVAL, who + ": " + nm + ".row_ptr is null");
    if (m.row_ptr[0] != 0) MI_FAIL(ctx, MI_EINVAL, who + ": " + nm + ".row_ptr[0] is not 0");
    const u64 n = d->n_constraints;
    for (u64 i = 0; i < n; i++)
        if (m.row_ptr[i + 1] < m.row_ptr[i]) MI_FAIL(ctx, MI_EINVAL, who + ": " + nm + ".row_ptr decreases at row " + std::to_string(i));
    const u64 nnz = m.row_ptr[n];
    if (nnz >> 32) MI_FAIL(ctx, MI_EINVAL, who + ": " + nm + ".row_ptr[n_constraints]: 2^32 entries or more");
    if (nnz && (!m.col || !m.coeff)) MI_FAIL(ctx, MI_EINVAL, who + ": " + nm + ".col / " + nm + ".coeff is null");
    // every index, on a few threads: the device never sees an index out of range
    std::vector<u64> bad_col(8, ~0ull), bad_coeff(8, ~0ull);
    parallel_ranges(nnz, [&](unsigned t, u64 lo, u64 hi) {
        for (u64 e = lo; e < hi; e++) {
            if (m.col[e] >= d->nb_wires && bad_col[t] == ~0ull) bad_col[t] = e;
            if (m.coeff[e] >= d->n_coeffs && bad_coeff[t] == ~0ull) bad_coeff[t] = e;
        }
    });
    for (unsigned t = 0; t < 8; t++) {
        if (bad_col[t] != ~0ull) MI_FAIL(ctx, MI_EINVAL, who + ": " + nm + ".col[" + std::to_string(bad_col[t]) + "] is not below nb_wires");
        if (bad_coeff[t] != ~0ull) MI_FAIL(ctx, MI_EINVAL, who + ": " + nm + ".coeff[" + std::to_string(bad_coeff[t]) + "] is not below n_coeffs");
    }
    sh.nnz[k] = (u32)nnz;
    sh.row_ptr[k].resize(n + 1);
    for (u64 i = 0; i <= n; i++) sh.row_ptr[k][i] = (u32)m.row_ptr[i];
    return MI_OK;
}

void free_handle(mi_r1cs *r) {
    if (!r) return;
    if (r->coeffs) (void)hipFree(r->coeffs);
    for (auto &m : r->m)
        for (void *p : {(void *)m.row_off, (void *)m.entries, (void *)m.long_rows, (void *)m.pieces}) if (p) (void)hipFree(p);
    delete r;
}

int32_t to_device(mi_ctx *ctx, mi_r1cs *r, void **dst, const void *src, size_t bytes) {
    MI_CHECK_HIP(ctx, hipMalloc(dst, bytes ? bytes : 64));
    r->bytes += bytes ? bytes : 64;
    if (bytes) MI_CHECK_HIP(ctx, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return MI_OK;
}

int32_t usable(mi_ctx *ctx, const mi_r1cs *r, const char *who) {
    if (!r) MI_FAIL(ctx, MI_EINVAL, std::string(who) + ": r1cs is null");
    if (r->dev != ctx->dev) MI_FAIL(ctx, MI_EINVAL, std::string(who) + ": the r1cs was loaded on another device");
    return MI_OK;
}

// the launches of one evaluation on ctx->stream; outs[k] for the matrices in `which`.  compact: the long rows' sums go to outs[k][index
// of the long row] and the short rows are left to the caller's kernel (the check)
int32_t enqueue_eval(mi_ctx *ctx, const mi_r1cs *r, const Fr *W, u32 which, Fr *const outs[3], bool compact) {
    hipStream_t st = ctx->stream;
    EvalArgs args{};
    u32 nm = 0;
    u64 n_pieces = 0, n_long = 0, entries = 0;
    for (int k = 0; k < 3; k++) if (which & (1u << k)) { n_pieces += r->m[k].n_pieces; n_long += r->m[k].n_long; entries += r->m[k].nnz; }
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_R1CS_PARTIAL], (n_pieces + 1) * sizeof(Fr)));
    Fr *partial = (Fr *)ctx->ws[WS_R1CS_PARTIAL].p;
    u32 max_pieces = 0, max_long = 0;
    for (int k = 0; k < 3; k++) {
        if (!(which & (1u << k))) continue;
        const R1csMatrixDev &m = r->m[k];
        args.m[nm++] = MatArg{m.row_off, m.entries, m.long_rows, m.pieces, outs[k], partial, m.n_long, m.n_pieces};
        partial += m.n_pieces;
        max_pieces = std::max(max_pieces, m.n_pieces); max_long = std::max(max_long, m.n_long);
    }
    MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_R1CS_BEGIN], st));
    if (nm && r->nc) {
        const RowTerm term{W, (const Fr *)r->coeffs};
        const unsigned wave_cap = (unsigned)ctx->cu_count * 8;   // blocks of 4 waves for the grid-stride passes
        if (!compact) hipLaunchKernelGGL(k_rows_short, dim3(mi_blocks_of(r->nc, 256), nm), dim3(256), 0, st, args, r->nc, term);
        if (max_pieces) hipLaunchKernelGGL(k_row_pieces, dim3(std::min(wave_cap, mi_blocks_of(max_pieces, 4)), nm), dim3(256), 0, st, args, term);
        if (max_long) hipLaunchKernelGGL(k_row_combine, dim3(std::min(wave_cap, mi_blocks_of(max_long, 4)), nm), dim3(256), 0, st, args, compact);
        MI_CHECK_HIP(ctx, hipGetLastError());
    }
    if (!compact) MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_R1CS_END], st));
    ctx->r1cs_stats = mi_r1cs_stats{0.f, nm, entries, n_long, n_pieces};
    ctx->r1cs_timed = true;
    return MI_OK;
}

int32_t check_which(mi_ctx *ctx, u32 which, const void *a, const void *b, const void *c, const char *who) {
    if (!which || (which & ~(MI_R1CS_A | MI_R1CS_B | MI_R1CS_C))) MI_FAIL(ctx, MI_EINVAL, std::string(who) + ": which names no matrix or an unknown one");
    if (((which & MI_R1CS_A) && !a) || ((which & MI_R1CS_B) && !b) || ((which & MI_R1CS_C) && !c)) MI_FAIL(ctx, MI_EINVAL, std::string(who) + ": the output of a requested matrix is null");
    return MI_OK;
}

}  // namespace

int32_t mi_r1cs_validate(mi_ctx *ctx, const char *who_c, const mi_r1cs_desc *d, R1csShape &sh) {
    const std::string who(who_c);
    if (!d) MI_FAIL(ctx, MI_EINVAL, who + ": r1cs is null");
    if (d->n_constraints > ((u64)1 << MI_SETUP_MAX_LOG_N)) MI_FAIL(ctx, MI_EINVAL, who + ": n_constraints: log_n above 27");
    u32 log_n = 0;
    while (((u64)1 << log_n) < d->n_constraints) log_n++;
    sh.log_n = log_n; sh.N = (u64)1 << log_n; sh.nc = d->n_constraints;
    if (d->nb_wires == 0 || d->nb_wires > MI_MSM_MAX_PAIRS) MI_FAIL(ctx, MI_EINVAL, who + ": nb_wires is 0 or above 2^27");
    if (d->nb_public == 0 || d->nb_public > d->nb_wires) MI_FAIL(ctx, MI_EINVAL, who + ": nb_public is 0 or above nb_wires");
    sh.nb_wires = d->nb_wires; sh.nb_public = d->nb_public;
    if (!d->coeffs && d->n_coeffs) MI_FAIL(ctx, MI_EINVAL, who + ": coeffs is null");
    if (d->n_coeffs >> 32) MI_FAIL(ctx, MI_EINVAL, who + ": n_coeffs: 2^32 entries or more");
    MI_TRY(check_matrix(ctx, who, "A", d->A, d, sh, 0));
    MI_TRY(check_matrix(ctx, who, "B", d->B, d, sh, 1));
    MI_TRY(check_matrix(ctx, who, "C", d->C, d, sh, 2));
    // commitments
    if (d->n_commitments > MI_PK_RAW_MAX_COMMITMENTS) MI_FAIL(ctx, MI_EINVAL, who + ": n_commitments above MI_PK_RAW_MAX_COMMITMENTS");
    sh.n_commitments = d->n_commitments;
    if (d->n_commitments && (!d->committed || !d->n_committed || !d->commitment_wire)) MI_FAIL(ctx, MI_EINVAL, who + ": committed / n_committed / commitment_wire is null");
    std::vector<u32> cw;
    for (u32 k = 0; k < d->n_commitments; k++) {
        if (d->n_committed[k] && !d->committed[k]) MI_FAIL(ctx, MI_EINVAL, who + ": committed[" + std::to_string(k) + "] is null");
        for (u64 i = 0; i < d->n_committed[k]; i++) {
            const u32 j = d->committed[k][i];
            if (j < d->nb_public || j >= d->nb_wires) MI_FAIL(ctx, MI_EINVAL, who + ": committed[" + std::to_string(k) + "][" + std::to_string(i) + "] is not a private wire");
            sh.removed.push_back(j);
        }
        const u32 j = d->commitment_wire[k];
        if (j < d->nb_public || j >= d->nb_wires) MI_FAIL(ctx, MI_EINVAL, who + ": commitment_wire[" + std::to_string(k) + "] is not a private wire");
        sh.removed.push_back(j);
        cw.push_back(j);
    }
    std::sort(sh.removed.begin(), sh.removed.end());
    if (std::adjacent_find(sh.removed.begin(), sh.removed.end()) != sh.removed.end())
        MI_FAIL(ctx, MI_EINVAL, who + ": committed / commitment_wire: a wire is listed twice");
    std::sort(cw.begin(), cw.end());
    for (u32 j = 0; j < d->nb_public; j++) sh.vk_wires.push_back(j);
    sh.vk_wires.insert(sh.vk_wires.end(), cw.begin(), cw.end());
    return MI_OK;
}

int32_t mi_r1cs_eval_ws(mi_ctx *ctx, const mi_r1cs *r, const mi_fr *W_dev, bool eval_c, const mi_fr **a, const mi_fr **b, const mi_fr **c) {
    const size_t bytes = (size_t)r->nc * sizeof(Fr) + 64;
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_R1CS_A], bytes));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_R1CS_B], bytes));
    if (eval_c) MI_TRY(mi_reserve(ctx, ctx->ws[WS_R1CS_C], bytes));
    Fr *const outs[3] = {(Fr *)ctx->ws[WS_R1CS_A].p, (Fr *)ctx->ws[WS_R1CS_B].p, eval_c ? (Fr *)ctx->ws[WS_R1CS_C].p : nullptr};
    MI_TRY(enqueue_eval(ctx, r, (const Fr *)W_dev, MI_R1CS_A | MI_R1CS_B | (eval_c ? MI_R1CS_C : 0u), outs, false));
    *a = (const mi_fr *)outs[0]; *b = (const mi_fr *)outs[1]; *c = (const mi_fr *)outs[2];
    return MI_OK;
}

extern "C" {

int32_t mi_r1cs_load(mi_ctx *ctx, const mi_r1cs_desc *d, mi_r1cs **out) {
    if (!ctx) return MI_EINVAL;
    if (!out) MI_FAIL(ctx, MI_EINVAL, "r1cs: out is null");
    *out = nullptr;
    R1csShape sh;
    MI_TRY(mi_r1cs_validate(ctx, "r1cs", d, sh));
    MI_CHECK_HIP(ctx, hipSetDevice(ctx->dev));
    // the coefficient table by value
    std::vector<uint8_t> cls((size_t)d->n_coeffs);
    {
        const Fr one = Fr::one(), minus_one = fe_neg(Fr::one());
        for (u64 i = 0; i < d->n_coeffs; i++) {
            Fr v; std::memcpy(&v, &d->coeffs[i], 32);
            cls[i] = v.is_zero() ? CLS_ZERO : v == one ? CLS_ONE : v == minus_one ? CLS_MINUS_ONE : CLS_ANY;
        }
    }
    mi_r1cs *r = new (std::nothrow) mi_r1cs();
    if (!r) return MI_ENOMEM;
    r->dev = ctx->dev; r->nc = sh.nc; r->nb_wires = sh.nb_wires; r->log_n = sh.log_n; r->n_coeffs = d->n_coeffs;
    auto body = [&]() -> int32_t {
        MI_TRY(to_device(ctx, r, &r->coeffs, d->coeffs, (size_t)d->n_coeffs * 32));
        const mi_r1cs_matrix *mats[3] = {&d->A, &d->B, &d->C};
        std::vector<uint2> packed;
        std::vector<SparseLong> long_rows;
        std::vector<uint2> pieces;
        for (int k = 0; k < 3; k++) {
            const mi_r1cs_matrix &m = *mats[k];
            const std::vector<u32> &rp = sh.row_ptr[k];
            const u32 nnz = sh.nnz[k];
            packed.resize(nnz);
            parallel_ranges(nnz, [&](unsigned, u64 lo, u64 hi) {
                for (u64 e = lo; e < hi; e++) packed[e] = make_uint2(m.col[e] | ((u32)cls[m.coeff[e]] << CLS_SHIFT), m.coeff[e]);
            });
            long_rows.clear(); pieces.clear();
            for (u64 i = 0; i < sh.nc; i++) {
                const u32 lo = rp[i], len = rp[i + 1] - lo;
                if (len <= SPARSE_SHORT) continue;
                const size_t first = pieces.size();
                long_rows.push_back(SparseLong{(u32)i, (u32)first, sparse_cut(lo, len, nullptr), 0});
                pieces.resize(first + long_rows.back().n_pieces);
                sparse_cut(lo, len, pieces.data() + first);
            }
            R1csMatrixDev &dm = r->m[k];
            dm.nnz = nnz; dm.n_long = (u32)long_rows.size(); dm.n_pieces = (u32)pieces.size();
            MI_TRY(to_device(ctx, r, (void **)&dm.row_off, rp.data(), rp.size() * 4));
            MI_TRY(to_device(ctx, r, (void **)&dm.entries, packed.data(), (size_t)nnz * 8));
            MI_TRY(to_device(ctx, r, (void **)&dm.long_rows, long_rows.data(), long_rows.size() * sizeof(SparseLong)));
            MI_TRY(to_device(ctx, r, (void **)&dm.pieces, pieces.data(), pieces.size() * 8));
        }
        return MI_OK;
    };
    int32_t rc = MI_ENOMEM;
    try { rc = body(); } catch (...) { mi_set_err(ctx, "r1cs: out of host memory"); }   // no exception crosses the C-ABI
    if (rc != MI_OK) { free_handle(r); return rc; }
    *out = r;
    return MI_OK;
}

int32_t mi_r1cs_free(mi_ctx *ctx, mi_r1cs *r) {
    if (!ctx || !r) return MI_EINVAL;
    (void)hipSetDevice(r->dev);
    (void)hipStreamSynchronize(ctx->stream);
    free_handle(r);
    return MI_OK;
}

int32_t mi_r1cs_bytes(const mi_r1cs *r, uint64_t *out) {
    if (!r || !out) return MI_EINVAL;
    *out = r->bytes;
    return MI_OK;
}

int32_t mi_r1cs_get_stats(mi_ctx *ctx, mi_r1cs_stats *out) {
    if (!ctx || !out) return MI_EINVAL;
    if (ctx->r1cs_timed) {   // the device time is read here, not in the call: a prove never waits for its evaluation on the host
        float ms = 0;
        if (hipEventSynchronize(ctx->ev[EV_R1CS_END]) != hipSuccess || hipEventElapsedTime(&ms, ctx->ev[EV_R1CS_BEGIN], ctx->ev[EV_R1CS_END]) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
        ctx->r1cs_stats.eval_ms = ms;
        ctx->r1cs_timed = false;
    }
    *out = ctx->r1cs_stats;
    return MI_OK;
}

int32_t mi_r1cs_eval_dev(mi_ctx *ctx, const mi_r1cs *r, const mi_fr *W_dev, uint32_t which, mi_fr *a_dev, mi_fr *b_dev, mi_fr *c_dev) {
    if (!ctx) return MI_EINVAL;
    MI_TRY(usable(ctx, r, "r1cs eval"));
    if (!W_dev) MI_FAIL(ctx, MI_EINVAL, "r1cs eval: W is null");
    MI_TRY(check_which(ctx, which, a_dev, b_dev, c_dev, "r1cs eval"));
    Fr *const outs[3] = {(Fr *)a_dev, (Fr *)b_dev, (Fr *)c_dev};
    return enqueue_eval(ctx, r, (const Fr *)W_dev, which, outs, false);
}

int32_t mi_r1cs_eval(mi_ctx *ctx, const mi_r1cs *r, const mi_fr *W, uint32_t which, mi_fr *a, mi_fr *b, mi_fr *c) {
    if (!ctx) return MI_EINVAL;
    MI_TRY(usable(ctx, r, "r1cs eval"));
    if (!W) MI_FAIL(ctx, MI_EINVAL, "r1cs eval: W is null");
    MI_TRY(check_which(ctx, which, a, b, c, "r1cs eval"));
    hipStream_t st = ctx->stream;
    const size_t rows = (size_t)r->nc * sizeof(Fr);
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_R1CS_W], (size_t)r->nb_wires * sizeof(Fr)));
    mi_fr *host[3] = {a, b, c};
    Fr *outs[3] = {nullptr, nullptr, nullptr};
    const int ws_of[3] = {WS_R1CS_A, WS_R1CS_B, WS_R1CS_C};
    for (int k = 0; k < 3; k++) {
        if (!(which & (1u << k))) continue;
        MI_TRY(mi_reserve(ctx, ctx->ws[ws_of[k]], rows + 64));
        outs[k] = (Fr *)ctx->ws[ws_of[k]].p;
    }
    MI_CHECK_HIP(ctx, hipMemcpyAsync(ctx->ws[WS_R1CS_W].p, W, (size_t)r->nb_wires * sizeof(Fr), hipMemcpyHostToDevice, st));
    MI_TRY(enqueue_eval(ctx, r, (const Fr *)ctx->ws[WS_R1CS_W].p, which, outs, false));
    for (int k = 0; k < 3; k++)
        if (outs[k] && rows) MI_CHECK_HIP(ctx, hipMemcpyAsync(host[k], outs[k], rows, hipMemcpyDeviceToHost, st));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
    return MI_OK;
}

int32_t mi_r1cs_check_dev(mi_ctx *ctx, const mi_r1cs *r, const mi_fr *W_dev, uint64_t *n_bad, uint64_t *first_bad) {
    if (!ctx) return MI_EINVAL;
    MI_TRY(usable(ctx, r, "r1cs check"));
    if (!W_dev || !n_bad || !first_bad) MI_FAIL(ctx, MI_EINVAL, "r1cs check: W, n_bad or first_bad is null");
    hipStream_t st = ctx->stream;
    // the long rows' sums, one per long row, behind the counters
    const u64 n_long = (u64)r->m[0].n_long + r->m[1].n_long + r->m[2].n_long;
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_R1CS_CHECK], 64 + (n_long + 1) * sizeof(Fr)));
    unsigned long long *ctr = (unsigned long long *)ctx->ws[WS_R1CS_CHECK].p;
    Fr *lv = (Fr *)((char *)ctx->ws[WS_R1CS_CHECK].p + 64);
    Fr *const outs[3] = {lv, lv + r->m[0].n_long, lv + r->m[0].n_long + r->m[1].n_long};
    MI_CHECK_HIP(ctx, hipMemsetAsync(ctr, 0, 8, st));
    MI_CHECK_HIP(ctx, hipMemsetAsync(ctr + 1, 0xff, 8, st));
    MI_TRY(enqueue_eval(ctx, r, (const Fr *)W_dev, MI_R1CS_A | MI_R1CS_B | MI_R1CS_C, outs, true));
    if (r->nc) {
        EvalArgs args{};
        for (int k = 0; k < 3; k++) args.m[k] = MatArg{r->m[k].row_off, r->m[k].entries, r->m[k].long_rows, r->m[k].pieces, outs[k], nullptr, r->m[k].n_long, r->m[k].n_pieces};
        hipLaunchKernelGGL(k_check, dim3(mi_blocks_of(r->nc, 256)), dim3(256), 0, st, args, r->nc, RowTerm{(const Fr *)W_dev, (const Fr *)r->coeffs}, ctr);
        MI_CHECK_HIP(ctx, hipGetLastError());
    }
    MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_R1CS_END], st));
    unsigned long long res[2] = {0, 0};
    MI_CHECK_HIP(ctx, hipMemcpyAsync(res, ctr, 16, hipMemcpyDeviceToHost, st));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
    *n_bad = res[0]; *first_bad = res[1];
    return MI_OK;
}

}  // extern "C"
