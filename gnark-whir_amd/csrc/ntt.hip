// Radix-2 NTT over Fr for gfx950 and the fused computeH pipeline.
// Replaces fft.Domain.FFT / FFTInverse (gnark-crypto ecc/bn254/fr/fft) and computeH (gnark
// backend/groth16/bn254/prove.go) on the path reached from /root/reference/mt.go:496
// (SURVEY.md 8a rows a3/a4).  Pass structure and index arithmetic: ntt_tile.cuh.
//
// HBM layout: the caller's array of 32-byte Montgomery elements, transformed in place.  Each pass
// is one launch; a workgroup owns one LDS tile (<= 2^log_e elements, two 16-byte planes), loads
// it with >= 256-byte contiguous runs, runs log2(R) butterfly stages out of LDS and stores it
// back.  Root tables of a generic transform (mi_ntt): one 2048-entry table serves every in-tile stage; inter-pass
// twiddles and coset powers come from two sqrt(N)-sized tables and one product (no N-sized table is read).
// computeH trades HBM for products: its strided passes read their stage twiddles by global index from
// M-entry tables (NttPass::tw_stage: no inter-pass product at all) and its coset shifts from N-entry ones.
// Bound: HBM for the load/store (64 B per element per pass), VALU (one 256-bit Montgomery product
// per butterfly) for the stages -- see DESIGN.md for the measured split.
#include "ctx.h"
#include "ntt_wave.cuh"
#include "msm2_core.cuh"   // the Z MSM's digit count rides in computeH's last launch (mi_ctx::zhook)
#include <cstring>
#include <cstdlib>

struct NttState {
    u32 log_n = 0xffffffffu;
    Fr *small_f = nullptr, *small_i = nullptr, *tw64k_f = nullptr, *tw64k_i = nullptr;   // N independent
    Fr *tw_lo_f = nullptr, *tw_hi_f = nullptr, *tw_lo_i = nullptr, *tw_hi_i = nullptr;
    Fr *g_lo = nullptr, *g_hi = nullptr, *gi_lo = nullptr, *gi_hi = nullptr, *ninv = nullptr;
    Fr *g_hi_n = nullptr, *gi_hi_nd = nullptr;   // computeH-internal: g^(j 2^h) / N  and  g^-(j 2^h) / N * den
    Fr *ninv_den = nullptr;                      // computeH-internal: den / N
    u32 tw_h = 0;
    // computeH's direct factor tables in the data's layout (NttPass::tw_direct / sc_direct), N entries each, built for one
    // (log_n, first radix): twiddles of the M = N pass for the inverse and the forward root, coset shifts g^bitrev(i) / N and
    // g^-bitrev(i) * den / N.  4 x 32 B x N of HBM (1 GiB at N = 2^23) bought 11 of the ~107 products per element computeH had
    // when they came (77 since; 71 with the stage twiddles below).
    // d_tw_* stay null while the stage-twiddle tables below are bound (they serve the same pass).
    Fr *d_tw_inv = nullptr, *d_tw_fwd = nullptr, *d_sc_fwd = nullptr, *d_sc_inv = nullptr;
    u32 d_log_n = 0xffffffffu, d_log_r0 = 0, d_npass = 0;
    // computeH's stage twiddles by global index (NttPass::tw_stage): one table of M = R S entries per strided pass of the plan and
    // root, instead of d_tw_* (the M = N pass) and tw64k_* (the inner ones).  Another ~6 products per element go: 71 of 77.
    Fr *s_tw_inv[3] = {nullptr, nullptr, nullptr}, *s_tw_fwd[3] = {nullptr, nullptr, nullptr};
    u32 s_log_r[3] = {0, 0, 0}, s_log_s[3] = {0, 0, 0}, s_n = 0;   // the passes they serve; s_n = 0: none built
    u32 stage_tw = 1;      // knob "ntt_stage_twiddles": build and bind them at the next table build (0: d_tw_* and the edge products)
    u32 d_radices = 0, d_stage_tw = 0;   // what the direct and stage tables were built for: the plan's radices (4 bits each) and the knob
    u32 direct_min_log_n = 12;   // below this the tables are not worth a launch
    // plan knobs (mi_debug_set_ntt_plan)
    // defaults from the tools/tune.py sweep at N = 2^23: 2^9-element tiles (16 KiB of LDS, 8 workgroups of 256
    // threads per CU), radices 2^7 * 2^7 * 2^9: 1.46 ms per transform vs 1.99 ms for 2^11 tiles
    u32 log_e = 9, max_contig = 9, max_strided = 7, threads = 256;
    u32 lds_floor = 0;     // bytes of LDS every pass workgroup requests at least: caps the workgroups per CU (0 = only what the tile needs)
    u32 plan_set = 0;      // the knobs above were set by the caller: no per-size defaults
    u32 wave_stages = 1;   // passes of radix >= 2^7 run their last / first seven stages in registers (k_ntt_pass_wave); 0 = all through LDS
    u32 fuse_pair = 1;     // computeH: inverse last pass + coset first pass of a and b as one launch (k_ntt_contig_pair)
    u32 fuse_triple = 1;   // computeH: coset last pass of a and of b + the product a b + the last transform's first pass as one launch (k_ntt_strided_triple)
    u32 fuse_last = 1;     // computeH: the last pass of den FFTInverse(c) + the last transform's last pass (which subtracts it) as one launch (k_ntt_contig_last_sub)
};
// Tile / radix knobs for a transform of 2^log_n: the caller's (mi_debug_set_ntt_plan) or, untouched, the measured best per size
// (tools/ntt_probe.py sweep, profiles/r02_tune_ntt_sweep.json): 2^9 tiles and radices 2^7 2^7 2^9 up to 2^23; 2^10 tiles and
// 2^8 2^8 2^8 at 2^24 (16.2 vs 17.4 ms per computeH); 2^10 tiles and 2^8 2^8(2^7) 2^10 from 2^25 on (71.9 vs 74.0 ms at 2^26).
static NttKnobs knobs_for(const struct NttState *st, u32 log_n);
static NttState *state_of(mi_ctx *ctx) {
    static_assert(sizeof(NttState) <= 384, "NttState lives in ctx->ntt_state");
    return reinterpret_cast<NttState *>(ctx->ntt_state);
}

// k_ntt_contig_last_sub with the Z MSM's digit count riding along, one instantiation per window width.  Named HERE, ahead of every
// kernel: naming them after the definitions changed their code (119 VGPRs for 117, profiles/ntt_schedule.txt)
template <int CC> __global__ void k_ntt_contig_last_sub_count(Fr *A, const Fr *Cin, NttPass pa, NttTables ta, NttPass pc, NttTables tc, Msm2Shape zs, u32 *C1);
typedef void (*LastSubCountKernel)(Fr *, const Fr *, NttPass, NttTables, NttPass, NttTables, Msm2Shape, u32 *);
static const LastSubCountKernel k_last_sub_count[6] = {   // by window width c - 17
    k_ntt_contig_last_sub_count<17>, k_ntt_contig_last_sub_count<18>, k_ntt_contig_last_sub_count<19>,
    k_ntt_contig_last_sub_count<20>, k_ntt_contig_last_sub_count<21>, k_ntt_contig_last_sub_count<22>};
bool mi_ntt_set_knob(mi_ctx *ctx, const char *name, int64_t value) {
    if (!std::strcmp(name, "ntt_lds_floor_kb") && value >= 0 && value <= 160) { state_of(ctx)->lds_floor = (u32)value * 1024u; return true; }
    if (!std::strcmp(name, "ntt_stage_twiddles") && (value == 0 || value == 1)) { state_of(ctx)->stage_tw = (u32)value; return true; }   // (ensure_direct rebuilds)
    return false;
}
static void free_stage_tables(NttState *st) {
    for (u32 k = 0; k < 3; k++)
        for (Fr **p : {&st->s_tw_inv[k], &st->s_tw_fwd[k]}) if (*p) { (void)hipFree(*p); *p = nullptr; }
    st->s_n = 0;
}
void mi_ntt_state_free(mi_ctx *ctx) {
    NttState *st = state_of(ctx);
    Fr **all[] = {&st->small_f, &st->small_i, &st->tw64k_f, &st->tw64k_i, &st->g_hi_n, &st->gi_hi_nd, &st->tw_lo_f, &st->tw_hi_f, &st->tw_lo_i, &st->tw_hi_i,
                  &st->g_lo, &st->g_hi, &st->gi_lo, &st->gi_hi, &st->ninv, &st->ninv_den, &st->d_tw_inv, &st->d_tw_fwd, &st->d_sc_fwd, &st->d_sc_inv};
    for (Fr **p : all) if (*p) { (void)hipFree(*p); *p = nullptr; }
    free_stage_tables(st);
}

// mi_ctx_trim: every table goes; the markers say "nothing built", the plan knobs stay
void mi_ntt_state_trim(mi_ctx *ctx) {
    mi_ntt_state_free(ctx);
    NttState *st = state_of(ctx);
    st->log_n = 0xffffffffu; st->d_log_n = 0xffffffffu; st->d_log_r0 = 0; st->d_npass = 0;
}
// bytes of device memory the context's NTT tables take (mi_get_mem_ledger)
size_t mi_ntt_table_bytes(mi_ctx *ctx) {
    const NttState *st = state_of(ctx);
    size_t b = 0;
    if (st->small_f) b += (size_t)(2 * 2048 + 2 * 65536) * sizeof(Fr);
    if (st->log_n != 0xffffffffu) {
        const size_t nlo = (size_t)1 << st->tw_h, nhi = (size_t)1 << (st->log_n - st->tw_h);
        b += (4 * nlo + 6 * nhi + 2) * sizeof(Fr);
    }
    for (const Fr *p : {st->d_tw_inv, st->d_tw_fwd, st->d_sc_fwd, st->d_sc_inv}) if (p) b += sizeof(Fr) << st->d_log_n;
    for (u32 k = 0; k < st->s_n; k++) b += 2 * (sizeof(Fr) << (st->s_log_r[k] + st->s_log_s[k]));
    return b;
}

static NttKnobs knobs_for(const NttState *st, u32 log_n) {
    if (st->plan_set) return NttKnobs{st->log_e, st->max_contig, st->max_strided};
    if (log_n == 24) return NttKnobs{10, 8, 8};
    if (log_n >= 25) return NttKnobs{10, 10, 8};
    return NttKnobs{st->log_e, st->max_contig, st->max_strided};
}

// out[j] = c * base^(j << shift)
__global__ void k_pow_table(Fr *out, u32 count, Fr base, Fr c, u32 shift) {
    u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    u64 e = (u64)j << shift;
    Fr acc = c, b = base;
    while (e) {
        if (e & 1) acc = acc * b;
        b = fe_sqr(b);
        e >>= 1;
    }
    out[j] = acc;
}

__global__ void __launch_bounds__(1024) k_ntt_pass(Fr *dst, const Fr *src, NttPass p, NttTables t) {
    extern __shared__ U4 lds[];
    const u64 tile = blockIdx.x;
    ntt_tile_load(p, t, src, tile, threadIdx.x, blockDim.x, lds);
    __syncthreads();
    for (u32 s = 0; s < p.log_r; s++) {
        ntt_tile_stage(p, t, s, threadIdx.x, blockDim.x, lds, tile);
        __syncthreads();
    }
    ntt_tile_store(p, t, dst, tile, threadIdx.x, blockDim.x, lds);
}

// The same pass with the seven stages at distance <= 64 of every 128-row group done in REGISTERS by one wavefront
// (ntt_wave.cuh): the tile makes two LDS round trips (in and out of the registers) plus one per stage at distance >= 128,
// instead of one per stage, and two barriers plus one per such stage.  Needs log_r >= 7.
#ifndef MI_NTT_WAVES_PER_EU
#define MI_NTT_WAVES_PER_EU 1   // experiment switch: 6 = no change (79 VGPRs either way), 8 = 64 VGPRs + 52 B of scratch, slower alone and in a proof
#endif
__global__ void __launch_bounds__(256, MI_NTT_WAVES_PER_EU) k_ntt_pass_wave(Fr *dst, const Fr *src, NttPass p, NttTables t) {
    extern __shared__ U4 lds[];
    const u64 tile = blockIdx.x;
    const u32 PL = ntt_plane_slots(p);
    ntt_tile_load(p, t, src, tile, threadIdx.x, blockDim.x, lds);
    __syncthreads();
    if (!p.dit)   // DIF: distances R/2 ... 128 first
        for (u32 s = 0; s + 7 < p.log_r; s++) {
            ntt_tile_stage(p, t, s, threadIdx.x, blockDim.x, lds, tile);
            __syncthreads();
        }
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const u32 nsub = 1u << (p.log_r + p.log_c - 7);
    for (u32 sb = wave; sb < nsub; sb += nwaves) {   // sub-block = 128 consecutive rows of one column: touched by this wave only
        const u32 col = sb & ((1u << p.log_c) - 1), base = (sb >> p.log_c) << 7;
        u32 ra, rb, wa, wb;
        if (!p.dit) { ra = base + lane; rb = ra + 64; wa = base + 2 * lane; wb = wa + 1; }
        else { ra = base + 2 * lane; rb = ra + 1; wa = base + lane; wb = wa + 64; }
        Fr x0 = lds_get(lds, PL, ntt_lds_slot(p, ra, col)), x1 = lds_get(lds, PL, ntt_lds_slot(p, rb, col));
        wave_ntt128(x0, x1, lane, p.dit != 0, t.small, ntt_stage_run(p, tile, col));
        lds_put(lds, PL, ntt_lds_slot(p, wa, col), x0);
        lds_put(lds, PL, ntt_lds_slot(p, wb, col), x1);
    }
    __syncthreads();
    if (p.dit)    // DIT: distances 128 ... R/2 last
        for (u32 s = 7; s < p.log_r; s++) {
            ntt_tile_stage(p, t, s, threadIdx.x, blockDim.x, lds, tile);
            __syncthreads();
        }
    ntt_tile_store(p, t, dst, tile, threadIdx.x, blockDim.x, lds);
}

// computeH's a and b: the LAST pass of the inverse transform (DIF, contiguous tiles) and the FIRST pass of the coset transform that
// follows (DIT, the same contiguous tiles, coset shift on the way in) as one launch -- the tile is loaded once, runs the inverse
// stages, is multiplied by the shift, runs the forward stages and is stored once; in the register stages the two transforms meet
// without an LDS round trip (a lane ends the DIF stages holding positions 2L, 2L + 1 -- what the DIT stages start from).  One store
// and one load of the vector (0.54 GB at N = 2^23) and one launch less per vector.  pi / ti: the inverse pass as launch_pass would have
// launched it, pf / tf: the forward one.  Radix >= 2^7, equal tile shapes.
__global__ void __launch_bounds__(256) k_ntt_contig_pair(Fr *data, NttPass pi, NttTables ti, NttPass pf, NttTables tf) {
    extern __shared__ U4 lds[];
    const u64 tile = blockIdx.x;
    const u32 PL = ntt_plane_slots(pi);
    ntt_tile_load(pi, ti, data, tile, threadIdx.x, blockDim.x, lds);
    __syncthreads();
    for (u32 s = 0; s + 7 < pi.log_r; s++) {   // DIF distances R/2 ... 128
        ntt_tile_stage(pi, ti, s, threadIdx.x, blockDim.x, lds);
        __syncthreads();
    }
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const u32 nsub = 1u << (pi.log_r + pi.log_c - 7);
    for (u32 sb = wave; sb < nsub; sb += nwaves) {
        const u32 col = sb & ((1u << pi.log_c) - 1), base = (sb >> pi.log_c) << 7;
        Fr x0 = lds_get(lds, PL, ntt_lds_slot(pi, base + lane, col)), x1 = lds_get(lds, PL, ntt_lds_slot(pi, base + lane + 64, col));
        wave_ntt128(x0, x1, lane, false, ti.small);
        // what the inverse pass would have stored at rows 2L, 2L + 1 and the forward pass loaded with its edge factor
        const u32 r0 = base + 2 * lane, r1 = r0 + 1;
        Fr f;
        if (ntt_edge_factor(pi, ti, r0, ntt_global_index(pi, tile, r0, col), 1, f)) x0 = fe_mul_lazy(x0, f);
        if (ntt_edge_factor(pf, tf, r0, ntt_global_index(pf, tile, r0, col), 0, f)) x0 = fe_mul_lazy(x0, f);
        if (ntt_edge_factor(pi, ti, r1, ntt_global_index(pi, tile, r1, col), 1, f)) x1 = fe_mul_lazy(x1, f);
        if (ntt_edge_factor(pf, tf, r1, ntt_global_index(pf, tile, r1, col), 0, f)) x1 = fe_mul_lazy(x1, f);
        wave_ntt128(x0, x1, lane, true, tf.small);
        lds_put(lds, PL, ntt_lds_slot(pf, base + lane, col), x0);
        lds_put(lds, PL, ntt_lds_slot(pf, base + lane + 64, col), x1);
    }
    __syncthreads();
    for (u32 s = 7; s < pf.log_r; s++) {   // DIT distances 128 ... R/2
        ntt_tile_stage(pf, tf, s, threadIdx.x, blockDim.x, lds);
        __syncthreads();
    }
    ntt_tile_store(pf, tf, data, tile, threadIdx.x, blockDim.x, lds);
}

// computeH's OTHER seam: the LAST pass of the coset FFT of a and of b (DIT, the strided M = N pass), the pointwise product a b, and the
// FIRST pass of the last transform (DIF, inverse on the coset, the same strided tiles) as one launch.  A workgroup loads a's tile
// (DIT pre-twiddle on the way in), runs the seven register stages and keeps the result in registers (a lane ends DIT holding rows L,
// L + 64 -- exactly what the DIF stages start from), loads b's tile into the same LDS, does the same, multiplies, runs the DIF stages
// and stores through LDS with the DIF post-twiddle.  Per element: the same products; four passes of a vector through HBM (store a,
// store b, load a, load b: 1.07 GB at N = 2^23) and two launches less.  pc / tc: the coset FFT's last pass as launch_pass would have
// launched it (for a and for b alike), pl / tl: the last transform's first pass (without load_mul).  Radix 2^7 exactly (no stage
// through LDS) and one 128-row sub-block per wave (blockDim = 64 x sub-blocks of the tile).
__global__ void __launch_bounds__(512) k_ntt_strided_triple(Fr *a, const Fr *b, NttPass pc, NttTables tc, NttPass pl, NttTables tl) {
    extern __shared__ U4 lds[];
    const u64 tile = blockIdx.x;
    const u32 PL = ntt_plane_slots(pc);
    const u32 lane = threadIdx.x & 63, sb = threadIdx.x >> 6;
    const u32 col = sb & ((1u << pc.log_c) - 1), base = (sb >> pc.log_c) << 7;
    const u32 s0 = ntt_lds_slot(pc, base + 2 * lane, col), s1 = ntt_lds_slot(pc, base + 2 * lane + 1, col);
    const Fr *const run_c = ntt_stage_run(pc, tile, col), *const run_l = ntt_stage_run(pl, tile, col);   // stage twiddles by global index, or null
    ntt_tile_load(pc, tc, a, tile, threadIdx.x, blockDim.x, lds);
    __syncthreads();
    Fr a0 = lds_get(lds, PL, s0), a1 = lds_get(lds, PL, s1);
    wave_ntt128(a0, a1, lane, true, tc.small, run_c);     // -> rows L, L + 64
    __syncthreads();                               // every wave has read a's tile
    ntt_tile_load(pc, tc, b, tile, threadIdx.x, blockDim.x, lds);
    __syncthreads();
    Fr x0 = lds_get(lds, PL, s0), x1 = lds_get(lds, PL, s1);
    wave_ntt128(x0, x1, lane, true, tc.small, run_c);
    x0 = ntt_mul_lazy2(x0, a0); x1 = ntt_mul_lazy2(x1, a1);   // DIT left both factors below 4p; the DIF stages want [0, 2p)
    wave_ntt128(x0, x1, lane, false, tl.small, run_l);    // rows L, L + 64 -> positions 2L, 2L + 1
    __syncthreads();                               // every wave has read b's tile
    lds_put(lds, PL, ntt_lds_slot(pl, base + 2 * lane, col), x0);
    lds_put(lds, PL, ntt_lds_slot(pl, base + 2 * lane + 1, col), x1);
    __syncthreads();
    ntt_tile_store(pl, tl, a, tile, threadIdx.x, blockDim.x, lds);
}
// The same seam for a first radix of 2^8 (the plans of N = 2^24 and 2^26): the DIT pass ends, and the DIF pass begins, with the stage at
// distance 128 -- on the SAME pairs (r, r + 128).  Each 128-row half of a column goes through the register stages of one wave and back
// to LDS; a thread then takes its pairs, does the DIT butterfly and keeps the two results in registers (for a), does the same for b,
// multiplies, does the DIF butterfly on the products and writes them to LDS for the DIF register stages.  256 threads per 256-row x
// 2^log_c-column tile: 2^log_c butterflies per thread at distance 128 (2^(log_c + 1) elements of a held in registers: log_c <= 2).
__global__ void __launch_bounds__(256) k_ntt_strided_triple8(Fr *a, const Fr *b, NttPass pc, NttTables tc, NttPass pl, NttTables tl) {
    extern __shared__ U4 lds[];
    const u64 tile = blockIdx.x;
    const u32 PL = ntt_plane_slots(pc);
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const u32 C = 1u << pc.log_c, nsub = 2u << pc.log_c;   // 128-row sub-blocks of the tile
    const u32 nb = C >> 1;                                  // butterflies at distance 128 per thread: 128 * C over 256 threads
    Fr keep[4];                                             // a's results of this thread's pairs (nb <= 2 pairs)
    auto reg_stages = [&](const NttPass &p, bool dit, const Fr *small) {
        for (u32 sbk = wave; sbk < nsub; sbk += nwaves) {
            const u32 col = sbk & (C - 1), base = (sbk >> p.log_c) << 7;
            u32 ra, rb, wa, wb;
            if (!dit) { ra = base + lane; rb = ra + 64; wa = base + 2 * lane; wb = wa + 1; }
            else { ra = base + 2 * lane; rb = ra + 1; wa = base + lane; wb = wa + 64; }
            Fr x0 = lds_get(lds, PL, ntt_lds_slot(p, ra, col)), x1 = lds_get(lds, PL, ntt_lds_slot(p, rb, col));
            wave_ntt128(x0, x1, lane, dit, small, ntt_stage_run(p, tile, col));
            lds_put(lds, PL, ntt_lds_slot(p, wa, col), x0);
            lds_put(lds, PL, ntt_lds_slot(p, wb, col), x1);
        }
    };
    // pair k of this thread: butterfly index bf = threadIdx.x + 256 k over (column, row j < 128), rows j and j + 128
    ntt_tile_load(pc, tc, a, tile, threadIdx.x, blockDim.x, lds);
    __syncthreads();
    reg_stages(pc, true, tc.small);
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < 2; k++) {   // (constant trip count: keep[] stays in registers)
        if (k >= nb) break;
        const u32 bf = threadIdx.x + 256 * k, col = bf & (C - 1), j = bf >> pc.log_c;
        Fr x = lds_get(lds, PL, ntt_lds_slot(pc, j, col));
        Fr y = lds_get(lds, PL, ntt_lds_slot(pc, j + 128, col));
        const Fr *run = ntt_stage_run(pc, tile, col);
        ntt_bfly_dit(x, y, run ? &run[128 + j] : j ? &tc.small[j << 4] : nullptr);           // w_256^j = w_4096^(16 j), or the global stage's
        keep[2 * k] = x; keep[2 * k + 1] = y;
    }
    __syncthreads();
    ntt_tile_load(pc, tc, b, tile, threadIdx.x, blockDim.x, lds);
    __syncthreads();
    reg_stages(pc, true, tc.small);
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < 2; k++) {
        if (k >= nb) break;
        const u32 bf = threadIdx.x + 256 * k, col = bf & (C - 1), j = bf >> pc.log_c;
        Fr x = lds_get(lds, PL, ntt_lds_slot(pc, j, col));
        Fr y = lds_get(lds, PL, ntt_lds_slot(pc, j + 128, col));
        const Fr *run_c = ntt_stage_run(pc, tile, col), *run_l = ntt_stage_run(pl, tile, col);
        ntt_bfly_dit(x, y, run_c ? &run_c[128 + j] : j ? &tc.small[j << 4] : nullptr);
        Fr p0 = ntt_mul_lazy2(x, keep[2 * k]), p1 = ntt_mul_lazy2(y, keep[2 * k + 1]);   // the products at rows j, j + 128, below 2p
        ntt_bfly_dif(p0, p1, run_l ? &run_l[128 + j] : j ? &tl.small[j << 4] : nullptr);                           // DIF butterfly at distance 128
        lds_put(lds, PL, ntt_lds_slot(pl, j, col), p0);
        lds_put(lds, PL, ntt_lds_slot(pl, j + 128, col), p1);
    }
    __syncthreads();
    reg_stages(pl, false, tl.small);
    __syncthreads();
    ntt_tile_store(pl, tl, a, tile, threadIdx.x, blockDim.x, lds);
}

// computeH's LAST seam: the last (contiguous, DIF) pass of den FFTInverse(c) and the last pass of the last transform work on the same
// contiguous tiles, and the second subtracts the first's output element by element.  One launch: c's tile goes through its stages and its
// den / N scaling and stays in REGISTERS (a thread keeps the elements it would have stored), the main tile follows through the same LDS,
// and the store subtracts, canonicalises and writes h.  c's last store and the store_sub read (0.54 GB at N = 2^23) and one launch go.
// pa / ta: the last transform's last pass as launch_pass would have launched it (store_sub unset), pc / tc: c's.  Equal tile shapes, radix >= 2^7,
// at most four elements per thread.
__device__ __forceinline__ void ntt_wave_pass_to_lds(const NttPass &p, const NttTables &t, const Fr *src, u64 tile, U4 *lds) {
    const u32 PL = ntt_plane_slots(p);
    ntt_tile_load(p, t, src, tile, threadIdx.x, blockDim.x, lds);
    __syncthreads();
    for (u32 s = 0; s + 7 < p.log_r; s++) {   // DIF distances R/2 ... 128
        ntt_tile_stage(p, t, s, threadIdx.x, blockDim.x, lds);
        __syncthreads();
    }
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const u32 nsub = 1u << (p.log_r + p.log_c - 7);
    for (u32 sb = wave; sb < nsub; sb += nwaves) {
        const u32 col = sb & ((1u << p.log_c) - 1), base = (sb >> p.log_c) << 7;
        Fr x0 = lds_get(lds, PL, ntt_lds_slot(p, base + lane, col)), x1 = lds_get(lds, PL, ntt_lds_slot(p, base + lane + 64, col));
        wave_ntt128(x0, x1, lane, false, t.small);
        lds_put(lds, PL, ntt_lds_slot(p, base + 2 * lane, col), x0);
        lds_put(lds, PL, ntt_lds_slot(p, base + 2 * lane + 1, col), x1);
    }
    __syncthreads();
}
// CC >= 17: the same launch also COUNTS the digits of every h coefficient it stores, for the fixed-base sort of the Z MSM that follows
// (msm2_core.cuh: a contiguous tile of E elements is E / MSM2_SLICE whole slices of that sort; counters in LDS behind the tile's two planes,
// written to C1[group][slice] exactly as k_msm2_count would have).  CC = -1: no count (the kernel every other caller gets).
template <int CC>
__device__ __forceinline__ void ntt_contig_last_sub_body(Fr *A, const Fr *Cin, const NttPass &pa, const NttTables &ta, const NttPass &pc, const NttTables &tc,
                                                         const Msm2Shape &zs, u32 *C1) {
    extern __shared__ U4 lds[];
    const u64 tile = blockIdx.x;
    const u32 E = 1u << (pa.log_r + pa.log_c), PL = ntt_plane_slots(pa);
    u32 *cnt = reinterpret_cast<u32 *>(lds + 2 * PL);
    const u32 nsl = E / MSM2_SLICE;
    if (CC >= 0) for (u32 k = threadIdx.x; k < nsl * zs.ngroups; k += blockDim.x) cnt[k] = 0;   // (barriers follow before the first count)
    Fr keep[4];
    ntt_wave_pass_to_lds(pc, tc, Cin, tile, lds);
#pragma unroll
    for (u32 k = 0; k < 4; k++) {   // (constant trip count: keep[] stays in registers)
        const u32 e = threadIdx.x + k * blockDim.x;
        if (e >= E) break;
        const u32 rho = e & ((1u << pc.log_r) - 1), col = e >> pc.log_r;   // contiguous pass: the order that is contiguous in global memory
        Fr v = lds_get(lds, PL, ntt_lds_slot(pc, rho, col)), f;
        if (ntt_edge_factor(pc, tc, rho, ntt_global_index(pc, tile, rho, col), 1, f)) v = fe_mul_lazy(v, f);
        keep[k] = v;
    }
    __syncthreads();   // every thread has read c's tile
    ntt_wave_pass_to_lds(pa, ta, A, tile, lds);
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
        const u32 e = threadIdx.x + k * blockDim.x;
        if (e >= E) break;
        const u32 rho = e & ((1u << pa.log_r) - 1), col = e >> pa.log_r;
        const u64 g = ntt_global_index(pa, tile, rho, col);
        Fr v = lds_get(lds, PL, ntt_lds_slot(pa, rho, col)), f;
        if (ntt_edge_factor(pa, ta, rho, g, 1, f)) v = fe_mul_lazy(v, f);
        const Fr hv = fe_canon(fe_sub_plus2p(fe_condsub_2p(v), fe_condsub_2p(keep[k])));
        A[g] = hv;
        if (CC >= 0 && g < zs.n) {
            Msm2Digits dg;
            dg.start(hv, true);
            msm2_count_one<(CC >= 0 ? (u32)CC : 0u)>(zs, dg, cnt + (e / MSM2_SLICE) * zs.ngroups);
        }
    }
    if (CC >= 0) {
        __syncthreads();
        const u32 s0 = (u32)tile * nsl;
        for (u32 k = threadIdx.x; k < nsl * zs.ngroups; k += blockDim.x) {
            const u32 j = k / zs.ngroups, gq = k % zs.ngroups;
            if (s0 + j < zs.nslices) C1[(size_t)gq * zs.nslices + s0 + j] = cnt[k];
        }
    }
}
__global__ void __launch_bounds__(256) k_ntt_contig_last_sub(Fr *A, const Fr *Cin, NttPass pa, NttTables ta, NttPass pc, NttTables tc) {
    ntt_contig_last_sub_body<-1>(A, Cin, pa, ta, pc, tc, Msm2Shape{}, nullptr);
}
template <int CC>
__global__ void __launch_bounds__(256) k_ntt_contig_last_sub_count(Fr *A, const Fr *Cin, NttPass pa, NttTables ta, NttPass pc, NttTables tc, Msm2Shape zs, u32 *C1) {
    ntt_contig_last_sub_body<CC>(A, Cin, pa, ta, pc, tc, zs, C1);
}
void mi_ntt_state_init(mi_ctx *ctx) {
    static_assert(sizeof(NttState) <= sizeof(ctx->ntt_state), "NttState lives in ctx->ntt_state");
    new (ctx->ntt_state) NttState();
    const void *const dynamic_lds[] = {(const void *)k_ntt_pass, (const void *)k_ntt_pass_wave, (const void *)k_ntt_contig_pair,
                                       (const void *)k_ntt_strided_triple, (const void *)k_ntt_strided_triple8, (const void *)k_ntt_contig_last_sub};
    for (const void *k : dynamic_lds) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    for (LastSubCountKernel k : k_last_sub_count) (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// direct factor tables (NttPass::tw_direct / sc_direct), one thread per entry, square-and-multiply
__global__ void k_tw_layout(Fr *out, u32 log_n, u32 log_r, Fr w) {   // the M = N pass: element g = (rho << log_s) | lo
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (1u << log_n)) return;
    const u32 log_s = log_n - log_r;
    u32 e = (g & ((1u << log_s) - 1)) * bitrev_u32(g >> log_s, log_r);   // < N
    Fr acc = Fr::one(), b = w;
    while (e) { if (e & 1) acc = acc * b; b = fe_sqr(b); e >>= 1; }
    out[g] = acc;
}
// stage twiddles by global index of the pass (log_r, log_s), NttPass::tw_stage: 2^(log_r + log_s) entries
__global__ void k_tw_stage_layout(Fr *out, u32 log_n, u32 log_r, u32 log_s, Fr w) {
    const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (1u << (log_r + log_s))) return;
    u32 e = ntt_stage_tw_exponent(log_n, log_r, log_s, idx);   // < N / 2
    Fr acc = Fr::one(), b = w;
    while (e) { if (e & 1) acc = acc * b; b = fe_sqr(b); e >>= 1; }
    out[idx] = acc;
}
__global__ void k_sc_layout(Fr *out, u32 log_n, Fr base, Fr c) {     // out[i] = c * base^bitrev_N(i)
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << log_n)) return;
    u32 e = bitrev_u32(i, log_n);
    Fr acc = c, b = base;
    while (e) { if (e & 1) acc = acc * b; b = fe_sqr(b); e >>= 1; }
    out[i] = acc;
}

static int32_t build_table(mi_ctx *ctx, Fr **slot, u32 count, const Fr &base, const Fr &c, u32 shift) {
    if (*slot) { MI_CHECK_HIP(ctx, hipFree(*slot)); *slot = nullptr; }
    MI_CHECK_HIP(ctx, hipMalloc((void **)slot, sizeof(Fr) * (count ? count : 1)));
    hipLaunchKernelGGL(k_pow_table, dim3((count + 127) / 128), dim3(128), 0, ctx->stream, *slot, count, base, c, shift);
    MI_CHECK_HIP(ctx, hipGetLastError());
    return MI_OK;
}

// the constants of the domain of size 2^log_n: its root, the coset generator, 1/N and den = 1 / (g^N - 1)
struct NttRoots { Fr w, wi, g, gi, ninv, den; };
static NttRoots ntt_roots(u32 log_n) {
    NttRoots r;
    r.w = fr_domain_generator(log_n); r.wi = fe_inv(r.w);
    r.g = fe_from_u32<FrParams>(5); r.gi = fe_inv(r.g);
    Fr nn = Fr::zero();
    nn.l[0] = (u32)(1u << log_n);  // log_n <= 28
    r.ninv = fe_inv(fe_to_mont(nn));
    Fr gn = r.g;
    for (u32 k = 0; k < log_n; k++) gn = fe_sqr(gn);
    r.den = fe_inv(gn - Fr::one());
    return r;
}

static int32_t ensure_tables(mi_ctx *ctx, u32 log_n) {
    NttState *st = state_of(ctx);
    if (!st->small_f) {
        Fr w4096 = fr_domain_generator(12);
        MI_TRY(build_table(ctx, &st->small_f, 2048, w4096, Fr::one(), 0));
        MI_TRY(build_table(ctx, &st->small_i, 2048, fe_inv(w4096), Fr::one(), 0));
        Fr w64k = fr_domain_generator(16);
        MI_TRY(build_table(ctx, &st->tw64k_f, 65536, w64k, Fr::one(), 0));
        MI_TRY(build_table(ctx, &st->tw64k_i, 65536, fe_inv(w64k), Fr::one(), 0));
    }
    if (st->log_n == log_n) return MI_OK;
    const NttRoots r = ntt_roots(log_n);
    u32 h = (log_n + 1) / 2;
    u32 nlo = 1u << h, nhi = 1u << (log_n - h);
    st->tw_h = h;
    MI_TRY(build_table(ctx, &st->tw_lo_f, nlo, r.w, Fr::one(), 0));
    MI_TRY(build_table(ctx, &st->tw_hi_f, nhi, r.w, Fr::one(), h));
    MI_TRY(build_table(ctx, &st->tw_lo_i, nlo, r.wi, Fr::one(), 0));
    MI_TRY(build_table(ctx, &st->tw_hi_i, nhi, r.wi, Fr::one(), h));
    MI_TRY(build_table(ctx, &st->g_lo, nlo, r.g, Fr::one(), 0));
    MI_TRY(build_table(ctx, &st->g_hi, nhi, r.g, Fr::one(), h));
    MI_TRY(build_table(ctx, &st->gi_lo, nlo, r.gi, Fr::one(), 0));
    MI_TRY(build_table(ctx, &st->gi_hi, nhi, r.gi, r.ninv, h));
    MI_TRY(build_table(ctx, &st->ninv, 1, Fr::one(), r.ninv, 0));
    // computeH folds the 1/N of FFTInverse(a|b|c) into the coset shift of the next transform and den = 1/(g^N - 1) into the
    // last inverse transform's scaling (both are linear): 4 of its 121 products per element disappear
    MI_TRY(build_table(ctx, &st->g_hi_n, nhi, r.g, r.ninv, h));
    MI_TRY(build_table(ctx, &st->gi_hi_nd, nhi, r.gi, r.ninv * r.den, h));
    MI_TRY(build_table(ctx, &st->ninv_den, 1, Fr::one(), r.ninv * r.den, 0));
    st->log_n = log_n;
    return MI_OK;
}

// computeH's direct and stage-twiddle tables for (log_n, current plan, knob "ntt_stage_twiddles"); a failure to allocate the stage
// twiddles only means the direct tables serve, a failure to allocate those that the composed-table path runs
static int32_t ensure_direct(mi_ctx *ctx, u32 log_n) {
    NttState *st = state_of(ctx);
    const NttKnobs kn = knobs_for(st, log_n);
    const NttPlan pl = ntt_make_plan(log_n, kn.max_contig, kn.max_strided);
    u32 radices = 0;
    for (u32 i = 0; i < pl.n_pass; i++) radices |= pl.log_r[i] << (4 * i);
    if (st->d_log_n == log_n && st->d_log_r0 == pl.log_r[0] && st->d_npass == pl.n_pass && st->d_radices == radices && st->d_stage_tw == st->stage_tw) return MI_OK;
    Fr **four[] = {&st->d_tw_inv, &st->d_tw_fwd, &st->d_sc_fwd, &st->d_sc_inv};
    for (Fr **p : four) if (*p) { (void)hipFree(*p); *p = nullptr; }
    free_stage_tables(st);
    st->d_log_n = 0xffffffffu;
    if (log_n < st->direct_min_log_n) return MI_OK;
    // one stage-twiddle table per strided pass and root (plans of up to three strided passes: every default plan)
    const u32 n_strided = pl.n_pass - 1;
    bool stage = st->stage_tw && n_strided >= 1 && n_strided <= 3;
    for (u32 k = 0, log_s = log_n; stage && k < n_strided; k++) {
        log_s -= pl.log_r[k];
        st->s_log_r[k] = pl.log_r[k]; st->s_log_s[k] = log_s;
        for (Fr **p : {&st->s_tw_inv[k], &st->s_tw_fwd[k]})
            if (stage && hipMalloc((void **)p, sizeof(Fr) << (pl.log_r[k] + log_s)) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; stage = false; }
    }
    if (!stage) free_stage_tables(st);
    const size_t bytes = sizeof(Fr) << log_n;
    for (Fr **p : four) {
        if (stage && (p == &st->d_tw_inv || p == &st->d_tw_fwd)) continue;   // the stage twiddles serve the M = N pass
        if (hipMalloc((void **)p, bytes) != hipSuccess) {   // no room: stay on the composed tables
            (void)hipGetLastError();
            *p = nullptr;
            for (Fr **q : four) if (*q) { (void)hipFree(*q); *q = nullptr; }
            free_stage_tables(st);
            return MI_OK;
        }
    }
    const NttRoots r = ntt_roots(log_n);
    const unsigned blocks = (unsigned)(((size_t)1 << log_n) + 255) / 256;
    if (stage) {
        st->s_n = n_strided;
        for (u32 k = 0; k < n_strided; k++) {
            const unsigned sb = (unsigned)((((size_t)1 << (st->s_log_r[k] + st->s_log_s[k])) + 255) / 256);
            hipLaunchKernelGGL(k_tw_stage_layout, dim3(sb), dim3(256), 0, ctx->stream, st->s_tw_inv[k], log_n, st->s_log_r[k], st->s_log_s[k], r.wi);
            hipLaunchKernelGGL(k_tw_stage_layout, dim3(sb), dim3(256), 0, ctx->stream, st->s_tw_fwd[k], log_n, st->s_log_r[k], st->s_log_s[k], r.w);
        }
    } else if (pl.n_pass > 1) {
        hipLaunchKernelGGL(k_tw_layout, dim3(blocks), dim3(256), 0, ctx->stream, st->d_tw_inv, log_n, pl.log_r[0], r.wi);
        hipLaunchKernelGGL(k_tw_layout, dim3(blocks), dim3(256), 0, ctx->stream, st->d_tw_fwd, log_n, pl.log_r[0], r.w);
    }
    hipLaunchKernelGGL(k_sc_layout, dim3(blocks), dim3(256), 0, ctx->stream, st->d_sc_fwd, log_n, r.g, r.ninv);            // NTT_COSET_FWD_NINV
    hipLaunchKernelGGL(k_sc_layout, dim3(blocks), dim3(256), 0, ctx->stream, st->d_sc_inv, log_n, r.gi, r.ninv * r.den);   // NTT_COSET_INV_DEN
    MI_CHECK_HIP(ctx, hipGetLastError());
    st->d_log_n = log_n; st->d_log_r0 = pl.log_r[0]; st->d_npass = pl.n_pass; st->d_radices = radices; st->d_stage_tw = st->stage_tw;
    return MI_OK;
}

// ---------------------------------------------------------------- a transform: build, bind, launch
static_assert(NTT_INVERSE == MI_NTT_INVERSE && NTT_COSET == MI_NTT_COSET && NTT_DIT == MI_NTT_DIT, "ntt_tile.cuh names the public flags");
// build: the passes of one transform under the context's current knobs (ntt_tile.cuh; nothing bound yet)
static NttTransform ntt_build(const NttState *st, u32 log_n, u32 flags, NttVariant variant, u32 n_valid) {
    return ntt_build_transform(log_n, flags, variant, knobs_for(st, log_n), st->wave_stages != 0, n_valid);
}
// bind: the context's tables (ensure_tables / ensure_direct have run) and the optional pointers of the passes.  load_mul / store_sub
// (computeH only, see NttPass): pointwise factor on the way into the first pass / pointwise subtrahend on the way out of the last.
static int32_t ntt_bind(mi_ctx *ctx, NttTransform &tr, const Fr *load_mul = nullptr, const Fr *store_sub = nullptr) {
    const NttState *st = state_of(ctx);
    const bool inverse = tr.flags & NTT_INVERSE, coset = tr.flags & NTT_COSET;
    NttTables &t = tr.t;
    t.small = inverse ? st->small_i : st->small_f;
    t.tw_lo = inverse ? st->tw_lo_i : st->tw_lo_f;
    t.tw_hi = inverse ? st->tw_hi_i : st->tw_hi_f;
    t.tw_h = st->tw_h;
    t.tw_64k = inverse ? st->tw64k_i : st->tw64k_f;
    if (coset && !inverse) { t.sc_lo = st->g_lo; t.sc_hi = tr.variant == NTT_COSET_FWD_NINV ? st->g_hi_n : st->g_hi; }
    else if (coset && inverse) { t.sc_lo = st->gi_lo; t.sc_hi = tr.variant == NTT_COSET_INV_DEN ? st->gi_hi_nd : st->gi_hi; }
    else if (inverse && tr.variant != NTT_INV_UNSCALED) t.sc_lo = t.sc_hi = tr.variant == NTT_INV_DEN_NINV ? st->ninv_den : st->ninv;
    NttPass &first = tr.pass[0];
    if (load_mul && (first.scale == 1 || first.scale == 2 || first.dit)) MI_FAIL(ctx, MI_EINVAL, "internal: load_mul on a pass whose load side already has a factor");
    first.load_mul = load_mul;
    tr.pass[tr.n_pass - 1].store_sub = store_sub;
    // computeH's stage twiddles of every strided pass, else the direct twiddle of the M = N pass; the coset shift of the contiguous pass
    if (tr.variant == NTT_PLAIN || st->d_log_n != tr.log_n || !st->d_sc_fwd) return MI_OK;
    for (u32 i = 0; i < tr.n_pass; i++) {
        NttPass &p = tr.pass[i];
        for (u32 k = 0; p.twiddle && k < st->s_n; k++)
            if (st->s_log_r[k] == p.log_r && st->s_log_s[k] == p.log_s) p.tw_stage = inverse ? st->s_tw_inv[k] : st->s_tw_fwd[k];
        if (p.twiddle && !p.tw_stage && p.log_r + p.log_s == tr.log_n) p.tw_direct = inverse ? st->d_tw_inv : st->d_tw_fwd;
        if (tr.variant == NTT_COSET_FWD_NINV && p.scale == 1) p.sc_direct = st->d_sc_fwd;
        if (tr.variant == NTT_COSET_INV_DEN && p.scale == 3) p.sc_direct = st->d_sc_inv;
    }
    return MI_OK;
}

// launch: one function per kernel family; each owns its grid, block, LDS size, error check and launch count
static u32 ntt_tiles(const NttPass &p) { return 1u << (p.log_n - p.log_r - p.log_c); }
static size_t ntt_lds_bytes(const NttPass &p) { return (size_t)32 * ntt_plane_slots(p); }
static int32_t ntt_launched(mi_ctx *ctx) {
    MI_CHECK_HIP(ctx, hipGetLastError());
    ctx->stats.ntt_launches++;
    return MI_OK;
}
static int32_t launch_pass(mi_ctx *ctx, Fr *dst, const Fr *src, const NttPass &p, const NttTables &t) {
    const NttState *st = state_of(ctx);
    const bool wave = p.log_r >= 7 && st->wave_stages;
    size_t lds_bytes = ntt_lds_bytes(p);
    if (st->lds_floor > lds_bytes) lds_bytes = st->lds_floor;   // occupancy cap of the pass kernels (mi_debug_set_knob "ntt_lds_floor_kb")
    const u32 E = 1u << (p.log_r + p.log_c);
    // one butterfly per thread per stage when the tile allows: 64 KiB of LDS admits two workgroups per CU,
    // so 1024-thread workgroups are what fills the SIMDs (8 waves each) and hides the mad->addc chains
    u32 threads = E / 2 >= st->threads ? st->threads : (E / 2 >= 64 ? E / 2 : 64);
    if (wave && threads > 256) threads = 256;
    void (*const kernel)(Fr *, const Fr *, NttPass, NttTables) = wave ? k_ntt_pass_wave : k_ntt_pass;
    hipLaunchKernelGGL(kernel, dim3(ntt_tiles(p)), dim3(threads), lds_bytes, ctx->stream, dst, src, p, t);
    return ntt_launched(ctx);
}
// computeH's a and b: the inverse transform's last pass pi and the coset transform's first pass pf (the same contiguous tiles)
static int32_t launch_contig_pair(mi_ctx *ctx, Fr *v, const NttPass &pi, const NttTables &ti, const NttPass &pf, const NttTables &tf) {
    hipLaunchKernelGGL(k_ntt_contig_pair, dim3(ntt_tiles(pi)), dim3(256), ntt_lds_bytes(pi), ctx->stream, v, pi, ti, pf, tf);
    return ntt_launched(ctx);
}
// the coset transform's last pass pc of a and of b, the product, the last transform's first pass pl (the same strided tiles).
// radix 2^7: one wave per 128-row sub-block of the tile, 64 * 2^log_c threads (256 at the default 2^9-element tiles); radix 2^8: 256 threads
static int32_t launch_strided_triple(mi_ctx *ctx, Fr *a, const Fr *b, const NttPass &pc, const NttTables &tc, const NttPass &pl, const NttTables &tl) {
    const bool r7 = pc.log_r == 7;
    void (*const kernel)(Fr *, const Fr *, NttPass, NttTables, NttPass, NttTables) = r7 ? k_ntt_strided_triple : k_ntt_strided_triple8;
    hipLaunchKernelGGL(kernel, dim3(ntt_tiles(pc)), dim3(r7 ? 64u << pc.log_c : 256u), ntt_lds_bytes(pc), ctx->stream, a, b, pc, tc, pl, tl);
    return ntt_launched(ctx);
}
// the last transform's last pass pa and c's last pass pc (the same contiguous tiles): h = A - C.  The Z MSM's digit count rides along when
// prove.hip armed the hook and this launch's tiles are whole slices of that sort
static int32_t launch_contig_last_sub(mi_ctx *ctx, Fr *A, const Fr *C, const NttPass &pa, const NttTables &ta, const NttPass &pc, const NttTables &tc) {
    const size_t n = (size_t)1 << pa.log_n;
    const u32 E = 1u << (pa.log_r + pa.log_c);
    size_t lds_bytes = ntt_lds_bytes(pa);
    Msm2Shape zs{};
    bool count = ctx->zhook.armed && ctx->zhook.C1;
    if (count) {
        std::memcpy(&zs, ctx->zhook.shape, sizeof(zs));
        const size_t with_counters = lds_bytes + (size_t)(E / MSM2_SLICE) * zs.ngroups * 4;
        count = E % MSM2_SLICE == 0 && E / MSM2_SLICE <= 4 && zs.n <= n && (u64)zs.nslices * MSM2_SLICE == n && zs.c >= 17 && zs.c <= 22 && !zs.wkeys &&
                with_counters <= 160 * 1024;
        if (count) lds_bytes = with_counters;
    }
    ctx->zhook.armed = false;
    if (count) {
        hipLaunchKernelGGL(k_last_sub_count[zs.c - 17], dim3(ntt_tiles(pa)), dim3(256), lds_bytes, ctx->stream, A, C, pa, ta, pc, tc, zs, ctx->zhook.C1);
        ctx->zhook.done = true; ctx->zhook.h = A;
        ctx->z_count_fused_launches++;
    } else {
        hipLaunchKernelGGL(k_ntt_contig_last_sub, dim3(ntt_tiles(pa)), dim3(256), lds_bytes, ctx->stream, A, C, pa, ta, pc, tc);
    }
    return ntt_launched(ctx);
}
// passes [from, to) of a bound transform, one launch each: pass 0 reads src, every later one works on dst in place
static int32_t launch_passes(mi_ctx *ctx, const NttTransform &tr, Fr *dst, const Fr *src, u32 from, u32 to) {
    for (u32 i = from; i < to; i++) MI_TRY(launch_pass(ctx, dst, i == 0 ? src : dst, tr.pass[i], tr.t));
    return MI_OK;
}

// One fft.Domain transform of size 2^log_n, in place: build, bind, launch
int32_t mi_ntt_dev_impl(mi_ctx *ctx, mi_fr *inout_dev, uint32_t log_n, uint32_t flags) {
    MI_TRY(ensure_tables(ctx, log_n));
    NttTransform tr = ntt_build(state_of(ctx), log_n, flags, NTT_PLAIN, 1u << log_n);
    MI_TRY(ntt_bind(ctx, tr));
    MI_TRY(launch_passes(ctx, tr, (Fr *)inout_dev, (const Fr *)inout_dev, 0, tr.n_pass));
    ctx->stats.ntt_elems += (u64)1 << log_n;
    return MI_OK;
}

// computeH in four parts on ctx->stream, so that a caller whose inputs arrive one vector at a time (the host-pointer prove: a, b, c cross
// PCIe one after the other) can start a's transforms while b is still on the bus:
//   part 0 (src = a), part 1 (src = b)   N FFTInverse(., DIF) and the coset FFT up to (not including) its last pass when that pass runs in
//                                        the strided triple, else all of it; a lives in h_out, b in ws[WS_H_B]
//   part 2 (src = c)                     den FFTInverse(c, DIF) into ws[WS_H_C]; src2 != null: c is not given and is formed as src o src2 (the ORIGINAL a and b,
//                                        row by row) on the way into the first pass -- what c is for every witness gnark's solver accepts
//   part 3                               the strided triple (or the coset FFTs' last passes) and the last transform -> h_out
// The same launches as the one-call form, in an order that differs only between independent vectors: identical h.
//
// The schedule: the four distinct transforms, each built once and bound, and which of the three seams between them run as one launch.
// A part launches its slice of these lists by index.  (Built per part, not kept: the knobs may change between calls.)
struct ComputeHPlan {
    NttTransform inv, cos, cinv, last;   // N FFTInverse of a / b; their coset FFT; den FFTInverse of c; den FFTInverse on the coset (-> h)
    u32 pair, triple, last_sub;          // 1: that seam is fused
};
// what a fused kernel needs of the two passes it joins: the same tile, in LDS too
static bool same_tile(const NttPass &p, const NttPass &q) {
    return p.log_r == q.log_r && p.log_s == q.log_s && p.log_c == q.log_c && p.lds_pad == q.lds_pad;
}
// n_valid: the rows of a, b, c that are given; c_mul: the part's src2.  B, C: where b and c live by part 3
static int32_t compute_h_plan(mi_ctx *ctx, u32 log_n, u32 n_valid, const Fr *c_mul, const Fr *B, const Fr *C, ComputeHPlan &cp) {
    const NttState *st = state_of(ctx);
    cp.inv = ntt_build(st, log_n, NTT_INVERSE, NTT_INV_UNSCALED, n_valid);
    cp.cos = ntt_build(st, log_n, NTT_DIT | NTT_COSET, NTT_COSET_FWD_NINV, 1u << log_n);
    cp.cinv = ntt_build(st, log_n, NTT_INVERSE, NTT_INV_DEN_NINV, n_valid);   // (part 3 takes only its last pass, which reads whole tiles whatever n_valid)
    cp.last = ntt_build(st, log_n, NTT_INVERSE | NTT_COSET, NTT_COSET_INV_DEN, 1u << log_n);
    const u32 m = cp.last.n_pass;
    const bool seams = st->wave_stages && m >= 2;   // every fused kernel runs the register stages and joins two different passes
    const NttPass &strided = cp.last.pass[0], &contig = cp.last.pass[m - 1];
    // a and b: the contiguous last pass of the inverse transform and the contiguous first pass of the coset transform run as ONE
    // launch on the same tiles (k_ntt_contig_pair) when the plan has such a pair of radix >= 2^7
    cp.pair = seams && st->fuse_pair && same_tile(cp.inv.pass[m - 1], cp.cos.pass[0]) && contig.log_r >= 7;
    // The coset FFT's LAST pass (of a and of b), the product and the last transform's FIRST pass share their strided tiles: one
    // launch when that pass has radix 2^7 (one wave per 128-row sub-block, up to 512 threads) or 2^8 (k_ntt_strided_triple8: 256 threads,
    // 1 or 2 pairs at distance 128 each)
    cp.triple = seams && st->fuse_triple && same_tile(cp.cos.pass[m - 1], strided) &&
                ((strided.log_r == 7 && strided.log_c <= 3) || (strided.log_r == 8 && strided.log_c >= 1 && strided.log_c <= 2));
    // c's last pass and the last transform's last pass, which subtracts it: one launch (k_ntt_contig_last_sub) at radix >= 2^7 and at
    // most four elements per thread
    cp.last_sub = seams && st->fuse_last && same_tile(cp.cinv.pass[m - 1], contig) && contig.log_r >= 7 && (1u << (contig.log_r + contig.log_c)) <= 4 * 256;
    // the product a b is taken on the way into the last transform's first pass and c subtracted on the way out of its last (no pointwise
    // kernel, no extra round trip through HBM), unless the fused kernel at that end does it
    MI_TRY(ntt_bind(ctx, cp.inv));
    MI_TRY(ntt_bind(ctx, cp.cos));
    MI_TRY(ntt_bind(ctx, cp.cinv, c_mul));
    return ntt_bind(ctx, cp.last, cp.triple ? nullptr : B, cp.last_sub ? nullptr : C);
}
int32_t mi_compute_h_part(mi_ctx *ctx, uint32_t log_n, int part, const mi_fr *src, size_t n_constraints, mi_fr *h_out, const mi_fr *src2) {
    static const char *const range_names[4] = {"mi.computeH.a.enqueue", "mi.computeH.b.enqueue", "mi.computeH.c.enqueue", "mi.computeH.last.enqueue"};
    const MiRange range(range_names[part & 3]);
    const u64 n = (u64)1 << log_n;
    // gnark's computeH (7 transforms): a, b, c <- FFTInverse; a, b, c <- FFT on the coset; a <- (a b - c) den; h <- FFTInverse on
    // the coset.  The last transform is linear and undoes the coset FFT of c exactly:
    //     h = cosetFFTInverse((ca cb - cc) den) = den cosetFFTInverse(ca cb) - den FFTInverse(c),
    // so the coset FFT of c is never computed -- SIX transforms, the same field elements (exact arithmetic), for ANY a, b, c.
    MI_TRY(ensure_tables(ctx, log_n));
    MI_TRY(ensure_direct(ctx, log_n));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_H_B], n * sizeof(Fr)));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_H_C], n * sizeof(Fr)));
    Fr *A = (Fr *)h_out, *B = (Fr *)ctx->ws[WS_H_B].p, *C = (Fr *)ctx->ws[WS_H_C].p;
    ComputeHPlan cp;
    MI_TRY(compute_h_plan(ctx, log_n, (u32)n_constraints, (const Fr *)src2, B, C, cp));
    const u32 m = cp.last.n_pass;
    if (part == 0 || part == 1) {
        // v <- N FFTInverse(v, DIF) (zero padding fused into the first pass's load; the 1/N rides in the coset shift), then
        // v <- FFT(v, DIT, OnCoset) without its last pass when that one runs in the triple
        Fr *v = part == 0 ? A : B;
        MI_TRY(launch_passes(ctx, cp.inv, v, (const Fr *)src, 0, m - cp.pair));
        if (cp.pair) MI_TRY(launch_contig_pair(ctx, v, cp.inv.pass[m - 1], cp.inv.t, cp.cos.pass[0], cp.cos.t));
        MI_TRY(launch_passes(ctx, cp.cos, v, v, cp.pair, m - cp.triple));
        ctx->stats.ntt_elems += 2 * n;
    } else if (part == 2) {
        // c <- den FFTInverse(c, DIF) (one constant den / N on the way out), bit-reversed like h; its last pass waits for part 3 when fused
        MI_TRY(launch_passes(ctx, cp.cinv, C, (const Fr *)src, 0, m - cp.last_sub));
        ctx->stats.ntt_elems += n;
    } else {
        // h <- den FFTInverse(a b, DIF, OnCoset) - c, left bit-reversed like gnark
        if (cp.triple) MI_TRY(launch_strided_triple(ctx, A, B, cp.cos.pass[m - 1], cp.cos.t, cp.last.pass[0], cp.last.t));
        MI_TRY(launch_passes(ctx, cp.last, A, A, cp.triple, m - cp.last_sub));
        if (cp.last_sub) MI_TRY(launch_contig_last_sub(ctx, A, C, cp.last.pass[m - 1], cp.last.t, cp.cinv.pass[m - 1], cp.cinv.t));
        ctx->stats.ntt_elems += n;
    }
    return MI_OK;
}
int32_t mi_compute_h_dev_impl(mi_ctx *ctx, uint32_t log_n, const mi_fr *a, const mi_fr *b, const mi_fr *c,
                              size_t n_constraints, mi_fr *h_out) {
    MI_TRY(mi_compute_h_part(ctx, log_n, 0, a, n_constraints, h_out));
    MI_TRY(mi_compute_h_part(ctx, log_n, 1, b, n_constraints, h_out));
    if (c) MI_TRY(mi_compute_h_part(ctx, log_n, 2, c, n_constraints, h_out));
    else MI_TRY(mi_compute_h_part(ctx, log_n, 2, a, n_constraints, h_out, b));   // c = a o b, formed on the device
    return mi_compute_h_part(ctx, log_n, 3, nullptr, n_constraints, h_out);
}

static void stats_begin(mi_ctx *ctx) { std::memset(&ctx->stats, 0, sizeof(ctx->stats)); }

extern "C" {
int32_t mi_debug_set_ntt_plan(mi_ctx *ctx, uint32_t log_e, uint32_t max_contig, uint32_t max_strided) {
    if (!ctx || log_e < 1 || log_e > 12 || max_contig < 1 || max_contig > 12 || max_contig > log_e || max_strided < 1 || max_strided > 12 || max_strided > log_e)
        return MI_EINVAL;
    NttState *st = state_of(ctx);
    st->log_e = log_e; st->max_contig = max_contig; st->max_strided = max_strided; st->plan_set = 1;
    return MI_OK;
}
int32_t mi_debug_set_ntt_wave_stages(mi_ctx *ctx, uint32_t on, uint32_t direct_min_log_n) {
    if (!ctx || on > 1) return MI_EINVAL;
    NttState *st = state_of(ctx);
    st->wave_stages = on; st->direct_min_log_n = direct_min_log_n;
    st->d_npass = 0;   // force the next computeH to re-decide about its direct tables
    return MI_OK;
}
int32_t mi_debug_set_ntt_fuse_pair(mi_ctx *ctx, uint32_t on) {
    if (!ctx || on > 7) return MI_EINVAL;
    state_of(ctx)->fuse_pair = on & 1u;          // bit 0: the contiguous pair (k_ntt_contig_pair)
    state_of(ctx)->fuse_triple = (on >> 1) & 1u;  // bit 1: the strided triple (k_ntt_strided_triple)
    state_of(ctx)->fuse_last = (on >> 2) & 1u;    // bit 2: c's last pass + the last transform's last pass (k_ntt_contig_last_sub)
    return MI_OK;
}
int32_t mi_debug_set_ntt_threads(mi_ctx *ctx, uint32_t threads) {
    if (!ctx || threads < 64 || threads > 1024 || (threads & (threads - 1))) return MI_EINVAL;
    state_of(ctx)->threads = threads;
    return MI_OK;
}
int32_t mi_ntt_dev(mi_ctx *ctx, mi_fr *inout_dev, uint32_t log_n, uint32_t flags) {
    if (!ctx || !inout_dev || log_n > 28 || (flags & ~7u)) return MI_EINVAL;
    stats_begin(ctx);
    MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_T0], ctx->stream));
    MI_TRY(mi_ntt_dev_impl(ctx, inout_dev, log_n, flags));
    MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_T1], ctx->stream));
    MI_CHECK_HIP(ctx, hipEventSynchronize(ctx->ev[EV_T1]));
    MI_CHECK_HIP(ctx, hipEventElapsedTime(&ctx->stats.ntt_kernel_ms, ctx->ev[EV_T0], ctx->ev[EV_T1]));
    return MI_OK;
}
int32_t mi_ntt(mi_ctx *ctx, mi_fr *inout, uint32_t log_n, uint32_t flags) {
    if (!ctx || !inout || log_n > 28 || (flags & ~7u)) return MI_EINVAL;
    size_t bytes = sizeof(Fr) << log_n;
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_HOST_IO0], bytes));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(ctx->ws[WS_HOST_IO0].p, inout, bytes, hipMemcpyHostToDevice, ctx->stream));
    MI_TRY(mi_ntt_dev(ctx, (mi_fr *)ctx->ws[WS_HOST_IO0].p, log_n, flags));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(inout, ctx->ws[WS_HOST_IO0].p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}
int32_t mi_compute_h_dev(mi_ctx *ctx, uint32_t log_n, const mi_fr *a, const mi_fr *b, const mi_fr *c,
                         size_t n_constraints, mi_fr *h_out) {
    if (!ctx || !a || !b || !h_out || log_n > 28 || n_constraints > ((size_t)1 << log_n)) return MI_EINVAL;   // c may be null: c = a o b
    stats_begin(ctx);
    MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_T0], ctx->stream));
    MI_TRY(mi_compute_h_dev_impl(ctx, log_n, a, b, c, n_constraints, h_out));
    MI_CHECK_HIP(ctx, hipEventRecord(ctx->ev[EV_T1], ctx->stream));
    MI_CHECK_HIP(ctx, hipEventSynchronize(ctx->ev[EV_T1]));
    MI_CHECK_HIP(ctx, hipEventElapsedTime(&ctx->stats.compute_h_ms, ctx->ev[EV_T0], ctx->ev[EV_T1]));
    ctx->stats.ntt_kernel_ms = ctx->stats.compute_h_ms;
    return MI_OK;
}
int32_t mi_compute_h(mi_ctx *ctx, uint32_t log_n, const mi_fr *a, const mi_fr *b, const mi_fr *c,
                     size_t n_constraints, mi_fr *h_out) {
    if (!ctx || !a || !b || !h_out || log_n > 28 || n_constraints > ((size_t)1 << log_n)) return MI_EINVAL;   // c may be null: c = a o b
    size_t nb = n_constraints * sizeof(Fr), full = sizeof(Fr) << log_n;
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_HOST_IO0], full));
    MI_TRY(mi_reserve(ctx, ctx->ws[WS_HOST_IO1], nb * 3 + 96));
    char *in = (char *)ctx->ws[WS_HOST_IO1].p;
    MI_CHECK_HIP(ctx, hipMemcpyAsync(in, a, nb, hipMemcpyHostToDevice, ctx->stream));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(in + nb, b, nb, hipMemcpyHostToDevice, ctx->stream));
    if (c) MI_CHECK_HIP(ctx, hipMemcpyAsync(in + 2 * nb, c, nb, hipMemcpyHostToDevice, ctx->stream));
    MI_TRY(mi_compute_h_dev(ctx, log_n, (mi_fr *)in, (mi_fr *)(in + nb), c ? (mi_fr *)(in + 2 * nb) : nullptr, n_constraints, (mi_fr *)ctx->ws[WS_HOST_IO0].p));
    MI_CHECK_HIP(ctx, hipMemcpyAsync(h_out, ctx->ws[WS_HOST_IO0].p, full, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}
}
