/* mi355x_groth16_debug.h -- NOT part of the surface a maintainer binds: synthetic-input generators, throughput probes, plan / schedule
 * knobs, counters, tracing and fault injection of libmi355x_groth16.so.  For tests/, bench.py and tools/ only (the product
 * header no longer carries the lab bench).  Nothing here changes a result. */
#ifndef MI355X_GROTH16_DEBUG_H
#define MI355X_GROTH16_DEBUG_H
#include "mi355x_groth16.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device-side test / bench utilities (not part of the reference surface) ---- */
#define MI_DIST_UNIFORM 0
#define MI_DIST_WHIR 1      /* 45% {0,1}, 25% bytes, 5% 64-bit, 25% uniform */
/* any other mix: per-mille shares of {0,1} / bytes / 64-bit values, the rest uniform Fr (each share <= 1000, their sum <= 1000).
 * tools/wire_census.py derives the shares the reference's circuit implies (profiles/r06_wire_census.txt). */
#define MI_DIST_MIX_FLAG 0x40000000
#define MI_DIST_MIX(bit_pm, byte_pm, u64_pm) (MI_DIST_MIX_FLAG | ((bit_pm) << 20) | ((byte_pm) << 10) | (u64_pm))
int32_t mi_gen_scalars_dev(mi_ctx *ctx, mi_fr *out_dev, size_t n, uint64_t seed, int dist);
int32_t mi_gen_g1_dev(mi_ctx *ctx, mi_g1_affine *out_dev, size_t n, uint64_t seed);
int32_t mi_gen_g2_dev(mi_ctx *ctx, mi_g2_affine *out_dev, size_t n, uint64_t seed);
/* elementwise field ops for parity tests of the device field layer:
 * field: 0 = Fr, 1 = Fp; op: 0 add, 1 sub, 2 mul, 3 inv(x), 4 to_mont(x), 5 from_mont(x),
 * 6 (xy + yx)/R and 7 (xy - yy)/R through the dual-product multiplier, 8 x^2 */
int32_t mi_field_op_dev(mi_ctx *ctx, int field, int op, void *z_dev, const void *x_dev,
                        const void *y_dev, size_t n);
/* out[i] = a[i] + b[i] on G1 (affine in, affine out; exercises add/double/inf cases) */
int32_t mi_g1_add_dev(mi_ctx *ctx, mi_g1_affine *out_dev, const mi_g1_affine *a_dev,
                      const mi_g1_affine *b_dev, size_t n);
int32_t mi_g2_add_dev(mi_ctx *ctx, mi_g2_affine *out_dev, const mi_g2_affine *a_dev,
                      const mi_g2_affine *b_dev, size_t n);
/* the 29-bit-limb arithmetic of the level-1 bucket accumulation (csrc/field29.cuh, curve29.cuh, curve29_g2.cuh), one record per lane:
 * in_dev holds n records of MI_LIMB29_IN_WORDS u32, out_dev receives n of MI_LIMB29_OUT_WORDS (words an op does not write are zero).  op and
 * layout are those of csrc/limb29_ops.cuh, which the host build of the tests runs too: 0..16 the primitives over Fp, 20..22 the G1 steps
 * (mixed addition, full addition of a stored partial sum, store + load), 23..25 the G2 steps through the level kernels' LDS accumulator.
 * Every input must meet the documented contract of its primitive.  MI_EINVAL for an unknown op, null buffers or n > 2^30. */
#define MI_LIMB29_IN_WORDS 144
#define MI_LIMB29_OUT_WORDS 80
int32_t mi_debug_limb29_op_dev(mi_ctx *ctx, int op, void *out_dev, const void *in_dev, size_t n);
/* the lazy 8 x 32-bit arithmetic under every NTT stage (csrc/field.cuh fe_add_nored / fe_sub_plus2p / fe_condsub_2p / fe_canon / fe_mul_lazy,
 * csrc/ntt_tile.cuh ntt_bfly_dif / ntt_bfly_dit / ntt_mul_lazy2 and the store_sub expression), over Fr, one record per lane: in_dev holds n
 * records of MI_LAZY_IN_WORDS u32 (x | y | w, eight limbs each), out_dev receives n of MI_LAZY_OUT_WORDS (two results of eight limbs; words an
 * op does not write are zero).  op and layout are those of csrc/lazy_ops.cuh, which the host build of the tests runs too: 0 add_nored,
 * 1 sub_plus2p, 2 condsub_2p, 3 canon, 4 mul_lazy, 5 mul_lazy2, 6 / 7 the DIF butterfly with / without a twiddle, 8 / 9 the DIT butterfly,
 * 10 store_sub.  Every input must meet the documented contract of its primitive.  MI_EINVAL for an unknown op, null buffers or n > 2^30. */
#define MI_LAZY_IN_WORDS 24
#define MI_LAZY_OUT_WORDS 16
int32_t mi_debug_lazy_op_dev(mi_ctx *ctx, int op, void *out_dev, const void *in_dev, size_t n);
/* the field arithmetic on operand shapes the compiler can see through -- literal factors, limbs that are provably zero, one value in two
 * operand positions, results written over their inputs, chains that start at a literal (csrc/shape_ops.cuh) -- one record per lane: in_dev
 * holds n records of MI_SHAPE_IN_WORDS u32 (x | y | u | v, eight limbs each; the curve, 29-bit and Fp12 shapes read the same words as
 * csrc/shape_ops.cuh states), out_dev receives n of MI_SHAPE_OUT_WORDS (words a shape does not write are zero).  Every shape is a kernel of
 * its own, so its body is compiled as its call site in the product is; the host build of the tests runs the same bodies.  shape: a
 * generic shape g of csrc/shape_ops.cuh over Fr is g, over Fp SHG_END + g, a typed shape t is 2 SHG_END + t.  Inputs are raw Montgomery
 * residues below the modulus (points on their curves, 29-bit limbs within the contract of csrc/field29.cuh).  No kernel has a
 * data-dependent address or trip count.  MI_EINVAL for an unknown shape, null buffers or n > 2^24. */
#define MI_SHAPE_IN_WORDS 32
#define MI_SHAPE_OUT_WORDS 32
int32_t mi_debug_field_shape_dev(mi_ctx *ctx, int shape, void *out_dev, const void *in_dev, size_t n);
/* the pairing behind mi355x_groth16_verify.h (csrc/fp12.cuh, pairing.cuh), one record per lane; the host build of the tests
 * (tests/emu/emu_pairing.cpp) runs the same bodies.  An Fp12 / GT record is 12 x mi_fp in the tower order C0.B0.A0, C0.B0.A1, C0.B1.A0,
 * ... C1.B2.A1 (Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3 - (9+u)), Fp12 = Fp6[w]/(w^2 - v)).
 * mi_debug_pairing_dev: gt_dev[i] = the Miller value of (p_dev[i], q_dev[i]) (flags = 0) or the pairing value f^d' (MI_PAIRING_FINAL_EXP),
 * d' = s (p^12 - 1) / r with s = 2 x0 (6 x0^2 + 3 x0 + 1) as csrc/pairing.cuh states it; 1 when either point is infinity.  The points must
 * lie on their curves, q in the r-torsion (not checked here).
 * mi_debug_fp12_op_dev: z[i] = op(x[i], y[i]); op as in csrc/pairing_ops.cuh: 0 mul, 1 sqr, 2 inv, 3 / 4 / 5 Frobenius p / p^2 / p^3,
 * 6 cyclotomic square, 7 conjugate, 8 easy part, 9 final exponentiation, 10 product by the sparse line (y.C0.B0, y.C1.B0, y.C1.B1),
 * 11 add, 12 sub, 13 / 14 / 15 the Fp6 product / square / inverse on both halves.  y_dev may be NULL for the one-operand ops.
 * MI_EINVAL for an unknown op or flag, null buffers or n > 2^24. */
#define MI_PAIRING_FINAL_EXP 1u
#define MI_FP12_WORDS 96
int32_t mi_debug_pairing_dev(mi_ctx *ctx, const mi_g1_affine *p_dev, const mi_g2_affine *q_dev, size_t n, mi_fp *gt_dev, uint32_t flags);
int32_t mi_debug_fp12_op_dev(mi_ctx *ctx, int op, mi_fp *z_dev, const mi_fp *x_dev, const mi_fp *y_dev, size_t n);
/* The same two with ONE WAVE per record (csrc/fp12_wave.cuh, pairing_wave.cuh; the host build of the tests: tests/emu/
 * emu_pairing_wave.cpp): the arguments, op numbers, flags and refusals of mi_debug_pairing_dev / mi_debug_fp12_op_dev, and word for word
 * their results -- the grid is n single-wave workgroups.  Inversion and the Fp6 ops run in one lane of the wave.
 * mi_debug_verify_wave_split: mi_groth16_verify_wave (mi355x_groth16_verify_wave.h) with its time split into MI_VERIFY_WAVE_SPLIT_PHASES
 * phases, in ms: [0] the host stage with the MSM calls (wall clock), then by events on the context's stream [1] the Bs checks, [2] the
 * Miller loops, [3] the judgement with the verdict bytes, [4] the copy back.  To be timed apart the checks and the Miller loops go as two
 * launches here; the product call sends them as one.  MI_EINVAL also for a null split pointer. */
#define MI_VERIFY_WAVE_SPLIT_PHASES 5
int32_t mi_debug_pairing_wave_dev(mi_ctx *ctx, const mi_g1_affine *p_dev, const mi_g2_affine *q_dev, size_t n, mi_fp *gt_dev, uint32_t flags);
int32_t mi_debug_fp12_op_wave_dev(mi_ctx *ctx, int op, mi_fp *z_dev, const mi_fp *x_dev, const mi_fp *y_dev, size_t n);
struct mi_vk; struct mi_verify_input;
int32_t mi_debug_verify_wave_split(mi_ctx *ctx, const struct mi_vk *vk, const struct mi_verify_input *in, size_t n, uint8_t *verdicts, float *split_ms);
/* The pairs of a staged batch: what mi_groth16_verify_batch and mi_groth16_verify_wave hand to their Miller loops for these inputs, before
 * the check of Bs.  p_out, q_out: HOST arrays of n x (3, or 4 + n_commitments with commitments) points in the order of
 * csrc/pairing_ops.cuh (verify_assemble); a proof that is not well formed has infinities.  The stage is the one the knob "verify_ksum"
 * selects, so the two stages can be compared word for word.  The refusals of mi_groth16_verify_batch under the prefix "verify pairs: ". */
int32_t mi_debug_verify_pairs_dev(mi_ctx *ctx, const struct mi_vk *vk, const struct mi_verify_input *in, size_t n, mi_g1_affine *p_out, mi_g2_affine *q_out);
/* the decoders and the hash behind mi355x_groth16_verify_bytes.h (csrc/decode_ops.cuh, sha256_h2f.cuh), one record per lane; the host
 * build of the tests (tests/emu/emu_decode.cpp) runs the same bodies.  All pointers are DEVICE pointers; the launches go to the context's
 * stream (mi_dev_sync before reading).
 * mi_debug_decode_g1_dev / _g2_dev: n compressed encodings of 32 / 64 bytes back to back -> n points and n bytes, 1 = malformed (the point
 * is then (0, 0)).
 * mi_debug_hash_to_field_dev: n messages of msg_len bytes back to back and ONE dst of dst_len bytes (1 .. 255) -> n Montgomery mi_fr.
 * MI_EINVAL for null buffers, a dst_len out of range or n > 2^24. */
int32_t mi_debug_decode_g1_dev(mi_ctx *ctx, const uint8_t *enc_dev, size_t n, mi_g1_affine *out_dev, uint8_t *bad_dev);
int32_t mi_debug_decode_g2_dev(mi_ctx *ctx, const uint8_t *enc_dev, size_t n, mi_g2_affine *out_dev, uint8_t *bad_dev);
int32_t mi_debug_hash_to_field_dev(mi_ctx *ctx, const uint8_t *dst_dev, uint32_t dst_len, const uint8_t *msgs_dev, size_t msg_len, size_t n, mi_fr *out_dev);
/* the decoder of the public witness behind mi_groth16_verify_files* (mi355x_groth16_vkfile.h; csrc/witness_ops.cuh, one value per lane;
 * the host build tests/emu/emu_witness.cpp runs the same body).  Device pointers of any alignment, enqueued on the context's stream.
 * values_dev: n witnesses of n_pub values of 32 bytes, big-endian, back to back (no headers) -> out_dev, n x n_pub Montgomery mi_fr; a
 * value not below r leaves zero and sets bad_dev[i] of its witness.  The kernel only ever sets a byte: clear bad_dev first.
 * MI_EINVAL for null buffers, n > 2^24 or n * n_pub > 2^32. */
int32_t mi_debug_witness_decode_dev(mi_ctx *ctx, const uint8_t *values_dev, size_t n, uint32_t n_pub, mi_fr *out_dev, uint8_t *bad_dev);

/* the two kernels mi355x_groth16_verify_combined.h adds in front of and behind the Miller loops (csrc/verify_combined.hip), alone; the
 * host build of the tests (tests/emu/emu_verify_combined.cpp) runs the same bodies.  Device pointers, enqueued on the context's stream.
 * mi_debug_fp12_product_dev: out_dev[0] = x_dev[0] x_dev[1] ... x_dev[n - 1], Fp12 records of 12 x mi_fp, by the verifier's tree (fan-in
 * 8, one launch per level; its scratch is the context's verifier workspace).  1 <= n <= 2^24 + 3, the most the verifier multiplies.
 * mi_debug_g1_scale128_dev: out_dev[i] = k_i p_dev[i], affine, k_i = k_dev[2 i] + 2^64 k_dev[2 i + 1] (a plain integer below 2^128);
 * (0, 0) = infinity in and out.  out_dev may be p_dev.  The points must lie on the curve. */
int32_t mi_debug_fp12_product_dev(mi_ctx *ctx, const mi_fp *x_dev, size_t n, mi_fp *out_dev);
int32_t mi_debug_g1_scale128_dev(mi_ctx *ctx, const mi_g1_affine *p_dev, const uint64_t *k_dev, size_t n, mi_g1_affine *out_dev);
/* the kernels mi355x_groth16_verify_locate.h adds (csrc/verify_locate.hip), alone; the host build of the tests
 * (tests/emu/emu_verify_locate.cpp) runs the same bodies.  Device pointers, enqueued on the context's stream, 1 <= n <= 2^24.
 * mi_debug_g1_sum_tree_dev: levels_dev receives every level above p_dev's of the sum tree of fan-in 8 over the n affine points, level 1
 * first: ceil(n / 8) points, then ceil of that / 8, ... down to one (n = 1: one level of one point); (0, 0) = infinity in and out.
 * mi_debug_locate_points_dev: one lane per proof, out_dev[a * n + i] = array a of proof i: 0: r Krs; with nc > 0 1: r sum_k C_k, 2: r pok;
 * with nc > 1 3 + k: (r c^k) C_k.  r_dev: n x 2 words as mi_debug_g1_scale128_dev's k_dev; cm_dev: n x nc points; fold_dev: n
 * scalars, read with nc > 1 only; pok_dev and cm_dev are read with nc > 0 only.  nc <= 16.
 * mi_debug_locate_colsums_dev: sums_dev[t * (ns + 1) + j] = sum of r_i scal_dev[i * ns + j] over the proofs i of node (level,
 * nodes_dev[t]) of the tree over n proofs, column ns = sum of r_i; m nodes, every one below the level's count; r_dev: n canonical
 * mi_fr records below 2^128.  Its partials live in the context's locate workspace.
 * mi_debug_set_locate_round_nodes: the node budget of one round of mi_groth16_verify_locate's descent on this context; 0 restores the
 * default (MI_LOCATE_ROUND_NODES).  Tests force deep descents at small n with it. */
int32_t mi_debug_g1_sum_tree_dev(mi_ctx *ctx, const mi_g1_affine *p_dev, size_t n, mi_g1_affine *levels_dev);
int32_t mi_debug_locate_points_dev(mi_ctx *ctx, const uint64_t *r_dev, const mi_g1_affine *krs_dev, const mi_g1_affine *cm_dev, const mi_g1_affine *pok_dev,
                                   const mi_fr *fold_dev, uint32_t nc, size_t n, mi_g1_affine *out_dev);
int32_t mi_debug_locate_colsums_dev(mi_ctx *ctx, const mi_fr *scal_dev, uint32_t ns, const mi_fr *r_dev, size_t n, uint32_t level, const uint32_t *nodes_dev,
                                    size_t m, mi_fr *sums_dev);
int32_t mi_debug_set_locate_round_nodes(mi_ctx *ctx, uint32_t cap);
/* random-gather throughput probe: n_threads lanes each chain `iters` dependent 64-byte gathers from a table of n_entries
 * (a power of two) 64-byte entries; scratch: 1 KiB.  The ceiling the level-1 bucket accumulation's point gathers run against. */
int32_t mi_bench_gather_dev(mi_ctx *ctx, const void *table_dev, size_t n_entries, size_t n_threads, uint32_t iters,
                            void *scratch_dev, float *ms_out);
/* modular-multiply throughput probe: chains `iters` dependent Fp products per thread */
int32_t mi_bench_modmul_dev(mi_ctx *ctx, int field, size_t n_threads, uint32_t iters,
                            void *scratch_dev, float *ms_out);
/* raw VALU issue-rate probe (the integer-MAC ceiling SURVEY 8d asks to report beside the MSM):
 * kind 0 = 32x32+64 mad, 1 = mul_lo+mul_hi u32, 2 = fma f64, 3 = 24-bit mul+add, 4 = 64-bit add;
 * each thread runs 8 independent chains x iters steps */
int32_t mi_bench_valu_dev(mi_ctx *ctx, int kind, size_t n_threads, uint32_t iters,
                          void *scratch_dev, float *ms_out);
/* tuning / test knobs (0 = automatic).  NTT: tile = 2^log_e elements, radix caps of the contiguous and the
 * strided passes, threads per workgroup.  MSM: window bits c (2..16), item sizes of level 1 / later levels,
 * bucket-reduce segment, slices per window.  Tests use them to force multi-pass / multi-level paths at small n. */
int32_t mi_debug_set_ntt_plan(mi_ctx *ctx, uint32_t log_e, uint32_t max_contig, uint32_t max_strided);
int32_t mi_debug_set_ntt_threads(mi_ctx *ctx, uint32_t threads);
/* on = 1 (default): passes of radix >= 2^7 run seven of their stages in registers (wavefront butterflies); 0: every stage through
 * LDS.  direct_min_log_n: computeH builds its data-layout twiddle / coset tables from this size on (default 12; 29 = never). */
int32_t mi_debug_set_ntt_wave_stages(mi_ctx *ctx, uint32_t on, uint32_t direct_min_log_n);
/* Fused launches of computeH, a bit mask (default 7 = all).  Bit 0: the contiguous last pass of FFTInverse(a | b) and the contiguous
 * first pass of the coset FFT that follows run as one launch on the same tiles (csrc/ntt.hip k_ntt_contig_pair).  Bit 1: the strided
 * last pass of the coset FFT of a and of b, the product a b and the strided first pass of the last transform run as one launch
 * (k_ntt_strided_triple; plans whose first radix is 2^7 or 2^8).  Bit 2: the last pass of den FFTInverse(c) and the last pass of the last
 * transform, which subtracts it, run as one launch (k_ntt_contig_last_sub).  Same h whatever the mask; parity tests run the combinations. */
int32_t mi_debug_set_ntt_fuse_pair(mi_ctx *ctx, uint32_t on);
int32_t mi_debug_set_msm_plan(mi_ctx *ctx, uint32_t c, uint32_t L1, uint32_t L2, uint32_t seg, uint32_t G);
int32_t mi_debug_set_msm_chunk(mi_ctx *ctx, uint32_t chunk);   /* fixed-base sort: entries per pass-2 chunk */
int32_t mi_debug_set_msm_group_bits(mi_ctx *ctx, uint32_t gbits);   /* fixed-base sort: log2 buckets per pass-1 group, 6..15 */
/* window widths of the fixed-base tables the NEXT mi_pk_load[_dev] on ctx builds for the MSM groups A+K, B1+B2, Z:
 * 0 = automatic (tables when the MSM has >= 2^20 points and they fit in a third of the free device memory),
 * 1 = never, 17..22 = that width whatever the size */
int32_t mi_debug_set_prove_fixed_base(mi_ctx *ctx, uint32_t c_ak, uint32_t c_b, uint32_t c_z);
/* hold_accum = 1: inside a prove whose inputs are in HBM the wire MSMs (A, B1, B2, K) sort at once but start their bucket
 * accumulations only when computeH is done; 0 (default): everything as soon as its inputs exist.  Same proofs.  Measured neutral on
 * throughput and 0.4 ms worse on the single-proof latency (a proof alone is work-bound, not schedule-bound: DESIGN.md 7b). */
int32_t mi_debug_set_prove_schedule(mi_ctx *ctx, uint32_t hold_accum);
/* on = 0 (default): an MSM runs as many item levels as the fullest bucket of its sort needs (one 4-byte read-back per sort, waited for on the
 * thread that enqueues the accumulation); 1: as many as the worst case would (every entry in one bucket).  Same sums; parity tests run both. */
int32_t mi_debug_set_msm_bound_levels(mi_ctx *ctx, uint32_t on);
/* 1: generic MSMs of >= 2^18 pairs keep the one-pass counting sort instead of the LDS-staged two-pass one (parity tests run both) */
int32_t mi_debug_set_msm_one_pass_sort(mi_ctx *ctx, uint32_t on);
/* on = 1 (default): the G1 level-1 bucket accumulation runs in nine 29-bit limbs (keys loaded afterwards keep their G1 points in
 * the matching packed form) and the G1 partial sums between the levels stay in that form; 2: the same level 1 with standard-form
 * partial sums; 0: the 8 x 32-bit kernels everywhere.  Set before mi_pk_load; parity tests run all three. */
int32_t mi_debug_set_msm_limb29(mi_ctx *ctx, uint32_t on);
/* 3 (default) or 2: which build of the G1 level-1 29-bit kernel runs -- three waves per SIMD (fastest alone, shortest launches) or two
 * (leaves registers for other kernels' waves on the same SIMD: +1.7 % proofs/s with three proofs in flight at N = 2^23, slower when
 * one proof fills the GPU).  Same results. */
int32_t mi_debug_set_msm_l1_waves(mi_ctx *ctx, uint32_t waves);
/* EXPERIMENT, default 0 (off).  rounds = 1..4: the G1 level-1 accumulation by batch-affine rounds (affine additions, one shared inversion
 * per 64 * K additions; csrc/msm_ba_g1.cuh) wherever the buckets hold >= 32 entries on average and the scratch (768 B per item) fits.
 * 32 % fewer multiplications per addition, the same results -- and half the speed on MI355X: every pass is bound by its random 64-byte
 * reads at ~3 TB/s.  Kept for the measurement and the parity test. */
int32_t mi_debug_set_msm_batch_affine(mi_ctx *ctx, uint32_t rounds);
/* on = 1 (default): the fixed-base window tables of mi_pk_load / mi_msm_precompute_* convert to affine with one inversion per 16 points
 * (needs n XYZZ + n coordinates of scratch while building; falls back by itself without room); 0: one inversion per point.  Same tables. */
int32_t mi_debug_set_msm_precompute_batched(mi_ctx *ctx, uint32_t on);
/* Named measurement / test knobs of one context (the switches that are not worth an entry point each; none changes a result).
 * MI_EINVAL for an unknown name or a value out of range.  The library reads NO environment variable for any of this: the only
 * variables it looks at are MI_GROUP_TIMEOUT_MS and MI_GROUP_SHM_CHUNK_KB of the device groups (documented at mi_group_create_rank_ex).
 *   "l1_wg" 1 | 2 | 4        waves per workgroup of the G1 level-1 bucket-accumulate kernel, default 4 (a workgroup takes one slot on each
 *                            SIMD of a CU and returns them together, so the other streams' multi-wave workgroups find room)
 *   "g2_wg" 1 | 2 | 4        the same for the G2 level-1 kernel (each wave has its own 18 KiB LDS accumulator image)
 *   "l1_waves" 2 | 3         = mi_debug_set_msm_l1_waves
 *   "z_waves" 0 | 2          2: the Z MSM's level-1 launch alone on the two-waves-per-SIMD build
 *   "g1_grid_per_cu", "g2_grid_per_cu"   resident-grid cap per CU of the level-1 launches, in waves (0 = 128)
 *   "count_per" 0..64        fixed-base sort: slices per counting workgroup (0 = 32)
 *   "plain_scatter" 0 | 1    fixed-base sort: pass 2 by the plain scatter instead of the LDS-staged one
 *   "finisher" 0 | 1         1 (default): once no bucket holds more than "finisher_max" partial sums the item levels end in ONE launch
 *                            (k_msm_finish_keys) instead of log_8 more levels of three launches each
 *   "z_count_fused" 0 | 1     1 (default): inside a proof the Z MSM's sort takes its digit count from computeH's last launch (the kernel that
 *                            stores h counts the digits of what it stores: h is read once less) instead of a count pass of its own.  Same
 *                            proofs; throughput equal (the count's instructions move, they do not go away), one proof alone 0.1-0.2 ms shorter
 *   "flat_item_l1" 0 | 1 | 4..64   entries per level-1 item of a FLAT sort (fullest bucket <= 2 x the average: uniform scalars, e.g. the h
 *                            coefficients of a proof's Z MSM).  0 (default) = automatic: average / L2^k where that falls into 17..32 (26 at
 *                            N = 2^23), so that the levels above are full L2-ary trees; 1 = off (the plan's L1); 4..64 = forced
 *   "dense_item_l1" 0 | 1 | 4..64   entries per level-1 item of a DENSE sort that is not flat (>= half of the n x windows digits non-zero: the wire
 *                            values of a witness of mostly full-width field elements, what the reference's circuit implies).  0 (default) = automatic
 *                            (32: half the partial sums for the upper levels); 1 = off (the plan's L1 = 16); 4..64 = forced
 *   "finisher_max" 0..2^20   0 = automatic (G1 4096, G2 1024)
 *   "finisher_min_level" 0..16   the finisher follows accumulate pass number this + 1 at the earliest (default 2: the first two passes
 *                            are where every ordinary bucket ends; a finisher over 2^19 buckets of 13 partial sums each measured -5 %)
 *   "item_l1", "item_l2", "reduce_seg"   = the L1, L2, seg of mi_debug_set_msm_plan, one at a time (a flat sort keeps its own item size: "flat_item_l1")
 *   "hold_accum" 0 | 1       = mi_debug_set_prove_schedule
 *   "ntt_lds_floor_kb" 0..160   LDS every NTT pass workgroup requests at least (caps the workgroups per CU)
 *   "ntt_stage_twiddles" 0 | 1   computeH's strided passes: 1 (default) = stage twiddles by global index from one M-entry table per pass and
 *                            root, no inter-pass product; 0 = tile-local stage twiddles and one product per element at the pass's edge (the
 *                            N-entry direct table), the yardstick.  Takes effect when computeH next builds its tables.  Same h, word for word
 *   "scale_powers_window" 0 | 2..5   phase 1's scalar multiplications (csrc/scale_powers.cuh): 2..5 = the fixed-window ladder of that width
 *                            (default 5, measured fastest: profiles/phase1.txt); 0 = the bit-by-bit xyzz_scale of the point NTT on the same scalars, the yardstick.  Same points
 *   "scale_powers_chunk" 0 | 64..2^24   lanes per chunk of that driver, which sizes its table workspace (0 = the default, 2^18)
 *   "verify_ksum" 0 | 1      the stage of the verdict-per-proof verifiers (mi355x_groth16_verify_ksum.h): 1 (default) = the sums of a whole
 *                            batch over the key's window table and the pairs laid out on the device; 0 = one MSM per proof and the group
 *                            law on the host, the yardstick.  Same pairs word for word, same verdicts
 *   "verify_ksum_min_batch" 1..2^24   the proofs from which knob 1 takes the table (default 8: at n = 1 three launches and a gather are not
 *                            faster than one MSM, profiles/verify.txt); smaller batches keep the older stage */
int32_t mi_debug_set_knob(mi_ctx *ctx, const char *name, int64_t value);
/* Counters the tests read to prove that an optional path really ran: "z_count_fused_launches" = computeH last launches of this context that
 * carried the Z MSM's digit count (knob "z_count_fused"); "dense_item_sorts" = bucket accumulations whose level-1 item size the dense-sort rule
 * chose (knob "dense_item_l1"); "generic_sorts_two_pass" / "generic_sorts_one_pass" = generic (no-table) MSM sorts that took the LDS-staged
 * two-pass sort (c = 16, 2^18 <= n, 16 n < 2^31) / the one-pass counting sort; "verify_ksum_batches" = batches the verdict-per-proof
 * verifiers staged through the key's window table (knob "verify_ksum"), "verify_ksum_launches" = the kernel launches of those stages (the
 * same number for every batch size); "hip_failure_countdown" = checked calls still to pass before
 * the failure armed by mi_debug_inject_hip_failure (process-wide; 0 = disarmed or spent).  MI_EINVAL for an unknown name. */
int32_t mi_debug_get_counter(mi_ctx *ctx, const char *name, uint64_t *out);
/* Process-wide, for contexts created afterwards: how the MSM slots of a context share streams (0: K's stream created, destroyed and
 * pointed at B1's, as rounds 4-5 did; 1, the default: never created; 2: A, B1 and K on one stream).  Same results; an experiment on which
 * chains end up on one hardware queue. */
int32_t mi_debug_set_stream_plan(int32_t plan);
/* the old name of mi_set_trace_ranges (mi355x_groth16.h) */
int32_t mi_debug_set_trace_ranges(int32_t on);
/* error-path tests: the nth MI-checked HIP call from now (library-wide, any thread) fails with hipErrorUnknown instead of
 * running; 0 disarms.  Used to prove that init / load / prove unwind without leaks or crashes. */
int32_t mi_debug_inject_hip_failure(int32_t nth);
/* The coefficients of the ceremony checks (mi355x_groth16_phase2_check.h) by the kernel those checks run, enqueued on the context's
 * stream: out_dev[k] = r_k as a Montgomery mi_fr, k < n <= 2^27; seed: 32 HOST bytes. */
int32_t mi_debug_ceremony_coeffs_dev(mi_ctx *ctx, const uint8_t seed[32], size_t n, mi_fr *out_dev);
/* The scalar multiplication of a phase-1 contribution (mi355x_groth16_phase1.h) by exactly the driver a contribution runs, for any n up to
 * 2^28, not only powers of two: out_host[i] = [c t^(k0 + i)] pts_host[i], affine points of G1 (g2 = 0) or G2 (g2 != 0), (0, 0) = infinity in
 * and out; t, c Montgomery and below r.  The knobs of mi_debug_set_knob choose what runs; mi_phase1_get_stats then tells row 0's times. */
int32_t mi_debug_scale_powers_dev(mi_ctx *ctx, int32_t g2, const void *pts_host, size_t n, const mi_fr *t, const mi_fr *c, uint64_t k0, void *out_host);
/* The two sides of every relation of the last mi_key_audit on ctx (mi355x_groth16_keyaudit.h) that got as far as its sums, as affine
 * points before any pairing: [0] = the side summed over the claimed key, [1] = the side summed over the SRS.  k_private, k_public, basis:
 * [0] is paired with delta2 / gamma2, [1] = T(r^P), T(r^V), T(r^C) with g2; z[1] is the difference of the two MSMs; sigma[k] = the sums
 * over Basis_k and BasisExpSigma_k for k < n_sigma.  MI_EINVAL when the context has run no such audit. */
typedef struct mi_key_audit_sums {
    mi_g1_affine a[2], b1[2], k_private[2], k_public[2], basis[2], z[2];
    mi_g2_affine b2[2];
    mi_g1_affine sigma[16][2];
    uint32_t n_sigma, valid;
} mi_key_audit_sums;
int32_t mi_debug_key_audit_sums(mi_ctx *ctx, mi_key_audit_sums *out);

#ifdef __cplusplus
}
#endif
#endif
