#include "key_handover.h"
#include "scan_u32.cuh"

namespace {
__global__ void k_clear_flags(u32 *flags, const u32 *idx, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[idx[i]] = 0;
}
// slot[j] = scanned flags (slot[j + 1] != slot[j] where the wire is kept; n + 1 entries: the lanes past n leave before they read it)
template <int W16> struct alignas(16) Words16 { uint4 w[W16]; };   // an element: W16 words of 16 bytes
template <int W16>
__global__ void __launch_bounds__(256) k_compact(Words16<W16> *dst, const Words16<W16> *src, const u32 *slot, u64 n) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 s = slot[j];
    if (slot[j + 1] != s) dst[s] = src[j];
}
}  // namespace

mi_pk_desc KeyArrays::desc() const {
    mi_pk_desc d;
    std::memset(&d, 0, sizeof(d));
    d.log_n = log_n; d.nb_public = nb_public; d.nb_wires = nb_wires;
    d.g1_a = (const mi_g1_affine *)arr[KEY_G1_A]; d.n_g1_a = n[KEY_G1_A];
    d.g1_b = (const mi_g1_affine *)arr[KEY_G1_B]; d.n_g1_b = n[KEY_G1_B];
    d.g1_k = (const mi_g1_affine *)arr[KEY_G1_K]; d.n_g1_k = n[KEY_G1_K];
    d.g1_z = (const mi_g1_affine *)arr[KEY_G1_Z]; d.n_g1_z = n[KEY_G1_Z];
    d.g2_b = (const mi_g2_affine *)arr[KEY_G2_B]; d.n_g2_b = n[KEY_G2_B];
    std::memcpy(&d.alpha1, &small1[0], 64); std::memcpy(&d.beta1, &small1[1], 64); std::memcpy(&d.delta1, &small1[2], 64);
    std::memcpy(&d.beta2, &small2[0], 128); std::memcpy(&d.delta2, &small2[1], 128);
    d.infinity_a = inf_a; d.infinity_b = inf_b; d.committed_wires = n_removed ? removed : nullptr; d.n_committed = n_removed;
    return d;
}

// ---------------------------------------------------------------------------------------------------- the handover
KeyHandover::~KeyHandover() {
    if (!armed) return;
    if (pk_out && *pk_out) { mi_pk_free(ctx, *pk_out); *pk_out = nullptr; }
    for (u32 k = 0; k < n_ped; k++) { mi_pedersen_pk_free(ctx, ped_out[k]); ped_out[k] = nullptr; }
}
int32_t KeyHandover::adopt_key(KeyArrays &ka, Arena *ar) {
    const mi_pk_desc d = ka.desc();
    bool took = false;
    const int32_t rc = mi_pk_load_range(ctx, &d, pk_out, true, nullptr, /*forced=*/nullptr, /*adopt=*/true, &took);
    for (void *&a : ka.arr) if (took) { if (ar) ar->disown(a); else a = nullptr; }
    return rc;
}
int32_t KeyHandover::adopt_pedersen(void **basis, void **bes, size_t n, Arena *ar) {
    MI_TRY(mi_pedersen_pk_adopt(ctx, *basis, *bes, n, &ped_out[n_ped]));
    for (void **p : {basis, bes}) { if (ar) ar->disown(*p); else *p = nullptr; }
    n_ped++;
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------- the streams
int32_t KeyStreams::check(mi_ctx *ctx, const char *who_c, const mi_pk_desc &counts, const mi_pedersen_arrays *ped, u32 n_commitments, u64 n_vk_k) const {
    const std::string who(who_c);
    size_t need = 0, vk_need = 0;
    if (mi_pk_stream_size(&counts, ped, n_commitments, encoding, &need) != MI_OK) MI_FAIL(ctx, MI_EINVAL, who + ": encoding is neither MI_KEYFILE_RAW nor MI_KEYFILE_COMPRESSED");
    if (len) *len = need;
    if (with_vk) {
        mi_vk_file_desc vc;
        std::memset(&vc, 0, sizeof(vc));
        vc.n_k = n_vk_k; vc.nb_public = counts.nb_public; vc.n_commitments = n_commitments;
        (void)mi_vk_stream_size(&vc, encoding, &vk_need);   // the encoding has passed above
        if (vk_len) *vk_len = vk_need;
    }
    if (!out || cap < need) MI_FAIL(ctx, MI_EINVAL, who + ": the key's stream takes " + std::to_string(need) + " bytes, out_host has room for " + std::to_string(out ? cap : 0));
    if (with_vk && (!vk_out || vk_cap < vk_need))
        MI_FAIL(ctx, MI_EINVAL, who + ": the verifying key's stream takes " + std::to_string(vk_need) + " bytes, vk_out_host has room for " + std::to_string(vk_out ? vk_cap : 0));
    return MI_OK;
}
int32_t KeyStreams::write_vk(mi_ctx *ctx, const KeyArrays &ka, const mi_g1_affine *k, u64 n_k, const mi_fr *sigma, u32 n_commitments) const {
    std::vector<mi_pedersen_vk> pvk(n_commitments);
    MI_TRY(mi_pedersen_vk_make(ctx, sigma, n_commitments, pvk.data()));
    return write_vk_points(ctx, ka, k, n_k, pvk.data(), n_commitments);
}
int32_t KeyStreams::write_vk_points(mi_ctx *ctx, const KeyArrays &ka, const mi_g1_affine *k, u64 n_k, const mi_pedersen_vk *ped, u32 n_commitments) const {
    mi_vk_file_desc vd;
    std::memset(&vd, 0, sizeof(vd));
    std::memcpy(&vd.alpha1, &ka.small1[0], 64); std::memcpy(&vd.beta1, &ka.small1[1], 64); std::memcpy(&vd.delta1, &ka.small1[2], 64);
    std::memcpy(&vd.beta2, &ka.small2[0], 128); std::memcpy(&vd.delta2, &ka.small2[1], 128); std::memcpy(&vd.gamma2, &ka.small2[2], 128);
    vd.k = k; vd.n_k = n_k; vd.nb_public = ka.nb_public; vd.n_commitments = n_commitments;
    vd.ped = ped;
    return mi_vk_write(ctx, &vd, encoding, vk_out, vk_cap, vk_len);
}

// ---------------------------------------------------------------------------------------------------- the wire selection
int32_t WireSelection::scan(mi_ctx *ctx, Arena &ar, const std::vector<u32> &removed) {
    hipStream_t st = ctx->stream;
    if (!removed.empty()) {
        u32 *rem = nullptr;
        MI_TRY(ar.alloc(ctx, &rem, removed.size()));
        MI_CHECK_HIP(ctx, hipMemcpyAsync(rem, removed.data(), removed.size() * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_clear_flags, dim3(mi_blocks_of(removed.size(), 256)), dim3(256), 0, st, slot_k, (const u32 *)rem, (u32)removed.size());
        MI_CHECK_HIP(ctx, hipGetLastError());
        MI_CHECK_HIP(ctx, hipStreamSynchronize(st));
        ar.release(rem);
    }
    // in == out: k_scan_final holds a block's values in registers before it stores the first of them, no block reads another's, and
    // the block sums come from an earlier launch.  The count of kept wires arrives in slot[nb_wires].
    for (u32 *s : {slot_a, slot_b, slot_k}) MI_TRY(exclusive_scan(ctx, st, s, nb_wires, s, ctx->ws[WS_SCAN]));
    return MI_OK;
}
int32_t WireSelection::fetch(mi_ctx *ctx, const uint8_t *inf_a_dev, const uint8_t *inf_b_dev, uint8_t *inf_a, uint8_t *inf_b) {
    const struct { void *dst; const void *src; size_t bytes; } copies[5] = {
        {inf_a, inf_a_dev, (size_t)nb_wires}, {inf_b, inf_b_dev, (size_t)nb_wires}, {&n_a, slot_a + nb_wires, 4}, {&n_b, slot_b + nb_wires, 4}, {&n_k, slot_k + nb_wires, 4}};
    for (const auto &c : copies) MI_CHECK_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, ctx->stream));
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MI_OK;
}
int32_t WireSelection::compact(mi_ctx *ctx, void *dst, const void *src, const u32 *slot, size_t elem_bytes) const {
    const dim3 grid(mi_blocks_of(nb_wires, 256)), block(256);
    switch (elem_bytes) {
    case 32: hipLaunchKernelGGL(k_compact<2>, grid, block, 0, ctx->stream, (Words16<2> *)dst, (const Words16<2> *)src, slot, nb_wires); break;
    case 64: hipLaunchKernelGGL(k_compact<4>, grid, block, 0, ctx->stream, (Words16<4> *)dst, (const Words16<4> *)src, slot, nb_wires); break;
    case 128: hipLaunchKernelGGL(k_compact<8>, grid, block, 0, ctx->stream, (Words16<8> *)dst, (const Words16<8> *)src, slot, nb_wires); break;
    default: return MI_EINVAL;
    }
    return MI_OK;
}
