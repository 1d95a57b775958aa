// What every maker of a proving key shares at its end (setup.hip, phase2.hip, keyfile.hip, pk_raw.hip; not part of the C-ABI): the
// key's arrays and their descriptor, the handover to the key with its rollback, the two streams' checks, the wire selection.
#pragma once
#include "prove_internal.h"
#include "dev_arena.h"
#include "../../include/mi355x_groth16_vkfile.h"
#include <vector>

enum { KEY_G1_A, KEY_G1_B, KEY_G1_K, KEY_G1_Z, KEY_G2_B, KEY_ARRAYS };   // mi_pk_desc's order
// the five device arrays of a key with everything else a mi_pk_desc names
struct KeyArrays {
    u32 log_n = 0, nb_public = 0;
    u64 nb_wires = 0;
    void *arr[KEY_ARRAYS] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // device, affine
    u64 n[KEY_ARRAYS] = {0, 0, 0, 0, 0};
    G1Aff small1[3];   // alpha, beta, delta
    G2Aff small2[3];   // beta, delta; gamma, which only the verifying key's stream reads
    const uint8_t *inf_a = nullptr, *inf_b = nullptr;   // host, a byte per wire
    const u32 *removed = nullptr;                        // host: committed + commitment wires (may be null)
    size_t n_removed = 0;
    KeyArrays(u32 log_n_, u32 nb_public_, u64 nb_wires_, const uint8_t *ia, const uint8_t *ib, const u32 *rem, size_t n_rem)
        : log_n(log_n_), nb_public(nb_public_), nb_wires(nb_wires_), inf_a(ia), inf_b(ib), removed(rem), n_removed(n_rem) {}
    mi_pk_desc desc() const;
};

// The key takes the arrays (mi_pk_load_range's adopt path), the Pedersen keys theirs.  The guard records a maker's outputs and what it has
// made so far: when it goes it frees the key and the Pedersen keys and clears their outputs, unless dismiss() was called.  It waits for
// nothing: a maker with work in flight synchronises first.  The arrays' owner is an Arena, or (ar == nullptr) the caller's own pointers,
// cleared where an Arena would disown.  pk_out null: no key is wanted; ped_out null: the Pedersen keys made stay the caller's (pk_raw.hip).
struct KeyHandover {
    mi_ctx *ctx;
    mi_pk **pk_out;
    mi_pedersen_pk **ped_out;
    u32 n_ped = 0;   // Pedersen keys made: ped_out[0 .. n_ped)
    bool armed = true;
    KeyHandover(mi_ctx *c, mi_pk **pk, mi_pedersen_pk **ped) : ctx(c), pk_out(pk), ped_out(ped) {}
    KeyHandover(const KeyHandover &) = delete;
    ~KeyHandover();
    void dismiss() { armed = false; }
    // once the key has taken ka's arrays they are its own whatever the call returns (a key that fails later releases them itself)
    int32_t adopt_key(KeyArrays &ka, Arena *ar);
    int32_t adopt_pedersen(void **basis, void **bes, size_t n, Arena *ar);   // the next Pedersen key takes the pair
};

// Where the stream of a key goes; with_vk: the verifying key's stream too, with a triple of its own.
struct KeyStreams {
    uint32_t encoding;
    uint8_t *out;
    size_t cap, *len;
    bool with_vk = false;
    uint8_t *vk_out = nullptr;
    size_t vk_cap = 0, *vk_len = nullptr;
    // Before any point is computed: both sizes go to *len / *vk_len, then a buffer that cannot hold its stream is refused with "<who>: ...".
    // counts / ped: what mi_pk_stream_size reads, no pointer is followed; n_vk_k: points of vk.G1.K
    int32_t check(mi_ctx *ctx, const char *who, const mi_pk_desc &counts, const mi_pedersen_arrays *ped, u32 n_commitments, u64 n_vk_k) const;
    // the verifying key's stream from ka's small points and vk.G1.K on the host; its Pedersen keys are made from sigma, its lists start empty
    int32_t write_vk(mi_ctx *ctx, const KeyArrays &ka, const mi_g1_affine *k, u64 n_k, const mi_fr *sigma, u32 n_commitments) const;
    // the same with the Pedersen keys handed over as pairs {g2, [-sigma]2}: for a maker that holds the points and no scalar (phase2.hip)
    int32_t write_vk_points(mi_ctx *ctx, const KeyArrays &ka, const mi_g1_affine *k, u64 n_k, const mi_pedersen_vk *ped, u32 n_commitments) const;
};

// Which wires own a point of pk.G1.A / pk.G1.B (+ pk.G2.B) / pk.G1.K.  slot_*: nb_wires + 1 words each on the device; the maker's own
// kernel fills the first nb_wires with flags (1 = the wire owns a point; slot_k: every private wire).  scan() clears slot_k at the removed
// wires and turns all three into the compaction's slots in place, the count of kept wires in slot[nb_wires]; fetch() brings the masks and
// the counts to the host and leaves the stream idle; compact(): dst[slot[j]] = src[j] where slot[j + 1] != slot[j], elements of 32, 64 or 128 bytes.
struct WireSelection {
    u32 *slot_a = nullptr, *slot_b = nullptr, *slot_k = nullptr;
    u64 nb_wires = 0;
    u32 n_a = 0, n_b = 0, n_k = 0;
    int32_t scan(mi_ctx *ctx, Arena &ar, const std::vector<u32> &removed);
    int32_t fetch(mi_ctx *ctx, const uint8_t *inf_a_dev, const uint8_t *inf_b_dev, uint8_t *inf_a, uint8_t *inf_b);
    int32_t compact(mi_ctx *ctx, void *dst, const void *src, const u32 *slot, size_t elem_bytes) const;
};
