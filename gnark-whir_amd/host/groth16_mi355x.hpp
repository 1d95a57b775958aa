// C++ host-side mirror of the reference's operator surface for the hot path, above the C-ABI of
// include/mi355x_groth16.h.  The reference is Go (gnark); no Go toolchain exists in the build image, so the
// compiled-language host side is written in C++ with gnark's names and argument meaning:
//
//   gnark (mt.go:447-497)                                   here
//   ------------------------------------------------------  ------------------------------------------------
//   pk, vk, _ := groth16.Setup(ccs)                         groth16::ProvingKey pk(ctx, desc)   // device-resident
//   proof, err := groth16.Prove(ccs, pk, witness, opts...)  groth16::Proof proof = groth16::Prove(ctx, pk, solution, r, s)
//   proof.WriteTo(w)                                        proof.WriteTo(bytes)
//
// `solution` is what gnark's r1cs.Solve hands to the prover (W, A, B, C); r and s are the two blinding scalars
// gnark samples with fr.SetRandom (inputs here so that CPU and GPU proofs of the same data are byte-identical).
// Errors surface as groth16::Error (gnark returns `error`); nothing is swallowed.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/mi355x_groth16.h"
#include "../../include/mi355x_groth16_group.h"
#include "../../include/mi355x_groth16_r1cs.h"
#include "../../include/mi355x_groth16_verify.h"
#include "../../include/mi355x_groth16_verify_bytes.h"
#include "../../include/mi355x_groth16_vkfile.h"
#include "../../include/mi355x_groth16_verify_combined.h"
#include "../../include/mi355x_groth16_verify_wave.h"
#include "../../include/mi355x_groth16_verify_ksum.h"
#include "../../include/mi355x_groth16_phase2.h"
#include "../../include/mi355x_groth16_phase2_check.h"
#include "../../include/mi355x_groth16_debug.h"   // (this mirror is the TEST side: generators and knobs)

namespace groth16 {

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string &what) : std::runtime_error(what), code(c) {}
};

class Context {
  public:
    explicit Context(int device = 0) {
        int32_t rc = mi_init(device, &ctx_);
        if (rc != MI_OK) throw Error(rc, "mi_init failed (no gfx950 device? there is no CPU path)");
    }
    ~Context() { if (ctx_) mi_shutdown(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    mi_ctx *get() const { return ctx_; }
    void check(int32_t rc) const { if (rc != MI_OK) throw Error(rc, mi_last_error(ctx_)); }

  private:
    mi_ctx *ctx_ = nullptr;
};

// Solution vectors of constraint/bn254 R1CSSolution: W (all wires), A, B, C (one value per constraint).
struct Solution {
    const mi_fr *W; size_t nWires;
    const mi_fr *A, *B, *C; size_t nConstraints;
};

// groth16/bn254 Proof
struct Proof {
    mi_g1_affine Ar;
    mi_g2_affine Bs;
    mi_g1_affine Krs;
    std::vector<mi_g1_affine> Commitments;   // BSB22 (filled by the caller when the circuit commits)
    mi_g1_affine CommitmentPok{};            // all-zero = point at infinity
    // Proof.WriteTo: Ar | Bs | Krs | u32-BE len | Commitments | CommitmentPok, compressed points
    void WriteTo(std::vector<uint8_t> &out) const {
        mi_proof_out p{Ar, Bs, Krs};
        out.resize(164 + 32 * Commitments.size());
        size_t n = mi_proof_write(&p, Commitments.data(), (uint32_t)Commitments.size(), &CommitmentPok, out.data());
        out.resize(n);
    }
};

// Device-resident proving key (the counterpart of gnark's icicle ProvingKey with its G1Device/G2Device members).
class ProvingKey {
  public:
    ProvingKey(const Context &ctx, const mi_pk_desc &desc) : ctx_(ctx) { ctx_.check(mi_pk_load(ctx_.get(), &desc, &pk_)); }
    ProvingKey(const Context &ctx, mi_pk *adopted) : ctx_(ctx), pk_(adopted) {}   // a key the library has built (Phase2::Seal)
    ~ProvingKey() { if (pk_) mi_pk_free(ctx_.get(), pk_); }
    ProvingKey(const ProvingKey &) = delete;
    ProvingKey &operator=(const ProvingKey &) = delete;
    mi_pk *get() const { return pk_; }

  private:
    const Context &ctx_;
    mi_pk *pk_ = nullptr;
};

// groth16.Prove after the solve.
inline Proof Prove(const Context &ctx, const ProvingKey &pk, const Solution &s, const mi_fr &r, const mi_fr &sBlind, mi_stats *stats = nullptr) {
    mi_proof_out out{};
    ctx.check(mi_groth16_prove(ctx.get(), pk.get(), s.W, s.nWires, s.A, s.B, s.C, s.nConstraints, &r, &sBlind, &out, stats));
    Proof p;
    p.Ar = out.ar; p.Bs = out.bs; p.Krs = out.krs;
    return p;
}

// Several groth16.Prove calls in flight on one GPU (what goroutines calling Prove concurrently get from gnark's CPU
// prover): Submit queues a proof and returns a handle, Wait blocks for it.  One device-resident key serves every context.
class Prover {
  public:
    class Pending {
      public:
        Proof Wait() {   // once
            int32_t rc = mi_prover_wait(p_, ticket_);
            if (rc != MI_OK) throw Error(rc, mi_prover_last_error(p_));
            Proof pr;
            pr.Ar = out_->ar; pr.Bs = out_->bs; pr.Krs = out_->krs;
            return pr;
        }
      private:
        friend class Prover;
        mi_prover *p_ = nullptr;
        uint64_t ticket_ = 0;
        std::unique_ptr<mi_proof_out> out_;   // written by a worker thread until Wait returns
    };
    explicit Prover(int device = 0, uint32_t inFlight = 3) {
        int32_t rc = mi_prover_create(device, inFlight, &p_);
        if (rc != MI_OK) throw Error(rc, "mi_prover_create failed (no gfx950 device? there is no CPU path)");
    }
    ~Prover() { if (p_) mi_prover_destroy(p_); }
    Prover(const Prover &) = delete;
    Prover &operator=(const Prover &) = delete;
    mi_ctx *ctx(uint32_t i = 0) const { return mi_prover_ctx(p_, i); }   // for mi_pk_load
    // the solution vectors must stay alive until Wait returns
    Pending Submit(mi_pk *pk, const Solution &s, const mi_fr &r, const mi_fr &sBlind) {
        Pending h;
        h.p_ = p_;
        h.out_.reset(new mi_proof_out{});
        int32_t rc = mi_prover_submit(p_, pk, s.W, s.nWires, s.A, s.B, s.C, s.nConstraints, &r, &sBlind, h.out_.get(), nullptr, &h.ticket_);
        if (rc != MI_OK) throw Error(rc, "mi_prover_submit failed");
        return h;
    }

  private:
    mi_prover *p_ = nullptr;
};

// One groth16.Prove spread over several GPUs of a node: contexts on `devices`, the key point-sharded at load,
// mode 0 = per-device partial sums, 1 = reduce-scatter of bucket sums (RCCL; include/mi355x_groth16.h, device groups).
class DeviceGroup {
  public:
    explicit DeviceGroup(const std::vector<int> &devices) {
        int32_t rc = mi_group_create(devices.data(), (int)devices.size(), &g_);
        if (rc != MI_OK) throw Error(rc, "mi_group_create failed (no gfx950 device? there is no CPU path)");
    }
    ~DeviceGroup() { if (spk_) mi_pk_sharded_free(g_, spk_); if (g_) mi_group_destroy(g_); }
    DeviceGroup(const DeviceGroup &) = delete;
    DeviceGroup &operator=(const DeviceGroup &) = delete;
    void check(int32_t rc) const { if (rc != MI_OK) throw Error(rc, mi_group_last_error(g_)); }
    void LoadKey(const mi_pk_desc &desc) { if (spk_) { mi_pk_sharded_free(g_, spk_); spk_ = nullptr; } check(mi_pk_load_sharded(g_, &desc, &spk_)); }
    Proof Prove(const Solution &s, const mi_fr &r, const mi_fr &sBlind, uint32_t mode = 0) {
        mi_proof_out out{};
        check(mi_groth16_prove_sharded(g_, spk_, s.W, s.nWires, s.A, s.B, s.C, s.nConstraints, &r, &sBlind, mode, &out, nullptr));
        Proof p;
        p.Ar = out.ar; p.Bs = out.bs; p.Krs = out.krs;
        return p;
    }
    mi_g1_jac MultiExpG1(const std::vector<mi_g1_affine> &points, const std::vector<mi_fr> &scalars, uint32_t mode = 0) {
        if (points.size() != scalars.size()) throw Error(MI_EINVAL, "MultiExp: len(points) != len(scalars)");
        mi_g1_jac out{};
        check(mi_msm_g1_sharded(g_, points.data(), scalars.data(), points.size(), 0, mode, &out));
        return out;
    }

  private:
    mi_group *g_ = nullptr;
    mi_pk_sharded *spk_ = nullptr;
};

// ecc/bn254 MultiExp
inline mi_g1_jac MultiExpG1(const Context &ctx, const std::vector<mi_g1_affine> &points, const std::vector<mi_fr> &scalars) {
    if (points.size() != scalars.size()) throw Error(MI_EINVAL, "MultiExp: len(points) != len(scalars)");   // gnark: same error
    mi_g1_jac out{};
    ctx.check(mi_msm_g1(ctx.get(), points.data(), scalars.data(), points.size(), 0, &out));
    return out;
}
inline mi_g2_jac MultiExpG2(const Context &ctx, const std::vector<mi_g2_affine> &points, const std::vector<mi_fr> &scalars) {
    if (points.size() != scalars.size()) throw Error(MI_EINVAL, "MultiExp: len(points) != len(scalars)");
    mi_g2_jac out{};
    ctx.check(mi_msm_g2(ctx.get(), points.data(), scalars.data(), points.size(), 0, &out));
    return out;
}
// The compiled constraint system kept on the device (include/mi355x_groth16_r1cs.h): what lets Prove take the solved wire vector alone.
class ResidentR1CS {
  public:
    ResidentR1CS(const Context &ctx, const mi_r1cs_desc &desc) : ctx_(ctx) { ctx_.check(mi_r1cs_load(ctx_.get(), &desc, &r_)); }
    ~ResidentR1CS() { if (r_) mi_r1cs_free(ctx_.get(), r_); }
    ResidentR1CS(const ResidentR1CS &) = delete;
    ResidentR1CS &operator=(const ResidentR1CS &) = delete;
    mi_r1cs *get() const { return r_; }
    uint64_t Bytes() const { uint64_t b = 0; ctx_.check(mi_r1cs_bytes(r_, &b)); return b; }
    // cs.IsSolved for a wire vector in device memory: rows with (A W)(B W) != C W, and the first of them
    uint64_t Unsatisfied(const mi_fr *W_dev, uint64_t *first_bad = nullptr) const {
        uint64_t n = 0, first = 0;
        ctx_.check(mi_r1cs_check_dev(ctx_.get(), r_, W_dev, &n, &first));
        if (first_bad) *first_bad = first;
        return n;
    }

  private:
    const Context &ctx_;
    mi_r1cs *r_ = nullptr;
};
// groth16.Prove from the solved wire vector alone (host memory): a = A W and b = B W are evaluated on the device
inline Proof ProveW(const Context &ctx, const ProvingKey &pk, const ResidentR1CS &r1cs, const std::vector<mi_fr> &W, const mi_fr &r, const mi_fr &s,
                    uint32_t flags = 0, mi_stats *stats = nullptr) {
    mi_proof_out out{};
    ctx.check(mi_groth16_prove_w(ctx.get(), pk.get(), r1cs.get(), W.data(), W.size(), flags, &r, &s, &out, stats));
    Proof p;
    p.Ar = out.ar; p.Bs = out.bs; p.Krs = out.krs;
    return p;
}
// Device-resident verifying key (include/mi355x_groth16_verify.h): validated and e(alpha, beta) computed once, at load.
class VerifyingKey {
  public:
    VerifyingKey(const Context &ctx, const mi_vk_desc &desc) : ctx_(ctx) { ctx_.check(mi_vk_load(ctx_.get(), &desc, &vk_)); }
    // from VerifyingKey.WriteTo's or WriteRawTo's bytes (include/mi355x_groth16_vkfile.h): decoded and checked on the device, the committed
    // lists installed.  flags: MI_KEYFILE_NO_SUBGROUP_CHECK, MI_KEYFILE_SUBGROUP_BY_R.  Throws MI_EINVAL naming the field that was refused.
    VerifyingKey(const Context &ctx, const std::vector<uint8_t> &stream, uint32_t flags = 0) : ctx_(ctx) {
        ctx_.check(mi_vk_load_stream(ctx_.get(), stream.data(), stream.size(), flags, &vk_));
    }
    ~VerifyingKey() { if (vk_) mi_vk_free(ctx_.get(), vk_); }
    VerifyingKey(const VerifyingKey &) = delete;
    VerifyingKey &operator=(const VerifyingKey &) = delete;
    mi_vk *get() const { return vk_; }
    // gnark's PublicAndCommitmentCommitted, one list of 1-based indices per commitment: what VerifyBytes hashes beside each commitment
    void SetPublicCommitted(const std::vector<std::vector<uint32_t>> &lists) {
        std::vector<uint32_t> off{0}, idx;
        for (const auto &l : lists) { idx.insert(idx.end(), l.begin(), l.end()); off.push_back((uint32_t)idx.size()); }
        ctx_.check(mi_vk_set_public_committed(ctx_.get(), vk_, off.data(), idx.empty() ? nullptr : idx.data()));
    }
    // The window table of K[1..] (include/mi355x_groth16_verify_ksum.h): built now under a byte budget (0 = 64 MiB), or again under
    // another one; without this call the first verdict-per-proof Verify on the key builds it.  window_bits == 0 in the info: no table.
    mi_vk_ksum_info PrepareKsum(uint64_t maxTableBytes = 0) {
        ctx_.check(mi_vk_ksum_prepare(ctx_.get(), vk_, maxTableBytes));
        return KsumInfo();
    }
    mi_vk_ksum_info KsumInfo() const {
        mi_vk_ksum_info info{};
        ctx_.check(mi_vk_ksum_get_info(ctx_.get(), vk_, &info));
        return info;
    }
    // sum_j scalars[i * bases + j] K[1 + j] for every row i, with no pairing attached (mi_vk_ksum_batch); skip: empty, or one byte per row
    std::vector<mi_g1_affine> PublicInputSums(const std::vector<mi_fr> &scalars, size_t n, const std::vector<uint8_t> &skip = {}) const {
        std::vector<mi_g1_affine> out(n);
        ctx_.check(mi_vk_ksum_batch(ctx_.get(), vk_, scalars.data(), skip.empty() ? nullptr : skip.data(), n, out.data()));
        return out;
    }
    // the same over device pointers, enqueued on the context's stream (mi_vk_ksum_batch_dev)
    void PublicInputSumsDev(const mi_fr *scalarsDev, const uint8_t *skipDev, size_t n, mi_g1_affine *outDev) const {
        ctx_.check(mi_vk_ksum_batch_dev(ctx_.get(), vk_, scalarsDev, skipDev, n, outDev));
    }

  private:
    const Context &ctx_;
    mi_vk *vk_ = nullptr;
};
// groth16.Verify: the verdict (MI_VERIFY_OK, _PAIRING, _PEDERSEN, _MALFORMED); a rejected proof is a verdict, not an exception.
// publicInputs: without the ONE wire; commitmentValues (the hash-to-field of each commitment) and foldChallenge come from the caller.
// Every coordinate and scalar must be reduced (its words below p, resp. r): one that is not makes the verdict MI_VERIFY_MALFORMED, and
// the VerifyingKey constructor throws MI_EINVAL for such a coordinate in the descriptor (ONE ENCODING in the header).
inline uint8_t Verify(const Context &ctx, const VerifyingKey &vk, const Proof &proof, const std::vector<mi_fr> &publicInputs,
                      const std::vector<mi_fr> &commitmentValues = {}, const mi_fr *foldChallenge = nullptr) {
    mi_verify_input in{};
    in.proof = mi_proof_out{proof.Ar, proof.Bs, proof.Krs};
    in.commitments = proof.Commitments.empty() ? nullptr : proof.Commitments.data();
    in.pok = &proof.CommitmentPok;
    in.public_inputs = publicInputs.empty() ? nullptr : publicInputs.data();
    in.commitment_values = commitmentValues.empty() ? nullptr : commitmentValues.data();
    in.fold_challenge = foldChallenge;
    uint8_t verdict = MI_VERIFY_MALFORMED;
    ctx.check(mi_groth16_verify(ctx.get(), vk.get(), &in, &verdict));
    return verdict;
}
// groth16.Verify from Proof.WriteTo's bytes (include/mi355x_groth16_verify_bytes.h): the points are decompressed and the BSB22 hashes
// computed on the device.  Throws MI_EINVAL when bytes.size() is not 164 + 32 * the key's commitments; anything else is a verdict.
inline uint8_t VerifyBytes(const Context &ctx, const VerifyingKey &vk, const std::vector<uint8_t> &bytes, const std::vector<mi_fr> &publicInputs) {
    uint8_t verdict = MI_VERIFY_MALFORMED;
    ctx.check(mi_groth16_verify_bytes(ctx.get(), vk.get(), bytes.data(), bytes.size(), publicInputs.empty() ? nullptr : publicInputs.data(), &verdict));
    return verdict;
}
// One proof, or a few, at low latency (include/mi355x_groth16_verify_wave.h): one wave per pairing instead of one lane, the verdicts of
// mi_groth16_verify_batch / mi_groth16_verify_bytes_batch byte for byte.  The header quotes the measured range; above it the batch,
// combined and locate calls remain the tools.
inline std::vector<uint8_t> VerifyWave(const Context &ctx, const VerifyingKey &vk, const std::vector<mi_verify_input> &in) {
    std::vector<uint8_t> verdicts(in.size(), MI_VERIFY_MALFORMED);
    ctx.check(mi_groth16_verify_wave(ctx.get(), vk.get(), in.data(), in.size(), verdicts.data()));
    return verdicts;
}
inline std::vector<uint8_t> VerifyBytesWave(const Context &ctx, const VerifyingKey &vk, const std::vector<mi_verify_bytes_input> &in) {
    std::vector<uint8_t> verdicts(in.size(), MI_VERIFY_MALFORMED);
    ctx.check(mi_groth16_verify_bytes_wave(ctx.get(), vk.get(), in.data(), in.size(), verdicts.data()));
    return verdicts;
}
// ONE verdict for a batch of proofs under one key (include/mi355x_groth16_verify_combined.h): the random linear combination of their
// equations -- n + 3 (+ commitments + 1) Miller loops, two final exponentiations and a constant number of MSMs for the whole batch.
// seed = nullptr: the library draws it from the operating system, which is what judging proofs from someone else requires (a seed the
// maker of the proofs can predict voids the soundness claim).  firstMalformed (may be null) = the lowest malformed index with
// MI_VERIFY_MALFORMED, n otherwise.  Verdicts 1 and 2 do not say which proof is at fault.
struct BatchProof {
    std::vector<uint8_t> bytes;          // Proof::WriteTo
    std::vector<mi_fr> publicInputs;     // without the ONE wire
};
inline uint8_t VerifyBytesCombined(const Context &ctx, const VerifyingKey &vk, const std::vector<BatchProof> &proofs, const uint8_t *seed = nullptr,
                                   uint64_t *firstMalformed = nullptr) {
    std::vector<mi_verify_bytes_input> in(proofs.size());
    for (size_t i = 0; i < proofs.size(); i++)
        in[i] = mi_verify_bytes_input{proofs[i].bytes.data(), proofs[i].bytes.size(), proofs[i].publicInputs.empty() ? nullptr : proofs[i].publicInputs.data()};
    uint8_t verdict = MI_VERIFY_MALFORMED;
    ctx.check(mi_groth16_verify_bytes_combined(ctx.get(), vk.get(), in.data(), in.size(), seed, &verdict, firstMalformed));
    return verdict;
}
// the same over proofs already taken apart (mi_verify_input: the caller computed the BSB22 hashes)
inline uint8_t VerifyCombined(const Context &ctx, const VerifyingKey &vk, const std::vector<mi_verify_input> &in, const uint8_t *seed = nullptr,
                              uint64_t *firstMalformed = nullptr) {
    uint8_t verdict = MI_VERIFY_MALFORMED;
    ctx.check(mi_groth16_verify_combined(ctx.get(), vk.get(), in.data(), in.size(), seed, &verdict, firstMalformed));
    return verdict;
}
// groth16.Verify from the two files a verifier holds beside the key (include/mi355x_groth16_vkfile.h): Proof.WriteTo's bytes and
// witness.WriteTo's.  The public inputs go up as bytes and are decoded on the device.  Throws MI_EINVAL for a framing error (a length
// that is not the key's proof length, resp. 12 + 32 n of the witness's own header); anything else is a verdict.
struct FileProof {
    std::vector<uint8_t> proof;          // Proof::WriteTo
    std::vector<uint8_t> witness;        // witness.WriteTo, public or full
};
inline uint8_t VerifyFiles(const Context &ctx, const VerifyingKey &vk, const std::vector<uint8_t> &proof, const std::vector<uint8_t> &witness) {
    uint8_t verdict = MI_VERIFY_MALFORMED;
    ctx.check(mi_groth16_verify_files(ctx.get(), vk.get(), proof.data(), proof.size(), witness.data(), witness.size(), &verdict));
    return verdict;
}
inline std::vector<mi_verify_files_input> FilesInputs(const std::vector<FileProof> &proofs) {
    std::vector<mi_verify_files_input> in(proofs.size());
    for (size_t i = 0; i < proofs.size(); i++)
        in[i] = mi_verify_files_input{proofs[i].proof.data(), proofs[i].proof.size(), proofs[i].witness.data(), proofs[i].witness.size()};
    return in;
}
inline std::vector<uint8_t> VerifyFilesBatch(const Context &ctx, const VerifyingKey &vk, const std::vector<FileProof> &proofs) {
    const auto in = FilesInputs(proofs);
    std::vector<uint8_t> verdicts(proofs.size(), MI_VERIFY_MALFORMED);
    ctx.check(mi_groth16_verify_files_batch(ctx.get(), vk.get(), in.data(), in.size(), verdicts.data()));
    return verdicts;
}
inline uint8_t VerifyFilesCombined(const Context &ctx, const VerifyingKey &vk, const std::vector<FileProof> &proofs, const uint8_t *seed = nullptr,
                                   uint64_t *firstMalformed = nullptr) {
    const auto in = FilesInputs(proofs);
    uint8_t verdict = MI_VERIFY_MALFORMED;
    ctx.check(mi_groth16_verify_files_combined(ctx.get(), vk.get(), in.data(), in.size(), seed, &verdict, firstMalformed));
    return verdict;
}
inline std::vector<uint8_t> VerifyFilesLocate(const Context &ctx, const VerifyingKey &vk, const std::vector<FileProof> &proofs, const uint8_t *seed = nullptr,
                                              mi_verify_locate_stats *stats = nullptr) {
    const auto in = FilesInputs(proofs);
    std::vector<uint8_t> verdicts(proofs.size(), MI_VERIFY_MALFORMED);
    ctx.check(mi_groth16_verify_files_locate(ctx.get(), vk.get(), in.data(), in.size(), seed, verdicts.data(), stats));
    return verdicts;
}
// VerifyingKey.WriteTo (MI_KEYFILE_COMPRESSED) / WriteRawTo (MI_KEYFILE_RAW) for a key in host memory (mi_vk_write)
inline std::vector<uint8_t> WriteVerifyingKey(const Context &ctx, const mi_vk_file_desc &desc, uint32_t encoding = MI_KEYFILE_COMPRESSED) {
    size_t len = 0;
    if (mi_vk_stream_size(&desc, encoding, &len) != MI_OK) throw Error(MI_EINVAL, "WriteVerifyingKey: more than MI_PK_RAW_MAX_COMMITMENTS commitments or an unknown encoding");
    std::vector<uint8_t> out(len);
    ctx.check(mi_vk_write(ctx.get(), &desc, encoding, out.data(), out.size(), &len));
    return out;
}
// witness.WriteTo of a public witness, and its inverse: false for a header that disagrees with the length or a value not below r
inline std::vector<uint8_t> WritePublicWitness(const std::vector<mi_fr> &values) {
    std::vector<uint8_t> out(12 + 32 * values.size());
    if (mi_public_witness_write(values.data(), values.size(), out.data(), out.size(), nullptr) != MI_OK) throw Error(MI_EINVAL, "WritePublicWitness: more than 2^32 - 1 values");
    return out;
}
inline bool ReadPublicWitness(const std::vector<uint8_t> &bytes, std::vector<mi_fr> &out) {
    out.resize(bytes.size() / 32);
    size_t n = 0;
    const bool ok = mi_public_witness_read(bytes.data(), bytes.size(), out.data(), out.size(), &n) == MI_OK;
    out.resize(ok ? n : 0);
    return ok;
}
// The inverse of Proof::WriteTo (mi_proof_read): false when the bytes are not one well-formed proof with nCommitments commitments
inline bool ReadProof(const std::vector<uint8_t> &bytes, uint32_t nCommitments, Proof &out) {
    mi_proof_out p;
    out.Commitments.resize(nCommitments);
    if (mi_proof_read(bytes.data(), bytes.size(), nCommitments, &p, nCommitments ? out.Commitments.data() : nullptr, &out.CommitmentPok) != MI_OK) return false;
    out.Ar = p.ar; out.Bs = p.bs; out.Krs = p.krs;
    return true;
}
// fr.Hash(msg, dst, 1)[0] (mi_hash_to_field): the BSB22 commitment values and fold challenge are such hashes
inline mi_fr HashToField(const std::string &dst, const std::vector<uint8_t> &msg) {
    mi_fr out;
    if (mi_hash_to_field((const uint8_t *)dst.data(), dst.size(), msg.data(), msg.size(), &out) != MI_OK) throw Error(MI_EINVAL, "HashToField: dst must have 1 .. 255 bytes");
    return out;
}
// mpcsetup's phase 2 (include/mi355x_groth16_phase2.h): the circuit's keys derived on the device from a powers-of-tau SRS, delta
// re-randomised by contributors.  The commitment keys' sigma is re-randomised with a proof per step and adopted by the next party
// (include/mi355x_groth16_phase2_check.h): ContributeSigmaProved / VerifyAdoptSigma / PedersenVk / ChainInfo below and
// VerifySigmaRecords beside the class.  NOT here: the pairing check of the SRS, delta's proofs, gnark's mpcsetup file formats.
//   p2 := mpcsetup.InitPhase2(r1cs, &srs)      groth16::Phase2 p2(ctx, r1cs, srs, sigma)
//   p2.Contribute()                            p2.Contribute(delta)            // the caller samples delta (and must forget it)
//   pk, vk := mpcsetup.ExtractKeys(...)        p2.Seal(vk) / p2.Streams(...)   // as often as wanted: sealing does not end the ceremony
class Phase2 {
  public:
    Phase2(const Context &ctx, const mi_r1cs_desc &r1cs, const mi_srs_desc &srs, const std::vector<mi_fr> &sigma = {}, uint32_t flags = 0) : ctx_(ctx) {
        ctx_.check(mi_phase2_init(ctx_.get(), &r1cs, &srs, sigma.empty() ? nullptr : sigma.data(), flags, &st_));
    }
    ~Phase2() { if (st_) mi_phase2_free(ctx_.get(), st_); }
    Phase2(const Phase2 &) = delete;
    Phase2 &operator=(const Phase2 &) = delete;
    mi_phase2 *get() const { return st_; }
    void Contribute(const mi_fr &delta, const std::vector<mi_fr> &sigmaFactor = {}) {
        ctx_.check(mi_phase2_contribute(ctx_.get(), st_, &delta, sigmaFactor.empty() ? nullptr : sigmaFactor.data()));
    }
    // the proving key as an ordinary device-resident key; vk (k / k_cap set by the caller) and ped (room for the commitments) as mi_groth16_setup
    std::unique_ptr<ProvingKey> Seal(mi_vk_out &vk, mi_pedersen_pk **ped = nullptr) const {
        mi_pk *pk = nullptr;
        ctx_.check(mi_phase2_seal(ctx_.get(), st_, &pk, ped, &vk));
        return std::unique_ptr<ProvingKey>(new ProvingKey(ctx_, pk));
    }
    // ProvingKey.WriteTo / VerifyingKey.WriteTo (MI_KEYFILE_COMPRESSED) or the raw forms (MI_KEYFILE_RAW)
    void Streams(std::vector<uint8_t> &pk, std::vector<uint8_t> &vk, uint32_t encoding = MI_KEYFILE_COMPRESSED) const {
        size_t len = 0, vkLen = 0;
        (void)mi_phase2_to_streams(ctx_.get(), st_, encoding, nullptr, 0, &len, nullptr, 0, &vkLen);   // the sizes
        pk.resize(len); vk.resize(vkLen);
        ctx_.check(mi_phase2_to_streams(ctx_.get(), st_, encoding, pk.data(), pk.size(), &len, vk.data(), vk.size(), &vkLen));
    }
    // ---- sigma (include/mi355x_groth16_phase2_check.h): the state's points, a proved step, a claimed state checked and taken
    // {g2, [-sigma_k]2} per commitment: what goes into mi_vk_desc.ped for the key Seal hands out
    std::vector<mi_pedersen_vk> PedersenVk() const {
        std::vector<mi_pedersen_vk> out(ChainInfo().n_commitments);
        ctx_.check(mi_phase2_get_pedersen_vk(ctx_.get(), st_, out.empty() ? nullptr : out.data()));
        return out;
    }
    mi_phase2_chain_info ChainInfo() const {
        mi_phase2_chain_info info;
        ctx_.check(mi_phase2_get_chain_info(ctx_.get(), st_, &info));
        return info;
    }
    // one factor per commitment; the nonces are the library's.  Returns the step's proofs, hash takes the chain value after it
    std::vector<mi_phase2_sigma_proof> ContributeSigmaProved(const std::vector<mi_fr> &sigmaFactor, uint8_t hash[32]) {
        std::vector<mi_phase2_sigma_proof> out(sigmaFactor.size());
        ctx_.check(mi_phase2_contribute_sigma_proved(ctx_.get(), st_, sigmaFactor.data(), nullptr, out.data(), hash));
        return out;
    }
    // failed == 0, and only then: the claimed BasisExpSigma arrays and [-sigma]2 points are the state's and the sigma chain has advanced
    uint32_t VerifyAdoptSigma(const mi_phase2_sigma_claim &claim, const std::vector<mi_phase2_sigma_proof> &proofs, const uint8_t (*hashes)[32], size_t steps,
                              uint64_t *badCommitments, uint64_t *firstBadRecord = nullptr) {
        uint32_t failed = 0;
        ctx_.check(mi_phase2_verify_adopt_sigma(ctx_.get(), st_, &claim, proofs.data(), hashes, steps, nullptr, &failed, badCommitments, firstBadRecord));
        return failed;
    }

  private:
    const Context &ctx_;
    mi_phase2 *st_ = nullptr;
};
// the sigma chain of `steps` steps continuing (start, startHash, firstIndex), on the host: the index of the first step that does not hold
inline uint64_t VerifySigmaRecords(const std::vector<mi_g2_affine> &start, const uint8_t startHash[32], uint64_t firstIndex,
                                   const std::vector<mi_phase2_sigma_proof> &proofs, const uint8_t (*hashes)[32], size_t steps) {
    uint64_t firstBad = 0;
    if (mi_phase2_sigma_records_verify(start.data(), (uint32_t)start.size(), startHash, firstIndex, proofs.data(), hashes, steps, &firstBad) != MI_OK)
        throw Error(MI_EINVAL, "VerifySigmaRecords: a null argument, no commitment, or a start point off the twist or at infinity");
    return firstBad;
}
// fft.Domain: FFT / FFTInverse with fft.DIF / fft.DIT and fft.OnCoset()
enum Decimation { DIF = 0, DIT = 1 };
inline void FFT(const Context &ctx, std::vector<mi_fr> &a, uint32_t logN, Decimation d, bool onCoset = false) {
    if (a.size() != ((size_t)1 << logN)) throw Error(MI_EINVAL, "FFT: len(a) != domain cardinality");
    ctx.check(mi_ntt(ctx.get(), a.data(), logN, (d == DIT ? MI_NTT_DIT : 0u) | (onCoset ? MI_NTT_COSET : 0u)));
}
inline void FFTInverse(const Context &ctx, std::vector<mi_fr> &a, uint32_t logN, Decimation d, bool onCoset = false) {
    if (a.size() != ((size_t)1 << logN)) throw Error(MI_EINVAL, "FFTInverse: len(a) != domain cardinality");
    ctx.check(mi_ntt(ctx.get(), a.data(), logN, MI_NTT_INVERSE | (d == DIT ? MI_NTT_DIT : 0u) | (onCoset ? MI_NTT_COSET : 0u)));
}

}  // namespace groth16
