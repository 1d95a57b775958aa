//go:build mi355x

// groth16.Verify (reilabs/gnark-whir mt.go:497) on the device: include/mi355x_groth16_verify.h.
//
// STATUS: SOURCE ONLY, like the rest of the shim (mi355x.go): never compiled here.  Verify computes what gnark's verify.go computes on
// the host -- the hash-to-field of every commitment (with the public committed values) and the fold challenge -- and hands the rest to
// mi_groth16_verify.  VerifyBytes takes Proof.WriteTo's bytes and leaves decoding and hashing to the device (mi_groth16_verify_bytes).
// VerifyBytesCombined judges a whole batch of such proofs with ONE verdict (mi_groth16_verify_bytes_combined).
// VerifyWave and VerifyBytesWave are Verify and VerifyBytes through the low-latency body (include/mi355x_groth16_verify_wave.h: one
// wave per pairing, the same verdicts): the calls for the single proof mt.go:497 verifies.
// VerifyFiles and VerifyFilesCombined take the public witness as witness.WriteTo's bytes too (include/mi355x_groth16_vkfile.h): with a
// key from LoadVerifyingKeyStream (keyfile.go) nothing of gnark is decoded on the host.
package mi355x

/*
#include <stdlib.h>
#include "mi355x_groth16_verify.h"
#include "mi355x_groth16_verify_bytes.h"
#include "mi355x_groth16_verify_combined.h"
#include "mi355x_groth16_verify_wave.h"
#include "mi355x_groth16_verify_ksum.h"
#include "mi355x_groth16_vkfile.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr/hash_to_field"
	groth16_bn254 "github.com/consensys/gnark/backend/groth16/bn254"
	"github.com/consensys/gnark/constraint"
)

// VerifyingKey is gnark's key plus its device-resident handle (mi_vk).
type VerifyingKey struct {
	groth16_bn254.VerifyingKey
	ctx *C.mi_ctx
	dev *C.mi_vk
}

// ErrRejected carries the verdict of a rejected proof: MI_VERIFY_PAIRING, MI_VERIFY_PEDERSEN or MI_VERIFY_MALFORMED.
// MI_VERIFY_MALFORMED covers words that are not reduced as well (a coordinate not below p, a scalar not below r: ONE ENCODING in the
// header).  gnark-crypto's fp.Element / fr.Element are always reduced, so values that went through its decoders cannot trigger it;
// words written into an Element from outside can.  mi_vk_load refuses such a coordinate in the key with MI_EINVAL.
type ErrRejected struct{ Verdict int }

func (e ErrRejected) Error() string { return fmt.Sprintf("mi355x: proof rejected (verdict %d)", e.Verdict) }

// LoadVerifyingKey uploads vk once (mi_vk_load): every point is validated and e(alpha, beta) is computed there.
func LoadVerifyingKey(vk *groth16_bn254.VerifyingKey, device int) (*VerifyingKey, error) {
	out := &VerifyingKey{VerifyingKey: *vk}
	if rc := C.mi_init(C.int(device), &out.ctx); rc != C.MI_OK {
		return nil, fmt.Errorf("mi355x: mi_init rc=%d", int(rc))
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	nc := len(vk.PublicAndCommitmentCommitted)
	ped := make([]C.mi_pedersen_vk, nc)
	for i := 0; i < nc; i++ {
		ped[i].g = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.CommitmentKeys[i].G))
		ped[i].g_sigma_neg = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.CommitmentKeys[i].GSigmaNeg))
	}
	var d C.mi_vk_desc
	d.alpha1 = *(*C.mi_g1_affine)(unsafe.Pointer(&vk.G1.Alpha))
	d.beta2 = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.G2.Beta))
	d.gamma2 = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.G2.Gamma))
	d.delta2 = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.G2.Delta))
	d.k = g1(&pin, vk.G1.K)
	d.n_k = C.uint64_t(len(vk.G1.K))
	d.nb_public = C.uint32_t(len(vk.G1.K) - nc)
	d.n_commitments = C.uint32_t(nc)
	if nc > 0 {
		pin.Pin(&ped[0])
		d.ped = &ped[0]
	}
	if err := status(out.ctx, C.mi_vk_load(out.ctx, &d, &out.dev)); err != nil {
		C.mi_shutdown(out.ctx)
		return nil, err
	}
	// PublicAndCommitmentCommitted in CSR form, for VerifyBytes: the device hashes each commitment with these values
	offsets := make([]C.uint32_t, nc+1)
	var indices []C.uint32_t
	for i, s := range vk.PublicAndCommitmentCommitted {
		for _, j := range s {
			indices = append(indices, C.uint32_t(j))
		}
		offsets[i+1] = C.uint32_t(len(indices))
	}
	var idx *C.uint32_t
	if len(indices) > 0 {
		idx = &indices[0]
	}
	if err := status(out.ctx, C.mi_vk_set_public_committed(out.ctx, out.dev, &offsets[0], idx)); err != nil {
		out.Close()
		return nil, err
	}
	return out, nil
}

// Close frees the device-resident key and its context.
func (vk *VerifyingKey) Close() {
	if vk.dev != nil {
		C.mi_vk_free(vk.ctx, vk.dev)
		vk.dev = nil
	}
	if vk.ctx != nil {
		C.mi_shutdown(vk.ctx)
		vk.ctx = nil
	}
}

// KsumInfo is mi_vk_ksum_info: the window table of the key's K[1..] (include/mi355x_groth16_verify_ksum.h).  WindowBits == 0: the key
// has no table, State (MI_KSUM_*) says why, and the verifiers keep one MSM per proof for it.
type KsumInfo struct {
	WindowBits, Windows      uint32
	TableBytes, Bases, Budget uint64
	State                    uint32
	BuildMs                  float32
}

// PrepareKsum builds the key's window table now under a byte budget (0 = MI_KSUM_DEFAULT_TABLE_BYTES, 64 MiB), or again under another
// one (mi_vk_ksum_prepare).  Without it the first Verify on the key builds the table under the default budget.
func (vk *VerifyingKey) PrepareKsum(maxTableBytes uint64) (KsumInfo, error) {
	if err := status(vk.ctx, C.mi_vk_ksum_prepare(vk.ctx, vk.dev, C.uint64_t(maxTableBytes))); err != nil {
		return KsumInfo{}, err
	}
	return vk.KsumInfo()
}

// KsumInfo reads mi_vk_ksum_get_info.
func (vk *VerifyingKey) KsumInfo() (KsumInfo, error) {
	var i C.mi_vk_ksum_info
	if err := status(vk.ctx, C.mi_vk_ksum_get_info(vk.ctx, vk.dev, &i)); err != nil {
		return KsumInfo{}, err
	}
	return KsumInfo{uint32(i.window_bits), uint32(i.windows), uint64(i.table_bytes), uint64(i.bases), uint64(i.budget_bytes), uint32(i.state),
		float32(i.build_ms)}, nil
}

// PublicInputSums is mi_vk_ksum_batch: rows[i] holds the scalars of statement i (public inputs, then commitment values: len(vk.G1.K) - 1
// of them); the result is sum_j rows[i][j] K[1 + j] for every i, with no pairing attached.  The key must have a table (PrepareKsum).
// mi_vk_ksum_batch_dev is the same over device pointers, for callers that keep their scalars on the device.
func (vk *VerifyingKey) PublicInputSums(rows []fr.Vector) ([]bn254.G1Affine, error) {
	ns := len(vk.G1.K) - 1
	flat := make(fr.Vector, 0, len(rows)*ns)
	for _, row := range rows {
		if len(row) != ns {
			return nil, errors.New("mi355x: a row has not one scalar per base of the key")
		}
		flat = append(flat, row...)
	}
	out := make([]bn254.G1Affine, len(rows))
	if len(rows) == 0 {
		return out, nil
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&flat[0])
	pin.Pin(&out[0])
	rc := C.mi_vk_ksum_batch(vk.ctx, vk.dev, (*C.mi_fr)(unsafe.Pointer(&flat[0])), nil, C.size_t(len(rows)), (*C.mi_g1_affine)(unsafe.Pointer(&out[0])))
	return out, status(vk.ctx, rc)
}

// Verify replaces groth16.Verify(proof, vk, publicWitness).  publicWitness holds the public inputs without the ONE wire, as
// witness.Vector() of the public witness does.
func Verify(vk *VerifyingKey, proof *groth16_bn254.Proof, publicWitness fr.Vector) error {
	return verify(vk, proof, publicWitness, false)
}

// VerifyWave is Verify through mi_groth16_verify_wave: one wave per pairing instead of one lane, the same verdict, a fraction of the
// latency for one proof (the measured range is in the header).
func VerifyWave(vk *VerifyingKey, proof *groth16_bn254.Proof, publicWitness fr.Vector) error {
	return verify(vk, proof, publicWitness, true)
}

func verify(vk *VerifyingKey, proof *groth16_bn254.Proof, publicWitness fr.Vector, wave bool) error {
	nc := len(vk.PublicAndCommitmentCommitted)
	if len(proof.Commitments) != nc {
		return errors.New("mi355x: the proof's commitments do not match the key")
	}
	if len(publicWitness) != len(vk.G1.K)-nc-1 {
		return errors.New("mi355x: wrong number of public inputs")
	}
	// verify.go: commitment i is hashed with the public committed values before it (later commitments may commit to earlier ones)
	values := make([]fr.Element, nc)
	full := append(fr.Vector{}, publicWitness...)
	h2f := hash_to_field.New([]byte(constraint.CommitmentDst))
	maxNb := 0
	for _, s := range vk.PublicAndCommitmentCommitted {
		if len(s) > maxNb {
			maxNb = len(s)
		}
	}
	buf := make([]byte, 0, fr.Bytes*maxNb+bn254.SizeOfG1AffineUncompressed)
	for i := 0; i < nc; i++ {
		buf = append(buf[:0], proof.Commitments[i].Marshal()...)
		for _, j := range vk.PublicAndCommitmentCommitted[i] {
			b := full[j-1].Bytes()
			buf = append(buf, b[:]...)
		}
		h2f.Write(buf)
		values[i].SetBytes(h2f.Sum(nil))
		h2f.Reset()
		full = append(full, values[i])
	}
	var challenge fr.Element
	if nc > 0 {
		ser := make([]byte, fr.Bytes*nc)
		for i := range values {
			copy(ser[fr.Bytes*i:], values[i].Marshal())
		}
		ch, err := fr.Hash(ser, []byte("G16-BSB22"), 1)
		if err != nil {
			return err
		}
		challenge = ch[0]
	}

	var pin runtime.Pinner
	defer pin.Unpin()
	var in C.mi_verify_input
	in.proof.ar = *(*C.mi_g1_affine)(unsafe.Pointer(&proof.Ar))
	in.proof.bs = *(*C.mi_g2_affine)(unsafe.Pointer(&proof.Bs))
	in.proof.krs = *(*C.mi_g1_affine)(unsafe.Pointer(&proof.Krs))
	if len(publicWitness) > 0 {
		pin.Pin(&publicWitness[0])
		in.public_inputs = (*C.mi_fr)(unsafe.Pointer(&publicWitness[0]))
	}
	if nc > 0 {
		in.commitments = g1(&pin, proof.Commitments)
		pin.Pin(&proof.CommitmentPok)
		in.pok = (*C.mi_g1_affine)(unsafe.Pointer(&proof.CommitmentPok))
		pin.Pin(&values[0])
		in.commitment_values = (*C.mi_fr)(unsafe.Pointer(&values[0]))
		pin.Pin(&challenge)
		in.fold_challenge = (*C.mi_fr)(unsafe.Pointer(&challenge))
	}
	var verdict C.uint8_t
	var rc C.int32_t
	if wave {
		rc = C.mi_groth16_verify_wave(vk.ctx, vk.dev, &in, 1, &verdict)
	} else {
		rc = C.mi_groth16_verify(vk.ctx, vk.dev, &in, &verdict)
	}
	if err := status(vk.ctx, rc); err != nil {
		return err
	}
	if verdict != C.MI_VERIFY_OK {
		return ErrRejected{Verdict: int(verdict)}
	}
	return nil
}

// VerifyBytes replaces groth16.Verify for a proof that arrives as Proof.WriteTo's bytes (164 + 32 * commitments): the points are
// decompressed and the BSB22 hashes computed on the device.  No host hashing, no gnark-crypto decoding.
func VerifyBytes(vk *VerifyingKey, proof []byte, publicWitness fr.Vector) error {
	return verifyBytes(vk, proof, publicWitness, false)
}

// VerifyBytesWave is VerifyBytes through mi_groth16_verify_bytes_wave (see VerifyWave).
func VerifyBytesWave(vk *VerifyingKey, proof []byte, publicWitness fr.Vector) error {
	return verifyBytes(vk, proof, publicWitness, true)
}

func verifyBytes(vk *VerifyingKey, proof []byte, publicWitness fr.Vector, wave bool) error {
	nc := len(vk.PublicAndCommitmentCommitted)
	if len(publicWitness) != len(vk.G1.K)-nc-1 {
		return errors.New("mi355x: wrong number of public inputs")
	}
	if len(proof) == 0 {
		return errors.New("mi355x: empty proof")
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&proof[0])
	var pub *C.mi_fr
	if len(publicWitness) > 0 {
		pin.Pin(&publicWitness[0])
		pub = (*C.mi_fr)(unsafe.Pointer(&publicWitness[0]))
	}
	var verdict C.uint8_t
	var rc C.int32_t
	if wave {
		in := C.mi_verify_bytes_input{proof: (*C.uint8_t)(unsafe.Pointer(&proof[0])), proof_len: C.size_t(len(proof)), public_inputs: pub}
		rc = C.mi_groth16_verify_bytes_wave(vk.ctx, vk.dev, &in, 1, &verdict)
	} else {
		rc = C.mi_groth16_verify_bytes(vk.ctx, vk.dev, (*C.uint8_t)(unsafe.Pointer(&proof[0])), C.size_t(len(proof)), pub, &verdict)
	}
	if err := status(vk.ctx, rc); err != nil {
		return err
	}
	if verdict != C.MI_VERIFY_OK {
		return ErrRejected{Verdict: int(verdict)}
	}
	return nil
}

// ErrBatchRejected carries the ONE verdict of a rejected batch.  FirstMalformed is the lowest malformed index when Verdict is
// MI_VERIFY_MALFORMED; verdicts MI_VERIFY_PAIRING and MI_VERIFY_PEDERSEN do not say which proof is at fault (VerifyBytes on each does).
type ErrBatchRejected struct {
	Verdict        int
	FirstMalformed uint64
}

func (e ErrBatchRejected) Error() string {
	return fmt.Sprintf("mi355x: batch rejected (verdict %d, first malformed %d)", e.Verdict, e.FirstMalformed)
}

// VerifyBytesCombined judges n proofs under one key by one pairing product: the random linear combination of their equations
// (include/mi355x_groth16_verify_combined.h).  The library draws the seed of the coefficients from the operating system, so a batch
// with a rejected proof passes with probability about 2^-128; a batch of accepted proofs always passes.  proofs[i] is Proof.WriteTo's
// bytes, publicWitnesses[i] its public inputs without the ONE wire.
func VerifyBytesCombined(vk *VerifyingKey, proofs [][]byte, publicWitnesses []fr.Vector) error {
	if len(proofs) != len(publicWitnesses) {
		return errors.New("mi355x: one public witness per proof")
	}
	if len(proofs) == 0 {
		return nil
	}
	nc := len(vk.PublicAndCommitmentCommitted)
	var pin runtime.Pinner
	defer pin.Unpin()
	in := (*[1 << 24]C.mi_verify_bytes_input)(C.calloc(C.size_t(len(proofs)), C.size_t(unsafe.Sizeof(C.mi_verify_bytes_input{}))))
	defer C.free(unsafe.Pointer(in))
	for i, p := range proofs {
		if len(publicWitnesses[i]) != len(vk.G1.K)-nc-1 {
			return errors.New("mi355x: wrong number of public inputs")
		}
		if len(p) == 0 {
			return errors.New("mi355x: empty proof")
		}
		pin.Pin(&p[0])
		in[i].proof = (*C.uint8_t)(unsafe.Pointer(&p[0]))
		in[i].proof_len = C.size_t(len(p))
		if len(publicWitnesses[i]) > 0 {
			pin.Pin(&publicWitnesses[i][0])
			in[i].public_inputs = (*C.mi_fr)(unsafe.Pointer(&publicWitnesses[i][0]))
		}
	}
	var verdict C.uint8_t
	var first C.uint64_t
	rc := C.mi_groth16_verify_bytes_combined(vk.ctx, vk.dev, &in[0], C.size_t(len(proofs)), nil, &verdict, &first)
	if err := status(vk.ctx, rc); err != nil {
		return err
	}
	if verdict != C.MI_VERIFY_OK {
		return ErrBatchRejected{Verdict: int(verdict), FirstMalformed: uint64(first)}
	}
	return nil
}

// VerifyFiles replaces groth16.Verify for a verifier that holds files: proof is Proof.WriteTo's bytes, witness is witness.WriteTo's
// (public, or full: the secret part is not read).  The public inputs go up as bytes and become Montgomery words on the device; a value
// that is not below r, or a header whose count is not the key's, rejects the proof as malformed.
func VerifyFiles(vk *VerifyingKey, proof []byte, witness []byte) error {
	if len(proof) == 0 || len(witness) == 0 {
		return errors.New("mi355x: empty proof or witness")
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&proof[0])
	pin.Pin(&witness[0])
	var verdict C.uint8_t
	rc := C.mi_groth16_verify_files(vk.ctx, vk.dev, (*C.uint8_t)(unsafe.Pointer(&proof[0])), C.size_t(len(proof)),
		(*C.uint8_t)(unsafe.Pointer(&witness[0])), C.size_t(len(witness)), &verdict)
	if err := status(vk.ctx, rc); err != nil {
		return err
	}
	if verdict != C.MI_VERIFY_OK {
		return ErrRejected{Verdict: int(verdict)}
	}
	return nil
}

// VerifyFilesCombined is VerifyBytesCombined over (proof bytes, witness bytes) pairs.
func VerifyFilesCombined(vk *VerifyingKey, proofs [][]byte, witnesses [][]byte) error {
	if len(proofs) != len(witnesses) {
		return errors.New("mi355x: one witness per proof")
	}
	if len(proofs) == 0 {
		return nil
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	in := (*[1 << 24]C.mi_verify_files_input)(C.calloc(C.size_t(len(proofs)), C.size_t(unsafe.Sizeof(C.mi_verify_files_input{}))))
	defer C.free(unsafe.Pointer(in))
	for i, p := range proofs {
		if len(p) == 0 || len(witnesses[i]) == 0 {
			return errors.New("mi355x: empty proof or witness")
		}
		pin.Pin(&p[0])
		pin.Pin(&witnesses[i][0])
		in[i].proof = (*C.uint8_t)(unsafe.Pointer(&p[0]))
		in[i].proof_len = C.size_t(len(p))
		in[i].witness = (*C.uint8_t)(unsafe.Pointer(&witnesses[i][0]))
		in[i].witness_len = C.size_t(len(witnesses[i]))
	}
	var verdict C.uint8_t
	var first C.uint64_t
	rc := C.mi_groth16_verify_files_combined(vk.ctx, vk.dev, &in[0], C.size_t(len(proofs)), nil, &verdict, &first)
	if err := status(vk.ctx, rc); err != nil {
		return err
	}
	if verdict != C.MI_VERIFY_OK {
		return ErrBatchRejected{Verdict: int(verdict), FirstMalformed: uint64(first)}
	}
	return nil
}
