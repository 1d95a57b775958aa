//go:build mi355x

// The circuit's keys from a powers-of-tau SRS, on the device: include/mi355x_groth16_phase2.h.
//
// STATUS: SOURCE ONLY, like the rest of the shim (mi355x.go): never compiled here.  It stands where gnark's mpcsetup stands:
//
//	p2 := mpcsetup.InitPhase2(r1cs, &srs)      p2, err := mi355x.InitPhase2(r1cs, srs, sigma, device)
//	p2.Contribute()                            err = p2.Contribute(delta, nil)        // the caller samples delta and forgets it
//	pk, vk := mpcsetup.ExtractKeys(...)        pkBytes, vkBytes, err := p2.Streams(mi355x.KeyCompressed)
//
// The keys leave as the streams of keyfile.go (LoadKeyStream / LoadVerifyingKeyStream read them back in any later process).
// What makes the result checkable (include/mi355x_groth16_phase2_check.h) is at the end of this file: CheckSRS (the pairing check
// that the rows are consistent powers; call it before InitPhase2), ContributeProved (a contribution with its Schnorr record),
// VerifyRecords and VerifyAdopt (a contributor's claimed state checked against one's own, then taken over), and the same for the
// commitment keys' sigma: ContributeSigmaProved, VerifySigmaRecords, VerifyAdoptSigma, ChainInfo, and PedersenVK for the verifying half
// of a sealed key -- a ceremony starts from sigma = 1 and nobody holds the scalar.  NOT here, and not in the
// library: gnark's mpcsetup file formats (their layout is not available to this project: the SRS and the records cross this interface
// as slices, in this project's own layout).  The SRS itself comes from a ceremony of its own: phase1.go.  The walk
// over gnark's constraints below
// (GetR1Cs, Term.CoeffID / WireID) is written from memory of gnark v0.11 and has never been compiled.
package mi355x

/*
#include <stdlib.h>
#include "mi355x_groth16_phase2.h"
#include "mi355x_groth16_phase2_check.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
	"github.com/consensys/gnark/constraint"
	cs "github.com/consensys/gnark/constraint/bn254"
)

// SRS is a powers-of-tau string: [tau^k]1 for k < 2N, [alpha tau^k]1, [beta tau^k]1 and [tau^k]2 for k < N, and [beta]2, where N is the
// circuit's domain size.  Longer rows are fine: only what the circuit needs is read.
type SRS struct {
	TauG1, AlphaTauG1, BetaTauG1 []bn254.G1Affine
	TauG2                        []bn254.G2Affine
	BetaG2                       bn254.G2Affine
}

// Phase2 is the device-resident state of a ceremony for one circuit.
type Phase2 struct {
	ctx      *C.mi_ctx
	st       *C.mi_phase2
	borrowed bool // the context is a Phase1's (Phase1.InitPhase2): Close leaves it alone
}

// csr is one matrix of the R1CS by rows: mi_r1cs_matrix.
type csr struct {
	rowPtr []uint64
	col    []uint32
	coeff  []uint32
}

func csrOf(r1cs *cs.R1CS) (a, b, c csr) {
	rows := r1cs.GetR1Cs()
	for _, m := range []*csr{&a, &b, &c} {
		m.rowPtr = make([]uint64, 1, len(rows)+1)
	}
	for _, r := range rows {
		for k, le := range []constraint.LinearExpression{r.L, r.R, r.O} {
			m := []*csr{&a, &b, &c}[k]
			for _, t := range le {
				m.col = append(m.col, uint32(t.WireID()))
				m.coeff = append(m.coeff, uint32(t.CoeffID()))
			}
			m.rowPtr = append(m.rowPtr, uint64(len(m.col)))
		}
	}
	return
}

// InitPhase2 derives the circuit's keys from srs with delta = 1.  sigma holds one value per BSB22 commitment of the circuit.
// Every SRS point is checked on the device (on its curve, in the r-torsion, not at infinity); the error names the row and the index.
func InitPhase2(r1cs *cs.R1CS, srs *SRS, sigma []fr.Element, device int) (*Phase2, error) {
	if r1cs == nil || srs == nil {
		return nil, errors.New("mi355x: nil constraint system or SRS")
	}
	p := &Phase2{}
	if rc := C.mi_init(C.int(device), &p.ctx); rc != C.MI_OK {
		return nil, fmt.Errorf("mi355x: mi_init rc=%d (no gfx950 device?)", int(rc))
	}
	err := initPhase2(p, r1cs, sigma, func(pin *runtime.Pinner, d *C.mi_r1cs_desc, sg *C.mi_fr) C.int32_t {
		s := srsDesc(pin, srs)
		return C.mi_phase2_init(p.ctx, d, &s, sg, 0, &p.st)
	})
	if err != nil {
		C.mi_shutdown(p.ctx)
		return nil, err
	}
	return p, nil
}

// initPhase2 lays the constraint system out as mi_r1cs_desc and hands it to call, which runs mi_phase2_init or its phase-1 form on p.ctx.
func initPhase2(p *Phase2, r1cs *cs.R1CS, sigma []fr.Element, call func(pin *runtime.Pinner, d *C.mi_r1cs_desc, sg *C.mi_fr) C.int32_t) error {
	var pin runtime.Pinner
	defer pin.Unpin()
	a, b, c := csrOf(r1cs)
	var d C.mi_r1cs_desc
	d.n_constraints = C.uint64_t(r1cs.GetNbConstraints())
	d.nb_wires = C.uint64_t(r1cs.NbInternalVariables + r1cs.GetNbPublicVariables() + r1cs.GetNbSecretVariables())
	d.nb_public = C.uint32_t(r1cs.GetNbPublicVariables())
	for k, m := range []*csr{&a, &b, &c} {
		dst := []*C.mi_r1cs_matrix{&d.A, &d.B, &d.C}[k]
		pin.Pin(&m.rowPtr[0])
		dst.row_ptr = (*C.uint64_t)(unsafe.Pointer(&m.rowPtr[0]))
		if len(m.col) > 0 {
			pin.Pin(&m.col[0])
			pin.Pin(&m.coeff[0])
			dst.col = (*C.uint32_t)(unsafe.Pointer(&m.col[0]))
			dst.coeff = (*C.uint32_t)(unsafe.Pointer(&m.coeff[0]))
		}
	}
	pin.Pin(&r1cs.Coefficients[0])
	d.coeffs = (*C.mi_fr)(unsafe.Pointer(&r1cs.Coefficients[0]))
	d.n_coeffs = C.uint64_t(len(r1cs.Coefficients))
	info := r1cs.CommitmentInfo.(constraint.Groth16Commitments)
	committed := info.GetPrivateCommitted()
	wires := info.CommitmentIndexes()
	if len(sigma) != len(committed) {
		return fmt.Errorf("mi355x: %d sigma values for %d commitments", len(sigma), len(committed))
	}
	if n := len(committed); n > 0 {
		lists := make([][]uint32, n)
		ptrs := (*[1 << 20]*C.uint32_t)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
		defer C.free(unsafe.Pointer(ptrs))
		counts := make([]uint64, n)
		cw := make([]uint32, n)
		for k := range committed {
			lists[k] = make([]uint32, len(committed[k]))
			for i, w := range committed[k] {
				lists[k][i] = uint32(w)
			}
			if len(lists[k]) > 0 { // an empty list keeps a nil pointer beside its count of 0
				pin.Pin(&lists[k][0])
				ptrs[k] = (*C.uint32_t)(unsafe.Pointer(&lists[k][0]))
			}
			counts[k] = uint64(len(committed[k]))
			cw[k] = uint32(wires[k])
		}
		pin.Pin(&counts[0])
		pin.Pin(&cw[0])
		d.n_commitments = C.uint32_t(n)
		d.committed = (**C.uint32_t)(unsafe.Pointer(ptrs))
		d.n_committed = (*C.uint64_t)(unsafe.Pointer(&counts[0]))
		d.commitment_wire = (*C.uint32_t)(unsafe.Pointer(&cw[0]))
	}
	var sg *C.mi_fr
	if len(sigma) > 0 {
		pin.Pin(&sigma[0])
		sg = (*C.mi_fr)(unsafe.Pointer(&sigma[0]))
	}
	return status(p.ctx, call(&pin, &d, sg))
}

// Contribute re-randomises delta (and, per commitment, sigma: nil leaves every sigma as it is).  Zero is refused.
func (p *Phase2) Contribute(delta fr.Element, sigmaFactor []fr.Element) error {
	var sf *C.mi_fr
	if len(sigmaFactor) > 0 {
		sf = (*C.mi_fr)(unsafe.Pointer(&sigmaFactor[0]))
	}
	return status(p.ctx, C.mi_phase2_contribute(p.ctx, p.st, (*C.mi_fr)(unsafe.Pointer(&delta)), sf))
}

// Streams writes both keys as they stand: ProvingKey.WriteTo / VerifyingKey.WriteTo for KeyCompressed, the raw forms for KeyRaw.
// The state lives on: it can be contributed to and written again.
func (p *Phase2) Streams(encoding int) (pk []byte, vk []byte, err error) {
	var n, nvk C.size_t
	C.mi_phase2_to_streams(p.ctx, p.st, C.uint32_t(encoding), nil, 0, &n, nil, 0, &nvk) // the sizes
	if n == 0 || nvk == 0 {
		return nil, nil, errors.New("mi355x: unknown encoding")
	}
	pk, vk = make([]byte, int(n)), make([]byte, int(nvk))
	rc := C.mi_phase2_to_streams(p.ctx, p.st, C.uint32_t(encoding), (*C.uint8_t)(unsafe.Pointer(&pk[0])), n, &n,
		(*C.uint8_t)(unsafe.Pointer(&vk[0])), nvk, &nvk)
	if err = status(p.ctx, rc); err != nil {
		return nil, nil, err
	}
	return pk, vk, nil
}

// The relations of CheckSRS's mask (MI_SRS_BAD_*) and of VerifyAdopt's (MI_PHASE2_BAD_*).
const (
	SRSBadGenerators = 1 << iota
	SRSBadTauG1
	SRSBadAlphaG1
	SRSBadBetaG1
	SRSBadTauG2
	SRSBadBetaG2
)
const (
	Phase2BadRecord = 1 << iota
	Phase2BadDelta
	Phase2BadZ
	Phase2BadK
	Phase2BadSigmaRecord // VerifyAdoptSigma's bits from here on (MI_PHASE2_BAD_SIGMA_RECORD, _SIGMA_LINK, _BES)
	Phase2BadSigmaLink
	Phase2BadBES
)

// Record is one contribution's proof of knowledge: mi_phase2_record, word for word.
type Record struct {
	Delta1, Commit bn254.G1Affine
	Response       fr.Element
	Hash           [32]byte
}

// Claim is what a contributor hands over: the arrays of mi_phase2_get_array (MI_PHASE2_G1_Z, MI_PHASE2_G1_K) and the two delta points.
type Claim struct {
	Z, K   []bn254.G1Affine
	Delta1 bn254.G1Affine
	Delta2 bn254.G2Affine
}

func srsDesc(pin *runtime.Pinner, srs *SRS) (s C.mi_srs_desc) {
	s.tau_g1, s.n_tau_g1 = g1(pin, srs.TauG1), C.uint64_t(len(srs.TauG1))
	s.alpha_tau_g1, s.n_alpha_tau_g1 = g1(pin, srs.AlphaTauG1), C.uint64_t(len(srs.AlphaTauG1))
	s.beta_tau_g1, s.n_beta_tau_g1 = g1(pin, srs.BetaTauG1), C.uint64_t(len(srs.BetaTauG1))
	s.tau_g2, s.n_tau_g2 = g2(pin, srs.TauG2), C.uint64_t(len(srs.TauG2))
	s.beta_g2 = *(*C.mi_g2_affine)(unsafe.Pointer(&srs.BetaG2))
	return
}

// CheckSRS decides by pairings whether the rows are [tau^k]1, [alpha tau^k]1, [beta tau^k]1, [tau^k]2, [beta]2 for one (tau, alpha,
// beta), for a circuit of domain size n (a power of two).  failed == 0: they are.  The seed of the test's coefficients is the
// operating system's: never pass one the maker of the SRS could have known.
func CheckSRS(srs *SRS, n uint64, device int) (failed uint32, err error) {
	var ctx *C.mi_ctx
	if rc := C.mi_init(C.int(device), &ctx); rc != C.MI_OK {
		return 0, fmt.Errorf("mi355x: mi_init rc=%d (no gfx950 device?)", int(rc))
	}
	defer C.mi_shutdown(ctx)
	var pin runtime.Pinner
	defer pin.Unpin()
	s := srsDesc(&pin, srs)
	var mask C.uint32_t
	err = status(ctx, C.mi_srs_check_powers(ctx, &s, C.uint64_t(n), nil, 0, &mask))
	return uint32(mask), err
}

// SetTranscriptID names the ceremony: the value the first record's hash continues.  Only before the first record.
func (p *Phase2) SetTranscriptID(id [32]byte) error {
	return status(p.ctx, C.mi_phase2_set_transcript_id(p.ctx, p.st, (*C.uint8_t)(unsafe.Pointer(&id[0]))))
}

// ContributeProved re-randomises delta as Contribute(delta, nil) does and returns the record of the step (the nonce is the library's).
func (p *Phase2) ContributeProved(delta fr.Element) (Record, error) {
	var r Record
	err := status(p.ctx, C.mi_phase2_contribute_proved(p.ctx, p.st, (*C.mi_fr)(unsafe.Pointer(&delta)), nil, (*C.mi_phase2_record)(unsafe.Pointer(&r))))
	return r, err
}

// VerifyRecords checks the chain of records continuing (delta1Start, startHash, firstIndex) on the host; firstBad == len(recs): all hold.
func VerifyRecords(delta1Start bn254.G1Affine, startHash [32]byte, firstIndex uint64, recs []Record) (firstBad uint64, err error) {
	var rp *C.mi_phase2_record
	if len(recs) > 0 {
		rp = (*C.mi_phase2_record)(unsafe.Pointer(&recs[0]))
	}
	var fb C.uint64_t
	if rc := C.mi_phase2_records_verify((*C.mi_g1_affine)(unsafe.Pointer(&delta1Start)), (*C.uint8_t)(unsafe.Pointer(&startHash[0])), C.uint64_t(firstIndex),
		rp, C.size_t(len(recs)), &fb); rc != C.MI_OK {
		return 0, fmt.Errorf("mi355x: mi_phase2_records_verify rc=%d", int(rc))
	}
	return uint64(fb), nil
}

// VerifyAdopt checks a contributor's claim and records against this state and, when failed == 0 and only then, takes the claimed
// arrays over and advances the chain by the records.
func (p *Phase2) VerifyAdopt(c *Claim, recs []Record) (failed uint32, firstBadRecord uint64, err error) {
	if c == nil || len(recs) == 0 {
		return 0, 0, errors.New("mi355x: nil claim or no record")
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	var cl C.mi_phase2_claim
	cl.g1_z, cl.n_z = g1(&pin, c.Z), C.uint64_t(len(c.Z))
	cl.g1_k, cl.n_k = g1(&pin, c.K), C.uint64_t(len(c.K))
	cl.delta1 = *(*C.mi_g1_affine)(unsafe.Pointer(&c.Delta1))
	cl.delta2 = *(*C.mi_g2_affine)(unsafe.Pointer(&c.Delta2))
	var mask C.uint32_t
	var fb C.uint64_t
	err = status(p.ctx, C.mi_phase2_verify_adopt(p.ctx, p.st, &cl, (*C.mi_phase2_record)(unsafe.Pointer(&recs[0])), C.size_t(len(recs)), nil, &mask, &fb))
	return uint32(mask), uint64(fb), err
}

// PedersenVK is one commitment's verifying pair: mi_pedersen_vk, word for word.
type PedersenVK struct {
	G, GSigmaNeg bn254.G2Affine
}

// SigmaProof is one commitment's part of a step of the sigma chain: mi_phase2_sigma_proof, word for word.
type SigmaProof struct {
	GSigmaNeg, Commit bn254.G2Affine
	Response          fr.Element
}

// SigmaClaim is what a contributor to sigma hands over: per commitment the array of mi_phase2_get_array (MI_PHASE2_BASIS + 2k + 1)
// and the point [-sigma_k]2.
type SigmaClaim struct {
	BasisExpSigma [][]bn254.G1Affine
	GSigmaNeg     []bn254.G2Affine
}

// ChainInfo says where the two chains of a state stand: mi_phase2_chain_info.
type ChainInfo struct {
	NCommitments  uint32
	NRecords      uint64
	Chain         [32]byte
	NSigmaRecords uint64
	SigmaChain    [32]byte
}

// PedersenVK returns the pairs {g2, [-sigma_k]2} of the state's points: what goes into the verifying key of a sealed state.
func (p *Phase2) PedersenVK() ([]PedersenVK, error) {
	info, err := p.ChainInfo()
	if err != nil || info.NCommitments == 0 {
		return nil, err
	}
	out := make([]PedersenVK, info.NCommitments)
	err = status(p.ctx, C.mi_phase2_get_pedersen_vk(p.ctx, p.st, (*C.mi_pedersen_vk)(unsafe.Pointer(&out[0]))))
	return out, err
}

// ChainInfo reads the record counts and chain values of the delta chain and of the sigma chain.
func (p *Phase2) ChainInfo() (ChainInfo, error) {
	var ci C.mi_phase2_chain_info
	if err := status(p.ctx, C.mi_phase2_get_chain_info(p.ctx, p.st, &ci)); err != nil {
		return ChainInfo{}, err
	}
	out := ChainInfo{NCommitments: uint32(ci.n_commitments), NRecords: uint64(ci.n_records), NSigmaRecords: uint64(ci.n_sigma_records)}
	copy(out.Chain[:], C.GoBytes(unsafe.Pointer(&ci.chain[0]), 32))
	copy(out.SigmaChain[:], C.GoBytes(unsafe.Pointer(&ci.sigma_chain[0]), 32))
	return out, nil
}

// ContributeSigmaProved re-randomises every commitment's sigma as Contribute(1, sigmaFactor) does and returns the step: one proof per
// commitment and the chain value after it (the nonces are the library's).  One factor per commitment.
func (p *Phase2) ContributeSigmaProved(sigmaFactor []fr.Element) ([]SigmaProof, [32]byte, error) {
	var h [32]byte
	if len(sigmaFactor) == 0 {
		return nil, h, errors.New("mi355x: no sigma factor")
	}
	out := make([]SigmaProof, len(sigmaFactor))
	err := status(p.ctx, C.mi_phase2_contribute_sigma_proved(p.ctx, p.st, (*C.mi_fr)(unsafe.Pointer(&sigmaFactor[0])), nil,
		(*C.mi_phase2_sigma_proof)(unsafe.Pointer(&out[0])), (*C.uint8_t)(unsafe.Pointer(&h[0]))))
	return out, h, err
}

// VerifySigmaRecords checks the chain of len(hashes) steps (proofs: len(start) per step) continuing (start, startHash, firstIndex) on
// the host; firstBad == len(hashes): all hold.
func VerifySigmaRecords(start []bn254.G2Affine, startHash [32]byte, firstIndex uint64, proofs []SigmaProof, hashes [][32]byte) (firstBad uint64, err error) {
	if len(start) == 0 || len(proofs) != len(start)*len(hashes) {
		return 0, errors.New("mi355x: no start point, or proofs that are not one per commitment and step")
	}
	var pp *C.mi_phase2_sigma_proof
	var hp *[32]C.uint8_t
	if len(hashes) > 0 {
		pp = (*C.mi_phase2_sigma_proof)(unsafe.Pointer(&proofs[0]))
		hp = (*[32]C.uint8_t)(unsafe.Pointer(&hashes[0]))
	}
	var fb C.uint64_t
	if rc := C.mi_phase2_sigma_records_verify((*C.mi_g2_affine)(unsafe.Pointer(&start[0])), C.uint32_t(len(start)), (*C.uint8_t)(unsafe.Pointer(&startHash[0])),
		C.uint64_t(firstIndex), pp, hp, C.size_t(len(hashes)), &fb); rc != C.MI_OK {
		return 0, fmt.Errorf("mi355x: mi_phase2_sigma_records_verify rc=%d", int(rc))
	}
	return uint64(fb), nil
}

// VerifyAdoptSigma checks a contributor's claimed BasisExpSigma arrays and [-sigma]2 points and the steps against this state and, when
// failed == 0 and only then, takes them over and advances the sigma chain.  badCommitments has bit k set where commitment k's
// relation fails.  The seed of the test's coefficients is the operating system's.
func (p *Phase2) VerifyAdoptSigma(c *SigmaClaim, proofs []SigmaProof, hashes [][32]byte) (failed uint32, badCommitments, firstBadRecord uint64, err error) {
	if c == nil || len(hashes) == 0 || len(c.BasisExpSigma) == 0 || len(c.BasisExpSigma) != len(c.GSigmaNeg) || len(proofs) != len(hashes)*len(c.GSigmaNeg) {
		return 0, 0, 0, errors.New("mi355x: nil claim, no step, or counts that do not agree")
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	nc := len(c.BasisExpSigma)
	// the two per-commitment arrays live in C memory: a Go array of Go pointers may not cross
	ptrs := (*[1 << 20]*C.mi_g1_affine)(C.malloc(C.size_t(nc) * C.size_t(unsafe.Sizeof(uintptr(0)))))
	counts := (*[1 << 20]C.uint64_t)(C.malloc(C.size_t(nc) * 8))
	defer C.free(unsafe.Pointer(ptrs))
	defer C.free(unsafe.Pointer(counts))
	for k, a := range c.BasisExpSigma {
		ptrs[k], counts[k] = g1(&pin, a), C.uint64_t(len(a))
	}
	var cl C.mi_phase2_sigma_claim
	cl.basis_exp_sigma = (**C.mi_g1_affine)(unsafe.Pointer(ptrs))
	cl.n = (*C.uint64_t)(unsafe.Pointer(counts))
	cl.g_sigma_neg = g2(&pin, c.GSigmaNeg)
	var mask C.uint32_t
	var bad, fb C.uint64_t
	err = status(p.ctx, C.mi_phase2_verify_adopt_sigma(p.ctx, p.st, &cl, (*C.mi_phase2_sigma_proof)(unsafe.Pointer(&proofs[0])),
		(*[32]C.uint8_t)(unsafe.Pointer(&hashes[0])), C.size_t(len(hashes)), nil, &mask, &bad, &fb))
	return uint32(mask), uint64(bad), uint64(fb), err
}

// Close frees the state and its context.
func (p *Phase2) Close() {
	if p.st != nil {
		C.mi_phase2_free(p.ctx, p.st)
		p.st = nil
	}
	if p.ctx != nil && !p.borrowed {
		C.mi_shutdown(p.ctx)
	}
	p.ctx = nil
}
