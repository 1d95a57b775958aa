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
// NOT here, and not in the library yet: the pairing check that the SRS rows are consistent powers, the contributions' proofs of
// knowledge and the verification of a transcript, and gnark's mpcsetup file formats (their layout is not available to this project:
// the SRS crosses this interface as slices of points).  The walk over gnark's constraints below (GetR1Cs, Term.CoeffID / WireID)
// is written from memory of gnark v0.11 and has never been compiled.
package mi355x

/*
#include <stdlib.h>
#include "mi355x_groth16_phase2.h"
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
	ctx *C.mi_ctx
	st  *C.mi_phase2
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
		C.mi_shutdown(p.ctx)
		return nil, fmt.Errorf("mi355x: %d sigma values for %d commitments", len(sigma), len(committed))
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
	var s C.mi_srs_desc
	s.tau_g1, s.n_tau_g1 = g1(&pin, srs.TauG1), C.uint64_t(len(srs.TauG1))
	s.alpha_tau_g1, s.n_alpha_tau_g1 = g1(&pin, srs.AlphaTauG1), C.uint64_t(len(srs.AlphaTauG1))
	s.beta_tau_g1, s.n_beta_tau_g1 = g1(&pin, srs.BetaTauG1), C.uint64_t(len(srs.BetaTauG1))
	s.tau_g2, s.n_tau_g2 = g2(&pin, srs.TauG2), C.uint64_t(len(srs.TauG2))
	s.beta_g2 = *(*C.mi_g2_affine)(unsafe.Pointer(&srs.BetaG2))
	var sg *C.mi_fr
	if len(sigma) > 0 {
		pin.Pin(&sigma[0])
		sg = (*C.mi_fr)(unsafe.Pointer(&sigma[0]))
	}
	if err := status(p.ctx, C.mi_phase2_init(p.ctx, &d, &s, sg, 0, &p.st)); err != nil {
		C.mi_shutdown(p.ctx)
		return nil, err
	}
	return p, nil
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

// Close frees the state and its context.
func (p *Phase2) Close() {
	if p.st != nil {
		C.mi_phase2_free(p.ctx, p.st)
		p.st = nil
	}
	if p.ctx != nil {
		C.mi_shutdown(p.ctx)
		p.ctx = nil
	}
}
