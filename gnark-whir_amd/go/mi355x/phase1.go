//go:build mi355x

// The powers-of-tau SRS itself, made on the device: include/mi355x_groth16_phase1.h.
//
// STATUS: SOURCE ONLY, like the rest of the shim (mi355x.go): never compiled here.  It stands where gnark's mpcsetup phase 1 stands:
//
//	p1 := mpcsetup.InitPhase1(power)            p1, err := mi355x.InitPhase1(logN, device)
//	p1.Contribute()                             rec, err := p1.ContributeProved(tau, alpha, beta)   // the caller samples them and forgets them
//	mpcsetup.VerifyPhase1(&prev, &next)         failed, firstBad, err := mine.VerifyAdopt(claimedSRS, recs)
//	mpcsetup.InitPhase2(r1cs, &p1)              p2, err := p1.InitPhase2(r1cs, sigma)               // the rows never leave the device
//
// The records are this project's own format (three Schnorr proofs under one challenge, chained by SHA-256), not gnark's; gnark's Phase1
// file format is not available to this project, so the rows cross this interface as the SRS of phase2.go.
package mi355x

/*
#include <stdlib.h>
#include "mi355x_groth16_phase1.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
	cs "github.com/consensys/gnark/constraint/bn254"
)

// The bits VerifyAdopt adds to CheckSRS's mask (MI_PHASE1_BAD_*).
const (
	Phase1BadRecord = 64
	Phase1BadLink   = 128
)

// Phase1 is the device-resident state of a phase-1 ceremony: the rows of an SRS for a domain of 2^logN, a record count and a chain value.
type Phase1 struct {
	ctx *C.mi_ctx
	st  *C.mi_phase1
}

// Phase1Record is one contribution's proof of knowledge of (tau, alpha, beta): mi_phase1_record, word for word.
type Phase1Record struct {
	Tau1, Alpha1, Beta1 bn254.G1Affine // tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] after the step
	Commit              [3]bn254.G1Affine
	Response            [3]fr.Element
	Hash                [32]byte
}

func newPhase1(device int) (*Phase1, error) {
	p := &Phase1{}
	if rc := C.mi_init(C.int(device), &p.ctx); rc != C.MI_OK {
		return nil, fmt.Errorf("mi355x: mi_init rc=%d (no gfx950 device?)", int(rc))
	}
	return p, nil
}

// InitPhase1 starts a ceremony: every row the generator (tau = alpha = beta = 1).
func InitPhase1(logN uint32, device int) (*Phase1, error) {
	p, err := newPhase1(device)
	if err != nil {
		return nil, err
	}
	if err = status(p.ctx, C.mi_phase1_init(p.ctx, C.uint32_t(logN), &p.st)); err != nil {
		C.mi_shutdown(p.ctx)
		return nil, err
	}
	return p, nil
}

// Phase1FromSRS takes an existing SRS in, for a domain of n (a power of two): every point is checked as InitPhase2 checks it.  The rows
// are not tested for being powers: Check does that.
func Phase1FromSRS(srs *SRS, n uint64, device int) (*Phase1, error) {
	if srs == nil {
		return nil, errors.New("mi355x: nil SRS")
	}
	p, err := newPhase1(device)
	if err != nil {
		return nil, err
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	s := srsDesc(&pin, srs)
	if err = status(p.ctx, C.mi_phase1_from_srs(p.ctx, &s, C.uint64_t(n), 0, &p.st)); err != nil {
		C.mi_shutdown(p.ctx)
		return nil, err
	}
	return p, nil
}

// SetTranscriptID names the ceremony: the value the first record's hash continues.  Only before the first record.
func (p *Phase1) SetTranscriptID(id [32]byte) error {
	return status(p.ctx, C.mi_phase1_set_transcript_id(p.ctx, p.st, (*C.uint8_t)(unsafe.Pointer(&id[0]))))
}

// ContributeProved multiplies tau, alpha, beta by the caller's values (none zero) and returns the record of the step; the nonces are
// the library's.  The caller forgets the three values.
func (p *Phase1) ContributeProved(tau, alpha, beta fr.Element) (Phase1Record, error) {
	var r Phase1Record
	err := status(p.ctx, C.mi_phase1_contribute_proved(p.ctx, p.st, (*C.mi_fr)(unsafe.Pointer(&tau)), (*C.mi_fr)(unsafe.Pointer(&alpha)),
		(*C.mi_fr)(unsafe.Pointer(&beta)), nil, (*C.mi_phase1_record)(unsafe.Pointer(&r))))
	return r, err
}

// VerifyPhase1Records checks the chain of records continuing (start = tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] before the first of them,
// startHash, firstIndex) on the host; firstBad == len(recs): all hold.
func VerifyPhase1Records(start [3]bn254.G1Affine, startHash [32]byte, firstIndex uint64, recs []Phase1Record) (firstBad uint64, err error) {
	var rp *C.mi_phase1_record
	if len(recs) > 0 {
		rp = (*C.mi_phase1_record)(unsafe.Pointer(&recs[0]))
	}
	var fb C.uint64_t
	if rc := C.mi_phase1_records_verify((*C.mi_g1_affine)(unsafe.Pointer(&start[0])), (*C.uint8_t)(unsafe.Pointer(&startHash[0])), C.uint64_t(firstIndex),
		rp, C.size_t(len(recs)), &fb); rc != C.MI_OK {
		return 0, fmt.Errorf("mi355x: mi_phase1_records_verify rc=%d", int(rc))
	}
	return uint64(fb), nil
}

// VerifyAdopt checks a contributor's claimed rows and records against this state, which stands where the contributor started, and,
// when failed == 0 and only then, takes the rows over and advances the chain by the records.  failed: the SRSBad* bits over the claim,
// Phase1BadRecord, Phase1BadLink.  The seed of the tests' coefficients is the operating system's.
func (p *Phase1) VerifyAdopt(claim *SRS, recs []Phase1Record) (failed uint32, firstBadRecord uint64, err error) {
	if claim == nil || len(recs) == 0 {
		return 0, 0, errors.New("mi355x: nil claim or no record")
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	s := srsDesc(&pin, claim)
	var mask C.uint32_t
	var fb C.uint64_t
	err = status(p.ctx, C.mi_phase1_verify_adopt(p.ctx, p.st, &s, (*C.mi_phase1_record)(unsafe.Pointer(&recs[0])), C.size_t(len(recs)), nil, &mask, &fb))
	return uint32(mask), uint64(fb), err
}

// Check runs CheckSRS's relations over the state's own rows, where they are.
func (p *Phase1) Check() (failed uint32, err error) {
	var mask C.uint32_t
	err = status(p.ctx, C.mi_phase1_check(p.ctx, p.st, nil, &mask))
	return uint32(mask), err
}

// Export copies the rows to the host.
func (p *Phase1) Export() (*SRS, error) {
	var n [4]C.uint64_t
	if err := status(p.ctx, C.mi_phase1_export(p.ctx, p.st, nil, nil, nil, nil, nil, 0, 0, 0, 0, &n[0])); err != nil {
		return nil, err
	}
	srs := &SRS{TauG1: make([]bn254.G1Affine, n[0]), AlphaTauG1: make([]bn254.G1Affine, n[1]), BetaTauG1: make([]bn254.G1Affine, n[2]),
		TauG2: make([]bn254.G2Affine, n[3])}
	var pin runtime.Pinner
	defer pin.Unpin()
	err := status(p.ctx, C.mi_phase1_export(p.ctx, p.st, g1(&pin, srs.TauG1), g1(&pin, srs.AlphaTauG1), g1(&pin, srs.BetaTauG1), g2(&pin, srs.TauG2),
		(*C.mi_g2_affine)(unsafe.Pointer(&srs.BetaG2)), n[0], n[1], n[2], n[3], &n[0]))
	if err != nil {
		return nil, err
	}
	return srs, nil
}

// InitPhase2 derives the circuit's keys from the state's rows on the device (InitPhase2 of phase2.go without the trip to the host).  The
// Phase2 works on this state's context: close it before closing the Phase1.
func (p *Phase1) InitPhase2(r1cs *cs.R1CS, sigma []fr.Element) (*Phase2, error) {
	if r1cs == nil {
		return nil, errors.New("mi355x: nil constraint system")
	}
	p2 := &Phase2{ctx: p.ctx, borrowed: true}
	err := initPhase2(p2, r1cs, sigma, func(_ *runtime.Pinner, d *C.mi_r1cs_desc, sg *C.mi_fr) C.int32_t {
		return C.mi_phase2_init_from_phase1(p.ctx, d, p.st, sg, 0, &p2.st)
	})
	if err != nil {
		return nil, err
	}
	return p2, nil
}

// Close frees the state and its context.
func (p *Phase1) Close() {
	if p.st != nil {
		C.mi_phase1_free(p.ctx, p.st)
		p.st = nil
	}
	if p.ctx != nil {
		C.mi_shutdown(p.ctx)
		p.ctx = nil
	}
}
