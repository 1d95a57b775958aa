//go:build mi355x

// Proving keys as files: include/mi355x_groth16_keyfile.h.
//
// STATUS: SOURCE ONLY, like the rest of the shim (mi355x.go): never compiled here.  LoadKeyStream takes the bytes of
// ProvingKey.WriteTo (compressed) or ProvingKey.WriteRawTo and decodes them on the device, with the checks of gnark's ReadFrom
// (unsafe = UnsafeReadFrom: no membership test of the G2 points).  WriteKeyStream writes a key gnark holds in host memory in either
// encoding through the device's encoders; a key made by mi_groth16_setup is written by mi_groth16_setup_to_stream, at the one
// place where its plain arrays exist.  The stream's layout is recalled, not pinned to gnark (see the header).
//
// Verifying keys as files: include/mi355x_groth16_vkfile.h.  LoadVerifyingKeyStream takes the bytes of VerifyingKey.WriteTo or
// WriteRawTo and decodes them on the device; WriteVerifyingKeyStream writes a key gnark holds in host memory.  Same status, same caveat.
package mi355x

/*
#include <stdlib.h>
#include "mi355x_groth16_keyfile.h"
#include "mi355x_groth16_vkfile.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	groth16_bn254 "github.com/consensys/gnark/backend/groth16/bn254"
	"github.com/consensys/gnark/constraint"
	cs "github.com/consensys/gnark/constraint/bn254"
)

// Stream encodings (MI_KEYFILE_RAW, MI_KEYFILE_COMPRESSED).
const (
	KeyRaw        = 0
	KeyCompressed = 1
)

// LoadKeyStream replaces pk.ReadFrom / pk.UnsafeReadFrom followed by the key upload: data is the whole stream, in either encoding.
// The embedded gnark key stays empty (nothing is decoded on the host); the result proves through Prove like any other ProvingKey.
// nb_public and the wires cut from K come from the constraint system, as for mi_pk_load.
func LoadKeyStream(data []byte, r1cs *cs.R1CS, device int, unsafeRead bool) (*ProvingKey, error) {
	if len(data) == 0 {
		return nil, errors.New("mi355x: empty key stream")
	}
	pk := &ProvingKey{}
	var err error
	pk.once.Do(func() {
		if rc := C.mi_init(C.int(device), &pk.ctx); rc != C.MI_OK {
			err = fmt.Errorf("mi355x: mi_init rc=%d (no gfx950 device?)", int(rc))
			return
		}
		if rc := C.mi_prover_create(C.int(device), C.uint32_t(InFlight), &pk.pool); rc != C.MI_OK {
			err = fmt.Errorf("mi355x: mi_prover_create rc=%d", int(rc))
			return
		}
		info := r1cs.CommitmentInfo.(constraint.Groth16Commitments)
		removed := sortedUint32(append(flatten(info.GetPrivateCommitted()), info.CommitmentIndexes()...))
		var cw *C.uint32_t
		if len(removed) > 0 {
			cw = (*C.uint32_t)(unsafe.Pointer(&removed[0])) // a flat array without pointers, read during the call only
		}
		var flags C.uint32_t
		if unsafeRead {
			flags = C.MI_KEYFILE_NO_SUBGROUP_CHECK
		}
		ped := make([]*C.mi_pedersen_pk, C.MI_PK_RAW_MAX_COMMITMENTS)
		var nPed C.uint32_t
		rc := C.mi_pk_load_stream(pk.ctx, (*C.uint8_t)(unsafe.Pointer(&data[0])), C.size_t(len(data)), flags, C.uint32_t(r1cs.GetNbPublicVariables()),
			cw, C.size_t(len(removed)), &pk.dev, &ped[0], &nPed)
		if err = status(pk.ctx, rc); err == nil {
			pk.ped = ped[:int(nPed)]
		}
	})
	pk.err = err
	if err != nil {
		return nil, err
	}
	return pk, nil
}

// WriteKeyStream replaces pk.WriteTo (KeyCompressed) / pk.WriteRawTo (KeyRaw) for a key gnark holds in host memory: the point
// arrays go up once, the encoders run on the device, the stream comes back.
func WriteKeyStream(pk *ProvingKey, r1cs *cs.R1CS, device int, encoding int) ([]byte, error) {
	var ctx *C.mi_ctx
	if rc := C.mi_init(C.int(device), &ctx); rc != C.MI_OK {
		return nil, fmt.Errorf("mi355x: mi_init rc=%d (no gfx950 device?)", int(rc))
	}
	defer C.mi_shutdown(ctx)
	var out []byte
	err := pk.withKeyDesc(r1cs, func(d *C.mi_pk_desc) error {
		// the writer wants device arrays: upload the five of the key and the Pedersen bases, point the descriptor at the copies
		var bufs []unsafe.Pointer
		defer func() {
			for _, b := range bufs {
				C.mi_dev_free(ctx, b)
			}
		}()
		up := func(src unsafe.Pointer, bytes C.size_t) (unsafe.Pointer, error) {
			var dev unsafe.Pointer
			if err := status(ctx, C.mi_dev_alloc(ctx, bytes, &dev)); err != nil {
				return nil, err
			}
			bufs = append(bufs, dev)
			return dev, status(ctx, C.mi_dev_upload(ctx, dev, src, bytes))
		}
		var err error
		var p unsafe.Pointer
		if p, err = up(unsafe.Pointer(d.g1_a), C.size_t(d.n_g1_a)*64); err != nil {
			return err
		}
		d.g1_a = (*C.mi_g1_affine)(p)
		if p, err = up(unsafe.Pointer(d.g1_b), C.size_t(d.n_g1_b)*64); err != nil {
			return err
		}
		d.g1_b = (*C.mi_g1_affine)(p)
		if p, err = up(unsafe.Pointer(d.g1_k), C.size_t(d.n_g1_k)*64); err != nil {
			return err
		}
		d.g1_k = (*C.mi_g1_affine)(p)
		if p, err = up(unsafe.Pointer(d.g1_z), C.size_t(d.n_g1_z)*64); err != nil {
			return err
		}
		d.g1_z = (*C.mi_g1_affine)(p)
		if p, err = up(unsafe.Pointer(d.g2_b), C.size_t(d.n_g2_b)*128); err != nil {
			return err
		}
		d.g2_b = (*C.mi_g2_affine)(p)
		var pin runtime.Pinner
		defer pin.Unpin()
		ped := make([]C.mi_pedersen_arrays, len(pk.CommitmentKeys)+1)
		for i := range pk.CommitmentKeys {
			k := &pk.CommitmentKeys[i]
			n := C.size_t(len(k.Basis)) * 64
			if p, err = up(unsafe.Pointer(g1(&pin, k.Basis)), n); err != nil {
				return err
			}
			ped[i].basis_dev = (*C.mi_g1_affine)(p)
			if p, err = up(unsafe.Pointer(g1(&pin, k.BasisExpSigma)), n); err != nil {
				return err
			}
			ped[i].basis_exp_sigma_dev = (*C.mi_g1_affine)(p)
			ped[i].n = C.uint64_t(len(k.Basis))
		}
		var need C.size_t
		if rc := C.mi_pk_stream_size(d, &ped[0], C.uint32_t(len(pk.CommitmentKeys)), C.uint32_t(encoding), &need); rc != C.MI_OK {
			return fmt.Errorf("mi355x: mi_pk_stream_size rc=%d", int(rc))
		}
		out = make([]byte, int(need))
		return status(ctx, C.mi_pk_write_dev(ctx, d, &ped[0], C.uint32_t(len(pk.CommitmentKeys)), C.uint32_t(encoding), (*C.uint8_t)(unsafe.Pointer(&out[0])), need, &need))
	})
	if err != nil {
		return nil, err
	}
	return out, nil
}

// LoadVerifyingKeyStream replaces vk.ReadFrom / vk.UnsafeReadFrom followed by LoadVerifyingKey: data is the whole stream, in either
// encoding.  Every point is decoded and checked on the device, e(alpha, beta) is computed there and PublicAndCommitmentCommitted is
// installed from the stream.  The embedded gnark key stays empty (nothing is decoded on the host), so the result serves VerifyFiles and
// VerifyFilesCombined, which ask the key for nothing; Verify and VerifyBytes read the embedded key and want LoadVerifyingKey.
func LoadVerifyingKeyStream(data []byte, device int, unsafeRead bool) (*VerifyingKey, error) {
	if len(data) == 0 {
		return nil, errors.New("mi355x: empty key stream")
	}
	out := &VerifyingKey{}
	if rc := C.mi_init(C.int(device), &out.ctx); rc != C.MI_OK {
		return nil, fmt.Errorf("mi355x: mi_init rc=%d (no gfx950 device?)", int(rc))
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&data[0])
	var flags C.uint32_t
	if unsafeRead {
		flags = C.MI_KEYFILE_NO_SUBGROUP_CHECK
	}
	if err := status(out.ctx, C.mi_vk_load_stream(out.ctx, (*C.uint8_t)(unsafe.Pointer(&data[0])), C.size_t(len(data)), flags, &out.dev)); err != nil {
		C.mi_shutdown(out.ctx)
		return nil, err
	}
	return out, nil
}

// WriteVerifyingKeyStream replaces vk.WriteTo (KeyCompressed) / vk.WriteRawTo (KeyRaw): K goes through the device's encoders, the
// single points and the lists are written on the host.
func WriteVerifyingKeyStream(vk *groth16_bn254.VerifyingKey, device int, encoding int) ([]byte, error) {
	var ctx *C.mi_ctx
	if rc := C.mi_init(C.int(device), &ctx); rc != C.MI_OK {
		return nil, fmt.Errorf("mi355x: mi_init rc=%d (no gfx950 device?)", int(rc))
	}
	defer C.mi_shutdown(ctx)
	var pin runtime.Pinner
	defer pin.Unpin()
	nc := len(vk.PublicAndCommitmentCommitted)
	ped := make([]C.mi_pedersen_vk, nc+1)
	offsets := make([]C.uint32_t, nc+1)
	indices := make([]C.uint32_t, 0, 1)
	for i := 0; i < nc; i++ {
		ped[i].g = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.CommitmentKeys[i].G))
		ped[i].g_sigma_neg = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.CommitmentKeys[i].GSigmaNeg))
		for _, j := range vk.PublicAndCommitmentCommitted[i] {
			indices = append(indices, C.uint32_t(j))
		}
		offsets[i+1] = C.uint32_t(len(indices))
	}
	var d C.mi_vk_file_desc
	d.alpha1 = *(*C.mi_g1_affine)(unsafe.Pointer(&vk.G1.Alpha))
	d.beta1 = *(*C.mi_g1_affine)(unsafe.Pointer(&vk.G1.Beta))
	d.delta1 = *(*C.mi_g1_affine)(unsafe.Pointer(&vk.G1.Delta))
	d.beta2 = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.G2.Beta))
	d.gamma2 = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.G2.Gamma))
	d.delta2 = *(*C.mi_g2_affine)(unsafe.Pointer(&vk.G2.Delta))
	d.k = g1(&pin, vk.G1.K)
	d.n_k = C.uint64_t(len(vk.G1.K))
	d.nb_public = C.uint32_t(len(vk.G1.K) - nc)
	d.n_commitments = C.uint32_t(nc)
	pin.Pin(&ped[0])
	pin.Pin(&offsets[0])
	d.ped = &ped[0]
	d.pc_offsets = &offsets[0]
	if len(indices) > 0 {
		pin.Pin(&indices[0])
		d.pc_indices = &indices[0]
	}
	var need C.size_t
	if rc := C.mi_vk_stream_size(&d, C.uint32_t(encoding), &need); rc != C.MI_OK {
		return nil, fmt.Errorf("mi355x: mi_vk_stream_size rc=%d", int(rc))
	}
	out := make([]byte, int(need))
	if err := status(ctx, C.mi_vk_write(ctx, &d, C.uint32_t(encoding), (*C.uint8_t)(unsafe.Pointer(&out[0])), need, &need)); err != nil {
		return nil, err
	}
	return out, nil
}
