// Host build of the per-value text of the witness codec (gnark-whir_amd/csrc/witness_ops.cuh): the same body k_witness_decode runs one
// lane each, compiled with -DMI_CHECK_NOWRAP so that every bound of the arithmetic underneath traps.
#include <cstddef>
#include "../../gnark-whir_amd/csrc/witness_ops.cuh"

extern "C" {
// n values of 32 bytes back to back at bytes (any alignment) -> out[i] Montgomery, below[i] = 1 where the integer was below r
int emu_witness_decode(const unsigned char *bytes, size_t n, void *out, unsigned char *below) {
    for (size_t i = 0; i < n; i++) below[i] = fr_from_be32((Fr *)out + i, bytes + 32 * i) ? 1 : 0;
    return 0;
}
}
