// The host-only walk over gnark's ProvingKey.WriteRawTo stream (layout notes in csrc/pk_raw.hip): offsets and counts of
// every section, every count cross-checked (pk_stream_walk.h, with the bytes of a raw point).  No HIP in this file: it reads bytes an
// outside party wrote, and the CPU build with -fsanitize=address,undefined (make sanitize; tests/test_parsers_sanitized.py) compiles it
// together with csrc/whir_ingest.hip.
#include "pk_stream_walk.h"

extern "C" {

// Host-only walk over the stream: offsets and counts of every section (no device needed; what the CPU tests check).
int32_t mi_pk_raw_inspect(const uint8_t *buf, size_t len, mi_pk_raw_info *info) { return pk_stream_walk(buf, len, info, 64, 128); }

}  // extern "C"
