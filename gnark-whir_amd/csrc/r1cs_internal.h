// The compiled R1CS inside the library: the host-side checks Setup (setup.hip) and the resident handle (r1cs.hip) share, and the handle.
#pragma once
#include "ctx.h"
#include "../../include/mi355x_groth16_r1cs.h"
#include <vector>

// what the host derives from a descriptor before any device work
struct R1csShape {
    uint32_t log_n = 0;
    uint64_t N = 0, nc = 0, nb_wires = 0;
    uint32_t nb_public = 0, n_commitments = 0;
    std::vector<uint32_t> row_ptr[3];   // the row starts in 32 bits (nnz < 2^32)
    uint32_t nnz[3] = {0, 0, 0};
    std::vector<uint32_t> removed;      // committed + commitment wires, ascending: the private wires without a pk.G1.K point
    std::vector<uint32_t> vk_wires;     // public wires, then the commitment wires ascending
};
// Every check of a descriptor that does not concern a trapdoor, on the host, before anything is allocated: MI_EINVAL with
// mi_last_error = "<who>: <field> ...".  d itself is checked by the caller (Setup reports a null trapdoor before the first field).
int32_t mi_r1cs_validate(mi_ctx *ctx, const char *who, const mi_r1cs_desc *d, R1csShape &sh);

// The matrices of a descriptor on the device one at a time, sorted by column (setup.hip; for phase2.hip too).  The five arrays are the
// caller's device scratch for all three: row_ptr[nc + 1], col / cf / rank[the largest nnz], cnt[nb_wires].  upload(k) enqueues matrix k's
// row starts, columns and coefficient indices on st; sort(k) its counting sort: cnt ends as the histogram, off[nb_wires + 1] as its
// exclusive scan (through ctx->ws[WS_SCAN]), sorted[off[j] ..] holds (row, coefficient index) of column j's entries in the atomics' order
struct MatrixSorter {
    const mi_r1cs_desc *d;
    const R1csShape *sh;   // (both outlive the sorter)
    uint32_t *row_ptr = nullptr, *col = nullptr, *cf = nullptr, *cnt = nullptr, *rank = nullptr;
    int32_t upload(mi_ctx *ctx, hipStream_t st, int k);
    int32_t sort(mi_ctx *ctx, hipStream_t st, int k, uint32_t *off, uint2 *sorted);
};

struct SparseLong;   // sparse_fr.cuh
struct R1csMatrixDev {
    uint32_t *row_off = nullptr;        // nc + 1
    uint2 *entries = nullptr;           // nnz x (col | class << 30, coefficient index)
    SparseLong *long_rows = nullptr;    // per row of more than SPARSE_SHORT entries, ascending by row (index = the row)
    uint2 *pieces = nullptr;            // (first entry, entries)
    uint32_t nnz = 0, n_long = 0, n_pieces = 0;
};
struct mi_r1cs {
    int dev = 0;
    uint64_t nc = 0, nb_wires = 0;
    uint32_t log_n = 0;
    void *coeffs = nullptr;             // the coefficient table, once
    uint64_t n_coeffs = 0;
    R1csMatrixDev m[3];
    uint64_t bytes = 0;                 // device bytes held
};

// a = A W, b = B W (c = C W with eval_c) into context workspace on ctx->stream, for prove.hip; the pointers stay valid until the
// next evaluation on ctx
int32_t mi_r1cs_eval_ws(mi_ctx *ctx, const mi_r1cs *r, const mi_fr *W_dev, bool eval_c, const mi_fr **a, const mi_fr **b, const mi_fr **c);
