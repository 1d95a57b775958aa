// The device allocations of one call (setup.hip, phase2.hip): freed when the call returns, whatever way it returns.
#pragma once
#include "ctx.h"
#include <vector>

struct Arena {   // (the key takes what it adopts out of the list: key_handover.h)
    struct Block { void *p; size_t bytes; };
    std::vector<Block> live;
    size_t held = 0, peak = 0;   // bytes the arena holds now, and the most it has held
    ~Arena() { for (const Block &b : live) if (b.p) (void)hipFree(b.p); }
    int32_t alloc(mi_ctx *ctx, void **out, size_t bytes) {
        *out = nullptr;
        if (!bytes) bytes = 64;
        MI_CHECK_HIP(ctx, hipMalloc(out, bytes));
        live.push_back({*out, bytes});
        held += bytes;
        if (held > peak) peak = held;
        return MI_OK;
    }
    template <class T> int32_t alloc(mi_ctx *ctx, T **out, size_t count) { return alloc(ctx, (void **)out, count * sizeof(T)); }
    void release(void *p) {   // free now
        if (!p) return;
        for (Block &b : live) if (b.p == p) { b.p = nullptr; held -= b.bytes; (void)hipFree(p); return; }
    }
    void disown(void *p) { for (Block &b : live) if (p && b.p == p) { b.p = nullptr; held -= b.bytes; } }
};
