// The device allocations of one call (setup.hip, the ceremony and audit files): freed when the call returns, whatever way it returns;
// and the device words in which the checking kernels of such a call leave their lowest bad index (BadSlots).
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

// Device words that collect the lowest refused index of a launch each (atomicMin in the kernel); all UINT64_MAX to begin with.  Taken
// from the caller's arena where it has one (the words count into its peak), else an allocation of their own; gone with the struct.
struct BadSlots {
    static constexpr unsigned long long NONE = ~0ull;
    unsigned long long *dev = nullptr;
    std::vector<unsigned long long> host;
    Arena *arena = nullptr;
    int32_t init(mi_ctx *ctx, size_t n, Arena *ar = nullptr) {
        host.assign(n, NONE);
        arena = ar;
        if (ar) MI_TRY(ar->alloc(ctx, &dev, n));
        else MI_CHECK_HIP(ctx, hipMalloc((void **)&dev, n * sizeof(*dev)));
        MI_CHECK_HIP(ctx, hipMemsetAsync(dev, 0xff, n * sizeof(*dev), ctx->stream));
        return MI_OK;
    }
    int32_t fetch(mi_ctx *ctx) {   // returns with the stream idle
        MI_CHECK_HIP(ctx, hipMemcpyAsync(host.data(), dev, host.size() * sizeof(*dev), hipMemcpyDeviceToHost, ctx->stream));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return MI_OK;
    }
    bool bad(size_t i) const { return host[i] != NONE; }
    BadSlots() = default;
    BadSlots(const BadSlots &) = delete;
    ~BadSlots() {
        if (arena) arena->release(dev);
        else if (dev) (void)hipFree(dev);
    }
};
