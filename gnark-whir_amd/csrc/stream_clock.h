// The two clocks of the ceremony and audit calls (phase1.hip, phase2.hip, phase2_check.hip, keyaudit.hip), whose phases are long and run
// one after the other: every lap here waits for the context's stream.  setup.hip's Timer (named marks, no waits) is another tool.
#pragma once
#include "ctx.h"
#include <utility>

// the host's clock around work that has been waited for
struct HostClock {
    double t = now_ms();
    void lap(float &into) { const double n = now_ms(); into += (float)(n - t); t = n; }
};
inline int32_t sync_lap(mi_ctx *ctx, HostClock &ck, float &into) {
    MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ck.lap(into);
    return MI_OK;
}

// the device's time of the stream's work since the last lap, between two events
struct StreamLaps {
    hipEvent_t ev[2]{};
    ~StreamLaps() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
    int32_t init(mi_ctx *ctx) {
        for (auto &e : ev) MI_CHECK_HIP(ctx, hipEventCreate(&e));
        MI_CHECK_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
        return MI_OK;
    }
    int32_t lap(mi_ctx *ctx, float &into) {
        MI_CHECK_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
        MI_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
        into += ms;
        std::swap(ev[0], ev[1]);
        return MI_OK;
    }
};
