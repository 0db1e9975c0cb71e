// chunk_run.h — the stream protocol of one chunk of a chunked window call (the calls cut their chunks with win_chunks.h): metadata
// up through the page-locked mirror of the device layout, timed launches, records down, the device error word, one synchronisation.
#pragma once
#include <type_traits>

#include "internal.h"

namespace impop {

// a kernel's dynamic LDS above the default 48 KiB is an opt-in, made on the device the caller made current
template <typename K>
int lds_opt_in(K kernel, size_t lds) {
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return IMPOP_OK;
}

// launch() (void, or an int status) between two events of T when the context times its kernels (impop_ctx_gram_timing)
template <typename F>
int timed(impop_ctx *ctx, EventPairs &T, F launch) {
    size_t slot = 0;
    int rc;
    if (ctx->gram_timing && (rc = T.begin(ctx->stream, &slot))) return rc;
    if constexpr (std::is_void_v<decltype(launch())>) launch();
    else if ((rc = launch())) return rc;
    HIP_TRY(hipGetLastError());
    if (ctx->gram_timing && (rc = T.end(ctx->stream, slot))) return rc;
    return IMPOP_OK;
}

// dc / hc: the device base of one Carve and the page-locked base that mirrors its first regions at the same offsets
struct ChunkRun {
    impop_ctx *ctx;
    const char *fn;
    char *dc, *hc;
    // one H2D copy of the mirrored bytes [off_begin, off_end)
    int up(size_t off_begin, size_t off_end) const {
        HIP_TRY(hipMemcpyAsync(dc + off_begin, hc + off_begin, off_end - off_begin, hipMemcpyHostToDevice, ctx->stream));
        return IMPOP_OK;
    }
    template <typename F>
    int timed(EventPairs &T, F launch) const { return impop::timed(ctx, T, launch); }
    // the end of a chunk: the mirrored records [off_begin, off_end) down, the error word behind them, then the synchronisation
    // that lets the next chunk reuse the staging.  Copies into the caller's own memory are queued before this.
    int finish(size_t off_begin, size_t off_end) const {
        HIP_TRY(hipMemcpyAsync(hc + off_begin, dc + off_begin, off_end - off_begin, hipMemcpyDeviceToHost, ctx->stream));
        const int rc = ctx_err_fetch(ctx);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return ctx_err_result(ctx, fn);
    }
};

}  // namespace impop
