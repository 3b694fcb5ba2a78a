// cov_decode.hpp -- the coverage of the last pass decoded to int32 on the device: the one launch sequence over pack.hpp's kernels,
// for the engine's materialise_cov and for the queries that need int32 where the pass holds an encoding.  Part of the host toolkit
// (query_host.hpp), in a header of its own because it puts pack.hpp's kernels into the translation unit: the libraries that never
// decode (ovl_class_lib.hip, frag_ovl_lib.hip) do not carry them.
#pragma once
#include "query_host.hpp"
#include "pack.hpp"

#include <string>

namespace raft {

// The codes or four-bit steps of the last pass (cov8, the exception list, delta4's anchors) -> int32 in dst, queued on the context's
// stream; `abs` takes delta4's escape flags.  No wait, and nothing of the context but the two buffers is written or marked.
inline int decode_cov(raft_hip_ctx *c, DevBuf &dst, DevBuf &abs, const char *who)
{
    const long long B = c->sum.n_bins;
    HIP_TRY(c, dst.ensure((size_t)std::max(B, 1LL) * 4));
    if (B <= 0) return RAFT_HIP_OK;
    int32_t *cov = dst.as<int32_t>();
    const bool d4 = c->pass_width == kCovDelta4;
    if (d4) {
        if (c->d4_shift != 0) return RAFT_HIP_ERR_STATE;      // (a pipeline lane's chunk: its blocks do not begin at its first window)
        HIP_TRY(c, abs.ensure(((size_t)B / 32 + 2) * 4));
        hipLaunchKernelGGL(delta4_expand_kernel, dim3(grid_for(B / 32, 256, 256 * 16)), dim3(256), 0, c->stream,
                           c->cov8.as<uint8_t>(), B, cov, abs.as<unsigned>());
    } else if (c->pass_width == 1)
        hipLaunchKernelGGL(unpack_cov_kernel<uint8_t>, dim3(grid_for(B / 4, 256, 256 * 16)), dim3(256), 0, c->stream, c->cov8.as<uint8_t>(), B, cov);
    else if (c->pass_width == 2)
        hipLaunchKernelGGL(unpack_cov_kernel<uint16_t>, dim3(grid_for(B / 4, 256, 256 * 16)), dim3(256), 0, c->stream, c->cov8.as<uint16_t>(), B, cov);
    else { c->last_error = std::string(who) + ": the pass holds neither int32 nor an encoding"; return RAFT_HIP_ERR_STATE; }
    if (c->n_exc > 0)      // the listed windows, over what the codes gave (delta4: before the walk that adds the steps up)
        hipLaunchKernelGGL(scatter_exceptions_kernel, dim3((unsigned)std::min<long long>((c->n_exc + 255) / 256, 4096)), dim3(256), 0, c->stream,
                           c->exc_idx.as<long long>(), c->exc_val.as<int32_t>(), c->n_exc, cov);
    if (d4)
        hipLaunchKernelGGL(delta4_walk_kernel, dim3(grid_for(B / kD4Block, 256, 256 * 16)), dim3(256), 0, c->stream,
                           B, c->cov_anchor.as<int32_t>(), abs.as<unsigned>(), cov);
    HIP_TRY(c, hipGetLastError());
    return RAFT_HIP_OK;
}

// The int32 array a query reads: the context's own when it holds one (a pass that wrote int32, or one somebody fetched), else decoded
// into the queries' shared pair (engine_ctx.hpp q_cov, q_abs).  Nothing of the engine's is allocated, written or marked.
inline int query_cov(raft_hip_ctx *c, const char *who, const int32_t **out)
{
    if (c->cov_valid) { *out = c->cov.as<int32_t>(); return RAFT_HIP_OK; }
    PHASE(decode_cov(c, c->q_cov, c->q_abs, who));
    *out = c->q_cov.as<int32_t>();
    return RAFT_HIP_OK;
}

} // namespace raft
