// select_harness.hip -- test-only launcher of the two selection kernels (groups.hpp, mates.hpp) on rows the caller makes by hand.
//
// The public entry points feed mate_select_kernel the rows of a score-only pass, whose status is always AIM_PAIR_OK, and choose the
// lanes per read pair (W) from the batch's shape. This helper takes host arrays -- result rows of any status, requests, text_pos, the
// CSR -- runs group_select_kernel and then mate_select_kernel at the W the caller asks for, and returns best, sel and mates. It is not
// part of libaim_hip.so; aim_amd.build compiles it into build/tests/libselect_harness.so.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "aim_hip.h"
#define AIM_TU_GROUPS 1   // this helper launches the kernels itself, so it instantiates them
#include "groups.hpp"
#include "mates.hpp"

namespace {

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    hipError_t upload(const void *src, size_t bytes)
    {
        hipError_t e = alloc(bytes);
        return e != hipSuccess ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    }
};

}  // namespace

#define TRY(x)                          \
    do {                                \
        hipError_t e_ = (x);            \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

// Host pointers throughout. res / req / tpos: [n_pairs]; roff: [n_reads + 1], non-decreasing, roff[n_reads] <= n_pairs;
// best / sel: [n_reads] out; mates: [n_reads / 2] out. best is zeroed first (a read without candidates keeps n_best = 0).
// Returns 0, -1 for arguments this helper refuses, or the hipError_t of the call that failed.
extern "C" int select_harness_run(uint32_t n_pairs, uint32_t n_reads, const aim_result_t *res, const aim_request_t *req, const uint64_t *tpos,
                                  const uint32_t *roff, int64_t min_span, int64_t max_span, int32_t unpaired_penalty, uint32_t lanes,
                                  aim_best_t *best, uint32_t *sel, aim_mate_t *mates)
{
    if (!n_pairs || n_reads < 2 || (n_reads & 1u) || !res || !req || !tpos || !roff || !best || !sel || !mates) return -1;
    if (!lanes || lanes > (uint32_t)aim::kWave || (lanes & (lanes - 1u))) return -1;
    if (roff[n_reads] > n_pairs) return -1;
    for (uint32_t r = 0; r < n_reads; ++r)
        if (roff[r] > roff[r + 1]) return -1;
    DevBuf d_res, d_req, d_tpos, d_roff, d_best, d_sel, d_mates;
    TRY(d_res.upload(res, (size_t)n_pairs * sizeof(aim_result_t)));
    TRY(d_req.upload(req, (size_t)n_pairs * sizeof(aim_request_t)));
    TRY(d_tpos.upload(tpos, (size_t)n_pairs * sizeof(uint64_t)));
    TRY(d_roff.upload(roff, ((size_t)n_reads + 1) * sizeof(uint32_t)));
    TRY(d_best.alloc((size_t)n_reads * sizeof(aim_best_t)));
    TRY(d_sel.alloc((size_t)n_reads * sizeof(uint32_t)));
    TRY(d_mates.alloc((size_t)(n_reads / 2) * sizeof(aim_mate_t)));
    TRY(hipMemset(d_best.p, 0, (size_t)n_reads * sizeof(aim_best_t)));
    TRY(hipMemset(d_sel.p, 0, (size_t)n_reads * sizeof(uint32_t)));
    TRY(hipMemset(d_mates.p, 0xA5, (size_t)(n_reads / 2) * sizeof(aim_mate_t)));

    const uint32_t waves = (n_reads + aim::kGroupReadsPerWave - 1) / aim::kGroupReadsPerWave;
    hipLaunchKernelGGL(aim::group_select_kernel, dim3((waves + 3) / 4), dim3(256), 0, 0, static_cast<const aim_result_t *>(d_res.p), n_pairs,
                       static_cast<const uint32_t *>(d_roff.p), n_reads, static_cast<aim_best_t *>(d_best.p), static_cast<uint32_t *>(d_sel.p));
    TRY(hipGetLastError());
    aim::KArgs ka{};
    ka.n_pairs = n_pairs;
    ka.req = static_cast<const aim_request_t *>(d_req.p);    // (p.flags = 0: 16-byte requests)
    aim::MateArgs ma{};
    ma.min_span = min_span;
    ma.max_span = max_span;
    ma.unpaired_penalty = unpaired_penalty;
    ma.n_mates = n_reads / 2;
    ma.lanes = lanes;
    const uint64_t threads = (uint64_t)ma.n_mates * lanes;
    hipLaunchKernelGGL(aim::mate_select_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, ka, ma,
                       static_cast<const aim_result_t *>(d_res.p), static_cast<const uint64_t *>(d_tpos.p), static_cast<const uint32_t *>(d_roff.p),
                       static_cast<const aim_best_t *>(d_best.p), static_cast<uint32_t *>(d_sel.p), static_cast<aim_mate_t *>(d_mates.p));
    TRY(hipGetLastError());
    TRY(hipDeviceSynchronize());
    TRY(hipMemcpy(best, d_best.p, (size_t)n_reads * sizeof(aim_best_t), hipMemcpyDeviceToHost));
    TRY(hipMemcpy(sel, d_sel.p, (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    TRY(hipMemcpy(mates, d_mates.p, (size_t)(n_reads / 2) * sizeof(aim_mate_t), hipMemcpyDeviceToHost));
    return 0;
}
