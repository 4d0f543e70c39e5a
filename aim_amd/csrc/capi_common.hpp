// capi_common.hpp -- what the units of the C-ABI share: aim_capi.hip (planner, device sets, alignment entry points), capi_pipeline.hip
// (index, seeding, classes and MAPQ, split, extension) and capi_host.hip (host-side formatters and generators). Internal, not installed.
// Every function declared here has ONE definition, in aim_capi.hip, next to the state it owns: fail() writes the thread-local buffer
// aim_last_error() returns, read_knobs() is the one reader of the AIM_* environment, with_chip() asks chip_cus()'s per-device cache.
#pragma once
#include <hip/hip_runtime.h>

#include "aim_hip.h"
#include "aim_device.hpp"

namespace aim {
namespace capi {
#pragma GCC visibility push(hidden)
int fail(int code, const char *fmt, ...);   // sets aim_last_error() for the calling thread and returns `code`
aim::Knobs read_knobs();                    // the AIM_* environment, as it is now
aim::Knobs with_chip(aim::Knobs k);         // ... for a plan on the current device: AIM_CHIP_CUS wins, else the device's own CU count
// Every length of a batch against READ_SIZE; AIM_EINVAL names the first pair that breaks it.
int check_lengths(const aim_params_t &p, uint32_t n_pairs, const void *requests);
// Dwords of a packed sequence row: aim::packed_row_dwords (batch_io.hpp) for the units that must not include its kernels.
uint32_t packed_row_dwords(int read_size);
// AIM_FLAG_REF_TEXTS: texts gathered from a device-resident reference (batch_io.hpp); no plan depends on it.
inline bool is_ref(const aim_params_t &p) { return (p.flags & AIM_FLAG_REF_TEXTS) != 0; }
#pragma GCC visibility pop
}  // namespace capi
}  // namespace aim

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return ::aim::capi::fail(e_ == hipErrorOutOfMemory ? AIM_ENOMEM : AIM_ENODEV, "%s failed: %s", #expr, \
                                     hipGetErrorString(e_));                                \
    } while (0)
