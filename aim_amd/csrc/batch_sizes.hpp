// batch_sizes.hpp -- host constants and size functions of batch_io.hpp's kernels that the launch planner (capi_plan.hip) needs too.
// No kernel and no launcher here; batch_io.hpp includes it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace aim {

// AIM_FLAG_WFA_ESCALATE (batch_io.hpp, escalate_select_kernel / escalate_list_kernel): one ballot mask per 64 pairs, one count per workgroup
constexpr uint32_t kEscTile = 4096;                          // pairs per workgroup: 4 wavefronts x 16 groups of 64
inline size_t escalate_mask_bytes(uint32_t n_pairs) { return (((size_t)n_pairs + 63) / 64 * 8 + 255) & ~(size_t)255; }
inline size_t escalate_count_bytes(uint32_t n_pairs) { return ((((size_t)n_pairs + kEscTile - 1) / kEscTile) * 4 + 255) & ~(size_t)255; }

}  // namespace aim
