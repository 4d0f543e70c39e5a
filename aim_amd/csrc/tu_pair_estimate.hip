// tu_pair_estimate.hip -- the translation unit that instantiates the kernels of pair_estimate.hpp (aim_amd/build.py compiles the
// tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_PAIR_ESTIMATE 1
#include "pair_estimate.hpp"
