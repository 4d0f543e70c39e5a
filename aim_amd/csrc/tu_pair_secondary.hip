// tu_pair_secondary.hip -- the translation unit that instantiates the kernels of pair_secondary.hpp (aim_amd/build.py compiles the
// tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_PAIR_SECONDARY 1
#include "pair_secondary.hpp"
