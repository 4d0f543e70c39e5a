// tu_pair.hip -- the translation unit that instantiates the kernels of pair.hpp (aim_amd/build.py compiles the
// tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_PAIR 1
#include "pair.hpp"
