// tu_secondary.hip -- the translation unit that instantiates the kernels of secondary.hpp (aim_amd/build.py compiles the
// tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_SECONDARY 1
#include "secondary.hpp"
