// tu_mapper.hip -- the translation unit that instantiates the kernels of mapper.hpp (aim_amd/build.py compiles the
// tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_MAPPER 1
#include "mapper.hpp"
