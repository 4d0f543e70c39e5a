// tu_index.hip -- the translation unit that instantiates the kernels of index.hpp (aim_amd/build.py compiles the tu_*.hip files in
// parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_INDEX 1
#include "index.hpp"
