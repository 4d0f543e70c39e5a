// tu_extend.hip -- the translation unit that instantiates the kernels of extend.hpp (aim_amd/build.py compiles the tu_*.hip files in
// parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_EXTEND 1
#include "extend.hpp"
