// tu_split.hip -- the translation unit that instantiates the kernel of split.hpp (aim_amd/build.py compiles the tu_*.hip files in
// parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_SPLIT 1
#include "split.hpp"
