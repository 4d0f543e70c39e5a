// tu_wfa_bidir.hip -- the translation unit that instantiates the kernels of wfa_bidir.hpp (aim_amd/build.py compiles the tu_*.hip files in
// parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_WFA_BIDIR 1
#include "wfa_bidir.hpp"
