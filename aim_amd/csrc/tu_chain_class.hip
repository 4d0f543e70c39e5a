// tu_chain_class.hip -- the translation unit that instantiates the kernels of chain_class.hpp (aim_amd/build.py compiles the
// tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_CHAIN_CLASS 1
#include "chain_class.hpp"
