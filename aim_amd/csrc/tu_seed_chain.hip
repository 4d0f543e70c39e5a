// tu_seed_chain.hip -- the translation unit that instantiates the kernels of seed_chain.hpp (aim_amd/build.py compiles the tu_*.hip files
// in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_SEED_DEVICE_CODE 1
#define AIM_TU_SEED_CHAIN 1
#include "seed_chain.hpp"
