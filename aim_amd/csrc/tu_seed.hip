// tu_seed.hip -- the translation unit that instantiates the kernel of seed.hpp (aim_amd/build.py compiles the tu_*.hip files in
// parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_SEED_DEVICE_CODE 1
#define AIM_TU_SEED 1
#include "seed.hpp"
