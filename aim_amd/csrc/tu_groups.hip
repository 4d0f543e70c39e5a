// tu_groups.hip -- the translation unit that instantiates the kernels of groups.hpp, hits.hpp and mates.hpp (aim_amd/build.py compiles
// the tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_GROUPS 1
#include "groups.hpp"
#include "hits.hpp"
#include "mates.hpp"
