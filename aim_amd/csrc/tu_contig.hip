// tu_contig.hip -- the translation unit that instantiates the kernel of contig.hpp (aim_amd/build.py compiles the
// tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_CONTIG 1
#include "contig.hpp"
