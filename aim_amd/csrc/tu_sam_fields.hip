// tu_sam_fields.hip -- the translation unit that instantiates the kernels of sam_fields.hpp (aim_amd/build.py compiles the tu_*.hip files in
// parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_SAM_FIELDS 1
#include "sam_fields.hpp"
