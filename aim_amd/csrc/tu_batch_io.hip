// tu_batch_io.hip -- the translation unit that instantiates the kernels of batch_io.hpp (aim_amd/build.py compiles the tu_*.hip files in
// parallel and links them with aim_capi.hip into libaim_hip.so).
#define AIM_TU_BATCH_IO 1
#include "batch_io.hpp"
