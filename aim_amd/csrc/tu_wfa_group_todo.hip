// tu_wfa_group_todo.hip -- the translation unit that instantiates the to-do-input variants of wfa_group.hpp's kernels (the second stage of
// AIM_FLAG_WFA_ESCALATE); aim_amd/build.py compiles the tu_*.hip files in parallel and links them with aim_capi.hip into libaim_hip.so.
#define AIM_TU_WFA_GROUP_TODO 1
#include "wfa_group.hpp"
