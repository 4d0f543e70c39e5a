#include "upmem_shim.h"
