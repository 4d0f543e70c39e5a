/* Energy probes of the UPMEM SDK stand-in: they measure nothing. */
#ifndef AIM_UPMEM_SHIM_DPU_PROBE_H
#define AIM_UPMEM_SHIM_DPU_PROBE_H
#include "dpu.h"

struct dpu_probe_t { int unused; };
typedef enum { DPU_ENERGY = 0, DPU_TIME = 1 } dpu_probe_metric_t;
typedef enum { DPU_AVERAGE = 0, DPU_MIN = 1, DPU_MAX = 2 } dpu_probe_kind_t;

dpu_error_t dpu_probe_init(const char *name, struct dpu_probe_t *probe);
dpu_error_t dpu_probe_start(struct dpu_probe_t *probe);
dpu_error_t dpu_probe_stop(struct dpu_probe_t *probe);
dpu_error_t dpu_probe_get(struct dpu_probe_t *probe, dpu_probe_metric_t metric, dpu_probe_kind_t kind, double *value);

#endif
