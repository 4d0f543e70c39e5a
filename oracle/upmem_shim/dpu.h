/* Host side of the UPMEM SDK stand-in (see upmem_shim.h): a set of DPUs is a set of MRAM images in this process. */
#ifndef AIM_UPMEM_SHIM_DPU_H
#define AIM_UPMEM_SHIM_DPU_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef enum { DPU_OK = 0, DPU_ERR_SHIM = 1 } dpu_error_t;
typedef enum { DPU_XFER_TO_DPU = 0, DPU_XFER_FROM_DPU = 1 } dpu_xfer_t;
typedef enum { DPU_XFER_DEFAULT = 0 } dpu_xfer_flags_t;
typedef enum { DPU_SYNCHRONOUS = 0, DPU_ASYNCHRONOUS = 1 } dpu_launch_policy_t;

#define DPU_MRAM_HEAP_POINTER_NAME "__sys_used_mram_end"
#define DPU_ALLOCATE_ALL 0xffffffffu

struct dpu_set_t {
    int is_single;  /* one DPU of the set (the iteration variable of DPU_FOREACH) */
    uint32_t idx;
};

#define DPU_ASSERT(statement)                                                                        \
    do {                                                                                             \
        dpu_error_t shim_err_ = (statement);                                                         \
        if (shim_err_ != DPU_OK) {                                                                   \
            fprintf(stderr, "%s:%d: %s failed (%d)\n", __FILE__, __LINE__, #statement, (int)shim_err_); \
            exit(EXIT_FAILURE);                                                                      \
        }                                                                                            \
    } while (0)

uint32_t shim_nr_dpus(void);
struct dpu_set_t shim_single(uint32_t i);

#define DPU_FOREACH(set, one, i) \
    for ((i) = 0, (one) = shim_single(0); (i) < shim_nr_dpus(); ++(i), (one) = shim_single(i))

dpu_error_t dpu_alloc(uint32_t nr_dpus, const char *profile, struct dpu_set_t *set);
dpu_error_t dpu_load(struct dpu_set_t set, const char *binary, void *program);
dpu_error_t dpu_get_nr_dpus(struct dpu_set_t set, uint32_t *nr_dpus);
dpu_error_t dpu_prepare_xfer(struct dpu_set_t one, void *buffer);
dpu_error_t dpu_push_xfer(struct dpu_set_t set, dpu_xfer_t xfer, const char *symbol, uint32_t offset, size_t length,
                          dpu_xfer_flags_t flags);
dpu_error_t dpu_launch(struct dpu_set_t set, dpu_launch_policy_t policy);
dpu_error_t dpu_log_read(struct dpu_set_t one, FILE *stream);
dpu_error_t dpu_free(struct dpu_set_t set);

#endif
