/* The UPMEM SDK stand-in's one translation unit: MRAM images, the WRAM arena, transfers and the launch loop. */
#include "upmem_shim.h"
#include "dpu.h"
#include "dpu_probe.h"

uint8_t *shim_mram;
uint32_t shim_tasklet;
uint8_t *shim_wram;
size_t shim_wram_used;

static uint32_t nr_dpus;
static uint8_t **images;  /* one MRAM image per DPU */
static void **xfer;       /* the host buffer dpu_prepare_xfer recorded per DPU */

int dpu_main(void);       /* the DPU program's main, renamed on the command line */

void shim_die(const char *what, unsigned long at, unsigned long n, unsigned long cap)
{
    fflush(stdout);
    fprintf(stderr, "upmem shim: %s out of bounds: %lu bytes at %lu, capacity %lu\n", what, n, at, cap);
    exit(SHIM_EXIT_BOUNDS);
}

uint32_t shim_nr_dpus(void) { return nr_dpus; }

struct dpu_set_t shim_single(uint32_t i)
{
    struct dpu_set_t s = {1, i};
    return s;
}

dpu_error_t dpu_alloc(uint32_t nr, const char *profile, struct dpu_set_t *set)
{
    (void)profile;
    if (nr == 0 || images)
        return DPU_ERR_SHIM;
    nr_dpus = nr;
    images = calloc(nr, sizeof *images);
    xfer = calloc(nr, sizeof *xfer);
    shim_wram = calloc(1, SHIM_WRAM_BYTES);
    if (!images || !xfer || !shim_wram)
        return DPU_ERR_SHIM;
    for (uint32_t i = 0; i < nr; ++i)
        if (!(images[i] = calloc(1, SHIM_MRAM_BYTES)))
            return DPU_ERR_SHIM;
    set->is_single = 0;
    set->idx = 0;
    return DPU_OK;
}

dpu_error_t dpu_load(struct dpu_set_t set, const char *binary, void *program)
{
    (void)set, (void)binary, (void)program;
    return DPU_OK;
}

dpu_error_t dpu_get_nr_dpus(struct dpu_set_t set, uint32_t *nr)
{
    *nr = set.is_single ? 1 : nr_dpus;
    return DPU_OK;
}

dpu_error_t dpu_prepare_xfer(struct dpu_set_t one, void *buffer)
{
    if (!one.is_single || one.idx >= nr_dpus)
        return DPU_ERR_SHIM;
    xfer[one.idx] = buffer;
    return DPU_OK;
}

dpu_error_t dpu_push_xfer(struct dpu_set_t set, dpu_xfer_t dir, const char *symbol, uint32_t offset, size_t length,
                          dpu_xfer_flags_t flags)
{
    (void)symbol, (void)flags;
    if (offset > SHIM_MRAM_BYTES || length > SHIM_MRAM_BYTES - offset)
        shim_die("host transfer", offset, length, SHIM_MRAM_BYTES);
    uint32_t lo = set.is_single ? set.idx : 0, hi = set.is_single ? set.idx + 1 : nr_dpus;
    for (uint32_t i = lo; i < hi; ++i) {
        if (!xfer[i])
            return DPU_ERR_SHIM;
        if (dir == DPU_XFER_TO_DPU)
            memcpy(images[i] + offset, xfer[i], length);
        else
            memcpy(xfer[i], images[i] + offset, length);
    }
    return DPU_OK;
}

dpu_error_t dpu_launch(struct dpu_set_t set, dpu_launch_policy_t policy)
{
    (void)policy;
    uint32_t lo = set.is_single ? set.idx : 0, hi = set.is_single ? set.idx + 1 : nr_dpus;
    for (uint32_t i = lo; i < hi; ++i) {
        shim_mram = images[i];
        for (shim_tasklet = 0; shim_tasklet < NR_TASKLETS; ++shim_tasklet)
            dpu_main();
    }
    return DPU_OK;
}

dpu_error_t dpu_log_read(struct dpu_set_t one, FILE *stream)
{
    (void)one, (void)stream;
    return DPU_OK;
}

dpu_error_t dpu_free(struct dpu_set_t set)
{
    (void)set;
    for (uint32_t i = 0; i < nr_dpus; ++i)
        free(images[i]);
    free(images);
    free(xfer);
    free(shim_wram);
    images = NULL;
    return DPU_OK;
}

dpu_error_t dpu_probe_init(const char *name, struct dpu_probe_t *probe) { (void)name, (void)probe; return DPU_OK; }
dpu_error_t dpu_probe_start(struct dpu_probe_t *probe) { (void)probe; return DPU_OK; }
dpu_error_t dpu_probe_stop(struct dpu_probe_t *probe) { (void)probe; return DPU_OK; }

dpu_error_t dpu_probe_get(struct dpu_probe_t *probe, dpu_probe_metric_t metric, dpu_probe_kind_t kind, double *value)
{
    (void)probe, (void)metric, (void)kind;
    *value = 0.0;
    return DPU_OK;
}
