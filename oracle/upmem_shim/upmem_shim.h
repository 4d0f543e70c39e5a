/* A stand-in for the UPMEM SDK, enough to compile the unmodified reference (host and DPU side) into one CPU
 * program: "MRAM" is a host buffer per DPU, "WRAM" one bump arena, tasklets run one after the other.
 * Written from SURVEY.md Appendix C and the list of SDK calls the reference makes; holds no reference text.
 * Sizes: -DSHIM_MRAM_BYTES (per DPU image) and -DSHIM_WRAM_BYTES (arena). Every access is bounds-checked, so an
 * overrun of either stops the program with a message and exit code 97 instead of corrupting the run. */
#ifndef AIM_UPMEM_SHIM_H
#define AIM_UPMEM_SHIM_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef SHIM_MRAM_BYTES
#define SHIM_MRAM_BYTES (64ul << 20)
#endif
#ifndef SHIM_WRAM_BYTES
#define SHIM_WRAM_BYTES (1ul << 30)
#endif
#ifndef NR_TASKLETS
#define NR_TASKLETS 1
#endif
#define SHIM_EXIT_BOUNDS 97

/* ---- DPU side ---- */
#define __mram_ptr
#define __mram_noinit
#define __mram
#define __host
#define __dma_aligned __attribute__((aligned(8)))
#define DPU_MRAM_HEAP_POINTER ((__mram_ptr void *)(uintptr_t)0)

extern uint8_t *shim_mram;     /* the image of the DPU that is running */
extern uint32_t shim_tasklet;  /* the tasklet that is running */
extern uint8_t *shim_wram;
extern size_t shim_wram_used;

void shim_die(const char *what, unsigned long at, unsigned long n, unsigned long cap);

static inline uint32_t me(void) { return shim_tasklet; }

static inline void shim_mram_check(uintptr_t at, unsigned long n)
{
    if (at > SHIM_MRAM_BYTES || n > SHIM_MRAM_BYTES - at)
        shim_die("MRAM access", at, n, SHIM_MRAM_BYTES);
}

static inline void mram_read(const __mram_ptr void *from, void *to, unsigned int n)
{
    shim_mram_check((uintptr_t)from, n);
    memcpy(to, shim_mram + (uintptr_t)from, n);
}

static inline void mram_write(const void *from, __mram_ptr void *to, unsigned int n)
{
    shim_mram_check((uintptr_t)to, n);
    memcpy(shim_mram + (uintptr_t)to, from, n);
}

static inline void mem_reset(void) { shim_wram_used = 0; }

static inline void *mem_alloc(size_t n)
{
    n = (n + 7) & ~(size_t)7;
    if (n > SHIM_WRAM_BYTES - shim_wram_used)
        shim_die("WRAM mem_alloc", shim_wram_used, n, SHIM_WRAM_BYTES);
    void *p = shim_wram + shim_wram_used;
    shim_wram_used += n;
    return p;
}

/* tasklets run in turn, so a barrier has nobody to wait for */
typedef struct { int unused; } barrier_t;
#define BARRIER_INIT(name, count) barrier_t name = {0}
static inline void barrier_wait(barrier_t *b) { (void)b; }

#endif
