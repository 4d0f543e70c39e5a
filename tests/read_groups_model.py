"""Selection model of AIM_FLAG_READ_GROUPS (include/aim_hip.h): per read, the AIM_PAIR_OK candidate of lowest score (lowest batch
index on a tie), the lowest score among the read's other OK candidates, and how many OK candidates share the best score."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
UINT32_MAX = 2 ** 32 - 1


def select(scores, status, read_offsets):
    """(best: aim_best_t rows as a structured array of capi.BEST_DTYPE's fields, sel: uint32 per read). `status` may be None (every
    candidate OK: the score-only rows of AIM_FLAG_RES8 carry no status)."""
    from aim_amd import capi
    scores = np.asarray(scores, dtype=np.int64)
    ok = np.ones(len(scores), dtype=bool) if status is None else np.asarray(status) == capi.PAIR_OK
    n_reads = len(read_offsets) - 1
    best = np.zeros(n_reads, dtype=capi.BEST_DTYPE)
    sel = np.zeros(n_reads, dtype=np.uint32)
    for r in range(n_reads):
        lo, hi = int(read_offsets[r]), int(read_offsets[r + 1])
        idx = lo + np.nonzero(ok[lo:hi])[0]
        if len(idx) == 0:
            best[r] = (UINT32_MAX, INT32_MAX, INT32_MAX, 0)
            sel[r] = lo
            continue
        s = scores[idx]
        b = int(s.min())
        first = int(idx[np.argmax(s == b)])            # lowest index among the best
        others = s[idx != first]
        second = int(others.min()) if len(others) else INT32_MAX
        best[r] = (first, b, second, int((s == b).sum()))
        sel[r] = first
    return best, sel
