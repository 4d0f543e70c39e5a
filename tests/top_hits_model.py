"""Ranking model of AIM_FLAG_TOP_HITS (include/aim_hip.h): per read, the AIM_PAIR_OK candidates by (score, batch index) ascending, then
the candidates that are not OK by batch index; read r gets the first min(K_r, max_hits) of them as rows [hit_offsets[r],
hit_offsets[r + 1])."""
import numpy as np


def hit_offsets(read_offsets, max_hits):
    """uint32[n_reads + 1]: the exclusive prefix sum of min(K_r, max_hits)."""
    k = np.diff(np.asarray(read_offsets, dtype=np.int64))
    out = np.zeros(len(k) + 1, dtype=np.uint32)
    out[1:] = np.cumsum(np.minimum(k, int(max_hits)))
    return out


def rank(scores, status, read_offsets, max_hits):
    """(hit_offsets, hit_pair): hit_pair[h] is the candidate (batch index) of hit row h. `status` may be None (every candidate OK)."""
    from aim_amd import capi
    scores = np.asarray(scores, dtype=np.int64)
    bad = np.zeros(len(scores), dtype=np.int64) if status is None else (np.asarray(status) != capi.PAIR_OK).astype(np.int64)
    key_score = np.where(bad == 1, 0, scores)                      # the score of a candidate that is not OK does not count
    hoff = hit_offsets(read_offsets, max_hits)
    hit_pair = np.zeros(int(hoff[-1]), dtype=np.uint32)
    for r in range(len(read_offsets) - 1):
        lo, hi = int(read_offsets[r]), int(read_offsets[r + 1])
        idx = np.arange(lo, hi)
        order = idx[np.lexsort((idx, key_score[lo:hi], bad[lo:hi]))]   # (last key first: class, score, index)
        n = int(hoff[r + 1]) - int(hoff[r])
        hit_pair[int(hoff[r]):int(hoff[r + 1])] = order[:n]
    return hoff, hit_pair
