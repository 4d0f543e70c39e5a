"""Selection model of AIM_FLAG_MATE_PAIRS (include/aim_hip.h), in plain Python: reads 2m and 2m + 1 are mates. Per read pair the proper
combination (both candidates OK, opposite strands, the strand-0 window not right of the strand-1 window, window span inside
[min_span, max_span]) of lowest cost score_i + score_j wins, ties by lowest i then lowest j, if its cost is at most the unpaired cost
(the independent READ_GROUPS winners' scores + unpaired_penalty); otherwise the independent winners stay."""
import numpy as np

import read_groups_model

INT32_MAX = 2 ** 31 - 1
UINT32_MAX = 2 ** 32 - 1
MINUS = 1 << 63
PROPER = 1


def clamp(v):
    return min(int(v), INT32_MAX - 1)


def select(scores, status, text_pos, text_len, read_offsets, min_span, max_span, unpaired_penalty):
    """(sel: uint32 per read, mates: aim_mate_t rows with capi.MATE_DTYPE's fields, best: the independent aim_best_t rows).
    `status` may be None (every candidate OK)."""
    from aim_amd import capi
    n_reads = len(read_offsets) - 1
    assert n_reads % 2 == 0
    scores = [int(x) for x in scores]
    ok = [True] * len(scores) if status is None else [int(x) == capi.PAIR_OK for x in status]
    start = [int(x) & (MINUS - 1) for x in text_pos]
    minus = [bool(int(x) & MINUS) for x in text_pos]
    end = [s + int(l) for s, l in zip(start, text_len)]
    best, sel = read_groups_model.select(scores, status, read_offsets)
    sel = sel.copy()
    mates = np.zeros(n_reads // 2, dtype=capi.MATE_DTYPE)
    for m in range(n_reads // 2):
        a, b = 2 * m, 2 * m + 1
        has_a, has_b = int(best["n_best"][a]) > 0, int(best["n_best"][b]) > 0
        row = mates[m]
        row["best_pair"] = (int(best["best_pair"][a]) if has_a else UINT32_MAX, int(best["best_pair"][b]) if has_b else UINT32_MAX)
        row["score_sum"], row["second_sum"] = INT32_MAX, INT32_MAX
        if not (has_a and has_b):
            continue
        proper = []                                   # (cost, i, j) in batch indices
        for i in range(int(read_offsets[a]), int(read_offsets[a + 1])):
            for j in range(int(read_offsets[b]), int(read_offsets[b + 1])):
                if not (ok[i] and ok[j]) or minus[i] == minus[j]:
                    continue
                f, r = (j, i) if minus[i] else (i, j)
                if start[f] <= start[r] and min_span <= end[r] - start[f] <= max_span:
                    proper.append((clamp(scores[i] + scores[j]), i, j))
        unpaired = clamp(int(best["best_score"][a]) + int(best["best_score"][b]) + int(unpaired_penalty))
        if proper and min(proper)[0] <= unpaired:
            cost, i, j = min(proper)
            others = [c for c, x, y in proper if (x, y) != (i, j)]
            row["best_pair"] = (i, j)
            row["score_sum"] = cost
            row["second_sum"] = min(others) if others else INT32_MAX
            row["n_best"] = sum(1 for c, _, _ in proper if c == cost)
            row["flags"] = PROPER
            sel[a], sel[b] = i, j
        else:
            row["score_sum"] = unpaired
            row["second_sum"] = min(proper)[0] if proper else INT32_MAX
    return sel, mates, best
