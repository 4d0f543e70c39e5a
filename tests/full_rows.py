"""Inputs whose sequences fill READ_SIZE, the table of kernel shapes they are run on, and the comparison both full-row test modules
use. Plain numpy; the library is only asked for gen_pairs rows and (by the callers) for plans. No device.

The ABI refuses only pattern_len > READ_SIZE. gen_pairs / launcher_sizes always leave l + edits + 1 <= READ_SIZE, so without this
module no test has a sequence in the last column of its row, a row without zero padding behind it, a completely full ops row
(plen + tlen == 2 * READ_SIZE operations) or a last row that ends at the arrays' last byte."""
import math

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ACGTN = np.frombuffer(b"ACGTN", dtype=np.uint8)
HEAD = 11          # hand-made pairs at the front of every batch
N_SPECIAL = 17     # head + identical + twins + their follower + A/C + N-in-the-last-column
MIN_PAIRS = N_SPECIAL + 1


def head_lengths(rs):
    """(plen, tlen) of the hand-made head."""
    return [(rs, rs), (rs, rs - 1), (rs - 1, rs), (rs, rs - 2), (rs, rs // 2 + 3), (rs, rs // 3), (rs, 1), (1, rs), (2, rs),
            (rs, 0), (0, rs)]


# places of the constructed pairs behind the head
IDENTICAL, TWIN_A, TWIN_B, AFTER_TWINS, A_VS_C, N_LAST = HEAD, HEAD + 1, HEAD + 2, HEAD + 3, HEAD + 4, HEAD + 5


def pairs_for(rs):
    """Batch size per READ_SIZE: more than two 64-pair units plus a ragged tail while the oracle is cheap, fewer pairs (never a
    smaller READ_SIZE) where one pair costs READ_SIZE^2 cells."""
    return 130 if rs <= 1024 else (40 if rs <= 2048 else 20)


def _derived_text(rng, p, tlen):
    """A text of `tlen` bases from pattern p: about 2 % substitutions (at least one) and a few indels, then trimmed or extended
    with random bases to the length."""
    t = p.copy()
    if len(t):
        for k in rng.integers(0, len(t), size=max(1, len(t) // 50)):
            t[k] = ACGT[(int(np.searchsorted(ACGT, t[k])) + 1 + int(rng.integers(0, 3))) % 4]
        for _ in range(3):
            at = int(rng.integers(0, len(t) + 1))
            if rng.integers(0, 2) and len(t) > 1:
                t = np.delete(t, min(at, len(t) - 1))
            else:
                t = np.insert(t, at, ACGT[rng.integers(0, 4)])
    if len(t) >= tlen:
        return t[:tlen].copy()
    return np.concatenate([t, ACGT[rng.integers(0, 4, size=tlen - len(t))]])


def full_row_batch(rs, n, seed, pad="zero"):
    """(requests, patterns[n][rs], texts[n][rs]) in the wire layout. Pairs 0..10: head_lengths(rs), each text derived from its
    pattern. IDENTICAL: one full pattern against itself. TWIN_A, TWIN_B: the same full pattern and the same full text twice in a
    row (an extend that runs past its row keeps matching in the next); AFTER_TWINS: the twins' rows with the first base of the
    text changed, so the two arrays differ right behind TWIN_B. A_VS_C: 'A' * rs against 'C' * rs. N_LAST: a full pair with 'N'
    in the last column of both sequences. Then gen_pairs rows at l = (rs - 8) * 100 // 104, e = 2 %, and a full / full pair
    last, so the batch ends at the arrays' last byte. pad = "zero" leaves the bytes behind each length 0, "noise" fills them
    with seeded bytes from ACGTN, the two arrays independently; the sequences themselves do not depend on `pad`."""
    from aim_amd import capi, engine
    if n < MIN_PAIRS:
        raise ValueError("a full-row batch has at least %d pairs" % MIN_PAIRS)
    if pad not in ("zero", "noise"):
        raise ValueError("pad is 'zero' or 'noise'")
    rng = np.random.default_rng([int(seed), int(rs), 0x66756C6C])
    req = np.zeros(n, dtype=capi.REQUEST_DTYPE)
    pat = np.zeros((n, rs), dtype=np.uint8)
    txt = np.zeros((n, rs), dtype=np.uint8)

    def put(i, p, t):
        pat[i, :len(p)], txt[i, :len(t)] = p, t
        req["pattern_len"][i], req["text_len"][i] = len(p), len(t)

    def full():
        return ACGT[rng.integers(0, 4, size=rs)]

    for i, (pl, tl) in enumerate(head_lengths(rs)):
        p = ACGT[rng.integers(0, 4, size=pl)]
        put(i, p, _derived_text(rng, p, tl))
    p = full()
    put(IDENTICAL, p, p)
    p = full()
    t = _derived_text(rng, p, rs)
    put(TWIN_A, p, t)
    put(TWIN_B, p, t)
    t2 = t.copy()
    t2[0] = ACGT[(int(np.searchsorted(ACGT, p[0])) + 1) % 4]          # pattern[0] != text[0] right behind TWIN_B's rows
    put(AFTER_TWINS, p, t2)
    put(A_VS_C, np.full(rs, ord("A"), np.uint8), np.full(rs, ord("C"), np.uint8))
    p = full()
    t = _derived_text(rng, p, rs)
    p[rs - 1] = t[rs - 1] = ord("N")
    put(N_LAST, p, t)
    body = n - N_SPECIAL - 1
    if body:
        l = max(1, (rs - 8) * 100 // 104)
        breq, bpat, btxt = engine.gen_pairs(int(seed), 0, body, l, 0.02, rs)
        s = slice(N_SPECIAL, N_SPECIAL + body)
        pat[s], txt[s] = bpat, btxt
        req["pattern_len"][s], req["text_len"][s] = breq["pattern_len"], breq["text_len"]
    p = full()
    put(n - 1, p, _derived_text(rng, p, rs))
    req["idx"] = 5000 + np.arange(n, dtype=np.uint32)
    if pad == "noise":
        nrng = np.random.default_rng([int(seed), int(rs), 0x6E6F6973])
        col = np.arange(rs)[None, :]
        for rows, key in ((pat, "pattern_len"), (txt, "text_len")):
            noise = ACGTN[nrng.integers(0, 5, size=rows.shape)]
            behind = col >= req[key].astype(np.int64)[:, None]
            rows[behind] = noise[behind]
    return req, pat, txt


def head_only(req, pat, txt, extra=()):
    """The head pairs (and the places in `extra`) of a batch, as a batch of their own."""
    sel = np.array(list(range(HEAD)) + list(extra))
    return req[sel].copy(), np.ascontiguousarray(pat[sel]), np.ascontiguousarray(txt[sel])


# ------------------------------------------------------------------ models
def nw_model(req, pat, txt, x=3, gi=4, gd=4, drop_last_column=False):
    """NW score per pair by the plain recurrence, one text base (row h) at a time over the whole pattern: moving along the
    pattern costs gd, along the text gi (nw.c:67-153). Valid where plen <= tlen: with a longer pattern the reference's flat table
    aliases and its score is no longer the recurrence's. drop_last_column: the mutation of test_full_rows_cpu's mutation check
    (a kernel that leaves out column tlen when tlen == READ_SIZE)."""
    out = np.zeros(len(req), dtype=np.int64)
    rs = pat.shape[1]
    for i in range(len(req)):
        pl, tl = int(req["pattern_len"][i]), int(req["text_len"][i])
        if drop_last_column and tl == rs:
            tl -= 1
        p = pat[i, :pl].astype(np.int64)
        v = np.arange(pl + 1, dtype=np.int64)
        row = v * gd
        for h in range(1, tl + 1):
            best = np.empty(pl + 1, dtype=np.int64)
            best[0] = h * gi
            best[1:] = np.minimum(row[:-1] + np.where(p == txt[i, h - 1], 0, x), row[1:] + gi)
            # the dependency along the pattern: cur[v] = min_k (best[k] + (v - k) * gd)
            row = np.minimum.accumulate(best - v * gd) + v * gd
        out[i] = row[pl]
    return out


def affine_model(req, pat, txt, x=3, o=4, e=1):
    """Global gap-affine optimum per pair (three-state Gotoh DP, tests/endsfree_model.py with no free ends)."""
    from endsfree_model import dp_scores
    return dp_scores(req, pat, txt, x=x, o=o, e=e, ends_free=(0, 0, 0, 0))


def extend_stops_on_zero(req, pat, txt, reach=64):
    """The batch as a kernel sees it whose extend stops on a 0 byte instead of on the length (the mutation check's second
    mutation): every sequence runs on through whatever follows it in its array -- its padding, then the next pair's row -- up to
    the first 0 byte, at most `reach` bytes. Returns (requests, patterns, texts) with rows `reach` wider."""
    n, rs = pat.shape
    out = req.copy()
    wide = [np.zeros((n, rs + reach), dtype=np.uint8), np.zeros((n, rs + reach), dtype=np.uint8)]
    for rows, w, key in ((pat, wide[0], "pattern_len"), (txt, wide[1], "text_len")):
        flat = np.concatenate([rows.reshape(-1), np.zeros(reach, dtype=np.uint8)])
        for i in range(n):
            ln = int(req[key][i])
            tail = flat[i * rs + ln:i * rs + ln + reach]
            stop = np.nonzero(tail == 0)[0]
            ln += int(stop[0]) if stop.size else reach
            w[i, :ln] = flat[i * rs:i * rs + ln]
            out[key][i] = ln
    return out, wide[0], wide[1]


# ------------------------------------------------------------------ the table
def launcher_score(rs, e, cost):
    """MAX_SCORE of a read that fills READ_SIZE at error rate e (the launchers' rule at read length rs / (1 + e))."""
    return max(1, math.ceil(rs / (1.0 + e) * e * cost))


def _fam(algo, ms, env=None, **kw):
    return dict(algo=algo, ms=ms, kw=kw, env=env or {})


FAMILIES = {
    "nw": _fam("nw", lambda rs: launcher_score(rs, 0.02, 4)),
    "nw_bt": _fam("nw", lambda rs: launcher_score(rs, 0.02, 4), backtrace=True),
    "nw_bt_733": _fam("nw", lambda rs: launcher_score(rs, 0.02, 4), backtrace=True, mismatch=7, gap_i=3, gap_d=3),
    "nw_noreg": _fam("nw", lambda rs: launcher_score(rs, 0.02, 4), env={"AIM_NO_NW_REG": "1"}),
    "nw_noreg_bt": _fam("nw", lambda rs: launcher_score(rs, 0.02, 4), env={"AIM_NO_NW_REG": "1"}, backtrace=True),
    "swg16": _fam("swg", lambda rs: launcher_score(rs, 0.05, 5), swg_w16=True),
    "swg16_bt": _fam("swg", lambda rs: launcher_score(rs, 0.05, 5), swg_w16=True, backtrace=True),
    "swg8_bt": _fam("swg", lambda rs: 100, backtrace=True),
    "wfa5": _fam("wfa", lambda rs: 5, reduce=True),
    "wfa5_bt": _fam("wfa", lambda rs: 5, reduce=True, backtrace=True),
    "wfa2": _fam("wfa", lambda rs: launcher_score(rs, 0.02, 5)),
    "wfa2_bt": _fam("wfa", lambda rs: launcher_score(rs, 0.02, 5), backtrace=True),
    "wfa2_red": _fam("wfa", lambda rs: launcher_score(rs, 0.02, 5), reduce=True),
    "wfa2_red_bt": _fam("wfa", lambda rs: launcher_score(rs, 0.02, 5), reduce=True, backtrace=True),
    "wfa_wave": _fam("wfa", lambda rs: launcher_score(rs, 0.02, 5), env={"AIM_FORCE_WAVE": "1"}),
    "wfa_wave_red_bt": _fam("wfa", lambda rs: launcher_score(rs, 0.02, 5), env={"AIM_FORCE_WAVE": "1"}, reduce=True, backtrace=True),
    "genasm": _fam("genasm", lambda rs: 0),
    "genasm_bt": _fam("genasm", lambda rs: 0, backtrace=True),
}

_G = "dp_group_kernel lanes_per_pair=%d"
_S = "dp_strip_kernel wavefronts_per_pair=%d cells_per_lane=20"
_W = "wfa_group_kernel G=%d"
_WFA5 = [(72, "wfa_lane_packed_kernel pack_first=1"), (80, "wfa_lane_kernel"), (88, _W % 2), (104, "wfa_lane_packed_kernel pack_first=1"),
         (112, "wfa_lane_kernel"), (120, _W % 2), (136, "wfa_lane_packed_kernel pack_first=1"), (176, "wfa_lane_packed_kernel pack_first=1"),
         (184, _W % 4), (544, _W % 64), (904, _W % 8), (2440, _W % 16)]
_WFA2 = [(8, _W % 1), (16, _W % 2), (56, _W % 4), (88, _W % 4), (144, _W % 8), (320, _W % 16), (664, _W % 32)]
_GENASM = [(rs, "genasm_wave_kernel") for rs in (8, 64, 104, 128, 1000)]

# family -> [(READ_SIZE, kernel name and shape token of aim_plan_describe at pairs_for(READ_SIZE) pairs, 16 GB, 256 CUs)].
# tests/test_full_rows_cpu.py checks every entry against the planner: when a planner change moves an edge, it prints the new line
# and the row takes the new first READ_SIZE of that shape.
TABLE = {
    "nw": [(40, "nw_reg_kernel"), (104, "nw_reg_kernel"), (120, "nw_reg_kernel"), (136, "nw_reg_kernel"), (176, "nw_reg_kernel"),
           (184, _G % 6), (192, _G % 6), (1024, _G % 32), (1032, _G % 19), (1280, _G % 32), (1288, _G % 27), (1536, _G % 32),
           (1544, _G % 28), (1792, _G % 56), (1800, _S % 2), (2568, _S % 3), (3848, _S % 4)],
    "nw_bt": [(40, "nw_reg_kernel"), (104, "nw_reg_kernel"), (136, "nw_reg_kernel"), (176, "nw_reg_kernel"), (184, _G % 6), (192, _G % 6),
              (1024, _G % 32), (1032, _G % 26), (1280, _G % 32), (1288, _S % 2), (1440, _G % 45), (2048, _G % 64), (2560, _G % 64),
              (2568, _S % 3)],
    "nw_bt_733": [(104, "nw_reg_kernel"), (192, _G % 6), (1024, _G % 32), (1288, _S % 2), (2048, _G % 64)],
    "nw_noreg": [(120, "nw_lane_kernel seq_lds=")],
    "nw_noreg_bt": [(104, "nw_lane_kernel seq_lds=")],
    "swg16": [(40, "swg_reg_kernel"), (136, "swg_reg_kernel"), (184, _G % 6), (192, _G % 6), (1024, _G % 32), (1032, _G % 26),
              (1536, _G % 32), (1544, _S % 2), (2568, _S % 3)],
    "swg16_bt": [(40, "swg_reg_kernel"), (136, "swg_reg_kernel"), (184, _G % 6), (192, _G % 6), (1000, _G % 32), (1024, _G % 32),
                 (1032, _S % 1), (1288, _S % 2), (1440, _G % 45), (2024, _G % 64), (2048, _G % 64), (2056, _S % 2), (2568, _S % 3),
                 (3848, _S % 4)],
    "swg8_bt": [(40, "swg_reg_kernel"), (136, "swg_lane_kernel seq_lds=1"), (800, "swg_lane_kernel seq_lds=0"),
                (1192, "swg_lane_kernel seq_lds=0"), (1200, "dp_wave_kernel wavefronts_per_pair=2"),
                (1544, "dp_wave_kernel wavefronts_per_pair=4")],
    "wfa5": _WFA5,
    "wfa5_bt": _WFA5,
    "wfa2": _WFA2 + [(3000, _W % 64)],
    "wfa2_bt": _WFA2 + [(3000, _W % 64)],
    "wfa2_red": _WFA2 + [(3000, _W % 32)],
    "wfa2_red_bt": _WFA2 + [(3000, _W % 32)],
    "wfa_wave": [(544, "wfa_wave_kernel seq_lds=1"), (1064, "wfa_wave_kernel seq_lds=1")],
    "wfa_wave_red_bt": [(544, "wfa_wave_kernel seq_lds=1"), (1064, "wfa_wave_kernel seq_lds=1")],
    "genasm": _GENASM,
    "genasm_bt": _GENASM,
}
# Feature rows: head pairs only, every pair under the cap (MAX_SCORE 2 * READ_SIZE + 8 holds a gap of READ_SIZE bases at 4 + 1 per
# base; gap-linear at 3 per base needs 4 * READ_SIZE + 8), each flag against its own model.
FEATURES = {
    "endsfree": dict(ends_free=(0, 0, 16, 16)),
    "affine2p": dict(gap2=(24, 1)),
    "linear": dict(linear=True, mismatch=2, gap_e=3),
    "w32": dict(w32=True),
    "bidir": dict(bidir=True),
}
FEATURE_ROWS = [(f, rs) for f in FEATURES for rs in (112, 1024) if not (f == "w32" and rs == 112)]


def feature_params(feature, rs, backtrace=True):
    from aim_amd import engine
    return engine.make_params("wfa", (4 if feature == "linear" else 2) * rs + 8, rs, backtrace=backtrace, **FEATURES[feature])


ROWS = [(fam, rs) for fam, rows in TABLE.items() for rs, _ in rows]
KERNEL_NAMES = ("wfa_wave_kernel", "wfa_bidir_kernel", "wfa_lane_kernel", "wfa_lane_packed_kernel", "wfa_group_kernel", "nw_lane_kernel",
                "swg_lane_kernel", "nw_reg_kernel", "swg_reg_kernel", "dp_wave_kernel", "dp_strip_kernel", "dp_group_kernel",
                "genasm_wave_kernel")      # kernel_name(), capi_plan.hip
SEED = 20261


# Pairs on the to-do list (aim_set_fallback_pairs) per row, as first measured on an MI355X; zero and noise padding give the same
# count. dp_group hands on the two pairs with an empty sequence; the WFA kernels with a list one pair (four under
# the reduction at READ_SIZE 3000); the register kernels also the walks that leave their band. Kernels without a
# list report 0.
_TODO_BY_KERNEL = {"dp_group_kernel": 2, "wfa_group_kernel": 1, "wfa_lane_packed_kernel": 1}
_TODO = {("nw", 40): 7, ("nw", 104): 7, ("nw", 120): 7, ("nw", 136): 7, ("nw", 176): 18, ("nw_bt", 40): 7, ("nw_bt", 104): 7,
         ("nw_bt", 136): 7, ("nw_bt", 176): 18, ("nw_bt_733", 104): 8, ("swg16", 40): 7, ("swg16", 136): 7, ("swg16_bt", 40): 8,
         ("swg16_bt", 136): 8, ("swg8_bt", 40): 8, ("wfa2_red", 3000): 4, ("wfa2_red_bt", 3000): 4}


def expected_todo(fam, rs):
    if (fam, rs) in _TODO:
        return _TODO[(fam, rs)]
    kernel = expected_plan(fam, rs).split()[0]
    assert kernel not in ("nw_reg_kernel", "swg_reg_kernel"), "a register-kernel row needs its own entry in _TODO"
    return _TODO_BY_KERNEL.get(kernel, 0)


def expected_plan(fam, rs):
    return dict(TABLE[fam])[rs]


def row_params(fam, rs):
    from aim_amd import engine
    f = FAMILIES[fam]
    return engine.make_params(f["algo"], f["ms"](rs), rs, **f["kw"])


def row_batch(rs, pad):
    return full_row_batch(rs, pairs_for(rs), SEED, pad)


def plan_matches(line, want):
    """aim_plan_describe's line names the kernel first; the shape tokens follow in the line's own order."""
    words = want.split()
    have = line.split()
    if have[0] != words[0]:
        return False
    return all(any(h.startswith(w) if w.endswith("=") else h == w for h in have[1:]) for w in words[1:])


# ------------------------------------------------------------------ the oracle and the comparison
def oracle_params(params, algo):
    from aim_amd import capi
    from oracle import oracle
    return oracle.params(algo, params.max_score, params.read_size, match=params.match, mismatch=params.mismatch, gap_o=params.gap_o,
                         gap_e=params.gap_e, gap_i=params.gap_i, gap_d=params.gap_d, backtrace=bool(params.flags & capi.FLAG_BACKTRACE),
                         reduce=bool(params.flags & capi.FLAG_REDUCE), swg_cell_bytes=2 if (params.flags & capi.FLAG_SWG_W16) else 0)


_ORACLE = {}


def oracle_row(fam, rs, pad):
    """(results, ops) of the oracle on a table row's batch; computed once per session and never changed afterwards."""
    key = (fam, rs, pad)
    if key not in _ORACLE:
        from oracle import oracle
        req, pat, txt = row_batch(rs, pad)
        op = oracle_params(row_params(fam, rs), FAMILIES[fam]["algo"])
        res, ops, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
        res.flags.writeable = False
        if ops is not None:
            ops.flags.writeable = False
        _ORACLE[key] = (res, ops)
    return _ORACLE[key]


FIELDS = ("score", "max_operations", "end_offset", "status")


def compare(res, ops, ores, oops, req, backtrace, idx=True):
    """_compare's strictness (test_gpu_parity.py): score, max_operations, end_offset and status of every pair, whatever its
    status; with CIGAR also begin_offset and every ops byte inside [begin_offset, end_offset) of every pair the oracle finishes
    (where it stops with a status the reference exits, and there is no traceback to compare; the statuses themselves must be
    equal pair by pair). Raises AssertionError naming the first pair that differs."""
    assert len(res) == len(ores) == len(req)
    if idx:          # (False: `res` is an oracle run too, which numbers its rows itself)
        assert np.array_equal(res["idx"], req["idx"]), "idx differs"
    for f in FIELDS:
        bad = np.nonzero(res[f] != ores[f])[0]
        assert bad.size == 0, "%s differs at pair %d: got %d, oracle %d (plen %d tlen %d; %d pairs differ)" % (
            f, bad[0], res[f][bad[0]], ores[f][bad[0]], req["pattern_len"][bad[0]], req["text_len"][bad[0]], bad.size)
    if backtrace:
        done = ores["status"] == 0
        bad = np.nonzero((res["begin_offset"] != ores["begin_offset"]) & done)[0]
        assert bad.size == 0, "begin_offset differs at pair %d: got %d, oracle %d (plen %d tlen %d)" % (
            bad[0], res["begin_offset"][bad[0]], ores["begin_offset"][bad[0]], req["pattern_len"][bad[0]], req["text_len"][bad[0]])
        for i in np.nonzero(done)[0]:
            b, e = int(ores["begin_offset"][i]), int(ores["end_offset"][i])
            if not np.array_equal(ops[i, b:e], oops[i, b:e]):
                raise AssertionError("ops differ at pair %d (plen %d tlen %d): got %r oracle %r" % (
                    i, req["pattern_len"][i], req["text_len"][i], ops[i, b:e].tobytes()[-60:], oops[i, b:e].tobytes()[-60:]))


# ------------------------------------------------------------------ workers (their own process: knobs are environment variables)
def _with_env(env):
    import os
    for k, v in env.items():
        os.environ[k] = v


def _without_env(env):
    import os
    for k in env:
        os.environ.pop(k, None)


def plan_line(params, n):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    buf = C.create_string_buffer(1024)
    rc = lib.aim_plan_describe(capi.params_ref(params), n, buf, len(buf))
    return buf.value.decode() if rc == 0 else "error %d: %s" % (rc, lib.aim_last_error().decode(errors="replace"))


def plan_lines():
    """{"family/READ_SIZE": aim_plan_describe's line} for every table row, under the row's own knobs."""
    out = {}
    for fam, rs in ROWS:
        env = FAMILIES[fam]["env"]
        _with_env(env)
        out["%s/%d" % (fam, rs)] = plan_line(row_params(fam, rs), pairs_for(rs))
        _without_env(env)
    return out


def align_row(fam, rs, pad):
    """(results, ops, plan line, fallback pairs) of a table row's batch on the device, under the row's own knobs."""
    from aim_amd import engine
    req, pat, txt = row_batch(rs, pad)
    params = row_params(fam, rs)
    env = FAMILIES[fam]["env"]
    _with_env(env)
    try:
        with engine.DeviceSet(1) as s:
            s.configure(params, len(req))
            s.push(0, req, pat, txt)
            s.launch()
            res, ops = s.pull(0, check=False)
            return res, ops, s.plan_describe(0), s.fallback_pairs(0)
    finally:
        _without_env(env)


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1] == "--plans":
        json.dump(plan_lines(), sys.stdout)
    elif sys.argv[1] == "--align":       # --align OUT.npz family/READ_SIZE ...: zero-padded rows, results and ops inside [begin, end)
        out = {}
        for key in sys.argv[3:]:
            fam, rs = key.split("/")
            res, ops, _, _ = align_row(fam, int(rs), "zero")
            out[key + "/res"] = res
            if ops is not None:
                col = np.arange(ops.shape[1])[None, :]
                inside = (col >= res["begin_offset"][:, None]) & (col < res["end_offset"][:, None])
                out[key + "/ops"] = np.where(inside, ops, 0)
        np.savez(sys.argv[2], **out)
