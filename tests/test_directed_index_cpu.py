"""The directed indexes (tests/directed_index.py) are what they claim, on the models alone: every scenario's claim -- both sides of
its edge -- is asserted on the model's own detail (n_hits and flags, the cluster list, pred, f and the trees), for the stride kernels'
index, the minimizer kernels' and each hit cap of the long kernel; the builder's output satisfies INDEX; a scenario marked high keeps a
hit with bit 31 of its position set; E4's raw arrays can form no index outside the allocations; and the obvious off-by-one at an edge,
applied to a copy of a model, changes the expected bytes of the scenario that sits on it. No device, no library."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_model as cm  # noqa: E402
import directed_index as d  # noqa: E402
import minimizer_model as mm  # noqa: E402
import seed_model as m  # noqa: E402

BIT31, BIT63 = 1 << 31, 1 << 63
RUNS = [(name, kernel, H) for name, kernel, H, K in d.runs() if K == (d.TABLE[name][0]["K"] if isinstance(d.TABLE[name][0]["K"], int) else 16)]


class View:
    """What one run of a model says about one read of a batch."""

    def __init__(self, name, kernel, H, K, r, out, detail):
        b = d.batch(name, d.MODE[kernel], H)
        self.b, self.P, self.q, self.K, self.kernel = b, b["params"], b["queries"][r], K, kernel
        self.k, self.rs, self.band = self.P["k"], self.P["read_size"], self.P["band"]
        self.cap = H if kernel == "long" else 1024
        self.req, self.tpos, self.votes = (x[r * K:(r + 1) * K] for x in out[:3])
        self.row = out[3][r]
        self.n = int(self.row["n_cands"])
        self.n_hits, self.flags = self.row["n_hits"].tolist(), int(self.row["flags"])
        self.start = [int(t) & (BIT63 - 1) for t in self.tpos]
        self.strand = [int(t) >> 63 for t in self.tpos]
        if kernel in d.VOTING:
            w = None if kernel == "cand" else d.W
            self.keys = []
            for s in (0, 1):
                query = self.q.read if s == 0 else m.revcomp(self.q.read)
                hits = (m.strand_hits(query, *b["index"], self.k, 1, self.P["max_occ"], self.rs) if w is None else
                        mm.strand_hits(query, *b["index"], self.k, w, self.P["max_occ"], self.rs)[:2])
                self.keys.append(hits[0])
            self.cl = [m.clusters(ks, self.band) for ks in self.keys]
        else:
            self.ch = out[4][r * K:(r + 1) * K]
            self.d = detail[2 * r:2 * r + 2]            # per strand (anchors, f, pred)


def kept_positions(v):
    """The positions of the read's kept hits, both strands; for a voting kernel key - read_size, which is p - j: no more than p."""
    if v.kernel in d.VOTING:
        return [key - v.rs for keys in v.keys for key in keys]
    return [p for a, _, _ in v.d for p, _ in a]


# ---- the claims: name -> function of a View. `hits` holds for every kernel, `vote` for the voting kernels, `chain` for the chaining ----
def hits_claims(v, name):
    cap = v.cap
    if name.startswith("H1"):
        s = int(name[-1])
        assert v.n_hits[s] == cap and v.n_hits[1 - s] == 0 and v.flags == (m.TRUNCATED if "+1" in name else 0)
    elif name == "H2":
        assert v.n_hits == [cap, 6] and v.flags == m.TRUNCATED
    elif name.startswith("H3"):
        runs = sorted(len(x) for x in occ_of(v))
        assert runs == [v.P["max_occ"], v.P["max_occ"] + 1] and v.n_hits == [v.P["max_occ"], 0] and v.flags == 0
    elif name == "H4":
        assert [len(x) for x in occ_of(v)] == [3000] and v.n_hits == [cap, 0] and v.flags == m.TRUNCATED
    elif name.startswith("H5"):
        assert v.n_hits == [1, 0] and v.flags == 0 and v.n == 1
        (c, run), = occ_items(v)
        j = v.rs - v.k if ".last" in name else 0
        assert c == int(v.q.code[0][j]) and v.q.L == v.rs and run == [d.REF_LEN - v.k if ".top" in name else 0]


def occ_items(v):
    """[(code, run)] of the codes the read looks up that have a run in the batch's index."""
    bucket, pos = v.b["index"]
    return [(c, pos[bucket[c]:bucket[c + 1]].tolist()) for c in sorted(v.q.looked_up()) if bucket[c + 1] > bucket[c]]


def occ_of(v):
    return [run for _, run in occ_items(v)]


def vote_claims(v, name):
    votes = [[c[0] for c in cl] for cl in v.cl]
    if name == "V5.few":
        assert votes == [[2], []] and v.n == 1
    elif name.startswith("V1"):
        assert votes == ([[2], []] if name.endswith(".at") else [[1, 1], []])
        a = sorted(v.keys[0])
        assert a[1] - a[0] == v.band + (0 if name.endswith(".at") else 1)
    elif name.startswith("V2"):
        (v1, lo1, hi1), (v2, lo2, hi2) = v.cl[0]
        assert (v1, v2) == (2, 2) and hi1 - lo1 == v.band == hi2 - lo2 and hi1 < 2 * v.rs and lo2 - hi1 > BIT31 and hi2 == d.REF_LEN - v.k + v.rs - v.q.js[0][3]
        assert v.n == (2 if v.P["min_votes"] <= 2 else 0)
    elif name == "V3":
        assert votes == [[1024], []] and v.n == 1 and int(v.votes[0]) == 1024 and v.cl[0][0][2] - v.cl[0][0][1] > 0xF0000000
    elif name == "V4.min1025":
        assert votes == [[1024], []] and v.n == 0 and not v.tpos.any() and not v.votes.any()
    elif name.startswith("V4"):
        mv = v.P["min_votes"]
        assert sorted(votes[0]) == [mv - 1, mv] and votes[1] == [] and v.n == 1 and int(v.votes[0]) == mv
    elif name == "V5":
        assert sorted(votes[0]) == [2] * 10 and sorted(votes[1]) == [2] * 10 + [3]
        want = sorted([(-c[0], s, c[1]) for s in (0, 1) for c in v.cl[s]])[:v.K]
        assert v.n == len(want) == v.K
        assert [(-int(x), s, t + v.rs + 8) for x, s, t in zip(v.votes, v.strand, v.start)] == want      # (start = a_lo - read_size - flank)
        assert want[0][:2] == (-3, 1) and [w[1] for w in want[1:11]] == [0] * len(want[1:11]) and [w[1] for w in want[11:]] == [1] * len(want[11:])
        lo0 = [c[1] for c in v.cl[0]]
        assert lo0 == sorted(lo0) and v.keys[0] != sorted(v.keys[0])      # (the hits do not come sorted)
    elif name.startswith("V6"):
        _, a_lo, a_hi = (v.cl[1] if name == "V6.s1" else v.cl[0])[0]
        lo = a_lo - v.rs - v.P["flank"]
        hi = lo + v.q.L + 2 * v.P["flank"] + min(a_hi - a_lo, v.rs)
        assert v.n == 1 and int(v.req["text_len"][0]) == v.rs
        if name == "V6.lo":
            assert lo < 0 and v.start[0] == 0
        elif name == "V6.hi":
            assert hi > d.REF_LEN and v.start[0] == lo and lo & BIT31
        elif name == "V6.span":
            assert a_hi - a_lo > v.rs and v.cl[0][0][0] == 20
        else:
            assert v.strand[0] == 1 and v.start[0] & BIT31 and int(v.tpos[0]) >> 63 == 1


def chain_claims(v, name):
    k = v.k
    a, f, pred = v.d[0]
    last = len(a) - 1
    kept = [c for c in v.ch[:v.n]]
    if name == "C8.few":
        assert pred.tolist() == [-1, 0] and v.n == 1
    elif name.startswith("C1"):
        fillers, at = int(name[3:5]), int(name.split("at")[1])
        assert last == at + fillers + 1 and a[at][1] == v.q.js[0][0] and a[last][0] - a[at][0] == a[last][1] - a[at][1]
        assert at in (0, 64 + 17) and all(pred[at + 1:last] == -1) and all(pred[:at + 1] == -1)
        assert pred[last] == (at if fillers == 63 else -1) and last - at == (64 if fillers == 63 else 65) and f[last] == (2 * k if fillers == 63 else k)
    elif name.startswith("C2"):
        g = abs((a[last][0] - a[last - 1][0]) - (a[last][1] - a[last - 1][1]))
        if name.endswith(".at"):
            assert g == v.band and pred[last] == last - 1 and f[last] > k
        else:
            assert g == v.band + 1 and pred[last] == -1 and f[last] == k
        if v.band == cm.MAX_BAND:
            assert last == 40 and f[39] == 40 * k and int(cm.cost(4096, 11)) == 358 and (name.endswith(".over") or f[last] == 93)
            assert a[last][1] == v.rs - k or v.kernel != "chain"       # (j = 4085 under stride 1; the last minimizer otherwise)
    elif name.startswith("C3"):
        d_p, d_q = a[1][0] - a[0][0], a[1][1] - a[0][1]
        score = k + min(d_p, d_q, k) - int(cm.cost(abs(d_p - d_q), k))
        assert last == 1 and d_p > 0 and d_q > 0 and abs(d_p - d_q) <= v.band
        assert (score, int(pred[1]), int(f[1]), v.n) == ((k, -1, k, 2) if name == "C3.k" else (k + 1, 0, k + 1, 1))
    elif name.startswith("C4"):
        apart = int(name[3:])
        assert pred[last] == last - 1 and all(pred[:last] == -1) and a[last - 1][1] == a[last - 1 - apart][1] and last - 1 - apart == 0
        assert cm.tied(a, f, pred, k, v.band) == 1
    elif name == "C5.tie":
        _, _, ends = cm.trees(f, pred)
        assert pred.tolist() == [-1, 0, 0] and f[1] == f[2] == 2 * k and ends == {0: 1} and int(kept[0]["ref_span"]) == a[1][0] + k - a[0][0]
    elif name == "C5.tail":
        _, _, ends = cm.trees(f, pred)
        assert pred.tolist() == [-1, 0, 1] and k < f[2] < f[1] and ends == {0: 1} and int(kept[0]["n_anchors"]) == 2
    elif name.startswith("C6"):
        assert last == 1 and pred.tolist() == [-1, -1]
        d_p, d_q = a[1][0] - a[0][0], a[1][1] - a[0][1]
        assert {"C6.p": d_p == 0 and 0 < d_q, "C6.j": d_q == 0 and 0 < d_p <= v.band, "C6.far": d_p > BIT31 and d_q > 0}[name]
    elif name.startswith("C7"):
        mv = v.P["min_votes"]
        _, depth, ends = cm.trees(f, pred)
        assert sorted(int(depth[e]) for e in ends.values()) == [mv - 1, mv] and v.n == 1 and int(kept[0]["n_anchors"]) == mv
    elif name == "C8":
        found = []
        for s in (0, 1):
            a_s, f_s, p_s = v.d[s]
            found += [(-c[0], s, c[2], c[3]) for c in cm.chains(a_s, f_s, p_s, k, 1)]
        assert sum(1 for c in found if c[1] == 0) > 16 and sum(1 for c in found if c[1] == 1) > 16
        want = sorted(found)[:v.K]
        assert v.n == v.K and want[0][:2] == (-2 * k, 1) and all(w[0] == -k for w in want[1:])
        assert [(-int(c["score"]), s, t + int(c["q_lo"]) + 8, int(c["q_lo"])) for c, s, t in zip(kept, v.strand, v.start)] == want
        if v.K >= 3:
            assert want[1][1:3] == want[2][1:3] and want[1][3] < want[2][3]         # equal (score, strand, p_lo): q_lo decides
        p_seed_order = [p for p, _ in sorted(v.d[0][0], key=lambda x: x[1])]
        assert p_seed_order != sorted(p_seed_order)
    elif name.startswith("C9"):
        s = int(name == "C9.s1")
        a, f, pred = v.d[s]
        lo = a[0][0] - a[0][1] - v.P["flank"]
        hi = a[1][0] + k + (v.q.L - a[1][1] - k) + v.P["flank"]
        assert v.n == 1 and pred.tolist() == [-1, 0] and int(v.req["text_len"][0]) == v.rs and hi - max(lo, 0) > v.rs and v.strand[0] == s
        if name == "C9.lo":
            assert lo < 0 and v.start[0] == 0
        elif name == "C9.hi":
            assert hi > d.REF_LEN and int(kept[0]["q_hi"]) == v.q.L == v.rs and v.start[0] & BIT31 and a[1][0] + k == d.REF_LEN
        else:
            assert v.start[0] & BIT31 and int(v.tpos[0]) >> 63 == 1 and int(kept[0]["ref_span"]) == a[1][0] + k - a[0][0]


def e4_claims(v):
    b, k = v.b, v.k
    bucket, pos = b["raw"]
    cap = d.E4_REF_LEN - k + 1
    info = b["info"]
    assert v.P["ref_len"] == d.E4_REF_LEN and int(bucket.max()) <= d.E4_POS_ALLOC == len(b["dev_pos"]) and len(bucket) == 4 ** k + 1
    assert (b["dev_pos"][:len(pos)] == pos).all() and (b["dev_pos"][len(pos):] == 0xEEEEEEEE).all() and len(pos) < cap
    affected = set(d.e4_affected(bucket).tolist())
    cb, cpos = b["clean"]
    with_run = {c for c in info["looked"] if cb[c + 1] > cb[c]}
    c_a = info["c_a"]
    assert affected & with_run == {c_a} | set(info["last"]) and len(with_run - affected) > 20
    assert bucket[c_a + 1] < bucket[c_a]                                                       # kind (a)
    b0, b1 = (bucket[info["last"]].astype(np.int64), bucket[np.array(info["last"]) + 1].astype(np.int64))
    assert (b1 > cap).all() and b0[0] <= cap and (b1 - b0 <= v.P["max_occ"]).all() and (b0[1:] > cap).all()   # kind (b): only the capacity check sees them
    # the code behind the lowered entry: looked up, not affected, a wrong run inside the array
    nxt = c_a + 1
    assert nxt in with_run and nxt not in affected and 0 <= bucket[nxt] < bucket[nxt + 1] <= cap
    wrong = pos[bucket[nxt]:bucket[nxt + 1]].tolist()
    assert wrong != cpos[cb[nxt]:cb[nxt + 1]].tolist() and len(wrong) == 1 + 3 + 2 <= v.P["max_occ"]
    # the expectation: the clean index without the affected codes, and with that one wrong run
    occ = {int(c): cpos[cb[c]:cb[c + 1]].tolist() for c in np.nonzero(cb[1:] != cb[:-1])[0] if int(c) not in affected}
    occ[nxt] = wrong
    want = d.index_from(k, occ)
    assert (want[0] == b["index"][0]).all() and (want[1] == b["index"][1]).all()
    assert sum(v.n_hits) == sum(len(occ[c]) for c in v.q.looked_up() if c in occ) > 40 and v.flags == 0 and v.n >= 1


@pytest.mark.parametrize("name,kernel,H", RUNS, ids=["%s-%s-H%d" % r for r in RUNS])
def test_scenarios_are_what_they_claim(name, kernel, H):
    params, scen = d.TABLE[name]
    b = d.batch(name, d.MODE[kernel], H)
    assert [sc["name"] for sc, _ in b["scen"]] == [sc["name"] for sc in scen] and len(b["rl"]) == len(scen) and (b["rl"] == params["read_size"]).all()
    # INDEX: bucket is a prefix sum that ends at len(pos), runs ascend (E4's model index holds one run in the raw array's order)
    bucket, pos = b["index"]
    assert len(bucket) == 4 ** params["k"] + 1 and bucket[0] == 0 and (np.diff(bucket.astype(np.int64)) >= 0).all() and bucket[-1] == len(pos)
    if name != "e4":
        inside = np.ones(len(pos), dtype=bool)
        inside[bucket[1:-1][bucket[1:-1] < len(pos)]] = False
        assert (np.diff(pos.astype(np.int64))[inside[1:]] >= 0).all() and (pos.astype(np.int64) <= params["ref_len"] - params["k"]).all()
        assert b["raw"] is b["index"]
    for q in b["queries"]:                  # distinct_read: the codes of both strands are pairwise distinct
        codes = np.concatenate(q.code)
        assert (codes >= 0).all() and len(set(codes.tolist())) == len(codes) == 2 * (params["read_size"] - params["k"] + 1)
    Ks = params["K"] if isinstance(params["K"], tuple) else (params["K"],)
    for K in Ks:
        detail = []
        out = d.model(kernel, b, K, H, detail=detail)
        assert out[0].tobytes() == d.expected(name, kernel, H, K)[0].tobytes()
        for sc, r in b["scen"]:
            v = View(name, kernel, H, K, r, out, detail)
            if name == "e4":
                e4_claims(v)
                continue
            hits_claims(v, sc["name"])
            if kernel in d.VOTING:
                vote_claims(v, sc["name"])
            else:
                chain_claims(v, sc["name"])
            if sc["high"]:
                assert any(p >= BIT31 for p in kept_positions(v)), sc["name"]
            # the empty slots of rule 7
            assert not v.req["text_len"][v.n:].any() and not v.tpos[v.n:].any() and not v.votes[v.n:].any()


def test_every_scenario_of_the_issue_is_in_the_table():
    names = {sc["name"].split(".")[0] for _, scen in d.TABLE.values() for sc in scen}
    assert names == {"H1", "H2", "H3", "H4", "H5", "V1", "V2", "V3", "V4", "V5", "V6", "C1", "C2", "C3", "C4", "C5", "C6", "C7", "C8", "C9", "E4"}
    assert {k for p, _ in d.TABLE.values() for k in p["kernels"]} == set(d.KERNELS)
    assert all(p["ref_len"] == d.REF_LEN for n, (p, _) in d.TABLE.items() if n != "e4")
    assert d.TABLE["a2048"][0]["H"] == (2048,) and d.TABLE["c2long"][0]["read_size"] == 65528 and d.K_LIST == (1, 2, 3, 5, 7, 9, 10, 11, 15, 16)


# ---- mutants: the obvious off-by-one in a copy of a model changes the expected bytes of the scenario on that edge ----------------------
def mutated(module, old, new, **deps):
    """A copy of a model module with `old` replaced by `new` in its source, once; deps: modules its imports resolve to."""
    src = open(module.__file__).read()
    assert src.count(old) == 1, old
    mod = types.ModuleType(module.__name__ + "_mutant")
    mod.__file__ = module.__file__
    saved = {n: sys.modules.get(n) for n in deps}
    sys.modules.update(deps)
    try:
        exec(compile(src.replace(old, new), module.__file__, "exec"), mod.__dict__)
    finally:
        for n, x in saved.items():
            sys.modules[n] = x
    return mod


INT32 = "((a - out[-1][2] + 2 ** 31) % 2 ** 32 - 2 ** 31) <= band"
MUTANTS = [
    # (id, model, old, new, batch, kernel, scenario, K)
    ("hit-cap", m, "return keys[:MAX_HITS], len(keys) > MAX_HITS", "return keys[:MAX_HITS - 1], len(keys) > MAX_HITS - 1", "a", "cand", "H1.cap.s0", 4),
    ("hit-cap-late", m, "return keys[:MAX_HITS], len(keys) > MAX_HITS", "return keys[:MAX_HITS + 1], len(keys) > MAX_HITS + 1", "a", "cand", "H1.cap+1.s1", 4),
    ("max-occ", m, "hi - lo > max_occ", "hi - lo >= max_occ", "c", "cand", "H3.occ16", 4),
    ("max-occ-late", m, "hi - lo > max_occ", "hi - lo > max_occ + 1", "b", "cand", "H3.occ1", 4),
    ("band-rule-4", m, "a - out[-1][2] <= band", "a - out[-1][2] < band", "a", "cand", "V1.band8.at", 4),
    ("band-rule-4-late", m, "a - out[-1][2] <= band", "a - out[-1][2] <= band + 1", "b", "cand", "V1.band0.over", 4),
    ("key-difference-int32", m, "a - out[-1][2] <= band", INT32, "a", "cand", "V2.band8", 4),
    ("min-votes", m, "if v >= min_votes", "if v > min_votes", "c", "cand", "V4.min5", 4),
    ("strand-tie-break", m, "cl.sort(key=lambda c: (-c[0], c[1], c[2]))", "cl.sort(key=lambda c: (-c[0], -c[1], c[2]))", "v5", "cand", "V5", 5),
    ("lookback-63", cm, "LOOKBACK = 64", "LOOKBACK = 63", "c1", "chain", "C1.63.at81", 4),
    ("lookback-65", cm, "LOOKBACK = 64", "LOOKBACK = 65", "c1", "chain", "C1.64.at0", 4),
    ("g-band", cm, "(g <= band)", "(g < band)", "c2", "chain", "C2.band4096.at", 4),
    ("g-band-late", cm, "(g <= band)", "(g <= band + 1)", "a", "chain", "C2.band8.over", 4),
    ("root-at-k", cm, "take = live & (best > k)", "take = live & (best >= k)", "f", "chain", "C3.k", 4),
    ("nearest", cm, "nearest = LOOKBACK - 1 - np.argmax(score[:, ::-1], axis=1)", "nearest = np.argmax(score, axis=1)", "c1", "chain", "C4.63", 4),
    ("end-on-a-tie", cm, "if t not in ends or f[i] > f[ends[t]]", "if t not in ends or f[i] >= f[ends[t]]", "a", "chain", "C5.tie", 4),
    ("chain-strand-tie-break", cm, "found.sort(key=lambda c: (-c[0], c[1], c[3], c[4]))", "found.sort(key=lambda c: (-c[0], -c[1], c[3], c[4]))", "c8", "chain", "C8", 5),
    ("q-lo-tie-break", cm, "found.sort(key=lambda c: (-c[0], c[1], c[3], c[4]))", "found.sort(key=lambda c: (-c[0], c[1], c[3], -c[4]))", "c8", "chain", "C8", 2),
]


@pytest.mark.parametrize("case", MUTANTS, ids=[c[0] for c in MUTANTS])
def test_an_off_by_one_changes_the_expected_bytes(case):
    _, module, old, new, name, kernel, scenario, K = case
    b = d.batch(name, d.MODE[kernel])
    r = [sc["name"] for sc, _ in b["scen"]].index(scenario)
    deps = dict(seed_model=m, minimizer_model=mm)
    mods = {module.__name__: mutated(module, old, new, **deps)}
    want, got = d.model(kernel, b, K), d.model(kernel, b, K, mods=mods)
    differs = [x.tobytes() != y.tobytes() for x, y in zip(want, got)]
    own = [slice(r, r + 1) if i == 3 else slice(r * K, (r + 1) * K) for i in range(len(want))]       # (the aim_seed_t rows are one per read)
    mine = [x[sl].tobytes() != y[sl].tobytes() for x, y, sl in zip(want, got, own)]
    assert any(differs) and any(mine), (scenario, differs)
