#!/usr/bin/env python3
"""Generate tests/golden/pipeline_refusals.json: what the read-mapping pipeline's entry points and the host-side helpers answer
to arguments they refuse -- the return code and the bytes of aim_last_error().

Every row is [entry point, what is violated, arguments, rc, error text]. There is one row per violated condition and one per pair
of conditions that follow each other in the entry point's order of checks ("a+b": a is checked first, so a is what must be
reported). Only refusals that come before the device probe are recorded, so the table is the same with and without a device;
valid calls and empty batches are left out.

Arguments are JSON values: a number is passed as it is, null is a NULL pointer, and a list names a pointer:
    ["dev", address]       a made-up device address (a refused call never dereferences it)
    ["zeros", bytes]       a zeroed host buffer
    ["bytes", text]        a host buffer holding the text
    ["u32", [values]]      a host array of uint32_t
    ["rows", size, [text]] host rows of `size` bytes, each holding one text, zero-padded
    ["req", [[pattern_len, text_len]]] / ["req8", ...]   host aim_request_t / aim_request8_t records
    ["params" | "seed" | "extend", {field: value}]      an aim_params_t / aim_seed_params_t / aim_extend_params_t

Needs only the built library (no device). tests/test_pipeline_refusals_cpu.py replays the table and compares both fields exactly:
a refactor of these entry points must leave every row as it is. Regenerate only when a refusal is meant to change (AIM_LIB
selects the library):
    python tests/golden/make_pipeline_refusals.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "pipeline_refusals.json")

MAX_REF = 0xFE000000          # AIM_SEED_MAX_REF_LEN
MANY = 1 << 28                # n_reads with n_reads * 16 = 2^32
FLAG_REQ8 = 8                 # AIM_FLAG_REQ8


def dev(i, align=256):
    return ["dev", 0x10000 * (i + 1) // align * align]


D = [dev(i) for i in range(16)]
SEED = dict(k=11, stride=1, max_occ=8, band=16, flank=8, min_votes=1, max_cands=4, read_size=128, idx_base=0, options=0)
MINI = 5 << 8                 # AIM_SEED_OPT_MINIMIZERS(5)
EXT = dict(match=1, mismatch=4, gap_o=6, gap_e=2, xdrop=20, max_cost=100, band=8, max_ext=64)


def _with(base, **kw):
    return dict(base, **kw)


def _variants(conds):
    """[(note, {name: value})] from [(note, overrides)]: every condition alone, then every adjacent pair that can be violated together."""
    out = [(n, o) for n, o in conds]
    for (n0, o0), (n1, o1) in zip(conds, conds[1:]):
        if any(k in o0 and o0[k] != o1[k] for k in o1):
            continue
        out.append((n0 + "+" + n1, dict(o0, **o1)))
    return out


def index_cases():
    out = []
    k_ref = [("k below", dict(k=7)), ("k above", dict(k=15)), ("ref_len", dict(ref_len=MAX_REF + 1))]
    for note, o in _variants(k_ref + [("NULL bucket_entries", dict(a=None))]) + [("NULL pos_capacity", dict(b=None))]:
        a = _with(dict(k=11, ref_len=1000, a=["zeros", 8], b=["zeros", 8]), **o)
        out.append(("aim_index_sizes", note, [a["k"], a["ref_len"], a["a"], a["b"]]))
    for note, o in _variants(k_ref + [("NULL scratch_bytes", dict(a=None))]):
        a = _with(dict(k=11, ref_len=1000, a=["zeros", 8]), **o)
        out.append(("aim_index_device_scratch", note, [a["k"], a["ref_len"], a["a"]]))
    base = dict(seq=["bytes", "ACGT" * 8], ref_len=32, k=11, w=5, bucket=["zeros", 8], pos=["zeros", 8], n_pos=["zeros", 8])
    nulls = [("NULL bucket", dict(bucket=None)), ("NULL seq", dict(seq=None)), ("NULL pos", dict(pos=None))]
    for note, o in _variants(k_ref + nulls[:1]) + nulls[1:]:
        a = _with(base, **o)
        out.append(("aim_index_build", note, [a["seq"], a["ref_len"], a["k"], a["bucket"], a["pos"], a["n_pos"], 2]))
    wins = [("w below", dict(w=0)), ("w above", dict(w=33))]
    for note, o in _variants(k_ref + wins[:1] + nulls[:1]) + wins[1:] + nulls[1:]:
        a = _with(base, **o)
        out.append(("aim_index_build_minimizers", note, [a["seq"], a["ref_len"], a["k"], a["w"], a["bucket"], a["pos"], a["n_pos"], 2]))
    # the device builds: the index arguments, then the pointers in the order they are looked at (ref_len 1000 >= k: all are needed)
    base = dict(ref=D[0], ref_len=1000, k=11, w=5, bucket=D[1], pos=D[2], scratch=D[3], bytes=1 << 40)
    ptrs = [("NULL d_bucket", dict(bucket=None)), ("NULL d_reference", dict(ref=None)), ("d_reference alignment", dict(ref=["dev", 0x10008])),
            ("NULL d_pos", dict(pos=None)), ("NULL d_scratch", dict(scratch=None)), ("d_scratch alignment", dict(scratch=["dev", 0x40010])),
            ("scratch_bytes", dict(bytes=0))]
    for note, o in _variants(k_ref + ptrs):
        a = _with(base, **o)
        out.append(("aim_index_build_device", note, [a["ref"], a["ref_len"], a["k"], a["bucket"], a["pos"], a["scratch"], a["bytes"], None]))
    for note, o in _variants(wins[:1] + k_ref + ptrs) + wins[1:]:
        a = _with(base, **o)
        out.append(("aim_index_build_device_minimizers", note,
                    [a["ref"], a["ref_len"], a["k"], a["w"], a["bucket"], a["pos"], a["scratch"], a["bytes"], None]))
    return out


def seed_cases():
    out = []
    for K, note in ((0, "K below"), (17, "K above")):
        out.append(("aim_seed_groups_offsets", note, [10, K, ["zeros", 64]]))
    out.append(("aim_seed_groups_offsets", "NULL read_offsets", [10, 4, None]))
    out.append(("aim_seed_groups_offsets", "n_reads * K", [MANY, 16, ["zeros", 64]]))
    out.append(("aim_seed_groups_offsets", "K above+NULL read_offsets", [10, 17, None]))
    out.append(("aim_seed_groups_offsets", "NULL read_offsets+n_reads * K", [MANY, 16, None]))

    fields = [("k below", dict(k=7)), ("k above", dict(k=15)), ("stride", dict(stride=0)), ("max_occ", dict(max_occ=0)), ("band", dict(band=-1)),
              ("flank", dict(flank=-1)), ("min_votes", dict(min_votes=0)), ("max_cands below", dict(max_cands=0)),
              ("max_cands above", dict(max_cands=17))]
    opts = [("options low byte", dict(options=MINI | 1)), ("options w above", dict(options=33 << 8)),
            ("stride with minimizers", dict(options=MINI, stride=2))]
    tail = [("ref_len", dict(ref_len=MAX_REF + 1)), ("n_reads * max_cands", dict(n_reads=MANY, max_cands=16)), ("null buffer", dict(read_len=None))]
    ptr_names = ("read_len", "reads", "bucket", "pos", "requests", "text_pos", "votes", "seed")

    def call(fn, o, long_hits=None):
        a = _with(dict(n_reads=10, ref_len=1000, chains=D[8], **{n: D[i] for i, n in enumerate(ptr_names)}), **{k: v for k, v in o.items() if k not in SEED})
        sp = None if o.get("sp_null") else ["seed", _with(SEED, **{k: v for k, v in o.items() if k in SEED})]
        args = [sp] + ([o.get("max_hits", long_hits)] if long_hits else []) + \
               [a["n_reads"], a["read_len"], a["reads"], a["bucket"], a["pos"], a["ref_len"], a["requests"], a["text_pos"], a["votes"], a["seed"]]
        if fn != "aim_seed_device":
            args.append(a["chains"])
        return args + [None]

    for fn in ("aim_seed_device", "aim_seed_chain_device"):
        chain = fn == "aim_seed_chain_device"
        sizes = [("read_size zero", dict(read_size=0)), ("read_size odd", dict(read_size=100)), ("read_size above", dict(read_size=4104))]
        conds = fields + sizes[:1] + opts + ([("band above", dict(band=4097))] if chain else []) + tail
        extra = sizes[1:] + [("null " + n, {n: None}) for n in ptr_names[1:]]
        for note, o in [("NULL sp", dict(sp_null=True))] + _variants(conds) + extra:
            out.append((fn, note, call(fn, o)))
        # (both name options, with different values: _variants leaves the pair out)
        out.append((fn, "options w above+stride with minimizers", call(fn, dict(options=33 << 8, stride=2))))
    fn = "aim_seed_chain_long_device"
    sizes = [("read_size zero", dict(read_size=0)), ("read_size odd", dict(read_size=100)), ("read_size above", dict(read_size=65536))]
    long_base = dict(options=MINI)
    conds = fields + sizes[:1] + [("options zero", dict(options=0)), ("band above", dict(band=4097)), ("max_hits below", dict(max_hits=512))] + tail
    extra = sizes[1:] + opts + [("max_hits above", dict(max_hits=16384)), ("max_hits no power of two", dict(max_hits=3000))] + \
        [("null " + n, {n: None}) for n in ptr_names[1:]]
    for note, o in [("NULL sp", dict(sp_null=True))] + _variants(conds) + extra:
        out.append((fn, note, call(fn, _with(long_base, **o), 2048)))
    out.append((fn, "stride with minimizers+band above", call(fn, dict(options=MINI, stride=2, band=4097), 2048)))
    return out


def segment_cases():
    out = []
    K = [("K below", dict(K=0)), ("K above", dict(K=17))]
    rs = [("read_size zero", dict(read_size=0)), ("read_size odd", dict(read_size=100)), ("read_size above", dict(read_size=65536))]
    nk = ("n_reads * K", dict(n_reads=MANY, K=16))
    ref = ("ref_len", dict(ref_len=MAX_REF + 1))

    def run(fn, conds, extra, order, base, nullable):
        for note, o in _variants(conds + [("null buffer", {nullable[0]: None})]) + extra + [("null " + n, {n: None}) for n in nullable[1:]]:
            a = _with(base, **o)
            out.append((fn, note, [a[n] for n in order] + [None]))

    base = dict(K=4, read_size=128, mask_q8=128, n_reads=10, read_len=D[0], text_pos=D[1], seed=D[2], chains=D[3], cls=D[4])
    run("aim_chain_classify_device", K[1:] + [("mask_q8 zero", dict(mask_q8=0)), rs[0], nk], K[:1] + [("mask_q8 above", dict(mask_q8=257))] + rs[1:],
        ("K", "read_size", "mask_q8", "n_reads", "read_len", "text_pos", "seed", "chains", "cls"), base, ("read_len", "text_pos", "seed", "chains", "cls"))
    base = dict(K=4, n_reads=10, score_unit=2, best=D[0], mates=None, cls=D[2], mapq=D[3])
    run("aim_read_mapq_device", K[1:] + [nk, ("score_unit", dict(score_unit=0)), ("odd n_reads with mates", dict(n_reads=11, mates=D[1]))], K[:1],
        ("K", "n_reads", "score_unit", "best", "mates", "cls", "mapq"), base, ("best", "cls", "mapq"))
    out.append(("aim_read_mapq_device", "K above+n_reads * K", [17, MANY, 2, D[0], None, D[2], D[3], None]))
    base = dict(K=4, read_size=128, flank=8, ref_len=1000, n_reads=10, **{"p%d" % i: D[i] for i in range(11)})
    ptrs = tuple("p%d" % i for i in range(11))
    run("aim_split_segments_device", K[1:] + [rs[0], nk, ("flank", dict(flank=-1)), ref], K[:1] + rs[1:],
        ("K", "read_size", "flank", "ref_len", "n_reads") + ptrs, base, ptrs)

    ext = [("match", dict(match=0)), ("mismatch", dict(mismatch=0)), ("gap_o", dict(gap_o=-1)), ("gap_e", dict(gap_e=0)), ("xdrop", dict(xdrop=-1)),
           ("max_cost below", dict(max_cost=0)), ("band below", dict(band=0)), ("max_ext below", dict(max_ext=7)),
           ("unit", dict(match=20, mismatch=20))]
    more = [("max_cost above", dict(max_cost=4096)), ("band above", dict(band=32)), ("max_ext above", dict(max_ext=1025)),
            ("unit by gaps", dict(gap_o=30, gap_e=10)), ("NULL parameters", dict(p_null=True)), ("n_reads * K+NULL parameters", dict(n_reads=MANY, K=16, p_null=True))]
    ptrs = tuple("p%d" % i for i in range(8))
    base = dict(K=4, read_size=128, ref_len=1000, n_reads=10, **{p: D[i] for i, p in enumerate(ptrs)})
    conds = K[1:] + [rs[0], nk] + ext + [ref, ("null buffer", dict(p0=None))]
    for note, o in _variants(conds) + K[:1] + rs[1:] + more + [("null " + n, {n: None}) for n in ptrs[1:]]:
        a = _with(base, **{k: v for k, v in o.items() if k not in EXT and k != "p_null"})
        p = None if o.get("p_null") else ["extend", _with(EXT, **{k: v for k, v in o.items() if k in EXT})]
        out.append(("aim_extend_segments_device", note, [p, a["K"], a["read_size"], a["ref_len"], a["n_reads"]] + [a[n] for n in ptrs] + [None]))
    return out


def host_cases():
    out = []
    o4, o8 = ["zeros", 8], ["zeros", 8]
    for note, args in (("NULL max_score", [0, 100, 0.02, 4, 6, 2, 4, None, o4]), ("NULL read_size", [0, 100, 0.02, 4, 6, 2, 4, o4, None]),
                       ("read_length zero", [0, 0, 0.02, 4, 6, 2, 4, o4, o8]), ("read_length negative", [1, -5, 0.02, 4, 6, 2, 4, o4, o8])):
        out.append(("aim_launcher_sizes", note, args))
    ops, buf = ["bytes", "MMMMIMMMDMMM"], ["zeros", 64]
    for note, args in (("NULL ops", [None, 0, 12, buf, 64]), ("NULL out", [ops, 0, 12, None, 64]), ("cap below 4", [ops, 0, 12, buf, 3]),
                       ("begin_offset negative", [ops, -1, 12, buf, 64]), ("too small inside", [["bytes", "MIMIMIMI"], 0, 8, buf, 4]),
                       ("too small at the end", [["bytes", "M" * 12], 0, 12, buf, 4]), ("cap below 4+too small", [["bytes", "MIMIMIMI"], 0, 8, buf, 3])):
        out.append(("aim_cigar_format", note, args))
    runs = ["u32", [(4 << 8) | 77, (1 << 8) | 73, (3 << 8) | 77]]
    alt = ["u32", [(1 << 8) | 77, (1 << 8) | 73, (1 << 8) | 77, (1 << 8) | 73]]
    for note, args in (("NULL runs", [None, 3, buf, 64]), ("NULL out", [runs, 3, None, 64]), ("cap below 4", [runs, 3, buf, 3]), ("no runs", [runs, 0, buf, 64]),
                       ("too small inside", [alt, 4, buf, 4]), ("too small at the end", [["u32", [(123 << 8) | 77]], 1, buf, 4]),
                       ("cap below 4+too small", [alt, 4, buf, 3])):
        out.append(("aim_cigar_format_runs", note, args))
    words = ["u32", [(100 << 4) | 0, (3 << 4) | 1]]
    for note, args in (("NULL out", [words, 2, None, 64]), ("cap below 2", [words, 2, buf, 1]), ("NULL words", [None, 2, buf, 64]),
                       ("unknown op", [["u32", [(5 << 4) | 7, (5 << 4) | 9]], 2, buf, 64]), ("too small", [words, 2, buf, 5]),
                       ("cap below 2+unknown op", [["u32", [(5 << 4) | 9]], 1, buf, 1]), ("unknown op+too small", [["u32", [(5 << 4) | 9]], 1, buf, 2])):
        out.append(("aim_sam_format_cigar", note, args))
    seq = ["bytes", "ACGTACGTAC"]
    for note, args in (("NULL seq", [None, 10, 16, buf]), ("NULL row", [seq, 10, 16, None]), ("len negative", [seq, -1, 16, buf]),
                       ("len above read_size", [seq, 10, 8, buf])):
        out.append(("aim_pack_sequence", note, args))
    big = ["zeros", 4096]
    for note, args in (("NULL requests", [1, 0, 2, 20, 0.1, 32, None, big, big]), ("NULL patterns", [1, 0, 2, 20, 0.1, 32, big, None, big]),
                       ("NULL texts", [1, 0, 2, 20, 0.1, 32, big, big, None]), ("len zero", [1, 0, 2, 0, 0.1, 32, big, big, big]),
                       ("read_size zero", [1, 0, 2, 20, 0.1, 0, big, big, big]), ("read_size too small", [1, 0, 2, 20, 0.1, 21, big, big, big]),
                       ("NULL patterns+read_size too small", [1, 0, 2, 20, 0.1, 21, big, None, big])):
        out.append(("aim_gen_pairs", note, args))

    def pack(params=None, n_pairs=2, req=(["req", [[4, 4], [4, 4]]]), pat=(["rows", 8, ["ACGT", "ACGT"]]), txt=(["rows", 8, ["ACGT", "ACGT"]]),
             pp=big, pt=big, max_raw=0, n_raw=o4, null_params=False, rs=8, flags=0):
        p = None if null_params else ["params", dict(algo=0, mismatch=4, gap_o=6, gap_e=2, max_score=5, read_size=rs, flags=flags)]
        return [p, n_pairs, req, pat, txt, pp, pt, big, big, big, max_raw, n_raw, 2]
    bad_len, raw = ["req", [[4, 4], [4, 9]]], ["rows", 8, ["ACNT", "ACGT"]]
    for note, args in (("NULL params", pack(null_params=True)), ("NULL n_raw", pack(n_raw=None)), ("NULL requests", pack(req=None)),
                       ("NULL patterns", pack(pat=None)), ("NULL packed_patterns", pack(pp=None)), ("NULL texts", pack(txt=None)),
                       ("NULL packed_texts", pack(pt=None)), ("read_size zero", pack(rs=0)), ("read_size odd", pack(rs=12)),
                       ("length above read_size", pack(req=bad_len)), ("length negative", pack(req=["req", [[-1, 4], [4, 4]]])),
                       ("length above read_size, 8-byte requests", pack(req=["req8", [[4, 4], [9, 4]]], flags=FLAG_REQ8)),
                       ("raw pairs above max_raw", pack(pat=raw)), ("NULL n_raw+read_size odd", pack(n_raw=None, rs=12)),
                       ("read_size odd+length above read_size", pack(rs=12, req=["req", [[4, 4], [4, 13]]])),
                       ("length above read_size+raw pairs above max_raw", pack(req=bad_len, pat=raw))):
        out.append(("aim_pack_batch", note, args))
    return out


def cases():
    return index_cases() + seed_cases() + segment_cases() + host_cases()


def _struct(cls, fields):
    s = cls()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def marshal(capi, arg, keep):
    """The ctypes value of one recorded argument; `keep` holds the buffers alive until the call returns."""
    import numpy as np
    if not isinstance(arg, list):
        return arg
    kind = arg[0]
    if kind == "dev":
        return C.c_void_p(arg[1])
    if kind in ("params", "seed", "extend"):
        s = _struct({"params": capi.Params, "seed": capi.SeedParams, "extend": capi.ExtendParams}[kind], arg[1])
        keep.append(s)
        return C.byref(s)
    if kind == "zeros":
        a = np.zeros(arg[1], np.uint8)
    elif kind == "bytes":
        a = np.frombuffer(arg[1].encode() + b"\0", np.uint8).copy()
    elif kind == "u32":
        a = np.array(arg[1], np.uint32)
    elif kind == "rows":
        a = np.zeros((len(arg[2]), arg[1]), np.uint8)
        for i, t in enumerate(arg[2]):
            a[i, :len(t)] = np.frombuffer(t.encode(), np.uint8)
    elif kind in ("req", "req8"):
        a = np.zeros(len(arg[1]), capi.REQUEST_DTYPE if kind == "req" else capi.REQUEST8_DTYPE)
        a["pattern_len"], a["text_len"] = [r[0] for r in arg[1]], [r[1] for r in arg[1]]
    else:
        raise ValueError(kind)
    keep.append(a)
    return C.cast(a.ctypes.data, C.c_void_p)


def run(lib, capi, fn, args):
    """(rc, error text) of one call. aim_last_error() is first set to another entry point's message, so that a refusal that did not
    reach it shows."""
    assert lib.aim_device_count(None) == capi.AIM_EINVAL and lib.aim_last_error() == b"count is NULL"
    keep = []
    f = getattr(lib, fn)
    vals = [marshal(capi, a, keep) for a in args]
    rc = f(*[C.cast(v, t) if isinstance(v, C.c_void_p) and t is not C.c_void_p else v for v, t in zip(vals, f.argtypes)])
    return int(rc), lib.aim_last_error().decode()


def main():
    sys.path.insert(0, ROOT)
    from aim_amd import capi
    lib = capi.load()
    rows = []
    for fn, note, args in cases():
        rc, err = run(lib, capi, fn, args)
        if rc >= 0 or rc == capi.AIM_ENODEV:
            raise SystemExit("%s (%s) was not refused before the device probe: rc %d, %s" % (fn, note, rc, err))
        rows.append([fn, note, args, rc, err])
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print("wrote %s: %d refusals of %d entry points" % (OUT, len(rows), len({r[0] for r in rows})))


if __name__ == "__main__":
    main()
