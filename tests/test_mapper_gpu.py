"""The mapper on the GPU. aim_map_records_device on synthetic slot tables against rule 12c's numpy model, every output byte, for each K
and batch size below, on a small and a large grid and under the poison knobs, and the tables of K = 3 padded with empty slots to every
group width against themselves (tests/slot_padding.py); aim_mapper_t end to end on the shared batch
(tests/mapper_batch.py: chimeric, unbroken and random reads) against the same stages driven by hand through the engine helpers plus the
record model, with and without the segment extension; two slots, a reused slot, an empty batch and capacities set too small; and
python -m aim_amd.map against samout over the mapper's own records."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
from gpu_buffers import Hip  # noqa: E402
from hand_stages import single_end as hand_path  # noqa: E402
from mapper_batch import map_alone  # noqa: E402

KS = (1, 2, 3, 4, 6, 7, 8, 9, 15, 16)  # the three group widths full (4, 8, 16), one lane short, just past the width before, and 2
N_READS = (1, 65, 2100)             # one group, across a wavefront, and 2 101 scan entries: three scan parts of 1 024
GUARD = 64


def tables(K, n):
    import map_records_model as mm
    return mm.synthetic_tables(11, K, n)


def run_map_records(h, K, n, seg, sam, cls):
    """aim_map_records_device over uploaded tables; d_rec_offsets, d_records (room for n * K records and a guard) and the scratch are
    prefilled with 0xEE: (rec_offsets, the whole record buffer as bytes)."""
    from aim_amd import engine
    d_off, d_rec = h.filled(4 * (n + 1) + GUARD), h.filled(64 * n * K + GUARD)
    sb = engine.map_records_scratch(n)
    engine.map_records_device(K, n, h.up(seg), h.up(sam), h.up(cls), d_off, d_rec, h.filled(sb), sb)
    return h.down(d_off, 4 * (n + 1) + GUARD), h.down(d_rec, 64 * n * K + GUARD)


def check_against_model(K, n, off_bytes, rec_bytes):
    import map_records_model as mm
    seg, sam, cls = tables(K, n)
    want_off, want = mm.map_records(K, n, seg, sam, cls)
    assert off_bytes[:4 * (n + 1)].tobytes() == want_off.tobytes(), (K, n)
    assert (off_bytes[4 * (n + 1):] == 0xEE).all(), "written past rec_offsets"
    total = int(want_off[n])
    got = rec_bytes[:64 * total].view(mm.RECORD_DTYPE)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint8).reshape(total, 64) != want.view(np.uint8).reshape(total, 64)).any(axis=1))[0]
        raise AssertionError((K, n, "records", bad[:8].tolist(), got[bad[0]], want[bad[0]]))
    assert (rec_bytes[64 * total:] == 0xEE).all(), "written past the records"


@pytest.mark.parametrize("K", KS)
def test_map_records_equal_model(K):
    import map_records_model as mm
    seg, sam, cls = tables(K, 65)
    mapped = mm.mapped_slots(K, 65, seg, sam)
    assert not mapped[0].any() and mapped[1].all() and len(set(seg["q_begin"][K:2 * K].tolist())) == 1 and (sam["status"][3 * K:4 * K] & mm.SAM_OVERFLOW).all()
    assert K == 1 or (not mapped[2, 0] and mapped[2, K - 1])
    with Hip() as h:
        for n in N_READS:
            check_against_model(K, n, *run_map_records(h, K, n, *tables(K, n)))
            h.free()
        from aim_amd import engine                       # an empty batch: rec_offsets[0] = 0 and nothing else
        d_off = h.filled(8)
        engine.map_records_device(K, 0, None, None, None, d_off, None, None, 0)
        assert h.down(d_off, 8).tolist() == [0, 0, 0, 0, 0xEE, 0xEE, 0xEE, 0xEE]


KNOB_CASES = ((4, 2100), (16, 65), (1, 2100), (6, 2100), (9, 65))      # the last two: 8 lanes per read, and 16 that K does not fill


def knob_batch():
    out = {}
    with Hip() as h:
        for i, (K, n) in enumerate(KNOB_CASES):
            out["off_%d" % i], out["rec_%d" % i] = run_map_records(h, K, n, *tables(K, n))
            h.free()
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 (8 workgroups walk the 33 blocks of reads) and 256 and under the three
    AIM_DEBUG_POISON_* knobs; the scan runs over three parts either way."""
    f = str(tmp_path / "k.npz")
    p = child.run("test_mapper_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    grid = 8 if env["AIM_CHIP_CUS"] == "1" else 33
    line = "[aim plan] map_count_kernel grid=%d block=256 lanes=4 reads=2100 K=4; scan parts=3 per_part=1024; map_records_kernel grid=%d block=256"
    assert line % (grid, grid) in p.stderr, p.stderr
    assert "lanes=16 reads=65 K=16; scan parts=1 per_part=1024" in p.stderr, p.stderr
    # the 8-lane path ran, and a 16-lane group of 9: the launcher's own rule, ceil(reads / (256 / lanes)) under the resident grid of
    # 8 workgroups per compute unit
    line = "[aim plan] map_count_kernel grid=%d block=256 lanes=%d reads=%d K=%d; scan parts=%d per_part=1024; map_records_kernel grid=%d block=256"
    for lanes, n, K, parts in ((8, 2100, 6, 3), (16, 65, 9, 1)):
        g = min(8 * int(env["AIM_CHIP_CUS"]), -(-n // (256 // lanes)))
        assert line % (g, lanes, n, K, parts, g) in p.stderr, p.stderr
    out = np.load(f)
    for i, (K, n) in enumerate(KNOB_CASES):
        check_against_model(K, n, out["off_%d" % i], out["rec_%d" % i])


def test_empty_slots_change_nothing():
    """tests/slot_padding.py on the device: the tables of K = 3 with every read padded to 4, 8 and 16 slots -- the same reads in groups
    of 4, 8 and 16 lanes -- give rec_offsets and, `slot` renamed, every record byte of K = 3, which are the model's."""
    import map_records_model as mm
    import slot_padding as sp
    K, n = 3, N_READS[1]
    seg, sam, cls = tables(K, n)
    with Hip() as h:
        off3, rec3 = run_map_records(h, K, n, seg, sam, cls)
        check_against_model(K, n, off3, rec3)
        total = int(off3[:4 * (n + 1)].view(np.uint32)[n])
        assert total > n
        for K2 in (4, 8, 16):
            off, rec = run_map_records(h, K2, n, sp.pad(seg, K, K2, n), sp.pad(sam, K, K2, n), sp.pad(cls, K, K2, n))
            h.free()
            assert off[:4 * (n + 1)].tobytes() == off3[:4 * (n + 1)].tobytes() and (off[4 * (n + 1):] == 0xEE).all(), K2
            assert rec[:64 * total].tobytes() == sp.records_renamed(rec3[:64 * total].view(mm.RECORD_DTYPE), K, K2).tobytes(), K2
            assert (rec[64 * total:] == 0xEE).all(), "written past the records"


# ---- the mapper end to end ---------------------------------------------------------------------------------------------------------
def end_to_end():
    """The shared batch through aim_mapper_t, with and without AIM_MAP_EXTEND, against hand_path: the same records byte for byte apart
    from the two offsets, the same words and MD bytes behind them; two records per chimeric read, one of them supplementary, CIGARs
    that consume the whole read; one record per unbroken read inside its true interval widened by flank + edits; one unmapped record
    per random read."""
    import chain_class_model as ccm
    import mapper_batch as mb
    import split_model as sm
    b = mb.batch()
    ref, rows, rl = b["ref"], b["rows"], b["read_len"]
    flank, K = ccm.CHIMERIC_ROW[5], ccm.CHIMERIC_ROW[7]
    n = len(rl)
    for extend in (False, True):
        got = map_alone(mb.mapper_params(n, extend), ref, rl, rows)
        want = hand_path(extend)
        g, w = mb.canon(got), mb.canon(want)
        assert g[1] == w[1], "rec_offsets"
        assert g[0] == w[0], ("records", np.nonzero(np.frombuffer(g[0], dtype=np.uint8) != np.frombuffer(w[0], dtype=np.uint8))[0][:8] // 64)
        assert g[2] == w[2] and g[3] == w[3], "CIGAR words or MD bytes"
        rec, off = got["records"], got["rec_offsets"]
        assert got["cigar_needed"] == len(got["cigar"]) and got["md_needed"] == len(got["md"]) and not (rec["sam"]["status"] & sm.SAM_OVERFLOW).any()
        counts = np.diff(off.astype(np.int64))
        assert counts[:mb.N_CHIMERIC].tolist() == [2] * mb.N_CHIMERIC and counts[mb.N_CHIMERIC:].tolist() == [1] * (mb.N_UNBROKEN + mb.N_RANDOM)
        words = g[2]
        for r in range(n):
            grp = range(int(off[r]), int(off[r + 1]))
            if r >= mb.N_CHIMERIC + mb.N_UNBROKEN:
                o = rec[grp[0]]
                assert o["sam"]["flags"] == sm.SAM_UNMAPPED and o["sam"]["n_cigar"] == 0 and o["read"] == r and o["slot"] == r * K and o["n_records"] == 1
                continue
            assert sum(int(rec[i]["sam"]["flags"]) & sm.SAM_SUPPLEMENTARY != 0 for i in grp) == len(grp) - 1
            for i in grp:
                o = rec[i]
                assert not int(o["sam"]["flags"]) & sm.SAM_UNMAPPED and o["read"] == r and o["n_records"] == len(grp) and o["mapq"] <= 60
                assert sm.read_consumed(words[i]) == int(rl[r]), (r, words[i])
                pos, span = int(o["sam"]["pos"]), int(o["sam"]["ref_span"])
                if r < mb.N_CHIMERIC:
                    hf = sm.half_of(b["halves"][r], int(o["q_begin"]), int(o["q_end"]))
                    lo, hi, strand, slack = hf["ref_lo"], hf["ref_hi"], hf["strand"], flank + hf["edits"]
                else:
                    lo, hi, strand = b["truth"][r - mb.N_CHIMERIC]
                    slack = flank + mb.UNBROKEN_EDITS
                assert (int(o["sam"]["flags"]) & sm.SAM_REVERSE != 0) == bool(strand) and lo - slack <= pos and pos + span <= hi + slack, (r, o, lo, hi)
        print("extend", extend, "records", len(rec), "words", got["cigar_needed"], "md", got["md_needed"])


def test_end_to_end_equals_the_stages_by_hand():
    p = child.run("test_mapper_gpu", "end_to_end", cuda_first=True, marker="MAPPER_END_TO_END_OK", check=False)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "MAPPER_END_TO_END_OK" in p.stdout, p.stdout + p.stderr


def test_two_slots_reuse_and_empty_batch():
    """Batches A and B submitted back to back on two slots, then waited, equal A and B run alone; a slot used three times returns the
    third batch's result; n_reads = 0 is a batch; a slot in flight refuses a second submit and an idle one a wait."""
    import mapper_batch as mb
    from aim_amd import capi, engine
    b = mb.batch()
    ref, rows, rl = b["ref"], b["rows"], b["read_len"]
    A, B, C3 = slice(0, 40), slice(40, 73), slice(20, 60)
    mp = mb.mapper_params(40, True, slots=2)
    alone = {k: mb.canon(map_alone(mp, ref, rl[s], rows[s])) for k, s in (("A", A), ("B", B), ("C", C3))}
    assert alone["A"] != alone["C"] and alone["B"] != alone["C"]
    with engine.Mapper(mp, ref) as m:
        m.submit(0, rl[A], rows[A])
        m.submit(1, rl[B], rows[B])
        with pytest.raises(capi.AimError) as e:
            m.submit(1, rl[A], rows[A])
        assert e.value.code == capi.AIM_ESTATE and "slot 1 is in flight" in str(e.value)
        assert mb.canon(m.wait(0)) == alone["A"] and mb.canon(m.wait(1)) == alone["B"]
        with pytest.raises(capi.AimError) as e:
            m.wait(1)
        assert e.value.code == capi.AIM_ESTATE
        for s in (B, A, C3):                              # the longer batch first: what it left behind must not show
            m.submit(1, rl[s], rows[s])
            last = mb.canon(m.wait(1))
        assert last == alone["C"]
        m.submit(0, rl[:0], rows[:0])
        out = m.wait(0)
        assert out["n_reads"] == 0 and len(out["records"]) == 0 and out["rec_offsets"].tolist() == [0] and len(out["cigar"]) == 0 and len(out["md"]) == 0
        with pytest.raises(capi.AimError) as e:
            m.submit(0, np.zeros(41, dtype=np.int32), np.zeros((41, 1024), dtype=np.uint8))
        assert "n_reads 41 is above max_reads 40" in str(e.value)
        m.submit(0, rl[A], rows[A])                       # and the slot still works
        assert mb.canon(m.wait(0)) == alone["A"]


def test_capacities_too_small_then_as_needed():
    import mapper_batch as mb
    import split_model as sm
    b = mb.batch()
    ref, rows, rl = b["ref"], b["rows"], b["read_len"]
    n = len(rl)
    full = map_alone(mb.mapper_params(n, True), ref, rl, rows)
    need_c, need_m = full["cigar_needed"], full["md_needed"]
    assert need_c > 64 and need_m > 256
    small = map_alone(mb.mapper_params(n, True, cigar_cap=need_c // 2, md_cap=need_m // 2), ref, rl, rows)
    over = (small["records"]["sam"]["status"] & sm.SAM_OVERFLOW) != 0
    assert (small["cigar_needed"], small["md_needed"]) == (need_c, need_m) and len(small["cigar"]) == need_c // 2 and len(small["md"]) == need_m // 2
    assert over.any() and not over.all() and (small["records"]["sam"]["n_cigar"][over] == 0).all()
    assert small["rec_offsets"].tobytes() == full["rec_offsets"].tobytes()             # an OVERFLOW row still counts as mapped
    s, f = mb.canon(small), mb.canon(full)
    for i in np.nonzero(~over)[0]:
        assert s[2][i] == f[2][i] and s[3][i] == f[3][i]
    exact = map_alone(mb.mapper_params(n, True, cigar_cap=need_c, md_cap=need_m), ref, rl, rows)
    assert not (exact["records"]["sam"]["status"] & sm.SAM_OVERFLOW).any() and mb.canon(exact) == f


def test_command_line_equals_samout_over_the_mappers_records(tmp_path):
    """python -m aim_amd.map in a child process, two batches over its two slots: as many lines as samout writes for the mapper's own
    records of the whole batch, with the same FLAG, POS and CIGAR columns (and the same MAPQ and tags)."""
    import chain_class_model as ccm
    import mapper_batch as mb
    from aim_amd import samout
    b = mb.batch()
    ref, rows, rl = b["ref"], b["rows"], b["read_len"]
    n = len(rl)
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    names = ["read%d" % r for r in range(n)]
    (tmp_path / "ref.fa").write_bytes(b">ref test reference\n" + b"\n".join(ref.tobytes()[i:i + 70] for i in range(0, len(ref), 70)) + b"\n")
    with open(tmp_path / "reads.fq", "wb") as f:
        for r in range(n):
            f.write(b"@%s\n%s\n+\n%s\n" % (names[r].encode(), rows[r, :rl[r]].tobytes(), b"I" * int(rl[r])))
    cmd = [sys.executable, "-m", "aim_amd.map", "--ref", str(tmp_path / "ref.fa"), "--reads", str(tmp_path / "reads.fq"), "-o", str(tmp_path / "out.sam"),
           "--batch", "40", "--read-size", str(ccm.CHIMERIC_SIZE), "-k", str(k), "-w", str(w), "--max-occ", str(max_occ), "--band", str(band), "--flank", str(flank),
           "--min-votes", str(min_votes), "--max-cands", str(K), "--max-score", str(mb.max_score()), "--extend"]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    text = open(tmp_path / "out.sam").read().splitlines()
    head, body = [l for l in text if l.startswith("@")], [l for l in text if not l.startswith("@")]
    assert [l[:3] for l in head] == ["@HD", "@SQ", "@PG"] and head[1] == "@SQ\tSN:ref\tLN:%d" % len(ref)
    # the reference of the test holds lower-case bases and an N run; the command line upper-cases it, so the mapper here gets the same
    want = samout.record_lines(map_alone(mb.mapper_params(n, True), np.frombuffer(ref.tobytes().upper(), dtype=np.uint8), rl, rows), names, rows, rl, "ref",
                               ["I" * int(x) for x in rl])
    assert len(body) == len(want) == 2 * mb.N_CHIMERIC + mb.N_UNBROKEN + mb.N_RANDOM
    cols = lambda lines: [tuple(l.split("\t")[i] for i in (0, 1, 3, 5)) for l in lines]
    assert cols(body) == cols(want)
    assert body == want
