"""(w, k) minimizers on the GPU. aim_index_build_device_minimizers equals the host build (itself pinned to tests/minimizer_model.py
by tests/test_minimizers_cpu.py) in the whole bucket[] and pos[:n_pos] -- lengths around k, the window, the wavefront and the tile with
its halo; references on which the halo decides; any CU count, poison knob and scratch contents. aim_seed_device with
AIM_SEED_OPT_MINIMIZERS equals the model in every byte of requests, text_pos, votes and aim_seed_t. And the chain: device index,
minimizer seeds, aim_align_device_groups."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
from gpu_buffers import Hip, cached  # noqa: E402
from pipeline_batches import index_tile  # noqa: E402

READ_SIZE = 128
T = index_tile()


def random_ref(n):
    """Seeded random A C G T; a shorter one is a prefix of a longer one."""
    full = cached("minimizer rand", lambda: np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(4711).integers(0, 4, 2 * T + 200)])
    assert n <= len(full)
    return full[:n]


# ---- the index ------------------------------------------------------------------------------------------------------------------

def build(ref, k, w, fill=0xEE):
    """aim_index_build_device_minimizers on `ref` over outputs and scratch full of `fill`: (bucket[4^k + 1], pos[:n_pos])."""
    from aim_amd import engine
    with Hip() as h:
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        be, pc = engine.index_sizes(k, len(ref))
        sb = engine.index_device_scratch(k, len(ref))
        d_ref = h.up(ref, 16)
        d_bucket = h.alloc(be * 4, fill)
        d_pos = h.alloc(pc * 4, fill) if pc else None
        d_scr = h.alloc(sb, fill) if sb else None
        engine.index_build_device_minimizers(d_ref, len(ref), k, w, d_bucket, d_pos, d_scr, sb)
        bucket = h.down(d_bucket, be * 4).view(np.uint32)
        n_pos = int(bucket[-1])
        assert n_pos <= pc
        pos = h.down(d_pos, n_pos * 4).view(np.uint32) if n_pos else np.zeros(0, dtype=np.uint32)
        return bucket, pos


def model_bucket(ref, k, w):
    """(bucket, pos) of minimizer_model.build_index with the 4^k + 1 bucket entries written as the step function they are -- at k = 14
    that is a fraction of the time a counting pass over 1 GiB takes."""
    import minimizer_model as mm
    import seed_model as m
    code = m.kmer_codes(ref, k)
    p = np.nonzero(mm.selected(ref, k, w))[0] if len(code) else np.zeros(0, dtype=np.int64)
    p = p[np.argsort(code[p], kind="stable")]
    u, cnt = np.unique(code[p], return_counts=True)
    values = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    edges = np.concatenate([[-1], u, [4 ** k]])
    return np.repeat(values, np.diff(edges)), p.astype(np.uint32)


def check(ref, k, w, fill=0xEE):
    """One device build against the host's (against the model's at k = 14, where the host's 1 GiB counting sort takes seconds and is
    itself compared with the model in tests/test_minimizers_cpu.py and once below)."""
    from aim_amd import engine
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    want_b, want_p = model_bucket(ref, k, w) if k == 14 else engine.index_build_minimizers(ref, k, w, threads=4)
    bucket, pos = build(ref, k, w, fill)
    assert len(bucket) == len(want_b) == 4 ** k + 1 and int(bucket[-1]) == len(want_p), (k, w, len(ref), int(bucket[-1]), len(want_p))
    assert np.array_equal(bucket, want_b), (k, w, len(ref), np.nonzero(bucket != want_b)[0][:8])
    assert np.array_equal(pos, want_p), (k, w, len(ref), np.nonzero(pos != want_p)[0][:8])
    return bucket, pos


LENGTHS = {"k-1": lambda k, w: k - 1, "k": lambda k, w: k, "k+w-2": lambda k, w: k + w - 2, "k+w-1": lambda k, w: k + w - 1, "63": lambda k, w: 63,
           "64": lambda k, w: 64, "65": lambda k, w: 65, "T+k-2": lambda k, w: T + k - 2, "T+k-1": lambda k, w: T + k - 1, "T+k": lambda k, w: T + k,
           "2T+w": lambda k, w: 2 * T + w}


@pytest.mark.parametrize("length", list(LENGTHS))
@pytest.mark.parametrize("w", [1, 2, 16, 32])
@pytest.mark.parametrize("k", [8, 14])
def test_lengths(k, w, length):
    """No position, one, one window short of full and exactly full, the wavefront, the tile with its k - 1 bytes of halo, one position
    more and less, and two tiles plus a window."""
    n = LENGTHS[length](k, w)
    bucket, pos = check(random_ref(n), k, w)
    if w == 1:
        assert len(pos) == max(n - k + 1, 0)
    elif n - k + 1 >= 2 * w:
        assert 0 < len(pos) < n - k + 1


def test_k14_equals_the_host_build():
    """The host build itself at k = 14 (test_lengths compares with the model there), with an N run and the highest code."""
    from aim_amd import engine
    ref = random_ref(T + 500).copy()
    ref[3000:3020] = ord("N")
    ref[T - 40:T + 40] = ord("G")
    k, w = 14, 16
    bucket, pos = build(ref, k, w)
    want_b, want_p = engine.index_build_minimizers(ref, k, w, threads=8)
    assert np.array_equal(bucket, want_b) and np.array_equal(pos, want_p)
    assert bucket[4 ** 14 - 1] < bucket[4 ** 14]          # poly-G: code 4^14 - 1, next to the sentinel key


@pytest.mark.parametrize("k,w", [(8, 2), (8, 16), (8, 32), (11, 16)])
def test_n_run_from_the_halo_across_a_tile_boundary(k, w):
    """An N run that starts w - 1 positions before a tile boundary and ends after it: the last valid k-mers of tile 0 see invalid
    neighbours up to the edge of what is staged, the first valid ones of tile 1 see them in their left halo."""
    ref = random_ref(2 * T + 100).copy()
    at, end = T - (w - 1), T + k + 3
    ref[at:end] = ord("N")
    bucket, pos = check(ref, k, w)
    covered = np.zeros(len(ref), dtype=bool)
    covered[pos] = True
    assert not covered[at - k + 1:end].any()
    # the k-mer just before the run's reach ends its sequence of valid keys: it is the leftmost minimum of a window of invalid ones
    assert covered[at - k - w + 1:at - k + 1].any() and covered[end:end + w].any()


@pytest.mark.parametrize("k,w", [(8, 16), (8, 32), (11, 5)])
def test_the_halo_decides(k, w):
    """A reference on which positions next to the tile boundary are selected, or not, because of keys on the other side: cut at the
    boundary, each half alone selects a different set there. The seed is searched for, the property is asserted."""
    import minimizer_model as mm
    for seed in range(50):
        rng = np.random.default_rng(seed)
        ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 2 * T + 64)]
        whole = mm.selected(ref[T - 4 * w:T + 4 * w + k - 1], k, w)                      # positions T - 4w .. T + 4w - 1
        left = mm.selected(ref[T - 4 * w:T + k - 1], k, w)                               # tile 0's positions alone
        right = mm.selected(ref[T:T + 4 * w + k - 1], k, w)                              # tile 1's alone
        if (whole[:4 * w] != left).any() and (whole[4 * w:] != right).any():
            break
    else:
        pytest.fail("no such reference among 50 seeds")
    bucket, pos = check(ref, k, w)
    covered = np.zeros(len(ref), dtype=bool)
    covered[pos] = True
    assert np.array_equal(covered[T - 3 * w:T + 3 * w], whole[w:-w])       # (w positions from the cut the piece's own ends decide)


@pytest.mark.parametrize("w", [2, 16, 32])
def test_poly_a_and_acac_across_two_tiles(w):
    """All keys tie (poly-A: the first position of every window, 0 .. n - w) or alternate (ACAC...: every window holds both k-mers, and
    the first position of the smaller one wins it: that parity up to n - w + 1), across a tile boundary."""
    import minimizer_model as mm
    k, n_bases = 8, 2 * T + 50
    n = n_bases - k + 1
    bucket, pos = check(np.full(n_bases, ord("A"), dtype=np.uint8), k, w)
    assert np.array_equal(pos, np.arange(n - w + 1, dtype=np.uint32))
    ref = np.tile(np.frombuffer(b"AC", dtype=np.uint8), n_bases // 2)
    bucket, pos = check(ref, k, w)
    keys = mm.keys(ref[:k + 1], k)
    first = 0 if keys[0] < keys[1] else 1
    assert np.array_equal(np.sort(pos), np.arange(first, n - w + 2, 2, dtype=np.uint32)), (w, first, pos[:8])


def test_scratch_and_outputs_are_only_that():
    """Scratch, d_bucket and d_pos full of 0xA5 and full of 0x00: the same bytes, the host's."""
    import seed_model as m
    ref = m.make_reference()
    a = check(ref, 11, 5, fill=0xA5)
    b = check(ref, 11, 5, fill=0x00)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


KNOB_ENVS = [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
             {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}]
KNOB_INDEX = [(8, 16), (11, 5), (8, 32)]
KNOB_SEED = [(11, 5), (8, 16)]


def knob_batch():
    """What the knob runs repeat: three index builds over three tiles with an N run, and two seeding cases."""
    out = {}
    ref = knob_ref()
    for k, w in KNOB_INDEX:
        bucket, pos = build(ref, k, w, fill=0xA5)
        out.update({"bucket%d_%d" % (k, w): bucket, "pos%d_%d" % (k, w): pos})
    d = seed_data()
    for k, w in KNOB_SEED:
        for name, arr in zip(("req", "tpos", "votes", "seed"), run_seed(seed_case(k, w), d["ref"], d["rows"], d["rl"])):
            out["%s%d_%d" % (name, k, w)] = arr.view(np.uint8)
    return out


def knob_ref():
    ref = random_ref(2 * T + 150).copy()
    ref[T - 10:T + 3] = ord("N")
    return ref


@pytest.mark.parametrize("env", KNOB_ENVS, ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the host build's and the model's -- at AIM_CHIP_CUS 1 and 256 and under the three AIM_DEBUG_POISON_* knobs."""
    from aim_amd import engine
    f = str(tmp_path / "k.npz")
    child.run("test_minimizers_gpu", "knob_batch", npz=f, env=env)
    out = np.load(f)
    for k, w in KNOB_INDEX:
        want_b, want_p = engine.index_build_minimizers(knob_ref(), k, w, threads=4)
        assert np.array_equal(out["bucket%d_%d" % (k, w)], want_b) and np.array_equal(out["pos%d_%d" % (k, w)], want_p), (k, w, env)
    for k, w in KNOB_SEED:
        for name, want in zip(("req", "tpos", "votes", "seed"), expected(seed_case(k, w))):
            assert out["%s%d_%d" % (name, k, w)].tobytes() == want.tobytes(), (name, k, w, env)


# ---- seeding --------------------------------------------------------------------------------------------------------------------

def seed_data():
    """seed_model's reference and 192 of its reads, made once."""
    def make():
        import seed_model as m
        ref = m.make_reference()
        rows, rl, true_pos, strand, plain = m.make_reads(ref, 192, READ_SIZE)
        return dict(ref=ref, rows=rows, rl=rl, strand=strand, plain=plain)
    return cached("minimizer seed_data", make)


def seed_case(k, w):
    """(k, w, max_occ, band, flank, min_votes, K): the two parameter rows of tests/test_seed_gpu.py that run at stride 1."""
    return (k, w, 64, 4, 16, 3, 16) if k == 8 else (k, w, 8, 8, 8, 2, 4)


def model_index(ref_key, ref, k, w):
    import minimizer_model as mm
    return cached(("minimizer index", ref_key, k, w), lambda: mm.build_index(ref, k, w))


def expected(case, ref_key="model", ref=None, rows=None, rl=None, read_size=READ_SIZE):
    """The model's output for a case over seed_data() (or the reads given, under ref_key), computed once."""
    import minimizer_model as mm
    k, w, max_occ, band, flank, min_votes, K = case
    d = seed_data()
    ref = d["ref"] if ref is None else ref
    rows, rl = (d["rows"], d["rl"]) if rows is None else (rows, rl)
    return cached(("minimizer expected", case, ref_key, read_size),
                  lambda: mm.seed(rows, rl, model_index(ref_key, ref, k, w), len(ref), k, w, max_occ, band, flank, min_votes, K, read_size))


def run_seed(case, ref, rows, rl, read_size=READ_SIZE, options=None):
    """aim_seed_device over buffers uploaded through the HIP runtime the library loaded; the index is the library's host build for
    (k, w). options: the value to send instead of AIM_SEED_OPT_MINIMIZERS(w)."""
    from aim_amd import capi, engine
    k, w, max_occ, band, flank, min_votes, K = case
    sp = engine.seed_params(k, read_size, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    if options is not None:
        sp.options = options
    bucket, pos = engine.index_build_minimizers(ref, k, w, threads=4)
    n = len(rl)
    with Hip() as h:
        d_b, d_p = h.up(bucket), h.up(pos)
        d_rl, d_rows = h.up(np.ascontiguousarray(rl, dtype=np.int32)), h.up(rows, 64)
        d_req, d_tp, d_v, d_s = h.filled(n * K * 16), h.filled(n * K * 8), h.filled(n * K * 4), h.filled(n * 16)
        engine.seed_device(sp, n, d_rl, d_rows, d_b, d_p, len(ref), d_req, d_tp, d_v, d_s)
        return (h.down(d_req, n * K * 16).view(capi.REQUEST_DTYPE), h.down(d_tp, n * K * 8).view(np.uint64),
                h.down(d_v, n * K * 4).view(np.uint32), h.down(d_s, n * 16).view(capi.SEED_DTYPE))


def assert_equal(got, want):
    for name, g, w in zip(("requests", "text_pos", "votes", "seed"), got, want):
        assert g.tobytes() == w.tobytes(), (name, np.nonzero(g != w)[0][:8])


@pytest.mark.parametrize("w", [1, 5, 16])
@pytest.mark.parametrize("k", [8, 11])
def test_seeds_equal_model(k, w):
    d = seed_data()
    case = seed_case(k, w)
    want = expected(case)
    n = d["rl"] - k + 1
    assert (d["rl"] < k).any() and ((n > 0) & (n < w)).any() == (w > 1) and (d["rl"] == READ_SIZE).any()    # shorter than k; 0 < n < w; a full row
    assert (d["rows"] == ord("N")).any() and set(d["strand"].tolist()) == {0, 1}
    assert (want[3]["n_cands"] > 0).any() and (want[3]["n_cands"] < case[6]).any() and (want[1] >> np.uint64(63)).any()
    assert_equal(run_seed(case, d["ref"], d["rows"], d["rl"]), want)


@pytest.mark.parametrize("k", [8, 11])
def test_w1_is_the_plain_seeder(k):
    """w = 1 at stride 1: the bytes of options = 0 over the same index, and seed_model's."""
    import seed_model as m
    d = seed_data()
    case = seed_case(k, 1)
    with_option = run_seed(case, d["ref"], d["rows"], d["rl"])
    plain = run_seed(case, d["ref"], d["rows"], d["rl"], options=0)
    assert_equal(with_option, plain)
    _, _, max_occ, band, flank, min_votes, K = case
    assert_equal(plain, m.seed(d["rows"], d["rl"], m.build_index(d["ref"], k), len(d["ref"]), k, 1, max_occ, band, flank, min_votes, K, READ_SIZE))
    if k == 8:
        assert (plain[3]["flags"] & m.TRUNCATED).any()


def test_truncation_in_a_repeat():
    """A 40-base unit in 60 copies and max_occ 64: every minimizer of a read from inside has 60 positions, a full row brings about
    40 of them per strand, and the 1 024 kept hits overflow -- in (j, p) order, which only an exact append position reproduces."""
    import seed_model as m
    rng = np.random.default_rng(5)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 12000)].copy()
    ref[4096:4096 + 2400] = np.tile(ref[4096:4136], 60)
    rows = np.zeros((12, READ_SIZE), dtype=np.uint8)
    rl = np.zeros(12, dtype=np.int32)
    for r in range(12):
        L = (READ_SIZE, 100, 60)[r % 3]
        p = 4096 + int(rng.integers(0, 2400 - L)) if r < 9 else int(rng.integers(0, 4000))
        read = ref[p:p + L]
        rows[r, :L] = m.revcomp(read) if r % 2 else read
        rl[r] = L
    case = (8, 5, 64, 4, 16, 3, 16)
    want = expected(case, "tandem", ref, rows, rl)
    assert (want[3]["flags"] & m.TRUNCATED).sum() >= 4 and (want[3]["n_hits"] == m.MAX_HITS).any() and (want[3]["flags"] == 0).any()
    assert_equal(run_seed(case, ref, rows, rl), want)


def test_read_size_4096():
    """Rows of 4 096: full rows, a long and a short read, both strands, one with N runs."""
    import seed_model as m
    rs = 4096
    rng = np.random.default_rng(6)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 40000)].copy()
    rows = np.zeros((6, rs), dtype=np.uint8)
    rl = np.zeros(6, dtype=np.int32)
    for r, L in enumerate((rs, rs, 3001, 40, rs, 11)):
        p = int(rng.integers(0, len(ref) - L))
        read = m.edit(rng, ref[p:p + L], L // 50)[:rs] if r in (1, 2) else ref[p:p + L].copy()
        if r == 4:
            read[100:130] = ord("N")
            read[2000] = ord("N")
        read = m.revcomp(read) if r % 2 else read
        rows[r, :len(read)] = read
        rl[r] = len(read)
    case = (11, 16, 8, 8, 8, 2, 4)
    want = expected(case, "rs4096", ref, rows, rl, read_size=rs)
    assert (want[3]["n_cands"][:5] >= 1).all() and want[3]["n_hits"].max() > 300 and (want[0]["text_len"] == rs).any()
    assert_equal(run_seed(case, ref, rows, rl, read_size=rs), want)


# ---- the chain ------------------------------------------------------------------------------------------------------------------

def test_chain_on_device():
    p = child.run("test_minimizers_gpu", "chain_on_device", cuda_first=True, marker="MINIMIZER_CHAIN_OK")
    assert "MINIMIZER_CHAIN_OK" in p.stdout, p.stdout + p.stderr


def chain_on_device():
    """The device's minimizer index, minimizer seeds from it, aim_align_device_groups on the seeder's device buffers: the aim_best_t
    rows equal those of the same alignment fed from the host -- the host build's index, the numpy model's candidates."""
    import torch
    import minimizer_model as mm
    from aim_amd import capi, engine
    lib = capi.load()
    d = seed_data()
    ref, n = d["ref"], 192
    rows, rl = np.ascontiguousarray(d["rows"][:n]), d["rl"][:n]
    k, w, max_occ, band, flank, min_votes, K = case = seed_case(11, 5)
    sp = engine.seed_params(k, READ_SIZE, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    d_bucket, d_pos, n_pos = engine.build_index_device(ref, k, w=w)
    host_index = engine.index_build_minimizers(ref, k, w)
    assert n_pos == len(host_index[1]) and np.array_equal(d_pos.cpu().numpy().view(np.uint32)[:n_pos], host_index[1])
    out = engine.seed_candidates(sp, (d_bucket, d_pos), len(ref), rl, rows)
    want = mm.seed(rows, rl, host_index, len(ref), k, w, max_occ, band, flank, min_votes, K, READ_SIZE)
    assert_equal((out["req"], out["text_pos"], out["votes"], out["seed"]), want)
    dev = torch.device("cuda:0")
    params = engine.make_params("wfa", 20, READ_SIZE, read_groups=True, ref_texts=True, ends_free=(0, 0, 2 * flank, 2 * flank))
    offs = engine.seed_groups_offsets(n, K)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = up(offs)
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[:len(ref)] = torch.from_numpy(ref).to(dev)
    sb = lib.aim_scratch_bytes(capi.params_ref(params), n * K)
    d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)

    def align(d_req, d_reads, d_tp):
        d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_best = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        engine.align_device_groups(params, n * K, n, d_req.data_ptr(), d_reads.data_ptr(), None, d_tp.data_ptr(), d_ref.data_ptr(), len(ref),
                                   d_off.data_ptr(), d_res.data_ptr(), None, d_best.data_ptr(), d_scr.data_ptr(), sb)
        torch.cuda.synchronize()
        return d_best.cpu().numpy().view(capi.BEST_DTYPE)
    on_device = align(out["d_req"], out["d_reads"], out["d_text_pos"])
    from_host = align(up(want[0]), out["d_reads"], up(want[1]))
    assert on_device.tobytes() == from_host.tobytes()
    plain = np.nonzero(d["plain"][:n])[0]
    assert len(plain) >= 8 and set(d["strand"][plain].tolist()) == {0, 1}
    assert np.array_equal(on_device["best_pair"][plain], plain.astype(np.uint32) * K) and (on_device["best_score"][plain] == 0).all()
