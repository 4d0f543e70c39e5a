"""The index built on the device (aim_index_build_device). The contract is byte equality with the host build, engine.build_index --
itself pinned to tests/seed_model.build_index: the whole bucket[] and pos[:n_pos], with n_pos == bucket[-1]. Lengths around k, the
wavefront and the tile; k = 14 with its 1 GiB bucket and 29-bit keys; bytes that are not indexed, also across tile boundaries; one
bucket that holds every position; any CU count and poison knob; any scratch contents; and the chain into seed_candidates."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
import pipeline_batches as pb  # noqa: E402
from gpu_buffers import Hip  # noqa: E402

T = pb.index_tile()

_REF = {}


def random_ref(n, seed=2025):
    """Seeded random A C G T; a shorter one is a prefix of a longer one."""
    if "rand" not in _REF:
        _REF["rand"] = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, 3 * T + 64)]
    assert n <= len(_REF["rand"])
    return _REF["rand"][:n]


model_ref = pb.reference


class Dev(Hip):
    """Hip with the index build on it."""

    def build(self, ref, k, scratch_fill=0xEE, out_fill=0xEE):
        """aim_index_build_device on `ref`: (bucket[4^k + 1], pos[pos_capacity], n_pos) as the device left them."""
        from aim_amd import engine
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        be, pc = engine.index_sizes(k, len(ref))
        sb = engine.index_device_scratch(k, len(ref))
        assert (sb == 0) == (pc == 0)
        d_ref = self.up(ref, 16)
        d_bucket = self.alloc(be * 4, out_fill)
        d_pos = self.alloc(pc * 4, out_fill) if pc else None
        d_scr = self.alloc(sb, scratch_fill) if sb else None
        engine.index_build_device(d_ref, len(ref), k, d_bucket, d_pos, d_scr, sb)
        bucket = self.down(d_bucket, be * 4).view(np.uint32)
        pos = self.down(d_pos, pc * 4).view(np.uint32) if pc else np.zeros(0, dtype=np.uint32)
        self.free()
        return bucket, pos, int(bucket[-1])


@pytest.fixture()
def dev():
    with Dev() as d:
        yield d


def check(dev, ref, k, **kw):
    """One device build against the host's; returns (bucket, pos[:n_pos])."""
    from aim_amd import engine
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    want_b, want_p = engine.build_index(ref, k, threads=4)
    bucket, pos, n_pos = dev.build(ref, k, **kw)
    assert n_pos == int(bucket[-1]) == len(want_p) <= len(pos), (k, len(ref), n_pos, len(want_p))
    assert np.array_equal(bucket, want_b), (k, len(ref), np.nonzero(bucket != want_b)[0][:8])
    assert np.array_equal(pos[:n_pos], want_p), (k, len(ref), np.nonzero(pos[:n_pos] != want_p)[0][:8])
    return bucket, pos[:n_pos]


@pytest.mark.parametrize("k", [8, 11])
def test_lengths(dev, k):
    """Around k (no position, one, two), the wavefront, the tile and its halo, and more than one tile with a ragged end."""
    for n in (0, k - 1, k, k + 1, 63, 64, 65, T - 1, T, T + 1, T + k - 1, 3 * T + 17):
        bucket, pos = check(dev, random_ref(n), k)
        assert len(pos) == max(n - k + 1, 0)              # random A C G T: every position is indexed


def test_k14(dev):
    """The 1 GiB bucket: the scan over 2^28 + 1 entries, four radix passes and the 29-bit sentinel key."""
    import seed_model as m
    rng = np.random.default_rng(14)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 100000)].copy()
    ref[50000:50020] = ord("N")
    ref[70000:70100] = ord("G")                            # the highest code, 4^14 - 1, next to the sentinel
    ref[69999] = ref[70100] = ord("A")
    bucket, pos = check(dev, ref, 14)
    assert len(pos) == 100000 - 13 - (20 + 13) and bucket[4 ** 14 - 1] + 87 == bucket[4 ** 14]
    assert int(m.kmer_codes(ref[70000:70014], 14)[0]) == 4 ** 14 - 1


def test_model_reference(dev):
    """seed_model.make_reference() as it is: the N run, the lower-case stretch, the tandem repeat and the planted triple."""
    import seed_model as m
    ref = model_ref()
    for k in (8, 11):
        bucket, pos = check(dev, ref, k)
        assert len(pos) < len(ref) - k + 1 - (m.N_RUN[1] + m.LOWER[1])


@pytest.mark.parametrize("k", [8, 11])
def test_n_runs_across_tile_boundaries(dev, k):
    """N runs of length 1, k - 1 and k, each on a tile boundary: the k-mers that see them start in the tile before (its halo)."""
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(k).integers(0, 4, 4 * T)].copy()
    runs = [(T, 1), (2 * T - (k - 1) // 2, k - 1), (3 * T - k // 2, k)]
    for at, n in runs:
        ref[at:at + n] = ord("N")
        assert at <= (at + n) // T * T <= at + n         # a boundary lies inside or at an end of the run
    bucket, pos = check(dev, ref, k)
    covered = np.zeros(len(ref), dtype=bool)
    covered[pos] = True
    for at, n in runs:
        assert not covered[at - k + 1:at + n].any() and covered[at - k] and covered[at + n]
    assert len(pos) == 4 * T - k + 1 - sum(n + k - 1 for _, n in runs)


def test_all_n(dev):
    for k in (8, 11):
        bucket, pos = check(dev, np.full(2 * T + 5, ord("N"), dtype=np.uint8), k)
        assert len(pos) == 0 and not bucket.any()


def test_one_bucket_holds_everything(dev):
    """Poly-A: every position in the bucket of code 0, in ascending order. Placement that depended on the order of arrival, or a
    big-bucket path that was missing, would show here."""
    k = 11
    bucket, pos = check(dev, np.full(200000, ord("A"), dtype=np.uint8), k)
    assert np.array_equal(pos, np.arange(200000 - k + 1, dtype=np.uint32))
    assert bucket[0] == 0 and (bucket[1:] == len(pos)).all()


def test_two_buckets_hold_everything(dev):
    """ACAC...: the even positions in one bucket and the odd ones in the other, each ascending."""
    import seed_model as m
    k = 11
    ref = np.tile(np.frombuffer(b"AC", dtype=np.uint8), 100000)
    bucket, pos = check(dev, ref, k)
    n = 200000 - k + 1
    c_even, c_odd = (int(m.kmer_codes(ref[i:i + k], k)[0]) for i in (0, 1))
    assert np.array_equal(pos[bucket[c_even]:bucket[c_even + 1]], np.arange(0, n, 2, dtype=np.uint32))
    assert np.array_equal(pos[bucket[c_odd]:bucket[c_odd + 1]], np.arange(1, n, 2, dtype=np.uint32))
    assert bucket[c_even + 1] - bucket[c_even] + bucket[c_odd + 1] - bucket[c_odd] == n == len(pos)


def test_scratch_is_only_scratch(dev):
    """Two builds of one input over a scratch (and outputs) full of 0xA5 and full of 0x00: the same bytes, tail included."""
    ref = model_ref()
    a = dev.build(ref, 11, scratch_fill=0xA5, out_fill=0xA5)
    b = dev.build(ref, 11, scratch_fill=0x00, out_fill=0x00)
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1][:a[2]], b[1][:b[2]])
    check(dev, ref, 11, scratch_fill=0xA5)


def knob_builds():
    d = Dev()
    out = {}
    for k in (8, 11):
        bucket, pos, n_pos = d.build(model_ref(), k)
        out.update({"bucket%d" % k: bucket, "pos%d" % k: pos[:n_pos]})
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256"}], ids=["cus1-poison", "cus256"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes as the default run (and the host build) at AIM_CHIP_CUS 1 and 256 and under the three AIM_DEBUG_POISON_* knobs."""
    from aim_amd import engine
    f = str(tmp_path / "k.npz")
    child.run("test_index_device_gpu", "knob_builds", npz=f, env=env)
    out = np.load(f)
    default = knob_builds()
    for k in (8, 11):
        want_b, want_p = engine.build_index(model_ref(), k, threads=4)
        for key, want in (("bucket%d" % k, want_b), ("pos%d" % k, want_p)):
            assert np.array_equal(out[key], default[key]) and np.array_equal(out[key], want), (key, env)


def test_chain_into_seeding():
    p = child.run("test_index_device_gpu", "chain_on_device", cuda_first=True, marker="INDEX_CHAIN_OK")
    assert "INDEX_CHAIN_OK" in p.stdout, p.stdout + p.stderr


def chain_on_device():
    """engine.build_index_device (bytes, an array and a device tensor in) and seed_candidates on the tensors it returned: every
    output array equals that of the same call with the host-built index."""
    import torch
    from aim_amd import engine
    ref = pb.reference()
    rows, rl = pb.short_reads()[:2]
    k, stride, w, max_occ, band, flank, min_votes, K = pb.FULL[0]
    assert k == 11 and w is None
    want_b, want_p = engine.build_index(ref, k, threads=4)
    dev = torch.device("cuda:0")
    d_ref = torch.zeros(len(ref) + 16, dtype=torch.uint8, device=dev)
    d_ref[:len(ref)] = torch.from_numpy(ref.copy()).to(dev)
    built = [engine.build_index_device(ref, k), engine.build_index_device(ref.tobytes(), k), engine.build_index_device(d_ref, k)]
    for d_bucket, d_pos, n_pos in built:
        assert d_bucket.dtype == torch.uint8 and d_pos.dtype == torch.uint8 and d_pos.numel() == 4 * (len(ref) - k + 1)
        assert n_pos == len(want_p) and np.array_equal(d_bucket.cpu().numpy().view(np.uint32), want_b)
        assert np.array_equal(d_pos.cpu().numpy().view(np.uint32)[:n_pos], want_p)
    sp = engine.seed_params(k, pb.READ_SIZE, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K)
    on_dev = engine.seed_candidates(sp, built[0][:2], len(ref), rl, rows)
    on_host = engine.seed_candidates(sp, (want_b, want_p), len(ref), rl, rows)
    assert (on_host["seed"]["n_cands"] > 0).any()
    for name in ("req", "text_pos", "votes", "seed"):
        assert on_dev[name].tobytes() == on_host[name].tobytes(), name
