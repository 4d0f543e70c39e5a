"""Builds the unmodified reference programs for the CPU, under the SDK stand-in of oracle/upmem_shim, into
oracle/_ref/<name>/host. TEST INFRASTRUCTURE ONLY (see oracle.py).

The reference's parameters are compile-time, so one configuration is one binary; oracle/ref_configs.json (written by
oracle/make_ref_configs.py from the tests' own tables) names them. Nothing of the reference is copied: its sources are compiled
where they lie, with the two renames the single-process build needs (-Dmain=dpu_main, -Dedit_cigar_print=dpu_edit_cigar_print)
on the DPU side's command line. Where the reference tree is absent, build_all() keeps what oracle/_ref holds."""
import concurrent.futures
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "upmem_shim")
OUT = os.path.join(HERE, "_ref")
TABLE = os.path.join(HERE, "ref_configs.json")
ROOT_ENV = "AIM_REFERENCE_ROOT"
MAX_JOBS = 16
VARIANTS = {"wfa": ("WFA/DPU-WRAM", "WFA/DPU-MRAM"), "nw": ("NW/DPU-WRAM", "NW/DPU-MRAM"), "swg": ("SWG/DPU-WRAM", "SWG/DPU-MRAM")}
# The int8 / int16 switch of SWG/DPU-WRAM (common.h:71-75); SWG/DPU-MRAM is always int16 (common.h:91).
SWG_W8_BELOW = 127
# WFA/DPU-MRAM, NW and SWG refuse WRAM_SEGMENT * NR_TASKLETS >= 62000 (*/dpu/dpu_allocator_wram.c init check), so their arena
# is the largest multiple of 8 below it. WFA/DPU-WRAM has no such check and keeps every wavefront of a pair in the arena.
WRAM_SEGMENT_CHECKED = 61992


def reference_root():
    return os.environ.get(ROOT_ENV, "/root/reference")


def table():
    return json.load(open(TABLE))["configs"]


def swg_variant(max_score, swg_cell_bytes):
    """The SWG tree whose cell width is `swg_cell_bytes` (0: whatever SWG/DPU-WRAM picks) at this MAX_SCORE."""
    if swg_cell_bytes == 2 and max_score < SWG_W8_BELOW:
        return "SWG/DPU-MRAM"
    assert swg_cell_bytes != 1 or max_score < SWG_W8_BELOW, "the reference has no int8 SWG at MAX_SCORE %d" % max_score
    return "SWG/DPU-WRAM"


def wfa_wram_segment(max_score, read_size):
    """Bytes that hold every wavefront WFA/DPU-WRAM allocates for one pair with 64-bit pointers: per score one wfa_component
    (64 bytes here) and three offset rows of at most 2 * score + 1 entries (wfa.c:143-183, 329-337), the pointer table
    (wfa.c:345 lies on the stack), both sequences and the ops row (wfa.c:417-418, 463). Never below the launcher's 60000."""
    per_score = 64 + 3 * ((2 * (max_score + 1) + 1) * 2 + 8)
    need = (max_score + 2) * per_score + 4 * read_size + 4096
    return max(60000, (need + 7) // 8 * 8)


def config(algo, variant, max_score, read_size, match=0, mismatch=3, gap_o=4, gap_e=1, gap_i=4, gap_d=4, backtrace=False,
           reduce=False, nr_dpus=1):
    """(name, table entry) of one reference build. The -D list is the one the variant's launcher prints
    (run-*-pim-*.py: MAX_SCORE, READ_SIZE, WRAM_SEGMENT, MATCH, MISMATCH, then GAP_O / GAP_E or GAP_D / GAP_I, REDUCE, BACKTRACE)."""
    assert variant in VARIANTS[algo], (algo, variant)
    segment = wfa_wram_segment(max_score, read_size) if variant == "WFA/DPU-WRAM" else WRAM_SEGMENT_CHECKED
    flags = ["-DMAX_SCORE=%d" % max_score, "-DREAD_SIZE=%d" % read_size, "-DWRAM_SEGMENT=%d" % segment, "-DMATCH=%d" % match,
             "-DMISMATCH=%d" % mismatch]
    if algo == "nw":
        flags += ["-DGAP_D=%d" % gap_d, "-DGAP_I=%d" % gap_i]
        costs = "m%dx%di%dd%d" % (match, mismatch, gap_i, gap_d)
    else:
        flags += ["-DGAP_O=%d" % gap_o, "-DGAP_E=%d" % gap_e]
        costs = "m%dx%do%de%d" % (match, mismatch, gap_o, gap_e)
    if reduce:
        assert algo == "wfa"
        flags.append("-DREDUCE")
    if backtrace:
        flags.append("-DBACKTRACE")
    name = "%s_ms%d_rs%d_%s%s%s_d%d" % (variant.lower().replace("/dpu-", "-"), max_score, read_size, costs,
                                        "_red" if reduce else "", "_bt" if backtrace else "", nr_dpus)
    # WRAM arena: the DP table of the WRAM trees (nw.c:187, swg.c:196: READ_SIZE^2 cells of 2, or 3 * 1 / 3 * 2, bytes) or the
    # segment, plus the fixed buffers; MRAM image: a DPU's 64 MiB, which the host's own allocator enforces (mram-management.h:45).
    cells = read_size * ((read_size + 7) // 8 * 8)
    table_bytes = {"NW/DPU-WRAM": 2 * cells, "SWG/DPU-WRAM": (3 if max_score < SWG_W8_BELOW else 6) * cells}.get(variant, 0)
    entry = dict(variant=variant, flags=flags, nr_dpus=nr_dpus, nr_tasklets=1, mram_bytes=64 << 20,
                 wram_bytes=(table_bytes + segment + 8 * read_size + (1 << 20)) // 4096 * 4096)
    return name, entry


def host_path(name):
    return os.path.join(OUT, name, "host")


def _shim_digest():
    h = hashlib.sha256()
    for f in sorted(os.listdir(SHIM)):
        h.update(f.encode())
        h.update(open(os.path.join(SHIM, f), "rb").read())
    return h.hexdigest()


def _stamp(entry, shim_digest):
    return json.dumps([entry, shim_digest], sort_keys=True)


def _build_one(name, entry, root, shim_digest):
    src = os.path.join(root, entry["variant"])
    dst = os.path.join(OUT, name)
    stamp = _stamp(entry, shim_digest)
    stamp_path = os.path.join(dst, "built_with.json")
    if os.path.exists(host_path(name)) and os.path.exists(stamp_path) and open(stamp_path).read() == stamp:
        return False
    os.makedirs(dst, exist_ok=True)
    defs = entry["flags"] + ["-DNR_TASKLETS=%d" % entry["nr_tasklets"], "-DNR_DPUS=%d" % entry["nr_dpus"],
                             "-DSHIM_MRAM_BYTES=%dul" % entry["mram_bytes"], "-DSHIM_WRAM_BYTES=%dul" % entry["wram_bytes"]]
    cc = [os.environ.get("CC", "gcc"), "-O2", "-w", "-std=gnu11", "-I" + SHIM, "-I" + os.path.join(src, "common")] + defs
    with tempfile.TemporaryDirectory(prefix="aim_ref_") as tmp:
        objs = []
        dpu = os.path.join(src, "dpu")
        for f in sorted(os.listdir(dpu)):
            if f.endswith(".c"):
                objs.append(os.path.join(tmp, "dpu_" + f[:-2] + ".o"))
                subprocess.check_call(cc + ["-I" + dpu, "-Dmain=dpu_main", "-Dedit_cigar_print=dpu_edit_cigar_print", "-c",
                                            os.path.join(dpu, f), "-o", objs[-1]])
        for f, o in ((os.path.join(src, "host", "host.c"), "host.o"), (os.path.join(SHIM, "shim.c"), "shim.o")):
            objs.append(os.path.join(tmp, o))
            subprocess.check_call(cc + ["-c", f, "-o", objs[-1]])
        subprocess.check_call(cc[:1] + ["-o", os.path.join(tmp, "host")] + objs)
        shutil.move(os.path.join(tmp, "host"), host_path(name))
    with open(stamp_path, "w") as f:
        f.write(stamp)
    return True


def build_all(names=None):
    """Compile every table entry (or `names`) that is missing or stale; returns how many were compiled. Without the reference
    tree nothing is compiled and oracle/_ref stays as it is."""
    root = reference_root()
    if not os.path.isdir(root):
        return 0
    configs = table()
    todo = sorted(configs) if names is None else list(names)
    digest = _shim_digest()
    jobs = max(1, min(MAX_JOBS, os.cpu_count() or 1))
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        return sum(pool.map(lambda n: _build_one(n, configs[n], root, digest), todo))


if __name__ == "__main__":
    import time
    t0 = time.time()
    print("compiled %d of %d reference configurations in %.1f s" % (build_all(), len(table()), time.time() - t0))
