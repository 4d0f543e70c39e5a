"""Every width of wfa_group_kernel under ends-free, dual-cost and gap-linear WFA and as the second stage of AIM_FLAG_WFA_ESCALATE
(tests/wfa_group_rows.py), on the GPU, against something that is not the kernel itself: the variant's DP model over the whole batch
(scores, capped), its CIGAR checker and cost function, wfa_wave_kernel's bytes on the same batch, and the oracle's global WFA
where the variant must degenerate to it and for every escalation row. Rows are zero-padded, the G = 1, 2 and 4 rows (which stage
their rows in LDS in 16-byte chunks) noise-padded too. Rows that only a knob reaches run in a process of their own under the knob.
tests/test_wfa_group_rows_cpu.py shows that the table reaches what it names and that the comparison used here is sharp."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

import wfa_group_rows as W
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, lib.aim_last_error()
    return lib


def _cases(rows):
    return [(k, pad) for k in rows for pad in (("zero", "noise") if k[1] in (1, 2, 4) else ("zero",))]


def _case_id(v):
    return W.row_id(v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def forced(gpu, tmp_path_factory):
    """run(key, pad): run_row() of a forced row, from a process started under the row's knobs; all rows of one knob setting and
    padding run in one process, once."""
    done = {}

    def run(key, pad):
        env = W.TABLE[key][3]
        k = (tuple(sorted(env.items())), pad)
        if k not in done:
            keys = [r for r, p in _cases(list(W.TABLE)) if p == pad and W.TABLE[r][3] == env]
            out = str(tmp_path_factory.mktemp("forced") / "out.npz")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wfa_group_rows.py"), "--run", out, pad] + [repr(r) for r in keys],
                               env=W.run_env(env), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
            z = np.load(out)
            done[k] = {r: {f.split("/", 1)[1]: z[f] for f in z.files if f.startswith("%d/" % i)} for i, r in enumerate(keys)}
        return done[k][key]
    return run


def _run(forced, monkeypatch, key, pad):
    if W.is_forced(key):
        return forced(key, pad)
    for k in [k for k in os.environ if k.startswith("AIM_") and k != "AIM_LIB"]:
        monkeypatch.delenv(k)
    return W.run_row(key, pad)


@pytest.mark.parametrize("key,pad", _cases(W.VARIANT_ROWS), ids=_case_id)
def test_variant_rows(gpu, forced, monkeypatch, key, pad):
    """A row of ends-free, dual-cost or gap-linear WFA on wfa_group_kernel<G>: the plan line names G and the flag; every score
    equals the variant's DP model, capped, with status AIM_PAIR_OK and the over-cap ops range the header documents; every under-cap
    CIGAR uses up both sequences, is truthful about 'M' / 'X' and re-scores to the reported score; wfa_wave_kernel gives the same
    result rows and ops bytes; with no free end, with two equal pieces and with a second piece that costs MAX_SCORE + 1 the
    kernels give the oracle's global WFA, every byte; at most a quarter of the pairs (the pinned count) left for wfa_wave_kernel."""
    W.check_row(key, pad, _run(forced, monkeypatch, key, pad))


@pytest.mark.parametrize("key,pad", _cases(W.ESCALATE_ROWS), ids=_case_id)
def test_escalate_rows(gpu, forced, monkeypatch, key, pad):
    """A row of AIM_FLAG_WFA_ESCALATE whose second stage is wfa_group_kernel<G, ..., TODO_IN> (kind escalate_modrows: on rows of
    96 entries): the plan line says so and ends in escalate=c, c > 0; every per-pair output equals the oracle's at MAX_SCORE; at
    least ten pairs, in more than one 64-pair unit, score over c and so went through the second stage's device-side list."""
    W.check_row(key, pad, _run(forced, monkeypatch, key, pad))


def test_the_worker_reads_what_it_is_given():
    """The row keys travel to the worker as their repr."""
    assert all(ast.literal_eval(repr(k)) == k for k in W.TABLE)
