"""Runs one reference binary of oracle/_ref (oracle/ref_build.py) on an input file. TEST INFRASTRUCTURE ONLY."""
import os
import subprocess
import tempfile

from oracle import ref_build

TIMEOUT_S = 600


class MissingBinary(AssertionError):
    pass


def run(name, input_bytes, n, timeout=TIMEOUT_S):
    """(exit code, output file bytes, stdout + stderr) of `host <input> <output> <n>`; a negative exit code is the signal that
    ended the program. The program runs in a fresh temporary directory (it writes `dpu-out` into its cwd)."""
    host = ref_build.host_path(name)
    if not os.path.exists(host):
        raise MissingBinary("no reference binary %s: __graft_entry__.build() makes oracle/_ref from oracle/ref_configs.json "
                            "where the reference tree is present" % host)
    with tempfile.TemporaryDirectory(prefix="aim_ref_run_") as tmp:
        with open(os.path.join(tmp, "in"), "wb") as f:
            f.write(input_bytes)
        p = subprocess.run([host, "in", "out", str(int(n))], cwd=tmp, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=timeout)
        out_path = os.path.join(tmp, "out")
        out = open(out_path, "rb").read() if os.path.exists(out_path) else b""
    return p.returncode, out, p.stdout
