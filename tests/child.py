"""One function of a test module in a fresh interpreter: how the GPU tests run a batch under other environment knobs, or with torch
initialised before the library. Always a new process started from the repository root, one at a time, never an exec in this one."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SOURCE = '''
import importlib
import sys
module, func, cuda_first, npz, marker = sys.argv[1:6]
if cuda_first:
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
out = getattr(importlib.import_module(module), func)()
if npz:
    import numpy as np
    np.savez(npz, **out)
if marker:
    print(marker)
'''


def run(module, func, cuda_first=False, npz=None, marker=None, env=None, timeout=300, check=True):
    """module.func() in a child process. cuda_first: torch.cuda.init() comes before the module (and with it the library) is loaded.
    npz: the path the dict that func returns is saved to. marker: printed once func has returned. env: added to this process's
    environment; a value of None takes the variable out. Fails unless the child exits with 0, with its stdout and stderr in the
    message (check=False leaves that to a caller that has more to do on a failure), and returns the completed process."""
    child_env = dict(os.environ)
    for k, v in (env or {}).items():
        if v is None:
            child_env.pop(k, None)
        else:
            child_env[k] = v
    p = subprocess.run([sys.executable, "-c", _SOURCE, module, func, "1" if cuda_first else "", npz or "", marker or ""], cwd=ROOT, env=child_env,
                       capture_output=True, text=True, timeout=timeout)
    assert not check or p.returncode == 0, "%s.%s exited with %d\n%s%s" % (module, func, p.returncode, p.stdout, p.stderr)
    return p
