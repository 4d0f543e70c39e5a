#!/usr/bin/env python3
"""bench.py on a library of another commit (AIM_LIB=<path>, e.g. a build of the parent made with `python -m aim_amd.build --variant
parent` in a checkout of it and copied to build_ab/): such a build exports fewer symbols than capi.SYMBOLS lists, so the library is
loaded with capi.load(strict=False) before bench.py runs. Without AIM_LIB it runs bench.py on this tree's library the same way, so that
the two sides of an A/B differ in the library alone. Arguments are bench.py's.

  for i in 1 2 3 4 5; do AIM_LIB=build_ab/lib_parent.so python tools/bench_ab.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-e2e; \\
                         python tools/bench_ab.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-e2e; done"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (torch's HIP runtime first, as in bench.py itself)
from aim_amd import capi  # noqa: E402

capi.load(strict=False)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
