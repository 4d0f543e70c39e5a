"""The C-ABI units are host code: every kernel is instantiated by its family's tu_*.hip, and the units call launchers."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aim_amd", "csrc")


def _code(path):
    return re.sub(r"//[^\n]*", "", open(path).read())


def test_no_capi_unit_compiles_or_launches_a_kernel():
    units = [os.path.join(CSRC, "aim_capi.hip")] + sorted(glob.glob(os.path.join(CSRC, "capi_*.hip")))
    assert len(units) >= 7, units            # aim_capi, capi_groups, capi_host, capi_launch, capi_mapper, capi_pipeline, capi_plan
    assert "capi_launch.hip" in [os.path.basename(u) for u in units]
    for u in units:
        code = _code(u)
        for word in ("__global__", "hipLaunchKernelGGL", "<<<"):
            assert word not in code, (os.path.basename(u), word)


@pytest.mark.parametrize("header,guard,unit", [("batch_io.hpp", "AIM_TU_BATCH_IO", "tu_batch_io.hip"), ("groups.hpp", "AIM_TU_GROUPS", "tu_groups.hip"),
                                               ("hits.hpp", "AIM_TU_GROUPS", "tu_groups.hip"), ("mates.hpp", "AIM_TU_GROUPS", "tu_groups.hip")])
def test_kernels_are_behind_the_unit_guard(header, guard, unit):
    code = _code(os.path.join(CSRC, header))
    assert code.count("#ifdef " + guard) == 1 and "#else" not in code
    begin = code.index("#ifdef " + guard)
    end = code.index("#endif", begin)
    assert code.count("#if", begin + 1, end) == 0                  # (no nested conditional: the first #endif closes the guard)
    outside = code[:begin] + code[end:]
    assert "__global__" in code[begin:end]
    for word in ("__global__", "hipLaunchKernelGGL"):
        assert word not in outside, (header, word)
    # the one unit that defines the guard includes the header
    tu = open(os.path.join(CSRC, unit)).read()
    assert re.search(r"#define\s+%s\b" % guard, tu) and '#include "%s"' % header in tu
    others = [f for f in glob.glob(os.path.join(CSRC, "*.hip")) if os.path.basename(f) != unit]
    assert not [f for f in others if re.search(r"#define\s+%s\b" % guard, open(f).read())]
