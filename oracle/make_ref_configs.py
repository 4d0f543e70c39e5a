"""Writes oracle/ref_configs.json: every reference configuration the tests run (tests/reference_live.py all_configs()).
Run it after changing a table the live-reference tests draw on; tests/test_reference_live_cpu.py checks the file is current."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]      # `oracle` is the package, not oracle/oracle.py
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))


def render():
    import reference_live
    doc = {"_about": "name -> reference tree, the -D list as that tree's launcher prints it, NR_DPUS / NR_TASKLETS and the "
                     "stand-in's arena sizes; written by oracle/make_ref_configs.py",
           "configs": reference_live.all_configs()}
    return json.dumps(doc, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(os.path.join(HERE, "ref_configs.json"), "w") as f:
        f.write(render())
