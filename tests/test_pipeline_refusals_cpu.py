"""What the pipeline entry points (index, seeding, classes and MAPQ, split, extension) and the host-side helpers refuse, locked:
tests/golden/pipeline_refusals.json holds the return code and the aim_last_error() text of every refused call that
tests/golden/make_pipeline_refusals.py builds -- each violated condition alone, and each two that follow each other in an entry
point's order of checks -- and the built library must answer every one of them with the same code and the same bytes. All of them
are refused before the device probe, so the table holds with and without a device.

Before every call aim_last_error() is set to a message of aim_device_count(): the entry points sit in several translation units,
and a unit with an error buffer of its own would leave that message in place."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_pipeline_refusals", os.path.join(GOLDEN, "make_pipeline_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_refusals_match_the_golden_table(built):
    from aim_amd import capi
    gen = _generator()
    lib = capi.load()
    want = json.load(open(os.path.join(GOLDEN, "pipeline_refusals.json")))
    # the table is the generator's own list of cases, argument for argument (JSON has no tuples)
    assert [[fn, note, json.loads(json.dumps(args))] for fn, note, args in gen.cases()] == [row[:3] for row in want]
    assert len(want) >= 300 and len({row[0] for row in want}) == 21
    problems = []
    for fn, note, args, rc, err in want:
        assert rc < 0 and rc != capi.AIM_ENODEV, (fn, note)     # a refusal, and none that needs a device to come about
        got = gen.run(lib, capi, fn, args)
        if got != (rc, err):
            problems.append("%s (%s): rc %d, %r; the golden has rc %d, %r" % (fn, note, got[0], got[1], rc, err))
    assert not problems, "\n".join(problems[:40])
