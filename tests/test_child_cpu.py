"""tests/child.py alone: a child that fails must fail its caller, whichever way it fails, and what a child returns and the
environment it is given must arrive. The children are functions of this module."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402

ME = "test_child_cpu"


def raises():
    raise RuntimeError("the child's own words")


def leaves_silently():
    os._exit(3)


def returns_an_array():
    return {"a": np.arange(5, dtype=np.uint32) * 3}


def reports_the_environment():
    print("GIVEN=%s TAKEN=%s" % (os.environ.get("CHILD_TEST_GIVEN"), os.environ.get("CHILD_TEST_TAKEN")))


def test_a_child_that_raises_fails_the_caller_with_its_traceback():
    with pytest.raises(AssertionError) as e:
        child.run(ME, "raises", marker="NEVER_PRINTED", timeout=60)
    text = str(e.value)
    assert "Traceback" in text and "RuntimeError: the child's own words" in text and "exited with 1" in text and "NEVER_PRINTED" not in text


def test_a_child_that_exits_nonzero_without_output_fails_too():
    with pytest.raises(AssertionError) as e:
        child.run(ME, "leaves_silently", timeout=60)
    assert "leaves_silently exited with 3" in str(e.value)
    p = child.run(ME, "leaves_silently", timeout=60, check=False)          # check=False hands the same process to the caller
    assert p.returncode == 3 and p.stdout == "" and p.stderr == ""


def test_a_missing_function_fails_the_caller():
    with pytest.raises(AssertionError) as e:
        child.run(ME, "no_such_function", timeout=60)
    assert "AttributeError" in str(e.value)


def test_the_returned_dict_arrives_through_the_npz_and_the_marker_is_printed(tmp_path):
    f = str(tmp_path / "out.npz")
    p = child.run(ME, "returns_an_array", npz=f, marker="CHILD_OK", timeout=60)
    assert p.returncode == 0 and p.stdout.splitlines() == ["CHILD_OK"]
    assert np.load(f)["a"].tolist() == [0, 3, 6, 9, 12]


def test_the_extra_environment_reaches_the_child(monkeypatch):
    monkeypatch.setenv("CHILD_TEST_TAKEN", "here")
    monkeypatch.delenv("CHILD_TEST_GIVEN", raising=False)
    assert "GIVEN=None TAKEN=here" in child.run(ME, "reports_the_environment", timeout=60).stdout
    p = child.run(ME, "reports_the_environment", env={"CHILD_TEST_GIVEN": "7", "CHILD_TEST_TAKEN": None}, timeout=60)
    assert "GIVEN=7 TAKEN=None" in p.stdout
    assert os.environ.get("CHILD_TEST_GIVEN") is None and os.environ["CHILD_TEST_TAKEN"] == "here"     # the caller's own is untouched
