"""Which library entry points every network calls, in order and with which arguments, against tests/golden/launch_plans.json.

The GPU tests compare the kernels with torch within a tolerance, so they pass whichever arm of a module's dispatch ran; an
eligibility test that starts failing falls through to a slower path silently.  Here the networks run on CPU tensors with the library
replaced by a recorder (tests/golden/make_launch_plans.py, which also writes the golden file): a block that stops taking its kernel,
or places its output at another channel offset, changes the recorded plan."""
import importlib.util
import json
import os

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_launch_plans", os.path.join(_HERE, "golden", "make_launch_plans.py"))
plans = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plans)

with open(plans.PATH) as _f:
    GOLDEN = plans.unpack(json.load(_f))
CASES = plans.cases()


def test_golden_covers_every_case():
    from strongsort_yolo_amd import nets
    assert sorted(GOLDEN) == sorted(c[0] for c in CASES)
    for n in list(nets.DETECTORS) + ["osnet"]:
        assert f"{n}/f16" in GOLDEN and f"{n}/fp32" in GOLDEN
    for n in plans.SWITCHED:
        for k, v in plans.SWITCHES:
            assert f"{n}/f16/{k}={int(v)}" in GOLDEN


def test_golden_file_is_small():
    assert os.path.getsize(plans.PATH) < 256 * 1024


@pytest.mark.parametrize("case,name,half,switch", CASES, ids=[c[0] for c in CASES])
def test_launch_plan(case, name, half, switch, monkeypatch):
    got = plans.run_case(name, half, switch, monkeypatch.setattr)
    want = GOLDEN[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: call {i} is {g}, the golden plan has {w}"
    assert len(got) == len(want), f"{case}: {len(got)} calls, the golden plan has {len(want)}"


def test_recorder_leaves_nothing_patched():
    from strongsort_yolo_amd import fused, lib
    assert lib.load.__module__ == lib.__name__ and fused.usable.__module__ == fused.__name__
