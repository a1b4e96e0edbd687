"""The time-stepping layer computes the bits it computed before its pieces were shared (r27): the fifteen hashes of
tools/time_step_bits.py -- every compiled form of the stage, leapfrog and boundary kernels, and rk4 / rk4_fused /
leapfrog on a P2 and a P4 box with and without a medium, on paths without atomic accumulation -- against the hashes
recorded from the commit before the refactor (tests/golden/time_step_bits.json; two runs of that commit and two of
the refactored tree gave the same fifteen).  A change that is meant to alter a result records new hashes and says so."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_time_step_bits():
    spec = importlib.util.spec_from_file_location("time_step_bits", os.path.join(ROOT, "tools", "time_step_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "time_step_bits.json")) as f:
        want = json.load(f)
    got = tool.hashes()
    assert sorted(got) == sorted(want)
    differ = [g for g in sorted(want) if got[g] != want[g]]
    assert not differ, f"other bits than recorded in: {differ}"
