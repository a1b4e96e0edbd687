"""The fourth-order leapfrog loop and both misfit gradients, bit for bit against tests/golden/two_level_bits.json: the
hashes of commit 0c79b90 on the two small boxes of tests/wave_loop_helpers.py, where a build reproduces its own bits.
tests/two_level_bits_helpers.py lists the runs and is the fixture's generator: leapfrog4 for four steps, for
max_steps = 0, 1 and 4 and for t0 >= tf; misfit_gradient of seven steps with either scheme for checkpoint_every = 1, 3,
7 and the default, and once more with a medium (the closing division by its coefficients)."""
import json

import pytest

import two_level_bits_helpers as tl
import wave_loop_helpers as wh
from support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=wh.BOXES, ids=lambda b: f"P{b[0]}")
def box(gpu, request):
    return wh.Box(*request.param, gpu)


@pytest.fixture(scope="module")
def golden():
    with open(tl.FIXTURE) as f:
        return json.load(f)


def compare(box, golden, names):
    specs = tl.runs(box)
    differ = [name for name in names if tl.run(box, *specs[name]) != golden[f"P{box.p}_{name}"]]
    assert names and not differ, f"other bits than commit 0c79b90 in: {differ}"


def test_the_fixture_holds_every_run(box, golden):
    names = tl.runs(box)
    assert sorted(f"P{p}_{name}" for p, _ in wh.BOXES for name in names) == sorted(golden)
    assert len(names) == 6 + 2 * (len(tl.CHECKPOINTS) + 1) and len(set(golden.values())) > len(golden) // 2


def test_leapfrog4_bits(box, golden):
    compare(box, golden, [name for name in tl.runs(box) if name.startswith("leapfrog4")])


@pytest.mark.parametrize("scheme", tl.SCHEMES)
def test_misfit_gradient_bits(box, golden, scheme):
    compare(box, golden, [f"gradient_{scheme}_S{S}" for S in tl.CHECKPOINTS])


@pytest.mark.parametrize("scheme", tl.SCHEMES)
def test_misfit_gradient_bits_with_a_medium(box, golden, scheme):
    compare(box, golden, [f"gradient_{scheme}_medium"])
