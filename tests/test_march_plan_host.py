"""The lattice-column planner (csrc/march_plan.cpp) on the host, without a GPU: tests/cxx/march_plan_walk.cpp builds
plans for small boxes -- shuffled, reoriented, renumbered, holed, periodic, irregular, non-manifold, non-conforming --
and checks each against the dofmap it was made from, together with the orientation helpers, the interior / interface
test and the numbering the plan's consumers call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_march_plan_sanitized(tmp_path):
    """march_plan.cpp alone (it links without the rest of the library) and the walk, built into a stand-alone program
    with AddressSanitizer and UndefinedBehaviorSanitizer (host code only; nothing of it is loaded into this process).
    Every check of the walk holds, and every plan and numbering is, hash for hash, the one recorded in
    tests/golden/march_plan_walk.txt from the planner as it was before it was split into steps (generic_plan.cpp)."""
    from wave_fenics_amd import build
    csrc = os.path.join(ROOT, "wave_fenics_amd", "csrc")
    exe = str(tmp_path / "march_plan_walk")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(ROOT, "include"),
                           "-I", csrc, os.path.join(csrc, "march_plan.cpp"), os.path.join(ROOT, "tests", "cxx", "march_plan_walk.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
    with open(os.path.join(ROOT, "tests", "golden", "march_plan_walk.txt")) as f:
        golden = f.read().splitlines()
    cases = [line for line in out.stdout.splitlines() if line.startswith("case ")]
    assert len(cases) == len(golden) > 150
    for got, want in zip(cases, golden):
        assert got == want
