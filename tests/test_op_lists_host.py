"""The index lists that operator set-up computes on the host and the kernels dereference without a check, walked
without a GPU: the interior / interface work-item lists of the box marching operators (csrc/box_items.cpp), the owner
kernel's run tables (csrc/box_run_plan.cpp) and the batch-unique gather/scatter lists (csrc/unique_lists.cpp).
tests/cxx/op_lists_walk.cpp holds the cases and what each must satisfy."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compiler():
    """a plain C++ compiler: $CXX, the system's, or the clang++ next to hipcc (as a C++ compiler it knows nothing of HIP)"""
    from wave_fenics_amd import build
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(build.hipcc()) or build.hipcc())))
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    raise RuntimeError("no C++ compiler found")


def test_op_lists_sanitized(tmp_path):
    """box_items.cpp, unique_lists.cpp and box_run_plan.cpp link alone, compiled as plain C++17 with the csrc directory as
    the only include path (no HIP header is in reach, so the files are HIP-free), into a stand-alone program with
    AddressSanitizer and UndefinedBehaviorSanitizer (host code only; nothing of it is loaded into this process).  Every
    check of the walk holds."""
    csrc = os.path.join(ROOT, "wave_fenics_amd", "csrc")
    exe = str(tmp_path / "op_lists_walk")
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc] + [os.path.join(csrc, s) for s in ("box_items.cpp", "unique_lists.cpp", "box_run_plan.cpp")]
                          + [os.path.join(ROOT, "tests", "cxx", "op_lists_walk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "0 failures", out.stdout[-4000:] + out.stderr[-4000:]
    # every family of cases ran: 8 cross-sections x 3 boxes x 3 segmentations and 12 exhaustive walks, 5 column counts
    # and 8 mutants of a run table, the tuner's candidate lists, their tables and its predicate, 9 hexahedral and 10 dense
    # dofmaps and the refusals
    count = lambda prefix: sum(line.startswith(prefix) for line in lines)
    assert (count("items "), count("runs "), count("runs timed cuts"), count("lists ")) == (84, 16, 3, 20), out.stdout[-4000:]
