"""Build libwavehip.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libwavehip.so")
# The one list of translation units: tools/diag_build.sh and tools/resources.sh read it from here.
SOURCES = [
    "tables.cpp", "mesh_io.cpp", "march_plan.cpp", "box_run_plan.cpp", "box_items.cpp", "unique_lists.cpp", "function_space.cpp", "box_space.cpp", "markers.cpp", "point_locate.cpp", "wave_loops.cpp",
    "hex_geometry.hip", "stiffness_batch.hip", "mass_batch.hip", "stiffness_march.hip", "stiffness_march_owner.hip", "stiffness_march_idx.hip", "stiffness_march_ks.hip",
    "mass_march.hip", "ordered.hip", "stiffness_dense.hip", "mass_dense_simplex.hip", "tsmm.hip", "vector_kernels.hip", "time_step.hip", "comm.hip", "updater.hip", "cg.hip", "points.hip", "adjoint.hip", "adjoint4.hip", "cell_form.hip", "api.hip",
    "hex_cell_geometry.cpp", "op_setup.hip", "op_create.hip", "op_create_box.hip", "op_apply.hip",
]
HEADERS = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "device_array.h"), os.path.join(CSRC, "op.h"), os.path.join(CSRC, "box_mesh.h"),
           os.path.join(CSRC, "stiffness_core.h"), os.path.join(CSRC, "cell_batch.h"), os.path.join(CSRC, "stiffness_elementwise.h"),
           os.path.join(CSRC, "march_column.h"), os.path.join(CSRC, "box_run_plan.h"), os.path.join(CSRC, "box_items.h"), os.path.join(CSRC, "unique_lists.h"), os.path.join(CSRC, "march_plan.h"), os.path.join(CSRC, "dense_simplex.h"), os.path.join(CSRC, "owner_pieces.h"), os.path.join(CSRC, "points_plan.h"), os.path.join(CSRC, "points_handles.h"), os.path.join(CSRC, "sweep.h"), os.path.join(CSRC, "comm.h"), os.path.join(CSRC, "tsmm_plan.h"), os.path.join(CSRC, "wave_source.h"),
           os.path.join(ROOT, "include", "wavehip.h")]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src: str, force: bool, verbose: bool) -> str:
    obj = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
    path = os.path.join(CSRC, src)
    deps = [path] + HEADERS
    if not force and os.path.exists(obj) and all(os.path.getmtime(d) <= os.path.getmtime(obj) for d in deps):
        return obj
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
           "-I",
           os.path.join(ROOT, "include"), "-I", CSRC, "-c", path, "-o", obj]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    subprocess.check_call(cmd)
    return obj


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=1 if verbose else min(8, len(SOURCES))) as ex:
        objs = list(ex.map(lambda s: _compile(s, force, verbose), SOURCES))
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
