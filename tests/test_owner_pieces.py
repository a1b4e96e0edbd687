"""Owner stiffness kernel at P4: the 16-byte pieces of a staged x plane ("r25").

wave_fenics_amd/csrc/owner_pieces.h classifies every piece of a column's rectangle as inside the mesh (one 16-byte
direct-to-LDS load), outside (never loaded) or straddling the mesh's last lattice line in x (one 8-byte load), and gives
the source offset.  The kernel and tests/cxx/owner_pieces_walk.cpp share that header; the program walks meshes of
nx, ny in {1, 2, 7, 8, 9, 16, 17, 54}, the three P4 cross-sections, every column, every plane of the first and the last
layer and both alignments of x, and checks that every load lies inside the vector, that every rectangle position inside
the mesh is filled exactly once with its own value, and that nothing outside the mesh is loaded.

Host code only, a program with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer: its loads are
done for real from a heap block of exactly the vector's size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pieces_walk_sanitized(tmp_path):
    from wave_fenics_amd import build
    exe = str(tmp_path / "owner_pieces_walk")
    # the sanitizers on the host side only, as tests/test_box_host.py builds its walk; the program has no device code
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san,
                           "-I", os.path.join(ROOT, "wave_fenics_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "owner_pieces_walk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "\n0 failures" in out.stdout, out.stdout + out.stderr
    for shape in ("4 x 4", "8 x 2", "2 x 8"):
        assert shape + ":" in out.stdout
