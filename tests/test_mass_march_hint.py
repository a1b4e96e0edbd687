"""WF_KERNEL_FORCE_MASS_MARCH (dense mass with a rectangular 1-D table on the marching kernel, on request): the value in
include/wavehip.h, its ctypes mirror and the name make_tuning knows it by.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_hints():
    hdr = open(os.path.join(ROOT, "include", "wavehip.h")).read()
    body = re.search(r"typedef enum \{([^}]*)\} wf_kernel_hint;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"(WF_KERNEL_\w+)\s*=\s*(\d+)", body)}


def test_header_value_matches_ctypes():
    from wave_fenics_amd import _lib
    hints = header_hints()
    assert hints["WF_KERNEL_FORCE_MASS_MARCH"] == 6
    assert len(set(hints.values())) == len(hints) == 7
    for name, value in hints.items():
        assert getattr(_lib, name) == value, name


def test_make_tuning_knows_the_name():
    from wave_fenics_amd import _lib
    from wave_fenics_amd.operators import make_tuning
    t = make_tuning({"kernel": "mass_march"})
    assert t.kernel == 6 == _lib.WF_KERNEL_FORCE_MASS_MARCH
    assert make_tuning({"kernel": "mass_march", "lz": 2, "block": (2, 2, 0)}).lz == 2
    assert "mass_march" in make_tuning.__doc__
    assert make_tuning({"kernel": "march"}).kernel == _lib.WF_KERNEL_FORCE_MARCH     # the neighbours keep their values
