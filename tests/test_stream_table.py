"""Every public entry that takes a stream has a row behind queued work (host test, no GPU).

include/wavehip.h is parsed for prototypes with a `void* stream` parameter.  Each must be exercised by a row of
tests/test_gpu_stream_order.py (ENTRIES), be referenced there with the existing test that covers it (REFERENCED), or
stand in EXEMPT with a one-line reason.  A new stream-taking entry with none of the three fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXEMPT = {}     # entry -> one line saying why no row can run it behind queued work


def stream_entries():
    """names of the prototypes `int wf_*(..., void* stream)` of the header, in its order"""
    with open(os.path.join(ROOT, "include", "wavehip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    out = []
    for m in re.finditer(r"\bint\s+(wf_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def test_header_is_parsed():
    """the count of today, so that a change of the header's style that hides prototypes from the parser shows"""
    names = stream_entries()
    assert len(names) == len(set(names)) >= 45
    for known in ("wf_memset", "wf_sync", "wf_op_apply", "wf_tsmm", "wf_rk4_stage_bc", "wf_leapfrog_step_bc", "wf_updater_rev_end",
                  "wf_op_apply_overlapped", "wf_cg", "wf_cell_form_eval", "wf_sources_add_values", "wf_leapfrog_correlate",
                  "wf_leapfrog4_predict", "wf_leapfrog4_correct", "wf_sources_add_stencil", "wf_leapfrog4_correlate", "wf_wave_leapfrog4"):
        assert known in names, known
    assert "wf_matvec_fn" not in names          # a callback type, not an entry


def test_every_stream_entry_has_a_row():
    import test_gpu_stream_order as t
    names = stream_entries()
    assert all(isinstance(reason, str) and reason.strip() for reason in {**EXEMPT, **t.REFERENCED}.values())
    missing = [n for n in names if n not in t.ENTRIES and n not in t.REFERENCED and n not in EXEMPT]
    assert not missing, f"stream-taking entries with no row in tests/test_gpu_stream_order.py and no exemption: {missing}"
    stale = [n for n in list(t.ENTRIES) + list(t.REFERENCED) + list(EXEMPT) if n not in names]
    assert not stale, f"rows or exemptions for entries the header does not declare with a stream: {stale}"
    assert not set(EXEMPT) & t.ENTRIES, "an entry with a row needs no exemption"


def test_rows_have_unique_ids():
    import test_gpu_stream_order as t
    ids = [r[0] for r in t.ROWS]
    assert len(ids) == len(set(ids))
