"""Return code and wf_last_error text of every refusal recorded in tests/golden/refusal_table.json, replayed through
wf_op_create, wf_op_create_box_coeff, wf_cell_form_create and wf_cell_form_create_box and compared exactly: one defect
or two per descriptor, so that the order of the shared checks (csrc/op.h: check_hex_degree, check_hex_arrays,
check_box_args, per_cell_refusal) is pinned with their texts.  No GPU: every refusal precedes the first device call.
The table is this library's own record (tests/refusal_helpers.py writes it)."""
import json

import refusal_helpers as rh
from support import wpackage  # noqa: F401


def test_refusal_table_replays_exactly(wpackage):
    from wave_fenics_amd import _lib as wlib
    with open(rh.FIXTURE) as f:
        want = json.load(f)
    # the table is complete: every case of the generator, each entry point's pairs included, and nothing else
    listed = [(entry, name) for entry in rh.SINGLES for name in rh.cases(entry)]
    assert [(r["entry"], r["case"]) for r in want[:len(listed)]] == listed and len(want) == len(listed) + 2
    for entry in rh.SINGLES:
        pairs = [name for name in rh.cases(entry)[len(rh.SINGLES[entry]):]]
        npool = len(rh.PAIRED) if entry in ("wf_op_create", "wf_cell_form_create") else len(rh.PAIRED) - len(rh.DESC_ONLY) + 2
        assert len(pairs) == npool * (npool - 1) // 2
    assert all(r["rc"] in (rh.INVALID, rh.UNSUPPORTED) and r["msg"] for r in want)
    got = rh.record(wlib)
    wrong = [(w, g) for w, g in zip(want, got) if w != g]
    assert not wrong and len(got) == len(want), wrong[:5]
