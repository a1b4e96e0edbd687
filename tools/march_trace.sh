#!/bin/bash
# Diagnostic: build a variant of libwavehip.so whose box marching kernel records per-wave phase
# timestamps (examples/bin/libwavehip_mtrace.so); tools/march_trace.py runs it and prints the timeline.
# Extra -D flags (e.g. -DWF_DIAG for the WF_ABLATE masks) can be given as arguments.
# The indexed marching kernel (dense mass, arbitrary-dofmap stiffness) has the same hooks: the script also
# builds examples/bin/libwavehip_itrace.so (-DWF_IDX_TRACE) for tools/idx_trace.py.
set -e
T="$(cd "$(dirname "$0")" && pwd)"
bash "$T/variant_lib.sh" mtrace stiffness_march.hip -DWF_MARCH_TRACE "$@"
bash "$T/variant_lib.sh" itrace stiffness_march_idx.hip -DWF_IDX_TRACE "$@"
