#!/bin/bash
# Diagnostic: build a variant of libwavehip.so whose tetrahedral MFMA kernel records per-wave phase
# timestamps (examples/bin/libwavehip_trace.so); tools/dense_trace.py runs it and prints the timeline.
set -e
bash "$(dirname "$0")/variant_lib.sh" trace stiffness_dense.hip -DWF_DENSE_TRACE
