#!/bin/bash
# Diagnostic: variant of libwavehip.so whose dense-mass marching kernel (k_mass_march) records per-wave phase
# timestamps (examples/bin/libwavehip_mstrace.so); tools/mass_trace.py runs it and prints the timeline.
set -e
bash "$(dirname "$0")/variant_lib.sh" mstrace mass_march.hip -DWF_MASS_TRACE "$@"
