#!/bin/bash
# Register / LDS / spill table of every kernel of libwavehip -> profiles/<tag>_resources.txt (runs without a GPU).
R="$(cd "$(dirname "$0")/.." && pwd)"
TAG=${1:-r03}
RAW=$(mktemp)
# the sources of the library (wave_fenics_amd/build.py) that define kernels
for f in $(cd "$R/wave_fenics_amd" && python3 -c "import build; print(*build.SOURCES)"); do
  case "$f" in *.hip) grep -q __global__ "$R/wave_fenics_amd/csrc/$f" || continue ;; *) continue ;; esac
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Rpass-analysis=kernel-resource-usage \
    -I "$R/include" -I "$R/wave_fenics_amd/csrc" -c "$R/wave_fenics_amd/csrc/$f" -o /dev/null 2>&1 \
    | grep -E "Function Name|TotalSGPRs|VGPRs:|AGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size" \
    | sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - - - - - - | sed "s/^/$f: /"
done > "$RAW"
python3 "$R/tools/resources_table.py" "$RAW" "$R/profiles/${TAG}_resources.txt"
rm -f "$RAW"
