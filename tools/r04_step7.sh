#!/bin/bash
# Round 4: k_pad = 128 data passes -- pinned TN fragment bases + two-tile fill, A/B against the build before them
set -u
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
O=$R/gpurun_out/r04_step7
mkdir -p "$O"
cd "$R"
python3 tools/ab_lib_versions.py 16384,8192,4096,128 60 > "$O/ab_c2.txt" 2>&1; tail -n 3 "$O/ab_c2.txt"
python3 tools/ab_lib_versions.py 16384,8192,4096,128 60 > "$O/ab_c2_b.txt" 2>&1; tail -n 3 "$O/ab_c2_b.txt"
python3 -m pytest tests/test_gpu_mu.py tests/test_gpu_fullsize.py -x -q -m gpu -k "mu or c2 or C2" > "$O/pytest_mu.txt" 2>&1; tail -n 3 "$O/pytest_mu.txt"
