#!/bin/bash
# tmc2_host_metrics_compute under -fsanitize=address,undefined as a stand-alone program (tools/metrics_host_sanitize.cpp): CPU only.
#   tools/metrics_host_sanitize.sh [case ...]          # default: duplicates lattice (tests/metrics_option_cases.py)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
CASES=${*:-duplicates lattice}
cd "$ROOT"
python - "$TMP" $CASES <<'PY'
import sys
sys.path[:0] = ["mpeg-pcc-tmc2_amd", "tests"]
import numpy as np
import metrics_option_cases as mc
for name in sys.argv[2:]:
    src, sc, rec, rc, nrm = mc.case(name)
    with open("%s/%s.cloud" % (sys.argv[1], name), "wb") as f:
        np.array([len(src), len(rec)], np.int64).tofile(f)
        for a, t in ((src, np.int16), (sc, np.uint8), (rec, np.int16), (rc, np.uint8), (nrm, np.float64)):
            np.ascontiguousarray(a, t).tofile(f)
PY
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Impeg-pcc-tmc2_amd/csrc \
    tools/metrics_host_sanitize.cpp mpeg-pcc-tmc2_amd/csrc/metrics_host.cpp -o "$TMP/metrics_host_sanitize"
FILES=""
for c in $CASES; do FILES="$FILES $TMP/$c.cloud"; done
"$TMP/metrics_host_sanitize" $FILES
