#!/bin/bash
# Alternating same-box A/B of tools/store_case_bench.py: this tree's library against another build
# (the parent commit's libnfcs.so), C1 and C3, ROUNDS rounds. Every GPU step runs under its own time
# limit and the steps are chained: the first one that fails ends the script.
#   tools/store_case_ab.sh /path/to/parent/libnfcs.so [rounds] > store_case_ab.jsonl
set -u -o pipefail
cd "$(dirname "$0")/.."
OTHER=${1:?path of the other libnfcs.so}
ROUNDS=${2:-3}
for r in $(seq "$ROUNDS"); do
  for cfg in 1 3; do
    timeout -k 10 120 python3 tools/store_case_bench.py --config "$cfg" &&
    NFCS_LIB="$OTHER" timeout -k 10 120 python3 tools/store_case_bench.py --config "$cfg" || exit 1
  done
done
