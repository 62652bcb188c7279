#!/bin/bash
# the full bench line's extra workloads (256^3, then 512^3 in eight boxes, then ONE 512^3 box, ...) with pooled-chunk fields and with hipMalloc fields: the one-box case after the pool has been churned
cd "$(dirname "$0")/.."; O=${1:-bench_outputs/alloc_ab}; mkdir -p $O          # $1: the output folder
run() { tag=$1; shift; env VDN_LIB_FLAVOUR=testing "$@" python bench.py --full --skip-cpu --no-pmc > $O/$tag.json 2> $O/$tag.err || return 1
  python - "$tag" "$O/$tag.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print("%-24s 256^3 %.2f ms | " % (sys.argv[1], d["ms_per_step"]) + "  ".join("%.1f" % e["ms_per_step"] for e in d["extra_workloads"]), flush=True)
PY
}
run line_default && run line_default_again
