#!/bin/bash
# A/B of ray-cast kernels on one box: runs bench.py --full (steady state, stage times, roofline) once per GMUPT_TRAVERSAL value given,
# writes $AB_OUT/ab_<mode>.json (default: ab_out/)
# usage: tools/ab_cast.sh cast0 wide [-- extra bench args]
set -e
OUT=${AB_OUT:-ab_out}
mkdir -p "$OUT"
modes=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do modes+=("$1"); shift; done
[ "$1" == "--" ] && shift
for m in "${modes[@]}"; do
  GMUPT_TRAVERSAL=$m python bench.py --full --no-cpu-baseline --no-full-frame --no-config5 "$@" > "$OUT/ab_$m.json" 2> "$OUT/ab_$m.err" || { echo "bench failed for $m"; tail -5 "$OUT/ab_$m.err"; exit 1; }
  python - "$m" "$OUT" <<'PY'
import json, sys
m, out = sys.argv[1], sys.argv[2]
j = json.loads(open("%s/ab_%s.json" % (out, m)).read().strip().splitlines()[-1])
r = j.get("roofline") or {}
print("         census %s  simd %s  redo/launch %s  general %s" % (r.get("lane_census"), r.get("simd_efficiency"), r.get("redo_rays_per_launch"), r.get("general_slab_test_share")))
print("%-8s value %.3f Mpaths/s  ms/step %.4f  raycast %.4f  logic %.4f  material %.4f  kernel %s  inner/ray %s  lds_top %s" % (
    m, j["value"], j["ms_per_step"], j["stage_ms"]["raycast"], j["stage_ms"]["logic"], j["stage_ms"]["material"], r.get("kernel"), r.get("inner_per_ray"), r.get("lds_top_share_of_node_visits")))
PY
done
