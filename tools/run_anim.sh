#!/bin/bash
# animate bench + summary (the line and its stderr stay in $OUT, a fresh temporary directory unless given)
OUT=${OUT:-$(mktemp -d)}
python bench.py --full --animate --no-cpu-baseline "$@" > "$OUT/b_anim.json" 2> "$OUT/b_anim.err"; tail -3 "$OUT/b_anim.err"
OUT="$OUT" python - <<PY
import json, os
d=json.loads(open(os.path.join(os.environ["OUT"], "b_anim.json")).read().strip().splitlines()[-1])
print({k:round(d[k],4) for k in ("ms_per_step","ms_per_step_sequential","host_enqueue_ms_per_step","host_wait_ms_per_step","ms_per_step_frames_posed_before_the_loop","animate_over_preposed")}, d["config"]["rays_in_bbox"], d["config"]["hit_pixels_per_frame"], d["roofline"]["frac"])
PY
