"""The binding's own cost around a host function: 10^5 Camera.update(0.0) + Camera.buffer calls, five times; no device involved.
Run from the root of the tree to measure: python profiles/capi_binding_split/wrapper_loop.py  (prints one JSON line)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import gmupt_pkg  # noqa: E402

capi = gmupt_pkg.load().capi
cam = capi.Camera(64, 36)
N = 100000
times = []
for _ in range(5):
    t0 = time.perf_counter()
    for _ in range(N):
        cam.update(0.0)
        cam.buffer
    times.append(time.perf_counter() - t0)
cam.close()
print(json.dumps({"calls": N, "seconds": [round(t, 4) for t in times], "best": round(min(times), 4), "spread": round(max(times) - min(times), 4),
                  "ns_per_pair_best": round(min(times) / N * 1e9, 1)}))
