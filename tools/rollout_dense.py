"""Rollout time of a dense Flock world (lists above 128 entries: every step loads), by device events.

    MACM_LIB=... python tools/rollout_dense.py START_SPREAD
"""
import json
import os
import sys

import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-macm_amd"))
from gym_macm.vec import FlockVec
E, N, K, spread = 4096, 64, 100, float(sys.argv[1])
v = FlockVec(E, n_agents=[N], seed=3, device="cuda:0", start_spread=spread)
g = torch.Generator(device="cuda:0"); g.manual_seed(1)
acts = torch.randint(0, 3, (K, E, N, 3), dtype=torch.uint8, device="cuda:0", generator=g)
v.rollout(acts[:20])
torch.cuda.synchronize()
ts = []
for r in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); v.rollout(acts); e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) * 1000 / K)
cc = v.get_state()["contact_count"]
print(json.dumps({"spread": spread, "us_per_step": ts, "spilled": int(v.spilled()), "status": int(v.status()),
                  "list_mean": float(cc.mean()), "list_over_128": float((cc > 128).mean())}))
