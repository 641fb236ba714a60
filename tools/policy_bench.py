"""What the policy rollout buys: Flock 4096 x 64, float32 obs, an MLP policy of two hidden layers of 32,
sampling with Gumbel noise, over a 20-step window after `--warmup` closed-loop steps from the same seed,
four forms alternating rep by rep in one process:

  a  rollout_policy: one launch (macm_world_rollout_policy)
  b  the loop step + macm_policy_flock, two launches per step
  c  the loop step + the same MLP in torch (nn.Linear float32, relu, argmax of logits + noise):
     what a user does without this feature
  d  rollout_bots: the same loop in one launch with the scripted bot, an actor that costs nothing

    timeout 600 python tools/policy_bench.py --warmup 5   --out profiles/policy_rollout/window.json
    timeout 600 python tools/policy_bench.py --warmup 300 --out profiles/policy_rollout/steady.json

--warmup 5 is the driver's window (steps 6 to 25), --warmup 300 the steady state. Prints (and writes to
--out) one JSON line: us per step of every rep of every form after one untimed pass of each, the medians,
their ratios, the spread (max - min) / median of each form's reps (the session's noise), and whether a
and b left the same state and actions (c's torch arithmetic is not the definition's, d's actor is another)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gym-macm_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_macm.bots import flock_actions  # noqa: E402
from gym_macm.policy import MlpPolicy  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

SEED = 0x6D61636D
FORMS = ("a_rollout_policy", "b_loop_policy_flock", "c_loop_torch_mlp", "d_rollout_bots")


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--n-hidden", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5, help="closed-loop steps before the window")
    ap.add_argument("--steps", type=int, default=20, help="the window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "policy_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    E, N, K, W = args.envs, args.agents, args.steps, args.warmup
    torch.manual_seed(SEED)
    dims = [4] + [args.hidden] * args.n_hidden + [9]
    layers = [torch.nn.Linear(i, o).to(dev) for i, o in zip(dims[:-1], dims[1:])]
    with torch.no_grad():  # Flock's distances reach tens of metres: keep the logits within the noise's reach
        for lin in layers:
            lin.weight.mul_(0.3)
    pol = MlpPolicy.from_linear_layers(layers, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED + 1)
    u = torch.rand((K, E, N, 9), device=dev, generator=gen).clamp_(1e-12, 1 - 1e-7)
    noise = -torch.log(-torch.log(u))
    del u
    worlds = {f: FlockVec(E, n_agents=[N], seed=SEED, device=dev).world for f in FORMS}
    acts = {f: torch.empty((E, N, 3), dtype=torch.uint8, device=dev) for f in FORMS}
    for f in FORMS[:3]:
        worlds[f].set_policy(pol)
    sh = torch.cuda.current_stream(dev).cuda_stream
    shp = ctypes.c_void_p(sh)
    L = worlds[FORMS[0]].L
    rows = E * N

    def start(f):
        """reset, the first actions, W closed-loop steps under the form's actor (the policy forms: the
        same launches, so the same state at the window's start)"""
        w, act = worlds[f], acts[f]
        w.reset(SEED, 0)
        if f == FORMS[3]:
            flock_actions(w.obs, out=act)
            if W:
                w.rollout_bots_raw(act.data_ptr(), W, sh)
            return
        pol.act(w.obs, out=act)
        for k0 in range(0, W, K):
            w.rollout_policy_raw(act.data_ptr(), min(K, W - k0), noise.data_ptr(), 0, sh)

    wb, wc = worlds[FORMS[1]], worlds[FORMS[2]]
    b_step = (wb.h, vp(acts[FORMS[1]]), ctypes.byref(wb._out), shp)
    b_pol = [(ctypes.byref(pol.struct()), vp(wb.obs), 0, rows, vp(noise[k]), vp(acts[FORMS[1]]), None, shp)
             for k in range(K)]
    c_step = (wc.h, vp(acts[FORMS[2]]), ctypes.byref(wc._out), shp)

    def form_a():
        worlds[FORMS[0]].rollout_policy_raw(acts[FORMS[0]].data_ptr(), K, noise.data_ptr(), 0, sh)

    def form_b():
        for k in range(K):
            L.macm_world_step(*b_step)
            L.macm_policy_flock(*b_pol[k])

    def form_c():
        act = acts[FORMS[2]]
        with torch.no_grad():
            for k in range(K):
                L.macm_world_step(*c_step)
                h = wc.obs
                for lin in layers[:-1]:
                    h = torch.relu(lin(h))
                z = layers[-1](h) + noise[k]
                act.copy_(z.view(E, N, 3, 3).argmax(-1))

    def form_d():
        worlds[FORMS[3]].rollout_bots_raw(acts[FORMS[3]].data_ptr(), K, sh)

    run = dict(zip(FORMS, (form_a, form_b, form_c, form_d)))
    res = {f: [] for f in FORMS}
    for rep in range(-1, args.reps):  # rep -1: one untimed pass of each form (first launches, cold caches)
        for f in FORMS:
            start(f)
            t = timed(run[f], K)
            if rep >= 0:
                res[f].append(t)
    sa, sb = worlds[FORMS[0]].get_state(), worlds[FORMS[1]].get_state()
    same = bool(all(np.array_equal(sa[k], sb[k]) for k in sa)) and bool(torch.equal(acts[FORMS[0]], acts[FORMS[1]]))
    med = {f: statistics.median(res[f]) for f in FORMS}
    taken = acts[FORMS[0]].reshape(-1, 3)
    out = dict(us_per_step=res, median_us_per_step=med,
               spread={f: (max(res[f]) - min(res[f])) / med[f] for f in FORMS},
               a_over_b=med[FORMS[0]] / med[FORMS[1]], a_over_c=med[FORMS[0]] / med[FORMS[2]],
               a_over_d=med[FORMS[0]] / med[FORMS[3]],
               agent_steps_per_s={f: E * N / med[f] * 1e6 for f in FORMS},
               a_b_state_and_actions_equal=same,
               action_fractions=[[float((taken[:, h] == c).float().mean()) for c in range(3)] for h in range(3)],
               status=int(max(w.status() for w in worlds.values())),
               envs=E, agents=N, hidden=args.hidden, n_hidden=args.n_hidden, warmup=W, steps=K, reps=args.reps,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
