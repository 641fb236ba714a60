"""What the in-launch autoreset buys: the autoreset rollout (macm_*_set_autoreset, one launch on the
wave path) against the only form there was without it, the per-step loop `step -> reset_envs(done)
[-> bots]`, over the same window from the same seed, alternating the two forms rep by rep in one
process. One case per invocation, so that a driver gives every GPU step its own time limit:

    timeout 300 python tools/autoreset_ab.py --case a --envs 512  --out profiles/autoreset/a_shard.json
    timeout 300 python tools/autoreset_ab.py --case a --envs 4096 --out profiles/autoreset/a_c4.json
    timeout 300 python tools/autoreset_ab.py --case b --out profiles/autoreset/b.json
    timeout 300 python tools/autoreset_ab.py --case c --out profiles/autoreset/c.json

  a  TDM 2 x 16, bots closed loop, `--steps` steps from the reset (episodes end by combat inside the
     window: the JSON counts the done flags): rollout_bots with autoreset on vs the loop
  b  Flock 64 x 4096, actions given, a 20-step trajectory window after `--warmup` steps with
     time_limit set so that every env ends once inside it: rollout_traj with autoreset on vs the loop
  c  b with no env ending in the window: rollout_traj with autoreset on vs off (the price of the
     variant's extra code when it is never taken)
Prints (and writes to --out) one JSON line: us per step of every rep of both forms, the ratio of the
medians, the spread (max - min) / median of each form's reps after one untimed pass of each (the
session's noise), and whether both forms left the same state."""
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

from gym_macm import _abi  # noqa: E402

SEED = 0x6D61636D


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def states_equal(a, b):
    sa, sb = a.get_state(), b.get_state()
    return bool(all(np.array_equal(sa[k], sb[k]) for k in sa))


def case_a(args, dev):
    from gym_macm.bots import combat_actions
    from gym_macm.tdm_world import TdmWorld, tdm_config
    E, N, K = args.envs, 32, args.steps
    loop_w = TdmWorld(tdm_config([16, 16]), E, device=dev)
    roll_w = TdmWorld(tdm_config([16, 16]), E, device=dev, autoreset=True)
    L, sh = loop_w.L, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    act_l = torch.empty((E, N, 4), dtype=torch.uint8, device=dev)
    act_r = torch.empty_like(act_l)
    out = ctypes.byref(loop_w._out)
    step_args = (loop_w.h, vp(act_l), out, sh)
    reset_args = (loop_w.h, vp(loop_w.done), out, sh)
    bots_args = (vp(loop_w.obs), vp(loop_w.mask), 1 if loop_w.cfg.obs_f64 else 0, N, E * N, vp(act_l), sh)

    def loop():
        for _ in range(K):
            L.macm_tdm_step(*step_args)
            L.macm_tdm_reset_envs(*reset_args)
            L.macm_bots_combat(*bots_args)

    def start(w, act):
        w.reset(SEED, 0)
        combat_actions(w.obs, w.mask, out=act)

    res = {"loop_us_per_step": [], "rollout_us_per_step": []}
    for rep in range(-1, args.reps):  # rep -1: one untimed pass of each form (first launches, cold caches)
        start(loop_w, act_l)
        c0 = loop_w.counters().copy()
        t = timed(loop, K)
        res["done_flags_in_window"] = int(loop_w.counters()[3] - c0[3])
        start(roll_w, act_r)
        r = timed(lambda: roll_w.rollout_bots_raw(act_r.data_ptr(), K, sh.value), K)
        if rep >= 0:
            res["loop_us_per_step"].append(t)
            res["rollout_us_per_step"].append(r)
    res["state_equal"] = states_equal(loop_w, roll_w) and bool(torch.equal(act_l, act_r))
    res["status"] = int(roll_w.status()) | int(loop_w.status())
    return res


def case_bc(args, dev, ending):
    from gym_macm.vec import FlockVec
    E, N, W, K = args.envs, 64, args.warmup, 20
    # done when time_passed = n / 60 > time_limit: at step W + 10 of every env, once in the window
    kw = {"time_limit": (W + 9.5) / 60.0} if ending else {}
    a = FlockVec(E, n_agents=[N], seed=SEED, device=dev, **kw).world  # b: the loop; c: autoreset off
    b = FlockVec(E, n_agents=[N], seed=SEED, device=dev, autoreset=True, **kw).world
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED + 1)
    acts = torch.randint(0, 3, (W + K, E, N, 3), dtype=torch.uint8, device=dev, generator=gen)
    stride, base = acts[0].numel(), acts.data_ptr()
    sh = torch.cuda.current_stream(dev).cuda_stream
    ta, tb = a.trajectory_buffers(K), b.trajectory_buffers(K)
    L, shp = a.L, ctypes.c_void_p(sh)
    rows = [_abi.MacmOutputs(*[vp(ta[f][k]) for f in ("obs", "nbr_id", "reward", "collided", "done")]) for k in range(K)]
    obs_rows = [_abi.MacmOutputs(vp(ta["obs"][k]), vp(ta["nbr_id"][k]), None, None, None) for k in range(K)]
    calls = [((a.h, ctypes.c_void_p(base + (W + k) * stride), ctypes.byref(rows[k]), shp),
              (a.h, vp(ta["done"][k]), ctypes.byref(obs_rows[k]), shp)) for k in range(K)]

    def loop():
        for sa, ra in calls:
            L.macm_world_step(*sa)
            L.macm_world_reset_envs(*ra)

    def warm(w):
        w.reset(SEED, 0)
        for k in range(W):
            w.step_raw(base + k * stride, sh)

    first = "loop_us_per_step" if ending else "off_us_per_step"
    res = {first: [], "rollout_us_per_step": []}
    for rep in range(-1, args.reps):  # rep -1: one untimed pass of each form (first launches, cold caches)
        warm(a)
        t = timed(loop if ending else (lambda: a.rollout_traj_raw(base + W * stride, K, ta, sh)), K)
        warm(b)
        r = timed(lambda: b.rollout_traj_raw(base + W * stride, K, tb, sh), K)
        if rep >= 0:
            res[first].append(t)
            res["rollout_us_per_step"].append(r)
    res["done_flags_in_window"] = int(tb["done"].sum())
    res["state_equal"] = states_equal(a, b) and all(bool(torch.equal(ta[f], tb[f])) for f in ta)
    res["status"] = int(a.status()) | int(b.status())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("a", "b", "c"), required=True)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400, help="case a: the window, from the reset")
    ap.add_argument("--warmup", type=int, default=5, help="cases b, c: steps before the 20-step window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = case_a(args, dev) if args.case == "a" else case_bc(args, dev, args.case == "b")
    base_key = [k for k in res if k.endswith("_us_per_step") and k != "rollout_us_per_step"][0]
    mb, mr = statistics.median(res[base_key]), statistics.median(res["rollout_us_per_step"])
    res.update(case=args.case, envs=args.envs, reps=args.reps, warmup=args.warmup,
               steps=args.steps if args.case == "a" else 20, device=torch.cuda.get_device_name(0),
               ratio_baseline_over_rollout=mb / mr,
               spread={k: (max(res[k]) - min(res[k])) / statistics.median(res[k])
                       for k in (base_key, "rollout_us_per_step")})
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
