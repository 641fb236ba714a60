"""What the TDM policy rollout buys: TDM 2 x 16, float32 obs, a set policy of H = 32 sampling with Gumbel
noise, one closed-loop step at 4096 envs and at the 512-env shard, over a window of K = 128 steps after
`--warmup` closed-loop steps from the same seed (the steady state), five forms alternating rep by rep in
one process:

  a  rollout_policy_traj, the policy on both teams: one launch (macm_tdm_rollout_policy_traj)
  b  the same with the policy on team 0 and bots.combat on team 1
  c  the loop step + macm_policy_tdm, two launches per step
  d  the loop step + TdmSetPolicy.torch_logits under no_grad + argmax of logits + noise: what a user
     does without this feature
  e  rollout_bots_traj: the same loop in one launch with the scripted bot on both teams, for scale

    timeout 900 python tools/tdm_policy_bench.py --out profiles/tdm_policy/steady.json

Prints (and writes to --out) one JSON line: per env count, us per step of every rep of every form after one
untimed pass of each, the medians, the spread (max - min) / median of each form's reps (the session's
noise), a/c, a/d and a/e, and whether a and c left the same state and actions (d's torch arithmetic is not
the definition's; b and e have other actors). Times are a host clock around work that ends in a device
synchronise."""
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

from gym_macm.bots import combat_actions  # noqa: E402
from gym_macm.tdm_policy import N_LOGITS, TdmSetPolicy  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402

SEED = 0x6D61636D
FORMS = ("a_rollout_policy_traj", "b_rollout_policy_team0_vs_bots", "c_loop_policy_tdm", "d_loop_torch_logits",
         "e_rollout_bots_traj")


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def bench(E, teams, H, K, W, reps, dev):
    N = sum(teams)
    torch.manual_seed(SEED)
    layers = [torch.nn.Linear(i, o).to(dev) for i, o in ((4, H), (H + 1, H), (H, N_LOGITS))]
    with torch.no_grad():  # distances reach tens of metres: keep the logits within the noise's reach
        layers[0].weight.mul_(0.3)
    pol = TdmSetPolicy.from_linear_layers(layers, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED + 1)
    u = torch.rand((K, E, N, N_LOGITS), device=dev, generator=gen).clamp_(1e-12, 1 - 1e-7)
    noise = -torch.log(-torch.log(u))
    del u
    worlds = {f: TdmWorld(tdm_config(teams), E, device=dev) for f in FORMS}
    for f in FORMS[:4]:
        worlds[f].set_policy(pol, [0] if f == FORMS[1] else None)
    act = {f: torch.empty((E, N, 4), dtype=torch.uint8, device=dev) for f in FORMS}
    rows_act = torch.empty((K + 1, E, N, 4), dtype=torch.uint8, device=dev)  # the trajectory forms share these
    rows_lg = torch.empty((K, E, N, N_LOGITS), dtype=torch.float32, device=dev)
    traj = worlds[FORMS[0]].trajectory_buffers(K)
    touts = {f: worlds[f].traj_outputs(traj) for f in (FORMS[0], FORMS[1], FORMS[4])}
    step_lg = torch.empty((E, N, N_LOGITS), dtype=torch.float32, device=dev)
    sh = torch.cuda.current_stream(dev).cuda_stream
    shp = ctypes.c_void_p(sh)
    L = worlds[FORMS[0]].L

    def start(f):
        """reset, the first actions, W closed-loop steps under the form's actors in the overwrite form (the
        forms with the same actors: the same launches, so the same state at the window's start)"""
        w, a = worlds[f], act[f]
        w.reset(SEED, 0)
        combat_actions(w.obs, w.mask, out=a)
        if f == FORMS[4]:
            if W:
                w.rollout_bots_raw(a.data_ptr(), W, sh)
            return
        pol.act(w.obs, w.mask, w.health, out=a, agents=w.policy_agents(w.policy_teams))
        for k0 in range(0, W, K):
            L.macm_tdm_rollout_policy(w.h, vp(a), min(K, W - k0), vp(noise), None, ctypes.byref(w._out), shp)

    def traj_form(f, fn):
        def go():
            rows_act[0].copy_(act[f])
            if f == FORMS[4]:
                fn(worlds[f].h, vp(rows_act), K, ctypes.byref(touts[f]), shp)
            else:
                fn(worlds[f].h, vp(rows_act), K, vp(noise), vp(rows_lg), ctypes.byref(touts[f]), shp)
            act[f].copy_(rows_act[K])
        return go

    wc, wd = worlds[FORMS[2]], worlds[FORMS[3]]
    c_step = (wc.h, vp(act[FORMS[2]]), ctypes.byref(wc._out), shp)
    c_pol = [(ctypes.byref(pol.struct()), vp(wc.obs), vp(wc.mask), vp(wc.health), 0, N, E * N, None, vp(noise[k]),
              vp(act[FORMS[2]]), vp(step_lg), shp) for k in range(K)]
    d_step = (wd.h, vp(act[FORMS[3]]), ctypes.byref(wd._out), shp)

    def form_c():
        for k in range(K):
            L.macm_tdm_step(*c_step)
            L.macm_policy_tdm(*c_pol[k])

    def form_d():
        a = act[FORMS[3]]
        with torch.no_grad():
            for k in range(K):
                L.macm_tdm_step(*d_step)
                z = pol.torch_logits(wd.obs, wd.mask, wd.health) + noise[k]
                a[..., :3] = z[..., :9].view(E, N, 3, 3).argmax(-1)
                a[..., 3] = z[..., 9:].argmax(-1)

    run = {FORMS[0]: traj_form(FORMS[0], L.macm_tdm_rollout_policy_traj),
           FORMS[1]: traj_form(FORMS[1], L.macm_tdm_rollout_policy_traj), FORMS[2]: form_c, FORMS[3]: form_d,
           FORMS[4]: traj_form(FORMS[4], L.macm_tdm_rollout_bots_traj)}
    res = {f: [] for f in FORMS}
    for rep in range(-1, reps):  # rep -1: one untimed pass of each form (first launches, cold caches)
        for f in FORMS:
            start(f)
            t = timed(run[f], K)
            if rep >= 0:
                res[f].append(t)
    sa, sc = worlds[FORMS[0]].get_state(), worlds[FORMS[2]].get_state()
    same = bool(all(np.array_equal(sa[k], sc[k]) for k in sa)) and bool(torch.equal(act[FORMS[0]], act[FORMS[2]]))
    med = {f: statistics.median(res[f]) for f in FORMS}
    taken = act[FORMS[0]].reshape(-1, 4)
    return dict(us_per_step=res, median_us_per_step=med,
                spread={f: (max(res[f]) - min(res[f])) / med[f] for f in FORMS},
                a_over_c=med[FORMS[0]] / med[FORMS[2]], a_over_d=med[FORMS[0]] / med[FORMS[3]],
                a_over_e=med[FORMS[0]] / med[FORMS[4]], b_over_e=med[FORMS[1]] / med[FORMS[4]],
                agent_steps_per_s={f: E * N / med[f] * 1e6 for f in FORMS},
                a_c_state_and_actions_equal=same,
                action_fractions=[[float((taken[:, h] == c).float().mean()) for c in range(3 if h < 3 else 2)]
                                  for h in range(4)],
                alive_fraction=float(worlds[FORMS[0]].alive.float().mean()),
                done_fraction=float(worlds[FORMS[0]].done.float().mean()),
                status=int(max(w.status() for w in worlds.values())), envs=E, teams=list(teams), hidden=H,
                warmup=W, steps=K, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 512])
    ap.add_argument("--teams", type=int, nargs="+", default=[16, 16])
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=128, help="closed-loop steps before the window")
    ap.add_argument("--steps", type=int, default=128, help="the window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tdm_policy_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0),
               runs=[bench(E, args.teams, args.hidden, args.steps, args.warmup, args.reps, dev) for E in args.envs])
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
