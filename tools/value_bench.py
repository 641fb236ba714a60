"""What the critic inside the launch and the GAE kernel buy: Flock 4096 x 64, float32 obs, autoreset on
with a 1 s time limit (an episode ends at its 61st step: two ends per env in a 128-step trajectory), actor
and critic both two hidden layers of 32, sampling with Gumbel noise, trajectories of K = 128 steps after
`--warmup` closed-loop steps from the same seed. Forms alternating rep by rep in one process:

  a  rollout_policy with values and boot (macm_world_rollout_policy_value_traj), then macm_gae: the feature
  b  rollout_policy as before (macm_world_rollout_policy_traj), then the same critic as a batched torch MLP
     over the stored [K, E, N, OD] obs plus final_obs, then GAE as a torch loop over K: what a user does
     without the feature. b cannot bootstrap more than one end per env: final_obs holds an env's last end only,
     so every earlier end takes V of the new episode's first observation.
  c  rollout_policy alone: against the rollout part of a, the price of the critic inside the launch
  d  macm_gae alone against the torch GAE loop alone, on the same buffers (21 B per agent-step)

    timeout 900 python tools/value_bench.py --warmup 5   --out profiles/policy_value/window.json
    timeout 900 python tools/value_bench.py --warmup 300 --out profiles/policy_value/steady.json

Before timing, a's values, boot, adv and ret are asserted equal, bit for bit, to the per-step loop's
(step, macm_value_flock, reset_envs(done), macm_policy_flock, macm_value_flock; then macm_gae) and, on a
seeded subset of columns, to tests/value_ref.py. Prints (and writes to --out) one JSON line: us per step of
every rep after one untimed pass of each form, medians, ratios and each form's spread (max - min) / median."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gym-macm_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import policy_ref as pr  # noqa: E402
import value_ref as vr  # noqa: E402
from gym_macm.policy import MlpCritic, MlpPolicy, gae  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

SEED = 0x6D61636D
HBM_PEAK = 8.0e12  # B/s, MI355X


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def torch_gae(reward, values, boot, done, gamma, lam):
    K = reward.shape[0]
    adv = torch.empty_like(reward)
    carry = torch.zeros_like(reward[0])
    for k in range(K - 1, -1, -1):
        delta = reward[k] + gamma * boot[k] - values[k]
        carry = delta + gamma * lam * carry * (1.0 - done[k].float()).unsqueeze(-1)
        adv[k] = carry
    return adv, adv + values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5, help="closed-loop steps before the trajectory")
    ap.add_argument("--steps", type=int, default=128, help="K")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "value_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    E, N, K, W = args.envs, args.agents, args.steps, args.warmup
    gamma, lam = 0.99, 0.95
    torch.manual_seed(SEED)

    def mlp(n_out):
        dims = [4, 32, 32, n_out]
        layers = [torch.nn.Linear(i, o).to(dev) for i, o in zip(dims[:-1], dims[1:])]
        with torch.no_grad():
            for lin in layers:
                lin.weight.mul_(0.3)
        return layers

    p_layers, v_layers = mlp(9), mlp(1)
    pol = MlpPolicy.from_linear_layers(p_layers, device=dev)
    crit = MlpCritic.from_linear_layers(v_layers, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED + 1)
    noise = -torch.log(-torch.log(torch.rand((K, E, N, 9), device=dev, generator=gen).clamp_(1e-12, 1 - 1e-7)))

    vecs = []

    def world(final=True):
        v = FlockVec(E, n_agents=[N], seed=SEED, device=dev, autoreset=True, time_limit=args.time_limit)
        vecs.append(v)
        v.set_policy(pol)
        v.set_critic(crit)
        if final:
            v.world.set_final_outputs(True)
        return v.world

    wa, wb, wc = world(), world(), world()
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    acts = {f: torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=dev) for f in "abc"}
    trajs = {f: w.trajectory_buffers(K) for f, w in (("a", wa), ("b", wb), ("c", wc))}
    touts = {f: w._traj_out(trajs[f], K) for f, w in (("a", wa), ("b", wb), ("c", wc))}
    vals, boot, adv, ret = f32(K + 1, E, N), f32(K, E, N), f32(K, E, N), f32(K, E, N)
    sh = torch.cuda.current_stream(dev).cuda_stream
    shp = ctypes.c_void_p(sh)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    L = wa.L

    def start(w, act):
        """reset, the first actions, W closed-loop steps: every form starts its trajectory from the same state"""
        w.reset(SEED, 0)
        if w.final_ends is not None:
            w.final_ends.zero_()
        a0 = act[0]
        pol.act(w.obs, out=a0)
        for k0 in range(0, W, K):
            w.rollout_policy_raw(a0.data_ptr(), min(K, W - k0), noise.data_ptr(), 0, sh)

    def a_rollout():
        crit.value(wa.obs, out=vals[0])
        L.macm_world_rollout_policy_value_traj(wa.h, vp(acts["a"]), K, vp(noise), None, vp(vals), vp(boot),
                                               ctypes.byref(touts["a"]), shp)

    def a_gae():
        L.macm_gae(vp(trajs["a"]["reward"]), vp(vals), vp(boot), vp(trajs["a"]["done"]), K, E, N, gamma, lam, vp(adv),
                   vp(ret), shp)

    def torch_critic(obs):
        h = obs
        for lin in v_layers[:-1]:
            h = torch.relu(lin(h))
        return v_layers[-1](h).squeeze(-1)

    b_out = {}

    def b_rollout(w=wb, f="b"):
        L.macm_world_rollout_policy_traj(w.h, vp(acts[f]), K, vp(noise), None, ctypes.byref(touts[f]), shp)

    def b_values():
        with torch.no_grad():
            t = trajs["b"]
            v = torch.cat([torch_critic(b_out["obs0"]).unsqueeze(0), torch_critic(t["obs"])])  # [K + 1, E, N]
            bt = v[1:].clone()
            # the last end of each env bootstraps from final_obs; earlier ends cannot
            done = t["done"].bool()
            ended = done.any(0)
            last = (K - 1) - done.flip(0).float().argmax(0)
            e = torch.nonzero(ended).squeeze(-1)
            bt[last[e], e] = torch_critic(wb.final_obs[e])
            b_out["v"], b_out["boot"] = v, bt

    def b_gae():
        with torch.no_grad():
            b_out["adv"], b_out["ret"] = torch_gae(trajs["b"]["reward"], b_out["v"][:K], b_out["boot"], trajs["b"]["done"],
                                                   gamma, lam)

    # ---- a's results against the per-step loop and value_ref, before anything is timed ----------------
    start(wa, acts["a"])
    a_rollout()
    a_gae()
    loop = world(final=False)
    lact = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=dev)
    start(loop, lact)  # the warmup as the other worlds', then the loop resets its envs itself
    loop.set_autoreset(False)
    cols = np.random.default_rng(SEED).choice(E * N, 64, replace=False)
    ce, cn = torch.as_tensor(cols // N, device=dev), torch.as_tensor(cols % N, device=dev)
    lv, lb, lr, ld = f32(K + 1, E, N), f32(K, E, N), f32(K, E, N), torch.empty((K, E), dtype=torch.uint8, device=dev)
    obs_pre, obs_post = [], [loop.obs[ce, cn].clone()]
    crit.value(loop.obs, out=lv[0])
    act = lact[0].clone()
    for k in range(K):
        loop.step(act)
        crit.value(loop.obs, out=lb[k])
        obs_pre.append(loop.obs[ce, cn].clone())
        lr[k], ld[k] = loop.reward, loop.done
        loop.reset_envs(loop.done.clone())
        pol.act(loop.obs, noise=noise[k], out=act)
        crit.value(loop.obs, out=lv[k + 1])
        obs_post.append(loop.obs[ce, cn].clone())
    ladv, lret = gae(lr, lv[:K], lb, ld, gamma, lam)
    ib = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(act, acts["a"][K]) and torch.equal(ld, trajs["a"]["done"]), "a: the loop's actions and done"
    for name, got, want in (("values", vals, lv), ("boot", boot, lb), ("adv", adv, ladv), ("ret", ret, lret)):
        assert torch.equal(ib(got), ib(want)), f"a: {name} differs from the per-step loop's"
    vparams = crit.params.cpu().numpy()
    want_b = vr.value_of(vparams, 4, 32, 2, torch.stack(obs_pre).cpu().numpy())  # [K, 64]
    want_v = vr.value_of(vparams, 4, 32, 2, torch.stack(obs_post).cpu().numpy())  # [K + 1, 64]
    assert pr.same_bits(boot[:, ce, cn].cpu().numpy(), want_b).all(), "a: boot differs from value_ref"
    assert pr.same_bits(vals[:, ce, cn].cpu().numpy(), want_v).all(), "a: values differ from value_ref"
    # value_ref.gae wants [K, E, N] with done [K, E]: each chosen column as an env of one agent
    wadv, wret = vr.gae(lr[:, ce, cn].cpu().numpy()[:, :, None], want_v[:K, :, None], want_b[:, :, None],
                        ld[:, ce].cpu().numpy(), gamma, lam)
    assert pr.same_bits(adv[:, ce, cn].cpu().numpy(), wadv[:, :, 0]).all(), "a: adv differs from value_ref"
    assert pr.same_bits(ret[:, ce, cn].cpu().numpy(), wret[:, :, 0]).all(), "a: ret differs from value_ref"
    ends_per_env = ld.sum(0)
    del lv, lb, lr, lact

    # ---- timing -------------------------------------------------------------------------------------------
    parts = ("a_rollout", "a_gae", "b_rollout", "b_torch_critic", "b_torch_gae", "c_rollout", "d_gae_kernel",
             "d_torch_gae")
    res = {p: [] for p in parts}
    for rep in range(-1, args.reps):  # rep -1: one untimed pass of each form
        t = {}
        start(wa, acts["a"])
        t["a_rollout"], t["a_gae"] = timed(a_rollout), timed(a_gae)
        start(wb, acts["b"])
        b_out["obs0"] = wb.obs.clone()
        t["b_rollout"], t["b_torch_critic"], t["b_torch_gae"] = timed(b_rollout), timed(b_values), timed(b_gae)
        start(wc, acts["c"])
        t["c_rollout"] = timed(lambda: b_rollout(wc, "c"))
        t["d_gae_kernel"] = timed(a_gae)  # the same buffers for both
        with torch.no_grad():
            t["d_torch_gae"] = timed(lambda: torch_gae(trajs["a"]["reward"], vals[:K], boot, trajs["a"]["done"], gamma, lam))
        if rep >= 0:
            for p in parts:
                res[p].append(t[p])
    med = {p: statistics.median(res[p]) for p in parts}
    a_total = [x + y for x, y in zip(res["a_rollout"], res["a_gae"])]
    b_total = [x + y + z for x, y, z in zip(res["b_rollout"], res["b_torch_critic"], res["b_torch_gae"])]
    ma, mb = statistics.median(a_total), statistics.median(b_total)
    spread = {p: (max(res[p]) - min(res[p])) / med[p] for p in parts}
    spread["a_total"] = (max(a_total) - min(a_total)) / ma
    spread["b_total"] = (max(b_total) - min(b_total)) / mb
    gae_bps = 21.0 * K * E * N / (med["d_gae_kernel"] * 1e-6)
    # how far b's advantages are from a's: the ends it cannot bootstrap, and torch's other arithmetic
    dadv = (b_out["adv"] - adv).abs()
    out = dict(us=res, median_us=med, a_total_us=ma, b_total_us=mb, spread=spread,
               us_per_step=dict(a=ma / K, b=mb / K, a_rollout=med["a_rollout"] / K, c_rollout=med["c_rollout"] / K),
               a_over_b=ma / mb, a_beats_b_by_more_than_the_spread=bool(mb - ma > max(spread["a_total"] * ma, spread["b_total"] * mb)),
               critic_in_launch_over_plain=med["a_rollout"] / med["c_rollout"],
               gae_kernel_over_torch=med["d_gae_kernel"] / med["d_torch_gae"],
               gae_beats_torch_by_more_than_the_spread=bool(
                   med["d_torch_gae"] - med["d_gae_kernel"] > max(spread["d_gae_kernel"] * med["d_gae_kernel"],
                                                                  spread["d_torch_gae"] * med["d_torch_gae"])),
               gae_bytes_per_s=gae_bps, gae_share_of_hbm_peak=gae_bps / HBM_PEAK,
               ends_per_env=[int(ends_per_env.min()), int(ends_per_env.max())],
               b_cannot_bootstrap_more_than_one_end_per_env=True,
               b_adv_max_abs_diff_from_a=float(dadv.max()), b_adv_rows_off_by_more_than_1e_3=int((dadv > 1e-3).sum()),
               a_equals_loop_and_value_ref=True,
               status=int(max(w.status() for w in (wa, wb, wc))), envs=E, agents=N, warmup=W, steps=K, reps=args.reps,
               time_limit=args.time_limit, device=torch.cuda.get_device_name(0))
    print("b cannot bootstrap more than one end per env (final_obs keeps the last end only); "
          f"ends per env in this trajectory: {out['ends_per_env']}", file=sys.stderr)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
