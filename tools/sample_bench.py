"""What drawing the Gumbel noise inside the launch buys: Flock 4096 x 64, float32 obs, autoreset on with a
1 s time limit, actor and critic both two hidden layers of 32, trajectories of K = 128 steps with logits,
values and boot (macm_world_rollout_policy_value_traj) after `--warmup` closed-loop steps from the same
seed. Three forms, alternating rep by rep in one process, each on a world of its own:

  a  what a user did before: torch makes the [K, E, N, 9] noise (rand, two logs, two negations), then
     rollout_policy(noise=). The two parts are timed separately; the total is their sum.
  b  gym_macm.policy.gumbel_noise (macm_policy_noise, one launch), then rollout_policy(noise=)
  c  a world with set_sampling: one launch, no noise tensor

    timeout 900 python tools/sample_bench.py --warmup 300 --out profiles/policy_sample/steady.json

The claim is c's total below a's by more than the sum of the two spreads; c's launch against b's launch is
the in-launch price of the draw (three Philox calls and eighteen float64 logs per agent-step against 36 B
read). Before timing, c's trajectory is asserted equal, bit for bit, to b's (the same seed and decision
index). Prints (and writes to --out) one JSON line: us of every rep after one untimed pass of each form,
medians, each form's spread (max - min) / median, and the bytes of the noise tensor c does not need."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gym-macm_amd"))

import torch  # noqa: E402

from gym_macm.policy import MlpCritic, MlpPolicy, gumbel_noise  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

SEED = 0x6D61636D
NOISE_SEED = 0x5EED_0000_0001


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=300, help="closed-loop steps before the trajectory")
    ap.add_argument("--steps", type=int, default=128, help="K")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--time-limit", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    E, N, K, W = args.envs, args.agents, args.steps, args.warmup
    torch.manual_seed(SEED)

    def mlp(n_out):
        dims = [4, 32, 32, n_out]
        layers = [torch.nn.Linear(i, o).to(dev) for i, o in zip(dims[:-1], dims[1:])]
        with torch.no_grad():
            for lin in layers:
                lin.weight.mul_(0.3)
        return layers

    pol = MlpPolicy.from_linear_layers(mlp(9), device=dev)
    crit = MlpCritic.from_linear_layers(mlp(1), device=dev)
    gen = torch.Generator(device=dev)

    forms = "abc"
    worlds, acts, trajs, lg, vals, boot = {}, {}, {}, {}, {}, {}
    for f in forms:
        v = FlockVec(E, n_agents=[N], seed=SEED, device=dev, autoreset=True, time_limit=args.time_limit)
        v.set_policy(pol)
        v.set_critic(crit)
        worlds[f] = v
        acts[f] = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=dev)
        trajs[f] = v.world.trajectory_buffers(K)
        lg[f] = torch.empty((K, E, N, 9), dtype=torch.float32, device=dev)
        vals[f] = torch.empty((K + 1, E, N), dtype=torch.float32, device=dev)
        boot[f] = torch.empty((K, E, N), dtype=torch.float32, device=dev)

    def start(f):
        """reset, the first actions, W sampled closed-loop steps: every form starts its trajectory from the same
        state, and the measured launch's first decision index is W + 1"""
        v = worlds[f]
        v.world.reset(SEED, 0)
        v.set_sampling(NOISE_SEED, 1)
        a0 = acts[f][0]
        pol.act(v.obs, seed=NOISE_SEED, decision=0, out=a0)
        for k0 in range(0, W, K):
            v.rollout_policy(a0, min(K, W - k0))
        assert v.sampling == (NOISE_SEED, W + 1)
        if f != "c":
            v.set_sampling(None)
        crit.value(v.obs, out=vals[f][0])

    def launch(f, noise):
        worlds[f].rollout_policy(acts[f], K, noise=noise, trajectory=True, traj=trajs[f], logits=lg[f], values=vals[f],
                                 boot=boot[f])

    def torch_noise():
        u = torch.rand((K, E, N, 9), device=dev, generator=gen)
        return -torch.log(-torch.log(u))

    def lib_noise():
        return gumbel_noise(NOISE_SEED, W + 1, K, (E, N), dev)

    # ---- c equals b, bit for bit, before anything is timed ------------------------------------------------
    gen.manual_seed(SEED + 1)
    start("b")
    launch("b", lib_noise())
    start("c")
    launch("c", None)
    torch.cuda.synchronize()
    ib = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(acts["b"], acts["c"]), "c: the actions differ from b's"
    for name, d in (("logits", lg), ("values", vals), ("boot", boot)):
        assert torch.equal(ib(d["b"]), ib(d["c"])), f"c: {name} differ from b's"
    for k in trajs["b"]:
        assert torch.equal(trajs["b"][k], trajs["c"][k]), f"c: traj[{k}] differs from b's"
    ends = trajs["c"]["done"].sum(0)

    # ---- timing -------------------------------------------------------------------------------------------
    parts = ("a_noise", "a_launch", "b_noise", "b_launch", "c_launch")
    res = {p: [] for p in parts}
    for rep in range(-1, args.reps):  # rep -1: one untimed pass of each form
        t = {}
        start("a")
        noise, t["a_noise"] = timed(torch_noise)
        _, t["a_launch"] = timed(lambda: launch("a", noise))
        del noise
        start("b")
        noise, t["b_noise"] = timed(lib_noise)
        _, t["b_launch"] = timed(lambda: launch("b", noise))
        del noise
        start("c")
        _, t["c_launch"] = timed(lambda: launch("c", None))
        if rep >= 0:
            for p in parts:
                res[p].append(t[p])
    med = {p: statistics.median(res[p]) for p in parts}
    spread = {p: (max(res[p]) - min(res[p])) / med[p] for p in parts}
    tot = {"a": [x + y for x, y in zip(res["a_noise"], res["a_launch"])],
           "b": [x + y for x, y in zip(res["b_noise"], res["b_launch"])], "c": res["c_launch"]}
    mtot = {f: statistics.median(tot[f]) for f in forms}
    stot = {f: (max(tot[f]) - min(tot[f])) / mtot[f] for f in forms}
    out = dict(us=res, median_us=med, spread=spread, total_us=mtot, total_spread=stot,
               us_per_step={f: mtot[f] / K for f in forms},
               launch_us_per_step=dict(a=med["a_launch"] / K, b=med["b_launch"] / K, c=med["c_launch"] / K),
               c_over_a=mtot["c"] / mtot["a"], c_over_b=mtot["c"] / mtot["b"],
               c_beats_a_by_more_than_the_spreads=bool(mtot["a"] - mtot["c"] > stot["a"] * mtot["a"] + stot["c"] * mtot["c"]),
               c_beats_b_by_more_than_the_spreads=bool(mtot["b"] - mtot["c"] > stot["b"] * mtot["b"] + stot["c"] * mtot["c"]),
               draw_in_launch_over_noise_read=med["c_launch"] / med["b_launch"],
               draw_in_launch_us_per_step=(med["c_launch"] - med["b_launch"]) / K,
               noise_bytes_not_needed=K * E * N * 9 * 4, c_equals_b_bit_for_bit=True,
               ends_per_env=[int(ends.min()), int(ends.max())],
               status=int(max(worlds[f].status() for f in forms)), envs=E, agents=N, warmup=W, steps=K, reps=args.reps,
               time_limit=args.time_limit, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
