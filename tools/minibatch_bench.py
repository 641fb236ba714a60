"""What row-indexed gradients buy a learner that shuffles: tools/ppo_bench.py's world (Flock 4096 x 64, float32
obs, autoreset on with a 1 s time limit), nets (actor and critic both two hidden layers of 32) and trajectory
(K = 128 steps from rollout_policy: 33.5 M rows), and one epoch over all of them as 32 minibatches of
1,048,576 rows (with old values and the clipped value loss) in these forms, alternating rep by rep in one process:

  a       contiguous K-slices through gym_macm.ppo.ppo_grads: the parent's form and the floor. It does not shuffle.
  b       what a user of the parent must do to shuffle: index_select of the six per-row tensors per minibatch, then
          ppo_grads on the copies (block-shuffled index, the same as c's).
  b_norm  b with the copies' advantages normalised in torch, (adv - adv.mean()) / (adv.std() + 1e-8).
  c       ppo_grads(index=...) with the block = 64 index of gym_macm.ppo.minibatches.
  d       the same with block = 1, a full row shuffle.
  e       c plus adv_moments and adv_norm: to be held against b_norm.

    timeout 900 python tools/minibatch_bench.py --out profiles/ppo_minibatch/update.json

Before timing it asserts on one minibatch that c's gradient and stat bits equal b's. Prints (and writes to
--out) one JSON line: ms of every rep after one untimed pass of each form, medians, each form's spread
(max - min) / median, and whether c beats b (e beats b_norm, b beats d) by more than the two spreads added."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gym-macm_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from grad_bench import SEED, timed  # noqa: E402
from gym_macm import ppo  # noqa: E402
from gym_macm.policy import MlpCritic, MlpPolicy, gae  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

VF_CLIP = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5, help="closed-loop steps before the trajectory")
    ap.add_argument("--steps", type=int, default=128, help="K")
    ap.add_argument("--minibatches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "minibatch_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    E, N, K, W, MB = args.envs, args.agents, args.steps, args.warmup, args.minibatches
    M = K * E * N
    assert K % MB == 0, "the contiguous form slices K"
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

    # ---- one trajectory: what the collector hands the learner (ppo_bench.py's) -----------------------------
    vec = FlockVec(E, n_agents=[N], seed=SEED, device=dev, autoreset=True, time_limit=1.0)
    vec.set_policy(pol)
    vec.set_critic(crit)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED + 1)
    noise = -torch.log(-torch.log(torch.rand((K, E, N, 9), device=dev, generator=gen).clamp_(1e-12, 1 - 1e-7)))
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=dev)
    pol.act(vec.obs, out=acts[0])
    if W:
        vec.rollout_policy(acts[0], W, noise=noise[:W].contiguous())
    old_logits, vals, boot = f32(K, E, N, 9), f32(K + 1, E, N), f32(K, E, N)
    crit.value(vec.obs, out=vals[0])
    traj = vec.rollout_policy(acts, K, noise=noise, trajectory=True, logits=old_logits, values=vals, boot=boot)
    # timing only: these rows are not aligned transitions (a learner takes them from gym_macm.ppo.transitions)
    adv, ret = gae(traj["reward"], vals[:K], boot, traj["done"], 0.99, 0.95)
    obs, actions, old_values = traj["obs"], acts[1:], vals[:K]
    old_logp = ppo.log_prob(old_logits, actions)
    del noise, boot, old_logits
    assert obs.shape == (K, E, N, 4) and obs.dtype == torch.float32 and vec.status() == 0

    pol.params.requires_grad_(True)
    crit.params.requires_grad_(True)
    nets = (pol, crit)
    kw = dict(vf_clip=VF_CLIP)
    flat = [obs.view(M, 4), actions.view(M, 3), old_logp.view(M), adv.view(M), ret.view(M), old_values.view(M)]

    def zero_grads():
        for m in nets:
            m.params.grad = None

    def grads(o, a, lp, ad, r, ov, **more):
        return ppo.ppo_grads(pol, crit, o, a, lp, ad, r, old_values=ov, **kw, **more)

    g = torch.Generator()
    g.manual_seed(SEED + 2)
    mb64 = ppo.minibatches(M, MB, generator=g, block=64, device=dev)
    mb1 = ppo.minibatches(M, MB, generator=g, block=1, device=dev)
    assert all(m.numel() == M // MB for m in mb64 + mb1)

    def a_epoch():
        step = K // MB
        for i in range(MB):
            s = slice(i * step, (i + 1) * step)
            grads(obs[s], actions[s], old_logp[s], adv[s], ret[s], old_values[s])

    def gather(index):
        return [t.index_select(0, index) for t in flat]

    def b_epoch():
        for index in mb64:
            grads(*gather(index))

    def b_norm_epoch():
        for index in mb64:
            o, a, lp, ad, r, ov = gather(index)
            grads(o, a, lp, (ad - ad.mean()) / (ad.std() + 1e-8), r, ov)

    def c_epoch():
        for index in mb64:
            grads(*flat, index=index)

    def d_epoch():
        for index in mb1:
            grads(*flat, index=index)

    def e_epoch():
        for index in mb64:
            grads(*flat, index=index, adv_norm=ppo.adv_moments(flat[3], index))

    # ---- c's bits are b's on one minibatch, before anything is timed -------------------------------------
    zero_grads()
    b_stats = grads(*gather(mb64[0]))
    b_grads = [m.params.grad.clone() for m in nets]
    zero_grads()
    c_stats = grads(*flat, index=mb64[0])
    for m, bg, net in zip(nets, b_grads, ("policy", "critic")):
        assert torch.equal(m.params.grad.view(torch.int32), bg.view(torch.int32)), f"c: the {net}'s bits are b's"
    assert torch.equal(c_stats.view(torch.int64), b_stats.view(torch.int64)), "c: the stats' bits are b's"
    moments = ppo.adv_moments(flat[3], mb64[0]).cpu().tolist()

    forms = dict(a=a_epoch, b=b_epoch, b_norm=b_norm_epoch, c=c_epoch, d=d_epoch, e=e_epoch)
    res = {k: [] for k in forms}
    for rep in range(-1, args.reps):  # rep -1: one untimed pass of each form
        for k, fn in forms.items():
            zero_grads()
            ms, _ = timed(fn)
            if rep >= 0:
                res[k].append(ms)

    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in res.items()}
    faster = lambda x, y: bool(med[y] - med[x] > spread[x] * med[x] + spread[y] * med[y])
    out = dict(ms=res, median_ms=med, spread=spread,
               c_faster_than_b_by_more_than_the_spreads=faster("c", "b"),
               b_faster_than_c_by_more_than_the_spreads=faster("b", "c"),
               e_faster_than_b_norm_by_more_than_the_spreads=faster("e", "b_norm"),
               b_norm_faster_than_e_by_more_than_the_spreads=faster("b_norm", "e"),
               d_faster_than_b_by_more_than_the_spreads=faster("d", "b"),
               b_faster_than_d_by_more_than_the_spreads=faster("b", "d"),
               b_over_c=med["b"] / med["c"], b_norm_over_e=med["b_norm"] / med["e"], c_over_a=med["c"] / med["a"],
               d_over_c=med["d"] / med["c"], d_over_b=med["d"] / med["b"],
               first_minibatch_moments=dict(zip(("mean", "rstd", "std", "n"), moments)),
               first_minibatch_stats=dict(zip(ppo.STATS, c_stats.cpu().tolist())),
               rows=M, minibatches=MB, rows_per_minibatch=M // MB, envs=E, agents=N, steps=K, warmup=W, reps=args.reps,
               peak_memory_gb=torch.cuda.max_memory_allocated() / 1e9, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
