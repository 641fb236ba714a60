"""What the optimiser on the device and the one-call update buy a PPO learner: one epoch of 32 shuffled
minibatches (block = 64 indices of gym_macm.ppo.minibatches, normalised advantages, old values and the clipped
value loss, global-norm clip 0.5) in three forms, alternating rep by rep in one process:

  a   the parent's way: adv_moments -> ppo_grads(index=, adv_norm=) -> clip_grad_norm_ -> torch.optim.Adam.step ->
      zero_grad. No .item(), so it does not even get a KL stop.
  b   the same loop with gym_macm.ppo.Adam.step(stats) in the place of the clip and torch's Adam.
  c   gym_macm.ppo.update: the whole epoch in one call.

at two sizes, each on tools/minibatch_bench.py's world (Flock, float32 obs, autoreset on with a 1 s time limit),
nets (actor and critic both two hidden layers of 32) and a trajectory from rollout_policy:

  flagship   4096 envs x 64 agents x K = 128: 33.5 M rows, minibatches of 1,048,576 rows
  small      256 envs x 64 agents x K = 32: 524,288 rows, minibatches of 16,384 rows

    timeout 900 python tools/update_bench.py --out profiles/ppo_update/update.json

Each form has nets and an optimiser of its own, all from the same values. Before timing it asserts that c's
params, optimiser state and stats have b's bits over one epoch. Prints (and writes to --out) one JSON line: per
size the ms of every rep after one untimed pass of each form, medians, each form's spread (max - min) / median,
the median time after which the form had returned on the host (everything enqueued, nothing waited for), and
whether c beats a (b beats a, c beats b, b beats c) by more than the two spreads added."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gym-macm_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from grad_bench import SEED  # noqa: E402
from gym_macm import ppo  # noqa: E402
from gym_macm.policy import MlpCritic, MlpPolicy, gae  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

VF_CLIP, MAX_NORM, LR = 0.2, 0.5, 3e-4
SIZES = {"flagship": (4096, 64, 128), "small": (256, 64, 32)}


def timed(fn):
    """(ms until the device has finished, ms until fn returned on the host)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3


def one_size(E, N, K, W, MB, reps, dev):
    M = K * E * N
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

    # ---- one trajectory: what the collector hands the learner (minibatch_bench.py's) -------------------------
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
    flat = [obs.view(M, 4), actions.view(M, 3), old_logp.view(M), adv.view(M), ret.view(M)]
    kw = dict(old_values=old_values.view(M), vf_clip=VF_CLIP)

    g = torch.Generator()
    g.manual_seed(SEED + 2)
    mbs = ppo.minibatches(M, MB, generator=g, block=64, device=dev)
    assert all(m.numel() == M // MB for m in mbs)

    def pair():
        """Nets of their own from the trajectory's values"""
        p, c = MlpPolicy(4, 32, 2, dev), MlpCritic(4, 32, 2, dev)
        p.params.copy_(pol.params)
        c.params.copy_(crit.params)
        return p, c

    pa, ca = pair()
    pa.params.requires_grad_(True)
    ca.params.requires_grad_(True)
    topt = torch.optim.Adam([pa.params, ca.params], lr=LR)

    def a_epoch():
        for mb in mbs:
            norm = ppo.adv_moments(flat[3], mb)
            ppo.ppo_grads(pa, ca, *flat, index=mb, adv_norm=norm, **kw)
            torch.nn.utils.clip_grad_norm_([pa.params, ca.params], MAX_NORM)
            topt.step()
            topt.zero_grad()

    def b_epoch_of(opt):
        def run():
            out = []
            for mb in mbs:
                norm = ppo.adv_moments(flat[3], mb)
                stats = ppo.ppo_grads(opt.pol, opt.crit, *flat, index=mb, adv_norm=norm, **kw)
                opt.step(stats)
                opt.zero_grad()
                out.append(stats)
            return out
        return run

    def c_epoch_of(opt):
        return lambda: ppo.update(opt, *flat, minibatches=mbs, **kw)

    bopt = ppo.Adam(*pair(), lr=LR, max_grad_norm=MAX_NORM)
    copt = ppo.Adam(*pair(), lr=LR, max_grad_norm=MAX_NORM)
    b_epoch, c_epoch = b_epoch_of(bopt), c_epoch_of(copt)

    # ---- c's bits are b's over one epoch, before anything is timed -------------------------------------------
    b_stats = torch.stack(b_epoch())
    c_stats = c_epoch()
    torch.cuda.synchronize()
    assert torch.equal(c_stats.view(torch.int64), b_stats.view(torch.int64)), "c: the stats' bits are b's"
    assert torch.equal(copt.state, bopt.state), "c: the optimiser state's bits are b's"
    for x, y, net in ((copt.pol, bopt.pol, "policy"), (copt.crit, bopt.crit, "critic")):
        assert torch.equal(x.params.view(torch.int32), y.params.view(torch.int32)), f"c: the {net}'s bits are b's"
    head = bopt.info()
    assert head["t"] == MB and head["skipped_nonfinite"] == 0

    forms = dict(a=a_epoch, b=b_epoch, c=c_epoch)
    res, host = {k: [] for k in forms}, {k: [] for k in forms}
    for rep in range(-1, reps):  # rep -1: one untimed pass of each form
        for k, fn in forms.items():
            ms, host_ms = timed(fn)
            if rep >= 0:
                res[k].append(ms)
                host[k].append(host_ms)

    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in res.items()}
    faster = lambda x, y: bool(med[y] - med[x] > spread[x] * med[x] + spread[y] * med[y])
    return dict(ms=res, median_ms=med, spread=spread, host_median_ms={k: statistics.median(v) for k, v in host.items()},
                c_faster_than_a_by_more_than_the_spreads=faster("c", "a"),
                a_faster_than_c_by_more_than_the_spreads=faster("a", "c"),
                b_faster_than_a_by_more_than_the_spreads=faster("b", "a"),
                c_faster_than_b_by_more_than_the_spreads=faster("c", "b"),
                b_faster_than_c_by_more_than_the_spreads=faster("b", "c"), a_over_c=med["a"] / med["c"],
                a_over_b=med["a"] / med["b"], b_over_c=med["b"] / med["c"],
                last_minibatch_stats=dict(zip(ppo.STATS, c_stats[-1].cpu().tolist())), optimiser=head, rows=M,
                minibatches=MB, rows_per_minibatch=M // MB, envs=E, agents=N, steps=K, warmup=W, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="flagship,small")
    ap.add_argument("--warmup", type=int, default=5, help="closed-loop steps before the trajectory")
    ap.add_argument("--minibatches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "update_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    out = {}
    for name in args.sizes.split(","):
        E, N, K = SIZES[name]
        out[name] = one_size(E, N, K, args.warmup, args.minibatches, args.reps, dev)
        torch.cuda.empty_cache()
    out["peak_memory_gb"] = torch.cuda.max_memory_allocated() / 1e9
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
