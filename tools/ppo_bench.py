"""What the PPO loss on device buys a learner: tools/grad_bench.py's world (Flock 4096 x 64, float32 obs, autoreset
on with a 1 s time limit), nets (actor and critic both two hidden layers of 32) and trajectory (K = 128 steps
from rollout_policy: 33.5 M rows), and one update pass over all of them in four forms, alternating rep by rep
in one process:

  a  forward, the torch loss of grad_bench.py, backward through MlpPolicy.forward / MlpCritic.forward: the
     parent's form, and the yardstick.
  b  log_prob once, then forward + gym_macm.ppo.ppo_loss + backward: the loss in two launches, the logits and
     dL/dlogits still in memory.
  c  gym_macm.ppo.ppo_grads: the loss inside the gradient launches.
  d  macm_ppo_loss alone (dL/dlogits, dL/dvalues and stats in one call): its bytes per row over its time.

    timeout 900 python tools/ppo_bench.py --out profiles/ppo_loss/update.json

Before timing it asserts that c's gradient bits equal b's on all rows, that b's gradients on a seeded subset
of rows are within grad_ref.tol of a's, and that the first epoch's approx_kl is 0. Prints (and writes to
--out) one JSON line: ms of every rep after one untimed pass of each form, medians and each form's spread
(max - min) / median. One form counts as faster than another only if the medians differ by more than the two
spreads added."""
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
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import grad_ref as gr  # noqa: E402
from grad_bench import SEED, ppo_loss as torch_ppo_loss, timed  # noqa: E402
from gym_macm import _abi, ppo  # noqa: E402
from gym_macm.policy import MlpCritic, MlpPolicy, gae  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5, help="closed-loop steps before the trajectory")
    ap.add_argument("--steps", type=int, default=128, help="K")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ppo_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    E, N, K, W = args.envs, args.agents, args.steps, args.warmup
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

    # ---- one trajectory: what the collector hands the learner (grad_bench.py's) ----------------------------
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
    obs, actions = traj["obs"], acts[1:]
    del noise, boot
    assert obs.shape == (K, E, N, 4) and obs.dtype == torch.float32 and vec.status() == 0

    pol.params.requires_grad_(True)
    crit.params.requires_grad_(True)
    nets = (pol, crit)

    def zero_grads():
        for m in nets:
            m.params.grad = None

    log_prob_ms, old_logp = timed(lambda: ppo.log_prob(old_logits, actions))

    # ---- b on a seeded subset against a, before anything is timed -----------------------------------------
    idx = torch.as_tensor(np.sort(np.random.default_rng(SEED).choice(M, 8192, replace=False)), device=dev)
    sub = lambda t, *tail: t.reshape((M,) + tail)[idx].contiguous()
    s_obs, s_act, s_adv, s_ret = sub(obs, 4), sub(actions, 3), sub(adv), sub(ret)
    lg, v = pol.forward(s_obs), crit.forward(s_obs)
    lg.retain_grad()
    v.retain_grad()
    torch_ppo_loss(lg, sub(old_logits, 9), s_act, s_adv, s_ret, v).backward()
    a_sub = [m.params.grad.clone() for m in nets]
    a_dout = (lg.grad.cpu().numpy().reshape(len(idx), -1), v.grad.cpu().numpy().reshape(len(idx), -1))
    zero_grads()
    ppo.ppo_loss(pol.forward(s_obs), crit.forward(s_obs), s_act, sub(old_logp), s_adv, s_ret)[0].backward()
    used = {}
    for i, (net, m) in enumerate((("policy", pol), ("critic", crit))):
        _, G = gr.grad(m.params.detach().cpu().numpy(), 4, 32, 2, gr.N_OUT[net], s_obs.cpu().numpy(), a_dout[i])
        err = np.abs(m.params.grad.cpu().numpy().astype(np.float64) - a_sub[i].cpu().numpy().astype(np.float64))
        bound = gr.tol(G, len(idx), 32)
        used[net] = float((err[G > 0] / bound[G > 0]).max())
        assert np.all(err <= bound), f"b: the {net}'s gradient is outside grad_ref.tol of a's ({used[net]:.3f} of it)"
    del lg, v, s_obs, a_sub, a_dout
    zero_grads()

    # ---- the forms ------------------------------------------------------------------------------------------
    def a_pass():
        lg, v = pol.forward(obs), crit.forward(obs)
        torch_ppo_loss(lg, old_logits, actions, adv, ret, v).backward()

    def b_forward():
        return pol.forward(obs), crit.forward(obs)

    def c_pass():
        return ppo.ppo_grads(pol, crit, obs, actions, old_logp, adv, ret)

    L = _abi.lib()
    sh = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    nbytes = ppo.workspace_bytes(M)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    d_lg, d_v = pol.forward(obs).detach(), crit.forward(obs).detach()
    d_dl, d_dv = torch.empty_like(d_lg), torch.empty_like(d_v)
    d_stats = torch.empty((8,), dtype=torch.float64, device=dev)
    cfg = ppo.config()
    d_bytes = 9 * 4 + 3 + 4 * 4 + 9 * 4 + 4  # in: logits, actions, old_logp, adv, values, ret; out: dlogits, dvalues

    def d_pass():
        _abi.check(L.macm_ppo_loss(ctypes.byref(cfg), M, vp(d_lg), vp(actions), vp(old_logp), vp(adv), vp(d_v), vp(ret),
                                   None, None, vp(d_dl), vp(d_dv), vp(d_stats), vp(ws), nbytes, sh), "macm_ppo_loss")

    parts = ("a_total", "b_forward", "b_loss", "b_backward", "c_total", "d_ppo_loss")
    res = {p: [] for p in parts}
    for rep in range(-1, args.reps):  # rep -1: one untimed pass of each form
        t = {}
        zero_grads()
        t["a_total"], _ = timed(a_pass)
        zero_grads()
        t["b_forward"], (lg, v) = timed(b_forward)
        t["b_loss"], (loss, b_stats) = timed(lambda: ppo.ppo_loss(lg, v, actions, old_logp, adv, ret))
        t["b_backward"], _ = timed(loss.backward)
        b_grads = [m.params.grad.clone() for m in nets]
        del lg, v, loss
        zero_grads()
        t["c_total"], c_stats = timed(c_pass)
        t["d_ppo_loss"], _ = timed(d_pass)
        if rep == -1:
            for m, g, net in zip(nets, b_grads, ("policy", "critic")):
                assert torch.equal(m.params.grad.view(torch.int32), g.view(torch.int32)), f"c: the {net}'s bits are b's"
            for s in (b_stats, c_stats, d_stats):
                s = s.cpu().numpy()
                assert s[4] == 0.0 and s[5] == 0.0 and s[6] == 1.0 and s[7] == M, "first epoch: the ratio is exactly 1"
        else:
            for p in parts:
                res[p].append(t[p])

    med = {p: statistics.median(res[p]) for p in parts}
    b_total = [x + y + z for x, y, z in zip(res["b_forward"], res["b_loss"], res["b_backward"])]
    res["b_total"] = b_total
    med["b_total"] = statistics.median(b_total)
    spread = {p: (max(res[p]) - min(res[p])) / med[p] for p in res}
    faster = lambda x, y: bool(med[y] - med[x] > spread[x] * med[x] + spread[y] * med[y])
    out = dict(ms=res, median_ms=med, spread=spread, log_prob_once_ms=log_prob_ms,
               b_faster_than_a_by_more_than_the_spreads=faster("b_total", "a_total"),
               c_faster_than_b_by_more_than_the_spreads=faster("c_total", "b_total"),
               a_over_b=med["a_total"] / med["b_total"], b_over_c=med["b_total"] / med["c_total"],
               d_bytes_per_row=d_bytes, d_tb_per_s=d_bytes * M / (med["d_ppo_loss"] * 1e-3) / 1e12,
               b_subset_share_of_tol_from_a=used, first_epoch_stats=dict(zip(ppo.STATS, c_stats.cpu().tolist())),
               rows=M, envs=E, agents=N, steps=K, warmup=W, reps=args.reps,
               peak_memory_gb=torch.cuda.max_memory_allocated() / 1e9, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
