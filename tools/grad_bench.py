"""What the gradient kernels buy a learner: Flock 4096 x 64, float32 obs, autoreset on with a 1 s time limit,
actor and critic both two hidden layers of 32, one trajectory of K = 128 steps from rollout_policy (33.5 M rows
of obs, action, logits, value, advantage, return), and one update pass of a PPO-shaped torch loss over all of
them. Forms alternating rep by rep in one process:

  a  forward, the torch loss and backward through MlpPolicy.forward / MlpCritic.forward: the feature. Timed in
     three parts (forward, loss, backward), so that the share of the caller's torch loss is visible.
  b  the same loss with the two nets as float32 nn.Linear stacks under torch autograd: what a user does without
     the feature. In minibatches of --b-rows rows (default: all rows at once; halved until it fits), the
     gradients accumulating over the minibatches.
  c  macm_policy_grad and macm_value_grad alone on a's dL/dlogits and dL/dvalue: rows per second and the
     share of the f32 MFMA and VALU issue they stand for (32 v_mfma_f32_32x32x2_f32 of 64 cycles per layer and
     tile; per lane and tile 2,464 v_fma_f32 for the actor, 2,208 for the critic, 4 cycles each at one wave
     per SIMD; 1,024 SIMDs at 2.4 GHz).

    timeout 900 python tools/grad_bench.py --out profiles/policy_grad/update.json

Before timing, a's params.grad on a seeded subset of rows is asserted within grad_ref.tol of tests/grad_ref.py
fed with the loss's own dL/dlogits and dL/dvalue. Prints (and writes to --out) one JSON line: ms of every rep
after one untimed pass of each form, medians and each form's spread (max - min) / median. a counts as faster
than b only if the medians differ by more than the two spreads added."""
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

import grad_ref as gr  # noqa: E402
from gym_macm import _abi  # noqa: E402
from gym_macm.policy import MlpCritic, MlpPolicy, gae  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

SEED = 0x6D61636D
SIMDS, CLOCK = 1024, 2.4e9
MFMA_CYCLES, FMA_CYCLES = 64, 4
FMAS = {"policy": 4 * 32 + 32 * 32 + 32 * 9 + 32 * 32, "critic": 4 * 32 + 32 * 32 + 32 * 1 + 32 * 32}  # 32 x 2 nets


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def ppo_loss(lg, old_logits, actions, adv, ret, v, clip=0.2):
    lp = torch.log_softmax(lg.view(lg.shape[:-1] + (3, 3)), -1)
    old = torch.log_softmax(old_logits.view(lp.shape), -1)
    a = actions.long().unsqueeze(-1)
    logp, old_logp = lp.gather(-1, a).squeeze(-1).sum(-1), old.gather(-1, a).squeeze(-1).sum(-1)
    ratio = torch.exp(logp - old_logp)
    pg = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    vloss = 0.5 * ((v - ret) ** 2).mean()
    entropy = -(lp.exp() * lp).sum((-1, -2)).mean()
    return pg + 0.5 * vloss - 0.01 * entropy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5, help="closed-loop steps before the trajectory")
    ap.add_argument("--steps", type=int, default=128, help="K")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--b-rows", type=int, default=0, help="b's minibatch in rows (0: all rows; halved until it fits)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "grad_bench.py needs a GPU"
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

    p_layers, v_layers = mlp(9), mlp(1)
    pol = MlpPolicy.from_linear_layers(p_layers, device=dev)
    crit = MlpCritic.from_linear_layers(v_layers, device=dev)

    # ---- one trajectory: what the collector hands the learner -------------------------------------------
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
    b_params = [p for lin in p_layers + v_layers for p in lin.parameters()]

    def zero_grads():
        for p in [pol.params, crit.params] + b_params:
            p.grad = None

    # ---- a on a seeded subset against grad_ref, before anything is timed ------------------------------------
    idx = torch.as_tensor(np.sort(np.random.default_rng(SEED).choice(M, 8192, replace=False)), device=dev)
    sub = lambda t, *tail: t.reshape((M,) + tail)[idx].contiguous()
    s_obs = sub(obs, 4)
    lg, v = pol.forward(s_obs), crit.forward(s_obs)
    lg.retain_grad()
    v.retain_grad()
    ppo_loss(lg, sub(old_logits, 9), sub(actions, 3), sub(adv), sub(ret), v).backward()
    used = {}
    for net, m, out in (("policy", pol, lg), ("critic", crit, v)):
        g, G = gr.grad(m.params.detach().cpu().numpy(), 4, 32, 2, gr.N_OUT[net], s_obs.cpu().numpy(),
                       out.grad.cpu().numpy().reshape(len(idx), -1))
        err = np.abs(m.params.grad.cpu().numpy().astype(np.float64) - g)
        bound = gr.tol(G, len(idx), 32)
        assert np.all(err <= bound), f"a: the {net}'s gradient is outside grad_ref.tol"
        used[net] = float((err[G > 0] / bound[G > 0]).max())
    del lg, v, s_obs
    zero_grads()

    # ---- the forms ------------------------------------------------------------------------------------------
    keep = {}

    def a_forward():
        lg, v = pol.forward(obs), crit.forward(obs)
        lg.retain_grad()  # (c takes a's dL/dlogits and dL/dvalue; without these two lines torch frees them)
        v.retain_grad()
        return lg, v

    def stack(layers, x):
        for lin in layers[:-1]:
            x = torch.relu(lin(x))
        return layers[-1](x)

    flat = dict(obs=obs.view(M, 4), old=old_logits.view(M, 9), act=actions.reshape(M, 3), adv=adv.view(M), ret=ret.view(M))

    def b_pass(rows):
        """forward, loss and backward of the nn.Linear nets over all M rows in minibatches of `rows`"""
        for lo in range(0, M, rows):
            sl = slice(lo, min(M, lo + rows))
            lg, v = stack(p_layers, flat["obs"][sl]), stack(v_layers, flat["obs"][sl]).squeeze(-1)
            loss = ppo_loss(lg, flat["old"][sl], flat["act"][sl], flat["adv"][sl], flat["ret"][sl], v)
            (loss * ((sl.stop - sl.start) / M)).backward()

    b_rows = args.b_rows or M
    while True:  # the largest minibatch that fits, found in the untimed pass
        try:
            zero_grads()
            b_pass(b_rows)
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            zero_grads()
            torch.cuda.empty_cache()
            b_rows = (b_rows + 1) // 2
            assert b_rows >= 65536, "b does not fit even in minibatches of 65536 rows"

    L = _abi.lib()
    sh = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    nbytes = ctypes.c_int64()
    _abi.check(L.macm_mlp_grad_workspace(M, ctypes.byref(nbytes)), "macm_mlp_grad_workspace")
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    gp, gv = torch.empty_like(pol.params, requires_grad=False), torch.empty_like(crit.params, requires_grad=False)

    def c_policy():
        _abi.check(L.macm_policy_grad(ctypes.byref(pol.struct()), vp(obs), 0, M, vp(keep["dlogits"]), vp(gp), vp(ws),
                                      nbytes.value, sh), "macm_policy_grad")

    def c_value():
        _abi.check(L.macm_value_grad(ctypes.byref(crit.struct()), vp(obs), 0, M, vp(keep["dvalues"]), vp(gv), vp(ws),
                                     nbytes.value, sh), "macm_value_grad")

    parts = ("a_forward", "a_loss", "a_backward", "b_total", "c_policy_grad", "c_value_grad")
    res = {p: [] for p in parts}
    for rep in range(-1, args.reps):  # rep -1: one untimed pass of each form
        t = {}
        zero_grads()
        t["a_forward"], (lg, v) = timed(a_forward)
        t["a_loss"], loss = timed(lambda: ppo_loss(lg, old_logits, actions, adv, ret, v))
        t["a_backward"], _ = timed(loss.backward)
        keep["dlogits"], keep["dvalues"] = lg.grad.contiguous(), v.grad.contiguous()
        a_grads = (pol.params.grad.clone(), crit.params.grad.clone())
        del lg, v, loss
        zero_grads()
        t["b_total"], _ = timed(lambda: b_pass(b_rows))
        t["c_policy_grad"], _ = timed(c_policy)
        t["c_value_grad"], _ = timed(c_value)
        assert torch.equal(gp.view(torch.int32), a_grads[0].view(torch.int32)), "c: the policy's bits are a's"
        assert torch.equal(gv.view(torch.int32), a_grads[1].view(torch.int32)), "c: the critic's bits are a's"
        if rep >= 0:
            for p in parts:
                res[p].append(t[p])
    # b's gradients against a's (other arithmetic: close, not equal)
    b_flat = torch.cat([torch.cat([lin.weight.grad.t().reshape(-1), lin.bias.grad]) for lin in p_layers])
    b_rel = float((b_flat - a_grads[0]).abs().max() / a_grads[0].abs().max())

    med = {p: statistics.median(res[p]) for p in parts}
    a_total = [x + y + z for x, y, z in zip(res["a_forward"], res["a_loss"], res["a_backward"])]
    c_total = [x + y for x, y in zip(res["c_policy_grad"], res["c_value_grad"])]
    ma, mb, mc = statistics.median(a_total), med["b_total"], statistics.median(c_total)
    spread = {p: (max(res[p]) - min(res[p])) / med[p] for p in parts}
    spread["a_total"] = (max(a_total) - min(a_total)) / ma
    spread["c_total"] = (max(c_total) - min(c_total)) / mc
    tiles = (M + 63) // 64
    issue = {}
    for net, key in (("policy", "c_policy_grad"), ("critic", "c_value_grad")):
        cycles = med[key] * 1e-3 * CLOCK * SIMDS
        issue[net] = dict(rows_per_s=M / (med[key] * 1e-3), mfma_share=tiles * 96 * MFMA_CYCLES / cycles,
                          valu_fma_share=tiles * FMAS[net] * FMA_CYCLES / cycles)
    out = dict(ms=res, median_ms=med, a_total_ms=ma, b_total_ms=mb, c_total_ms=mc, spread=spread, a_over_b=ma / mb,
               a_faster_than_b_by_more_than_the_spreads=bool(mb - ma > spread["a_total"] * ma + spread["b_total"] * mb),
               a_split=dict(forward=med["a_forward"] / ma, torch_loss=(med["a_loss"] + med["a_backward"] - mc) / ma,
                            grad_kernels=mc / ma),
               c=issue, b_minibatch_rows=b_rows, b_minibatches=-(-M // b_rows), b_policy_grad_max_rel_diff_from_a=b_rel,
               a_subset_share_of_tol=used, rows=M, envs=E, agents=N, steps=K, warmup=W, reps=args.reps,
               peak_memory_gb=torch.cuda.max_memory_allocated() / 1e9, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
