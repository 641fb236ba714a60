"""gym_macm.ppo.transitions and tests/iteration_ref.py, without a GPU.

(a) transitions on label tensors whose every element encodes (k, e, n): row j of the result is the decision
    taken from obs row j: obs[j], logits[j], actions[j + 1], values[j + 1], reward[j + 1], done[j + 1],
    boot[j + 1], element for element, as views of the buffers, and every malformed input is refused.
(b) The textbook GAE (float64, the usual backward recursion) equals value_ref.gae (float32, the device's fma
    chain) on inputs where every operation is exact in float32.
(c) One textbook minibatch step is tied, link by link, to the references the suite already holds to torch:
    the advantages' moments to minibatch_ref within its bounds, the stats to ppo_ref.loss, the gradients to
    grad_ref.grad within grad_ref.tol, and the step to adam_ref's float64 mode within test_adam_ref's 1e-12.
(d) The old pairing (every advantage one row late) moves the textbook's first gradient by more than 100 times
    the bound of (c): the comparison the GPU tests make can tell the two apart.

The inputs of (c) and (d) are dyadic: params in {-1, 0, 1} / 4 (the first layer / 2), obs half-integers in
[-2, 2]. Every product and partial sum of the forward pass is then a multiple of 2^-6 below 2^7, exact in float32
in any association, so the float32 fma chain of policy_ref and the float64 matmul of the textbook give the same
logits and values (asserted), and what is left between the textbook and the definition are the two roundings
the definition makes and a textbook does not:

    logp is rounded to float32 before the ratio:      |d logp| <= 2^-24 |logp|
    the normalised advantage is rounded to float32:   |d A|    <= 2^-24 |A|

To first order, per row: the surrogate min(r A, clip(r) A) moves by at most r |A| (|d logp| + 2^-24), since
|d r| = r |d logp| and the clipped branch moves less; (r - 1) - log r has derivative r - 1 in logp; r itself moves
by r |d logp|. The bounds below are twice those (the slack covers the second order and the textbook's own
float64 roundings in log_softmax), added to ppo_ref's own bound for the stat; entropy and value_loss see neither
rounding and keep ppo_ref's bound alone, widened only by log_softmax's association (a few 2^-53 of the logits'
magnitude per row, inside the same factor of the stat's magnitude). clip_frac is compared exactly: no row's
ratio lies within 2^-18 of a clip edge (asserted), 2^-24 |logp| r being below 2^-19 for |logp| < 16.
For the gradients grad_ref.tol is already a float32 bound, (rows + 2 hidden + 16) 2^-24 G; the two roundings
move dL/dlogits by at most 2^-24 (|logp| + 1) of its policy part, which takes (|logp| + 1) <= 17 of those
rows + 2 hidden + 16 >= 112 units."""
import numpy as np
import pytest
import torch

import adam_ref as A
import iteration_ref as it
import minibatch_ref as M
import policy_ref as pr
import ppo_ref as R
import value_ref as vr

from gym_macm import ppo

F32, F64 = np.float32, np.float64


# ---- (a) the pairing, as views -------------------------------------------------------------------------
def labels(K, E, N):
    """The trajectory-form buffers of a K-step launch; the element of row k, env e, agent n holds 25 k + 5 e + n"""
    assert K + 1 <= 10 and E <= 5 and N <= 5  # a uint8 holds every code
    def code(rows, *trail, dtype=torch.float32, agents=True):
        k = torch.arange(rows).view(rows, 1, 1) * 25 + torch.arange(E).view(1, E, 1) * 5
        c = k + torch.arange(N).view(1, 1, N) if agents else k[:, :, 0]
        for d in trail:
            c = c.unsqueeze(-1).expand(*c.shape, d)
        return c.to(dtype).contiguous()
    traj = dict(obs=code(K, 4), reward=code(K), done=code(K, dtype=torch.uint8, agents=False),
                nbr_id=code(K, dtype=torch.int32), collided=code(K, dtype=torch.uint8))
    return traj, code(K + 1, 3, dtype=torch.uint8), code(K, 9), code(K + 1), code(K)


@pytest.mark.parametrize("K,E,N", [(2, 1, 1), (5, 2, 3), (9, 5, 5)])
def test_transitions_pairs_each_decision_with_its_own_step(K, E, N):
    traj, acts, lg, vals, boot = labels(K, E, N)
    t = ppo.transitions(traj, acts, lg, vals, boot)
    assert sorted(t) == ["actions", "boot", "done", "logits", "obs", "reward", "values"]
    for j in range(K - 1):
        for e in range(E):
            assert int(t["done"][j, e]) == 25 * (j + 1) + 5 * e, "done: the step that executed the decision"
            for n in range(N):
                seen, stepped = 25 * j + 5 * e + n, 25 * (j + 1) + 5 * e + n
                assert t["obs"][j, e, n].tolist() == [seen] * 4, "obs: the row the decision was taken from"
                assert t["logits"][j, e, n].tolist() == [seen] * 9, "logits: the same row"
                assert t["actions"][j, e, n].tolist() == [stepped] * 3, "actions: the row the decision was written to"
                assert float(t["values"][j, e, n]) == stepped, "values: V of the obs the decision was taken from"
                assert float(t["reward"][j, e, n]) == stepped and float(t["boot"][j, e, n]) == stepped
    # views of the buffers: nothing copied, every one contiguous, K - 1 rows
    src = dict(obs=traj["obs"][0], logits=lg[0], actions=acts[1], values=vals[1], reward=traj["reward"][1],
               done=traj["done"][1], boot=boot[1])
    own = dict(obs=traj["obs"], logits=lg, actions=acts, values=vals, reward=traj["reward"], done=traj["done"], boot=boot)
    for f, v in t.items():
        assert v.shape[0] == K - 1 and v.is_contiguous(), f
        assert v.data_ptr() == src[f].data_ptr(), f"{f}: not a view at the expected row"
        assert v.untyped_storage().data_ptr() == own[f].untyped_storage().data_ptr(), f"{f}: a copy"
    vals[1, 0, 0] = -7.0  # a write to the buffer shows in the view
    assert float(t["values"][0, 0, 0]) == -7.0


def test_transitions_refusals():
    K, E, N = 4, 2, 3
    traj, acts, lg, vals, boot = labels(K, E, N)
    ok = dict(traj=traj, actions=acts, logits=lg, values=vals, boot=boot)
    ppo.transitions(**ok)

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            ppo.transitions(**dict(ok, **kw))

    # leading sizes that do not agree on one K
    refused("^actions is ", actions=acts[:K].contiguous())
    refused("^logits is ", logits=torch.cat([lg, lg[:1]]))
    refused("^values is ", values=vals[:K].contiguous())
    refused("^boot is ", boot=boot[:K - 1].contiguous())
    refused("^done is ", traj=dict(traj, done=torch.cat([traj["done"], traj["done"][:1]])))
    refused("^obs is ", traj=dict(traj, obs=traj["obs"][:K - 1].contiguous()))
    refused("^values is ", values=vals[:, :1].contiguous())  # another E
    refused("^actions is ", actions=acts[..., :2].contiguous())  # not 3 heads
    refused("^logits is ", logits=lg[..., :8].contiguous())
    # K < 2
    t1, a1, l1, v1, b1 = labels(1, E, N)
    with pytest.raises(ValueError, match="fewer than 2 steps"):
        ppo.transitions(t1, a1, l1, v1, b1)
    # non-contiguous inputs
    wide = torch.zeros((K + 1, E, 2 * N))
    refused("^values must be contiguous", values=wide[:, :, ::2])
    refused("^boot must be contiguous", boot=torch.zeros((E, K, N)).transpose(0, 1))
    refused("^obs must be contiguous", traj=dict(traj, obs=torch.zeros((K, E, N, 8))[..., ::2]))
    refused("^actions must be contiguous", actions=torch.zeros((K + 1, E, N, 6), dtype=torch.uint8)[..., ::2])
    # the overwrite form's shapes
    over = dict(obs=traj["obs"][0], reward=traj["reward"][0], done=traj["done"][0])
    with pytest.raises(ValueError, match="trajectory form"):
        ppo.transitions(over, acts[0], lg[0], vals[0], boot[0])
    refused("^actions is ", actions=acts[0])
    refused("^logits is ", logits=lg[0])
    refused("^values is ", values=vals[0])
    refused("^boot is ", boot=boot[0])
    # a field that is not there
    refused("missing", traj={k: v for k, v in traj.items() if k != "done"})


# ---- (b) the textbook GAE against value_ref.gae --------------------------------------------------------
def test_textbook_gae_equals_value_ref_on_exact_inputs():
    """gamma = lambda = 0.5 and quarter-integer inputs in [-2, 2]: delta is a multiple of 1/8 below 8, and each
    step of the recursion adds two fraction bits, 3 + 2 * 6 = 15 over T = 7, with 3 integer bits: exact in float32"""
    T, E, N = 7, 4, 5
    rng = np.random.default_rng(41)
    q = lambda *s: (rng.integers(-8, 9, s) / 4.0).astype(F32)
    reward, values, nxt = q(T, E, N), q(T, E, N), q(T, E, N)
    done = (rng.random((T, E)) < 0.3).astype(np.uint8)
    live = done[:-1] == 0
    nxt[:-1][live] = values[1:][live]  # where the episode goes on, v(s') is the next row's value
    assert done.any() and (done == 0).any() and done[:-1].any()
    adv, ret = it.gae(reward, values, nxt, done, 0.5, 0.5)
    want_adv, want_ret = vr.gae(reward, values, nxt, done, 0.5, 0.5)
    assert np.array_equal(adv.numpy(), want_adv.astype(F64)) and np.array_equal(ret.numpy(), want_ret.astype(F64))
    a32, r32 = it.gae(reward, values, nxt, done, 0.5, 0.5, dtype=torch.float32)
    assert np.array_equal(a32.numpy(), want_adv) and np.array_equal(r32.numpy(), want_ret)
    # a done row cuts the recursion: the advantage there is its own delta
    k, e = np.argwhere(done)[0]
    assert np.array_equal(adv.numpy()[k, e], (reward[k, e] + 0.5 * nxt[k, e] - values[k, e]).astype(F64))
    assert len(np.unique(adv.numpy())) > T * E * N // 4


# ---- (c), (d) one textbook minibatch step against the chain of the references --------------------------
SHAPES = [(4, 16, 1), (6, 32, 2)]
HP = it.Hyper(lr=1e-2, max_grad_norm=0.05)  # below these gradients' norms: the clip is active
T_, E_, N_ = 12, 3, 8


def dyadic_params(shapes, rng):
    flat = []
    for l, (i, o) in enumerate(shapes):
        d = 2.0 if l == 0 else 4.0
        flat += [rng.integers(-1, 2, i * o) / d, rng.integers(-1, 2, o) / 4.0]
    return np.concatenate(flat).astype(F32)


def synthetic(od, H, nh, seed=0):
    """The nets and T_ x E_ x N_ rows: exact-forward nets and obs, sampled actions, old_logp near the nets' own (ratios
    on both sides of the clip range), advantages that follow the row index (a shift by one row changes them),
    returns and old values around the values"""
    rng = np.random.default_rng([8800 + seed, od, H, nh])
    pshapes, cshapes = pr.layer_shapes(od, H, nh), vr.layer_shapes(od, H, nh)
    pp, pc = dyadic_params(pshapes, rng), dyadic_params(cshapes, rng)
    rows = T_ * E_ * N_
    obs = (rng.integers(-4, 5, (rows, od)) / 2.0).astype(F32)
    logits, values = pr.logits_of(pp, od, H, nh, obs), vr.value_of(pc, od, H, nh, obs)
    actions = pr.actions_of(logits, pr.gumbel_noise((rows, 9), 8801 + seed))
    logp, _, _ = R.log_prob(logits, actions)
    draw = lambda s: (s * rng.standard_normal(rows)).astype(F32)
    step = np.repeat(np.arange(T_), E_ * N_)
    adv = (np.sin(1.3 * step) + draw(0.5)).astype(F32)  # a strong dependence on the step: rows are not exchangeable
    r = dict(obs=obs, actions=actions, logits=logits, values=values, old_logp=(logp + draw(0.15)).astype(F32), adv=adv,
             ret=(values + draw(1.0)).astype(F32), old_values=(values + draw(0.3)).astype(F32))
    mb = np.random.default_rng(8802 + seed).permutation(rows)[:150]
    return dict(pp=pp, pc=pc, pshapes=pshapes, cshapes=cshapes, rows=r, mb=mb, shape=(od, H, nh))


def torch_rows(r, dtype=torch.float64):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return dict(obs=f(r["obs"]), actions=torch.from_numpy(r["actions"]).long(), old_logp=f(r["old_logp"]),
                old_values=f(r["old_values"]), adv=f(r["adv"]), ret=f(r["ret"]))


def stat_bounds(L, adv, cfg=HP):
    """|textbook - ppo_ref| allowed per stat: ppo_ref's own bound and the two float32 roundings (module docstring)"""
    u = 2.0 ** -24
    r, logp, a = L["ratio"], np.abs(L["logp"]), np.abs(adv.astype(F64))
    b = (L["rows"] + 64) * 2.0 ** -52 * L["stat_mag"]
    b[6] = 64 * 2.0 ** -52 * L["stat_mag"][6]
    extra = np.zeros(8)
    extra[1] = 2 * u * np.mean(r * a * (logp + 1.0))
    extra[4] = 2 * u * np.mean(np.abs(r - 1.0) * logp)
    extra[6] = 2 * u * np.max(r * logp)
    extra[0] = extra[1]
    return b + extra


@pytest.mark.parametrize("use_old_values", [True, False], ids=["old_values", "no_old_values"])
@pytest.mark.parametrize("od,H,nh", SHAPES)
def test_one_textbook_step_agrees_with_the_chain_of_references(od, H, nh, use_old_values):
    s = synthetic(od, H, nh)
    r, mb = s["rows"], s["mb"]
    rows64 = torch_rows(r)
    # the forward pass is exact on these inputs: the textbook's float64 outputs are the float32 chain's
    assert np.array_equal(it.mlp(torch.from_numpy(s["pp"]).double(), s["pshapes"], rows64["obs"]).numpy(), r["logits"].astype(F64))
    assert np.array_equal(it.mlp(torch.from_numpy(s["pc"]).double(), s["cshapes"], rows64["obs"]).numpy()[:, 0], r["values"].astype(F64))
    trace = []
    stats, pp1, pc1 = it.learn(rows64, s["pp"], s["pc"], s["pshapes"], s["cshapes"], [mb], HP, use_old_values, trace=trace)
    tb = trace[0]
    ch = it.chain_step(r, mb, s["pp"], s["pc"], s["shape"], s["shape"], HP, use_old_values)
    # minibatch_ref: the moments within its bounds
    mom, bound = ch["moments"], M.bounds(ch["moments"])
    assert mom["n"] == len(mb) and abs(tb["mean"] - mom["mean"]) <= bound["mean"] and abs(tb["std"] - mom["std"]) <= bound["std"]
    assert np.abs(tb["adv"] - ch["adv"].astype(F64)).max() <= 2.0 ** -24 * np.abs(ch["adv"]).max() * 1.01
    # ppo_ref: the stats
    L = ch["loss"]
    assert not L["undecided"].any() and stats[0, 7] == len(mb) == L["stats"][7]
    edge = np.minimum(np.abs(L["ratio"] - (1 - HP.clip)), np.abs(L["ratio"] - (1 + HP.clip)))
    assert edge.min() > 2.0 ** -18 and np.abs(L["logp"]).max() < 16
    assert 0.05 < L["stats"][5] < 0.95 and L["ratio"].min() < 0.8 and L["ratio"].max() > 1.2, "ratios on both sides of the clip range"
    err, allowed = np.abs(stats[0] - L["stats"]), stat_bounds(L, ch["adv"])
    for i, name in enumerate(R.STATS):
        print(f"{s['shape']} {name}: textbook {stats[0, i]!r} reference {L['stats'][i]!r} err {err[i]:.3e} bound {allowed[i]:.3e}")
    assert stats[0, 5] == L["stats"][5] and (err <= allowed).all(), (err, allowed)
    # grad_ref: the gradients before the clip
    for got, want, tol, name in ((tb["grads"][0], ch["grad_policy"], ch["tol_policy"], "policy"),
                                 (tb["grads"][1], ch["grad_value"], ch["tol_value"], "critic")):
        e = np.abs(got - want)
        share = float(np.max(e[tol > 0] / tol[tol > 0]))
        print(f"{s['shape']} {name}: |textbook - grad_ref| uses {share:.4f} of grad_ref.tol")
        assert (e <= tol).all() and np.abs(want).max() > 0
    # adam_ref: the step from the textbook's own gradients
    params = [s["pp"].astype(F64), s["pc"].astype(F64)]
    st = A.zero_state(params[0].size, params[1].size, F64)
    cfg = A.Cfg(lr=HP.lr, beta1=HP.betas[0], beta2=HP.betas[1], eps=HP.eps, max_grad_norm=HP.max_grad_norm)
    assert A.step(params, [g.copy() for g in tb["grads"]], st, cfg) == "step" and st["head"][5] < 1.0, "the clip is active"
    for got, want in zip((pp1, pc1), params):
        assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 1e-12
        assert not np.array_equal(got, s["pp"] if got is pp1 else s["pc"])


@pytest.mark.parametrize("od,H,nh", SHAPES)
def test_the_old_pairing_moves_the_first_gradient_far_outside_the_bound(od, H, nh):
    s = synthetic(od, H, nh)
    r, mb = s["rows"], s["mb"]
    ch = it.chain_step(r, mb, s["pp"], s["pc"], s["shape"], s["shape"], HP)
    late = dict(r, adv=np.roll(r["adv"].reshape(T_, E_ * N_), 1, axis=0).reshape(-1))  # adv[k] beside the rows of k + 1
    grads = []
    for rows in (r, late):
        trace = []
        it.learn(torch_rows(rows), s["pp"], s["pc"], s["pshapes"], s["cshapes"], [mb], HP, trace=trace)
        grads.append(trace[0]["grads"][0])
    tol = ch["tol_policy"]
    moved = np.abs(grads[1] - grads[0])
    ratio = float(np.max(moved[tol > 0] / tol[tol > 0]))
    print(f"{s['shape']}: the old pairing moves the policy's gradient by {ratio:.1f} times grad_ref.tol at the most")
    assert ratio > 100.0
