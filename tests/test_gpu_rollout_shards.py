"""Policy rollouts on env shards: a world that holds envs [e0, e0 + Es) of a job (FlockVec(env_offset=e0))
computes, for those envs, what the world that holds the whole job computes, in every form of rollout_policy.

The reference of every case is the whole job: one FlockVec(E, seed=s) with its policy and critic. The worlds
under test are its shards on the same device, each given the whole job's rows [e0, e0 + Es) of the first
actions (and of `noise` where it is used); the critic's value of the obs on entry, the first values row of a
collector, is compared too. Whole and shard run different code: another instantiation (32 or 64 lanes, the
scalar sweep from 2048 envs), rollout_sched's order computed from another env set, the workgroup path's loop
at E = 1. They must agree in bits, so every comparison is bit equality:

  per shard   every trajectory field, the action rows, logits, values, boot; the final outputs with autoreset;
              get_state with the ordered contact list; the per-env reward sums
  over shards the counters sum to the whole job's, status is 0, dist.reduce_reward_sums of the concatenated
              per-env sums is the whole job's total

in three forms: (a) the argmax, (b) one whole-job noise tensor of which each shard passes its env slice,
(c) sampling on in every world, the shard's draw registered at the job's row e0 * N (set_sampling's first_row,
which FlockVec takes from env_offset). Two checks give (c) its teeth: a shard registered at row 0 must not
reproduce the whole job's slice but shard 0's draw, and every sampled shard equals its twin given
gumbel_noise(..., first_row=e0 * N). The refusals of first_row that need a world are at the end."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_rollout_policy as tp
import test_gpu_rollout_value as tv
from test_gpu_rollout_autoreset import FKEYS
from test_gpu_rollout_policy import F64C, seeded_policy
from test_gpu_rollout_value import ibits, seeded_critic

pytestmark = pytest.mark.gpu

from gym_macm import _abi, dist  # noqa: E402
from gym_macm._abi import MacmError  # noqa: E402
from gym_macm.policy import gumbel_noise  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

DEV = "cuda:0"
SEED = 0x0BAD_5EED_0123_4567  # >= 2**32
D0 = 2**32 - 3                # the launch's decisions cross the carry into hi32(d)
FINAL = ("final_obs", "final_nbr_id", "final_length", "final_ends")
AR2 = dict(autoreset=True, final_obs=True, time_limit=1.5 / 60.0)  # an end at every 2nd step


def split(E, n_shards):
    """[(first env, env count)] of every rank, as dist.strong_split cuts a job"""
    return [dist.strong_split(E, n_shards, r) for r in range(n_shards)]


# id -> E, N, the shards, K, the env seed, the worlds' settings, debug flags
# ends: "every2nd" (time_limit = 1.5 / 60: ends after steps 1 and 3), "all" (time_limit = 0.25: every env ends inside the launch)
CASES = {
    "5x8polar":     dict(E=5, N=8, shards=split(5, 2), K=9, seed=11, kw={}),
    "5x33f64cart":  dict(E=5, N=33, shards=split(5, 2), K=9, seed=11, kw=F64C),
    "4x64ar-2+2":   dict(E=4, N=64, shards=split(4, 2), K=5, seed=21, kw=AR2, ends="every2nd"),
    "4x64ar-3+1":   dict(E=4, N=64, shards=[(0, 3), (3, 1)], K=5, seed=21, kw=AR2, ends="every2nd"),
    "16x64ar-k33":  dict(E=16, N=64, shards=split(16, 2), K=33, seed=11,
                         kw=dict(autoreset=True, final_obs=True, time_limit=0.25), ends="all"),
    "2048x64":      dict(E=2048, N=64, shards=split(2048, 2), K=2, seed=11, kw={}),
    "2x96wg":       dict(E=2, N=96, shards=split(2, 2), K=3, seed=31, kw=dict(start_spread=12)),
    "2x96wg-ar":    dict(E=2, N=96, shards=split(2, 2), K=3, seed=31, kw=dict(start_spread=12, **AR2), ends="every2nd"),
    "4x64spill":    dict(E=4, N=64, shards=split(4, 2), K=5, seed=23, kw={}, debug=_abi.DEBUG_FORCE_SPILL),
}
assert CASES["5x8polar"]["shards"] == [(0, 3), (3, 2)] and CASES["2048x64"]["shards"] == [(0, 1024), (1024, 1024)]
OVER = ("5x8polar", "5x33f64cart")  # these also in the overwrite form
RUNS = [(c, True) for c in CASES] + [(c, False) for c in OVER]
RUN_IDS = [f"{c}-{'traj' if t else 'over'}" for c, t in RUNS]
NOSPILL = [(r, i) for r, i in zip(RUNS, RUN_IDS) if r[0] != "4x64spill"]


def bits(t):
    """A tensor as integers of its element width: equality of these is equality in bits (NaNs, zero signs)"""
    if t.dtype == torch.float32:
        return ibits(t)
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def make(case, e0=0, Es=None):
    c = CASES[case]
    v = FlockVec(c["E"] if Es is None else Es, n_agents=[c["N"]], seed=c["seed"], env_offset=e0, device=DEV, **c["kw"])
    if c.get("debug"):
        v.world.set_debug(c["debug"])
    return v


def run(vec, pol, crit, act0, K, noise, traj):
    """One launch with logits, values and boot (tv.launch: guarded buffers), and everything read afterwards"""
    vec.set_policy(pol)
    vec.set_critic(crit)
    go, acts, lg, gv, gb = tv.launch(vec, act0, K, noise, traj)
    w = vec.world
    per, tot = vec.reward_sums()
    final = {f: None if getattr(w, f) is None else getattr(w, f).clone() for f in FINAL}
    return dict(out={f: go[f] for f in FKEYS}, acts=acts, logits=lg, values=gv, boot=gb, final=final,
                state=vec.get_state(), per=per, tot=tot, counters=vec.counters(), status=vec.status(),
                spilled=vec.spilled())


def assert_shard_is_slice(whole, shard, e0, Es, traj, ctx):
    """Everything `run` read of the shard against rows [e0, e0 + Es) of the whole job's, bit for bit"""
    cut = (lambda t: t[:, e0:e0 + Es]) if traj else (lambda t: t[e0:e0 + Es])
    for f in FKEYS:
        assert same_bits(cut(whole["out"][f]), shard["out"][f]), f"{ctx}: {f}"
    assert same_bits(cut(whole["acts"]), shard["acts"]), f"{ctx}: action rows"
    assert same_bits(cut(whole["logits"]), shard["logits"]), f"{ctx}: logits"
    lo = 1 if traj else 0  # row 0 of a trajectory's values is the caller's (tv.launch: untouched in every world)
    assert same_bits(cut(whole["values"])[lo:], shard["values"][lo:]), f"{ctx}: values"
    assert same_bits(cut(whole["boot"]), shard["boot"]), f"{ctx}: boot"
    for f in FINAL:
        x, y = whole["final"][f], shard["final"][f]
        assert (x is None) == (y is None), f"{ctx}: {f}"
        assert x is None or same_bits(x[e0:e0 + Es], y), f"{ctx}: {f}"
    sa, sb = whole["state"], shard["state"]
    assert set(sa) == set(sb)
    for k in sa:
        a, b = sa[k][e0:e0 + Es], sb[k]
        if k in ("contact_ab", "contact_imp"):  # rows of max(contact_count) entries of each world, zero past an env's count
            n = b.shape[1]
            assert a.shape[1] >= n and not a[:, n:].any(), f"{ctx}: state[{k}]: an entry past the shard's longest list"
            a = a[:, :n]
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{ctx}: state[{k}]"
    assert whole["per"][e0:e0 + Es].tobytes() == shard["per"].tobytes(), f"{ctx}: per-env reward sums"


def assert_job(whole, shards, ctx):
    """What holds over all shards of a job"""
    np.testing.assert_array_equal(sum(s["counters"] for s in shards), whole["counters"], err_msg=f"{ctx}: counters")
    assert whole["status"] == 0 and all(s["status"] == 0 for s in shards), f"{ctx}: status"
    assert sum(s["spilled"] for s in shards) == whole["spilled"], f"{ctx}: spilled"
    total = dist.reduce_reward_sums(np.concatenate([s["per"] for s in shards]))
    assert np.float64(total).tobytes() == np.float64(whole["tot"]).tobytes(), f"{ctx}: the job's reward total"


def assert_ends(case, r, traj):
    c = CASES[case]
    if c.get("ends") == "every2nd":
        done = r["out"]["done"].bool()
        assert traj and bool(done[1::2].all()) and not bool(done[0::2].any()), "a time-limit end after every 2nd step"
        assert bool((r["final"]["final_ends"] == c["K"] // 2).all())
    elif c.get("ends") == "all":
        done = r["out"]["done"].bool()
        assert bool(done.all(dim=1).any()) and bool((r["final"]["final_ends"] >= 1).all()), "every env ends at its time limit"
    if c.get("debug"):
        assert r["spilled"] > 0


def run_job(case, traj, form):
    """The whole job and its shards in one form; returns (whole, [(e0, Es, shard's results)], what the teeth need)"""
    c = CASES[case]
    E, N, K = c["E"], c["N"], c["K"]
    whole = make(case)
    od = whole.world.OD
    pol, crit = seeded_policy(od), seeded_critic(od)
    noise = None
    if form == "argmax":
        act0 = pol.act(whole.obs)
    elif form == "noise":
        noise = tp.noise_rows(K, E, N)
        act0 = pol.act(whole.obs, noise=tp.noise_rows(1, E, N, seed=6)[0])
    else:
        whole.set_sampling(SEED, D0)
        assert whole.first_row == 0 and whole.world.sampling_first_row == 0
        act0 = pol.act(whole.obs, seed=SEED, decision=D0 - 1, first_row=whole.first_row)
    v0 = crit.value(whole.obs)  # the first values row of a collector
    obs0 = whole.obs.clone()
    rw = run(whole, pol, crit, act0, K, noise, traj)
    assert_ends(case, rw, traj)
    if form != "argmax":
        assert len(torch.unique(rw["acts"])) == 3, f"{case}: the decisions differ"
    if form == "sampled":
        assert whole.sampling == (SEED, D0 + K)
    results = []
    for e0, Es in c["shards"]:
        ctx = f"{case} {form}, envs [{e0}, {e0 + Es})"
        sh = make(case, e0, Es)
        assert same_bits(sh.obs, obs0[e0:e0 + Es]), f"{ctx}: the initial obs"
        assert same_bits(crit.value(sh.obs), v0[e0:e0 + Es]), f"{ctx}: the first values row"
        if form == "sampled":
            sh.set_sampling(SEED, D0)
            assert sh.first_row == e0 * N == sh.world.sampling_first_row
            own = pol.act(sh.obs, seed=SEED, decision=D0 - 1, first_row=sh.first_row)
            assert torch.equal(own, act0[e0:e0 + Es]), f"{ctx}: the first actions, drawn by the shard at its first_row"
        rs = run(sh, pol, crit, act0[e0:e0 + Es].contiguous(), K,
                 None if noise is None else noise[:, e0:e0 + Es].contiguous(), traj)
        assert_shard_is_slice(rw, rs, e0, Es, traj, ctx)
        if form == "sampled":
            assert sh.sampling == (SEED, D0 + K), f"{ctx}: the shard's decision advanced by n_steps"
        results.append((e0, Es, rs))
    assert_job(rw, [r for _, _, r in results], f"{case} {form}")
    return rw, results, dict(pol=pol, crit=crit, act0=act0)


# ---- (a) the argmax -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,traj", [r for r, _ in NOSPILL], ids=[i for _, i in NOSPILL])
def test_argmax_shards_equal_the_whole_job(case, traj):
    run_job(case, traj, "argmax")


# ---- (b) one noise tensor of the whole job, each shard passing its env slice ----------------------------------
@pytest.mark.parametrize("case,traj", [r for r, _ in NOSPILL], ids=[i for _, i in NOSPILL])
def test_given_noise_shards_equal_the_whole_job(case, traj):
    run_job(case, traj, "noise")


# ---- (c) sampling on in every world: the draw follows the job's rows ------------------------------------------
@pytest.mark.parametrize("case,traj", RUNS, ids=RUN_IDS)
def test_sampled_shards_equal_the_whole_job(case, traj):
    run_job(case, traj, "sampled")


# ---- the teeth of (c), on 4 x 64 -------------------------------------------------------------------------------
def test_sampled_shard_equals_its_twin_given_the_noise_at_its_first_row():
    """Each sampled shard against a twin with sampling off that is given gumbel_noise(SEED, D0, K, (Es, N),
    first_row=e0 * N): that tensor is the whole job's rows [e0 * N, (e0 + Es) * N), in bits."""
    case = "4x64ar-3+1"
    c = CASES[case]
    E, N, K = c["E"], c["N"], c["K"]
    rw, results, x = run_job(case, True, "sampled")
    job_noise = gumbel_noise(SEED, D0, K, (E, N), DEV)
    for e0, Es, rs in results:
        ctx = f"twin of envs [{e0}, {e0 + Es})"
        noise = gumbel_noise(SEED, D0, K, (Es, N), DEV, first_row=e0 * N)
        assert same_bits(noise, job_noise[:, e0:e0 + Es]), f"{ctx}: the noise at first_row = e0 * N is the job's rows"
        twin = make(case, e0, Es)
        assert twin.sampling is None
        rt = run(twin, x["pol"], x["crit"], x["act0"][e0:e0 + Es].contiguous(), K, noise, True)
        assert_shard_is_slice(rt, rs, 0, Es, True, ctx)
        assert_job(rt, [rs], ctx)


def test_shard_registered_at_row_0_draws_shard_0s_noise():
    """A shard with e0 > 0 that registers first_row = 0 (what every rank did before first_row existed) does not
    reproduce the whole job's slice: its actions differ. It draws what shard 0 draws: it equals its twin given
    gumbel_noise(SEED, D0, K, (Es, N)), and that tensor is rows [0, Es * N) of the job's noise."""
    case = "4x64ar-2+2"
    c = CASES[case]
    E, N, K = c["E"], c["N"], c["K"]
    rw, results, x = run_job(case, True, "sampled")
    e0, Es, right = results[1]
    assert e0 == 2 and Es == 2
    act0 = x["act0"][e0:e0 + Es].contiguous()
    bad = make(case, e0, Es)
    bad.set_sampling(SEED, D0, first_row=0)
    assert bad.world.sampling_first_row == 0 and bad.first_row == e0 * N
    rb = run(bad, x["pol"], x["crit"], act0, K, None, True)
    assert not torch.equal(rb["acts"], rw["acts"][:, e0:e0 + Es]), "registered at row 0, the shard must not draw the job's rows"
    assert torch.equal(right["acts"], rw["acts"][:, e0:e0 + Es])
    noise0 = gumbel_noise(SEED, D0, K, (Es, N), DEV)  # first_row = 0
    assert same_bits(noise0, gumbel_noise(SEED, D0, K, (E, N), DEV)[:, :Es]), "rows [0, Es * N) of the job's noise"
    twin = make(case, e0, Es)
    rt = run(twin, x["pol"], x["crit"], act0, K, noise0, True)
    assert_shard_is_slice(rt, rb, 0, Es, True, "registered at row 0: shard 0's draw")
    assert len(torch.unique(rb["acts"])) == 3


# ---- first_row against a world's rows ----------------------------------------------------------------------------
def test_first_row_refusals_and_read_back():
    E, N = 3, 8
    vec = FlockVec(E, n_agents=[N], seed=1, device=DEV, env_offset=3)
    w = vec.world
    assert vec.first_row == 3 * N and w.sampling_first_row == 0 and vec.sampling is None
    vec.set_sampling(SEED)
    assert vec.sampling == (SEED, 0) and w.sampling_first_row == 3 * N == vec.first_row
    vec.set_sampling(SEED, 40, first_row=17)
    assert vec.sampling == (SEED, 40) and w.sampling_first_row == 17
    # first_row + E * N > 2**32: refused, the registration left as it was
    top = 2**32 - E * N
    for bad in (top + 1, 2**32):
        with pytest.raises(MacmError, match="first_row") as ei:
            vec.set_sampling(7, 1, first_row=bad)
        assert ei.value.code == _abi.E_INVALID
        assert vec.sampling == (SEED, 40) and w.sampling_first_row == 17
    cfg = _abi.MacmSampleConfig(7, 1, (ctypes.c_int32 * 4)(0, 0, 0, 0))
    assert w.L.macm_world_set_sampling_at(w.h, ctypes.byref(cfg), -1) == _abi.E_INVALID
    assert b"first_row" in w.L.macm_last_error()
    bad_cfg = _abi.MacmSampleConfig(7, 1, (ctypes.c_int32 * 4)(0, 1, 0, 0))
    assert w.L.macm_world_set_sampling_at(w.h, ctypes.byref(bad_cfg), 5) == _abi.E_INVALID
    assert w.L.macm_world_get_sampling_row(w.h, None) == _abi.E_INVALID
    assert vec.sampling == (SEED, 40) and w.sampling_first_row == 17
    for bad in (-1, 2**32 + 1, 2**64):  # outside what the Python layer hands to an int64
        with pytest.raises(ValueError, match="first_row"):
            vec.set_sampling(7, 1, first_row=bad)
    # the last rows a 32-bit word can name are accepted
    vec.set_sampling(SEED, 40, first_row=top)
    assert w.sampling_first_row == top
    row = ctypes.c_int64(-5)
    assert w.L.macm_world_get_sampling_row(w.h, ctypes.byref(row)) == 1 and row.value == top
    # the entry point without _at registers row 0
    assert w.L.macm_world_set_sampling(w.h, ctypes.byref(cfg)) == 0
    assert vec.sampling == (7, 1) and w.sampling_first_row == 0
    # set_sampling(None) clears it
    vec.set_sampling(SEED, 40, first_row=17)
    vec.set_sampling(None)
    assert vec.sampling is None and w.sampling_first_row == 0
    assert w.L.macm_world_get_sampling_row(w.h, ctypes.byref(row)) == 0 and row.value == 0
    # an env_offset whose rows have no 32-bit row word: an explicit first_row is asked for
    far = FlockVec(E, n_agents=[N], seed=1, device=DEV, env_offset=2**29)
    with pytest.raises(ValueError, match="explicit first_row"):
        far.set_sampling(SEED)
    with pytest.raises(ValueError, match="explicit first_row"):
        _ = far.first_row
    assert far.sampling is None
    far.set_sampling(SEED, first_row=5)
    assert far.world.sampling_first_row == 5
