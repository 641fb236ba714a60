"""The wave step kernel tests only the moved fat AABBs for new pairs (b2BroadPhase::UpdatePairs
queries the move buffer): every case steps the HIP world beside the CPU oracle and compares, after
every step, the state, the ordered contact list with its impulses, nbr_id, reward, collided, done,
the observations and the counters. Each case also counts, per env and step, the oracle's moved
proxies (fat AABB differs from the step before) and asserts the coverage it is there for, so that
none passes without having walked the moved-record loop at the lengths it names."""
import numpy as np
import pytest
import torch

from parity import assert_state_equal
from test_gpu_parity import make_pair, obs_check, rand_actions

pytestmark = pytest.mark.gpu

BENCH_SEED = 0x6D61636D


class Pair:
    """A HIP world and its oracle stepped together; moved[t][e]: the oracle's moved proxies."""

    def __init__(self, vec, orc, obs_f64=False):
        self.vec, self.orc, self.obs_f64 = vec, orc, obs_f64
        self.C = vec.world.C
        self.fat = orc.get_state(self.C)["fat"].copy()
        self.moved = []
        self.ctr = np.zeros(4, np.int64)
        self.t = 0
        vec.world.reset_counters()

    def account(self, r):
        """The oracle's step t: moved counts, counters; returns its state."""
        so = self.orc.get_state(self.C)
        self.moved.append((so["fat"] != self.fat).any(-1).sum(-1))
        self.fat = so["fat"].copy()
        E, N = r["collided"].shape
        self.ctr += (E * N, int(r["collided"].sum()), int((r["reward"] > 0).sum()), int(r["done"].sum()))
        return so

    def step(self, a):
        vec, t = self.vec, self.t
        obs, nbr, rew, done = vec.step(torch.from_numpy(a).cuda())
        r = self.orc.step(a)
        so = self.account(r)
        np.testing.assert_array_equal(rew.cpu().numpy(), r["reward"].astype(np.float32), err_msg=f"reward step {t}")
        np.testing.assert_array_equal(nbr.cpu().numpy(), r["nbr_id"], err_msg=f"nbr step {t}")
        np.testing.assert_array_equal(done.cpu().numpy(), r["done"], err_msg=f"done step {t}")
        np.testing.assert_array_equal(vec.world.collided.cpu().numpy(), r["collided"], err_msg=f"coll step {t}")
        obs_check(obs.cpu().numpy(), r["obs"], self.obs_f64, f"step {t}")
        assert_state_equal(vec.get_state(), so, f"step {t}")
        np.testing.assert_array_equal(vec.counters(), self.ctr, err_msg=f"counters step {t}")
        assert vec.status() == 0
        self.t += 1
        return r, so

    def moved_counts(self):
        return np.array(self.moved)


def test_from_reset_metric_shape():
    """A: 64 envs x 64 agents from reset with the benchmark's seed, 30 single-step launches."""
    E, N = 64, 64
    vec, orc = make_pair(E, [N], seed=BENCH_SEED)
    p = Pair(vec, orc)
    rng = np.random.default_rng(BENCH_SEED + 1)
    for _ in range(30):
        p.step(rand_actions(rng, E, N))
    mv = p.moved_counts()
    assert mv.min() == 0 and mv.max() >= 8, (mv.min(), mv.max())


def fast_start(E, N, seed):
    """The reset state with velocities of magnitude 20 in uniform random directions, in both worlds."""
    vec, orc = make_pair(E, [N], seed=seed)
    st = orc.get_state(vec.world.C)
    th = np.random.default_rng(5).uniform(0.0, 2.0 * np.pi, size=(E, N))
    st["vel"] = (20.0 * np.stack([np.cos(th), np.sin(th)], -1)).astype(np.float32)
    orc.set_state(st)
    vec.set_state(st)
    return vec, orc


@pytest.mark.parametrize("N", [64, 33, 12])
def test_all_moved(N):
    """B: every proxy of an env moves in one step (both row words, the dummy lanes, NCAP 32 and 64),
    none in another; the same start as one rollout launch and as a trajectory rollout."""
    E, K = 8, 8
    acts = np.random.default_rng(6).integers(0, 3, size=(K, E, N, 3)).astype(np.uint8)
    vec, orc = fast_start(E, N, 11)
    p = Pair(vec, orc)
    steps = [p.step(acts[k]) for k in range(K)]
    mv = p.moved_counts()
    assert mv.max() == N, mv.max()
    if N < 64:
        assert mv.min() == 0, mv.min()
    final = steps[-1][1]

    dev = torch.from_numpy(acts).cuda()
    vec1, _ = fast_start(E, N, 11)
    vec1.world.reset_counters()
    obs, nbr, rew, done = vec1.rollout(dev)
    last = steps[-1][0]
    np.testing.assert_array_equal(rew.cpu().numpy(), last["reward"].astype(np.float32), err_msg="rollout reward")
    np.testing.assert_array_equal(nbr.cpu().numpy(), last["nbr_id"], err_msg="rollout nbr")
    np.testing.assert_array_equal(vec1.world.collided.cpu().numpy(), last["collided"], err_msg="rollout coll")
    obs_check(obs.cpu().numpy(), last["obs"], False, "rollout")
    assert_state_equal(vec1.get_state(), final, "rollout")
    np.testing.assert_array_equal(vec1.counters(), p.ctr, err_msg="rollout counters")
    assert vec1.status() == 0

    vec2, _ = fast_start(E, N, 11)
    vec2.world.reset_counters()
    tr = {k: v.cpu().numpy() for k, v in vec2.rollout(dev, trajectory=True).items()}
    for k in range(K):
        r = steps[k][0]
        np.testing.assert_array_equal(tr["reward"][k], r["reward"].astype(np.float32), err_msg=f"traj reward {k}")
        np.testing.assert_array_equal(tr["nbr_id"][k], r["nbr_id"], err_msg=f"traj nbr {k}")
        np.testing.assert_array_equal(tr["collided"][k], r["collided"], err_msg=f"traj coll {k}")
        np.testing.assert_array_equal(tr["done"][k], r["done"], err_msg=f"traj done {k}")
        obs_check(tr["obs"][k], r["obs"], False, f"traj step {k}")
    assert_state_equal(vec2.get_state(), final, "trajectory rollout")
    np.testing.assert_array_equal(vec2.counters(), p.ctr, err_msg="trajectory counters")
    assert vec2.status() == 0


@pytest.mark.parametrize("E,steps,obs_dtype", [(2100, 5, torch.float32), (32, 10, torch.float64)])
def test_other_instantiations(E, steps, obs_dtype):
    """C: the scalar-sweep instantiation (>= 2048 envs) and float64 observations, from reset."""
    N = 64
    vec, orc = make_pair(E, [N], seed=BENCH_SEED, obs_dtype=obs_dtype)
    p = Pair(vec, orc, obs_f64=obs_dtype == torch.float64)
    rng = np.random.default_rng(3)
    for _ in range(steps):
        p.step(rand_actions(rng, E, N))
    mv = p.moved_counts()
    assert mv.min() == 0 and mv.max() >= 2, (mv.min(), mv.max())


def test_injected_list_lacking_a_resting_overlap():
    """D: two resting bodies whose fat AABBs overlap, injected with an empty list. Box2D creates the
    contact only once one of the two proxies moves: never while both idle, then at the step in which
    the pushed agent's fat AABB is first rewritten."""
    E, N = 1, 6
    vec, orc = make_pair(E, [N], seed=3)
    st = orc.get_state(vec.world.C)
    pos = np.array([[0, 0], [1.15, 0], [10, 10], [-10, 10], [10, -10], [-10, -10]], np.float32)
    hw = np.float32(vec.world.cfg.radius) + np.float32(0.1)
    assert 2 * vec.world.cfg.radius < 1.15 < 2 * hw  # apart, fat AABBs overlapping
    st["pos"][0] = pos
    st["fat"][0] = np.concatenate([pos - hw, pos + hw], -1)
    for k in ("vel", "angle", "sleep", "contact_ab", "contact_imp"):
        st[k][:] = 0
    st["contact_count"][:] = 0
    orc.set_state(st)
    vec.set_state(st)
    p = Pair(vec, orc)
    counts = []
    for t in range(15):
        a = np.ones((E, N, 3), np.uint8)
        if t >= 3:
            a[0, 0, 0] = 2  # push agent 0 forward (angle 0: towards agent 1)
        r, so = p.step(a)
        counts.append(int(so["contact_count"][0]))
    mv = p.moved_counts()[:, 0]
    first = counts.index(1)
    assert first > 3 and counts[:first] == [0] * first and mv[:first].sum() == 0 and mv[first] == 1, (counts, mv)
