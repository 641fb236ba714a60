"""numpy float32 restatement of the Flock rollout kernels' nearest neighbour from per-agent candidate
lists (csrc/flock_step_w64.hip, above near_build): the rule, with the kernel's arithmetic and margins.

At a rebuild step agent i keeps S_i = { j != i : d2(i, j) <= thr2_i } and its position c0_i, where
thr2_i = ((sqrt(best_i) + s)^2) (1 + 2^-18) in float32 and best_i is the plain sweep's squared
distance. The lists are valid while every agent's float32 squared displacement from c0 is at most
(s / 4)^2 (1 - 2^-20). While valid, the nearest of S_i in ascending j with strict '<' is the plain
sweep's nearest. An env in which a list exceeds the cap at a rebuild takes the plain sweep for the
next RETRY steps before it tries again, and for twice as many after every further failure in a row,
up to RETRY_MAX.

Every float32 operation is rounded on its own (numpy float32 arrays), as the kernel is compiled
without contraction. The square root is numpy's correctly rounded one, the kernel's is within an
ulp: a record exactly at a threshold may be in one mask and not the other, the nearest is the same."""
import numpy as np

S = np.float32(1.0)
CAP = 12
RETRY, RETRY_MAX = 8, 64
PAD = np.float32(1.0) + np.float32(2.0 ** -18)
MOVE2 = (S * np.float32(0.25)) * (S * np.float32(0.25)) * (np.float32(1.0) - np.float32(2.0 ** -20))
PLAIN, LIST, REBUILD = 0, 1, 2
NONE, VALID, DENSE = 0, 1, 2  # DENSE + n: n more plain steps before the retry

_INF = np.float32(np.inf)


def d2_matrix(pos):
    """[N, N] float32: row i holds the sweep's d2 of agent i to every j (other - self, each product
    and the sum rounded on their own); the diagonal is +inf (self is never taken)."""
    pos = np.ascontiguousarray(pos, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = pos[None, :, 0] - pos[:, None, 0]
        dy = pos[None, :, 1] - pos[:, None, 1]
        d2 = dx * dx + dy * dy
    assert d2.dtype == np.float32
    np.fill_diagonal(d2, _INF)
    return d2


def _scan(d2):
    """Ascending j, strict '<' from best = +inf, bj = 1 for agent 0 and 0 for the others."""
    N = d2.shape[0]
    with np.errstate(invalid="ignore"):
        key = np.where(d2 < _INF, d2, _INF)  # a NaN or +inf record is never taken
    bj = key.argmin(axis=1).astype(np.int32)  # the first of equal minima: the lowest index
    best = key[np.arange(N), bj]
    none = ~(best < _INF)
    bj[none] = np.where(np.arange(N) == 0, 1, 0)[none]
    return best, bj


def plain_nearest(pos):
    """The all-pairs sweep: (best d2 float32 [N], index int32 [N])."""
    return _scan(d2_matrix(pos))


class NearLists:
    """The list state of one env, stepped with the env's final positions of each step."""

    def __init__(self, s=S, cap=CAP, retry=RETRY, retry_max=RETRY_MAX):
        self.s, self.cap, self.retry, self.retry_max = np.float32(s), int(cap), int(retry), int(retry_max)
        self.failed = 0  # the plain steps after the last failed rebuild (0: the last rebuild succeeded)
        self.pad, self.move2 = PAD, (self.s * np.float32(0.25)) * (self.s * np.float32(0.25)) * (
            np.float32(1.0) - np.float32(2.0 ** -20))
        self.clear()

    def clear(self):
        """No list: a launch's first step, a spill step, a raised status bit, an in-launch reset."""
        self.state, self.mask, self.c0 = NONE, None, None

    def step(self, pos, may_build=True):
        """-> (best, bj, kind, largest list). may_build False: a step that may only use or clear the
        lists (the carried kernel's loading steps)."""
        pos = np.ascontiguousarray(pos, np.float32)
        N = pos.shape[0]
        d2 = d2_matrix(pos)
        if N < 2:
            self.clear()
            return (*_scan(d2), PLAIN, 0)
        if self.state >= DENSE:
            self.state = NONE if self.state == DENSE else self.state - 1
            return (*_scan(d2), PLAIN, 0)
        if not may_build:
            self.clear()
            return (*_scan(d2), PLAIN, 0)
        if self.state == VALID:
            m = pos - self.c0
            m2 = m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]
            if bool((m2 <= self.move2).all()):  # a NaN fails it
                best, bj = _scan(np.where(self.mask, d2, _INF))
                return best, bj, LIST, int(self.mask.sum(axis=1).max())
        best, bj = _scan(d2)
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.sqrt(best) + self.s
            thr2 = t * t * self.pad
            mask = d2 <= thr2[:, None]
        np.fill_diagonal(mask, False)
        largest = int(mask.sum(axis=1).max())
        self.mask, self.c0 = mask, pos.copy()
        if largest <= self.cap:
            self.state, self.failed = VALID, 0
        else:
            self.failed = self.retry if self.failed == 0 else min(2 * self.failed, self.retry_max)
            self.state = DENSE + self.failed - 1
        return best, bj, REBUILD, largest


def run_trace(trace, first_step_plain=False, **kw):
    """trace [K, E, N, 2]: every env's lists over the K steps. Returns (wrong, kinds [K, E], largest
    [K, E]); wrong counts the agent-steps whose (best, index) differ from the plain sweep's."""
    K, E = trace.shape[:2]
    kinds = np.zeros((K, E), np.int8)
    largest = np.zeros((K, E), np.int32)
    wrong = 0
    for e in range(E):
        nl = NearLists(**kw)
        for k in range(K):
            best, bj, kinds[k, e], largest[k, e] = nl.step(trace[k, e], may_build=not (first_step_plain and k == 0))
            pb, pj = plain_nearest(trace[k, e])
            wrong += int(((bj != pj) | (best.view(np.uint32) != pb.view(np.uint32))).sum())
    return wrong, kinds, largest


def oracle_trace(E, N, K, seed, act_seed=1, **kw):
    """[K, E, N, 2] float32: the CPU oracle's positions after each of K steps from the reset under
    uniform random discrete actions (also returned: [K, E, N, 3] uint8)."""
    from gym_macm.settings import flockSettings, to_config
    from parity import oracle_for
    orc = oracle_for(to_config(flockSettings(**kw), N, 1, obs_f64=True), None, E, seed)
    rng = np.random.default_rng(act_seed)
    acts = rng.integers(0, 3, size=(K, E, N, 3)).astype(np.uint8)
    trace = np.zeros((K, E, N, 2), np.float32)
    for k in range(K):
        orc.step(acts[k])
        trace[k] = orc.get_state(N * N)["pos"]
    return trace, acts
