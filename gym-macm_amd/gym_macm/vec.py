"""FlockVec — the batched throughput API for cm-flock-v0.

E independent Flock envs (reference gym_macm/envs/mvmnt.py) stepped by one HIP
launch per step, with actions and outputs as device tensors:

    env = FlockVec(num_envs=4096, n_agents=[64], seed=0)
    obs, nbr_id = env.obs, env.nbr_id            # initial observation
    obs, nbr_id, reward, done = env.step(actions)  # actions uint8 [E, N, 3] on the GPU

Env e is the reference env constructed after ``random.seed(seed + env_offset + e)``;
each env keeps that stream on the device, so ``reset_envs(mask)`` / ``autoreset=True``
start new episodes exactly as the env's own ``reset()`` would draw them.
With ``autoreset=True, final_obs=True`` the observation each ended episode ended on, which the
reset overwrites in the step's outputs, is kept per env in ``final_obs`` / ``final_nbr_id``, with
``final_length`` and ``final_ends`` (a gym VecEnv's ``info["terminal_observation"]`` is
``final_obs[done]``).
``seed`` must be >= 0 and every env's seed ``seed + env_offset + e`` must lie in [0, 2**64): the
C-ABI cannot honour ``random.seed``'s meaning outside it (a negative seed's absolute value, keys of
three or more words), so the constructor and ``reset`` raise ValueError there (World.reset).
Shard a job over GPUs by giving each rank its contiguous ``env_offset``; ``set_sampling`` then draws the
job's rows (``first_row``), so sampled policy rollouts are those of the whole job too.
Settings keyword arguments are the reference's (flockSettings, settings.py:110-146).
Returned tensors are views of buffers reused by the next call.
"""
from __future__ import annotations

import numpy as np
import torch

from gym_macm.settings import flockSettings, to_config
from gym_macm.world import World


class FlockVec(object):
    def __init__(self, num_envs, n_agents=(10,), targets=None, seed=0, env_offset=0, device=None,
                 obs_dtype=torch.float32, max_contacts=0, autoreset=False, validate_actions=False, final_obs=False,
                 **kwargs):
        self.settings = flockSettings(**kwargs)
        self.num_envs = int(num_envs)
        self.n_agents = list(n_agents) if not isinstance(n_agents, int) else [n_agents]
        N = int(sum(self.n_agents))
        self.n_targets = 1 if targets is None else len(np.unique(targets))
        self.targets_idx = np.zeros(N, np.int32) if targets is None else np.asarray(targets, np.int32)
        cfg = to_config(self.settings, N, self.n_targets, obs_f64=(obs_dtype == torch.float64),
                        validate_actions=validate_actions)
        self.world = World(cfg, self.targets_idx, self.num_envs, device=device, max_contacts=max_contacts)
        self.device = self.world.device
        self.N = N
        self.seed = int(seed)
        self.env_offset = int(env_offset)
        self.autoreset = bool(autoreset)
        if self.autoreset:
            self.world.set_autoreset(True)
        if final_obs:  # the ended episodes' last observations (World.set_final_outputs)
            self.world.set_final_outputs(True)
        self.obs, self.nbr_id = self.world.reset(self.seed, self.env_offset)

    @property
    def obs_dim(self):
        return self.world.OD

    # final_obs=True: what the autoreset overwrote, per env (World.set_final_outputs); None otherwise
    @property
    def final_obs(self):
        """[E, N, OD]: row e is the observation env e's last ended episode ended on."""
        return self.world.final_obs

    @property
    def final_nbr_id(self):
        return self.world.final_nbr_id

    @property
    def final_length(self):
        """[E] int32: the steps of env e's last ended episode."""
        return self.world.final_length

    @property
    def final_ends(self):
        """[E] int32: env e's episode ends since the tensor was last zeroed."""
        return self.world.final_ends

    def reset(self, seed=None):
        if seed is not None:
            self.seed = int(seed)
        self.obs, self.nbr_id = self.world.reset(self.seed, self.env_offset)
        return self.obs, self.nbr_id

    def step(self, actions):
        """One step of every env. With ``autoreset``, envs whose episode ended in this
        step start their next episode right away (reset_envs on the done flags, on
        the device): the returned done marks them and obs already holds the new
        episode's initial observation for those envs (with ``final_obs=True`` the observation the
        episode ended on is ``final_obs[done]``).

        Raises MacmOverflowError (a MacmLibraryError) once an earlier step has overflowed a
        capacity (the contact list's max_contacts; dense touching contacts never overflow: the
        spill step takes them) — on the first call after the device reported it, which without a
        synchronisation may be a few queued steps later (check_status() is exact) —
        MacmInvalidActionError with ``validate_actions=True`` and an
        action outside the action space (no env is stepped, as the reference asserts first)."""
        return self.world.step(actions)

    def rollout(self, actions, trajectory=False, traj=None):
        """K steps of every env with actions given in advance ([K, E, N, 3] on the device, e.g. a
        random-action rollout), one launch (World.rollout): each env runs its K steps back to back.
        Same results as K step() calls; returns the last step's outputs, or with
        ``trajectory=True`` every step's (World.rollout_traj: a dict of [K, ...] tensors, written
        into ``traj`` if given). With ``autoreset`` an env whose episode ends at step k restarts
        inside the launch before step k + 1 (World.set_autoreset): row k keeps the terminal done,
        reward and collided, and its obs / nbr_id hold the new episode's initial observation."""
        if trajectory:
            return self.world.rollout_traj(actions, traj)
        return self.world.rollout(actions)

    def rollout_bots(self, actions, n_steps, trajectory=False, traj=None):
        """n_steps of the closed loop step -> bots.flock -> step in one launch (World.rollout_bots);
        ``actions`` (uint8 [E, N, 3]) holds the first step's actions on entry, the next on return.
        ``trajectory=True``: actions is [n_steps + 1, E, N, 3] and every step's outputs and actions
        are kept (World.rollout_bots_traj). With ``autoreset`` the envs that end restart inside the
        launch, and the bot's next action of such an env is taken from its new initial observation,
        as in the loop step -> reset_envs(done) -> bots."""
        if trajectory:
            return self.world.rollout_bots_traj(actions, n_steps, traj)
        return self.world.rollout_bots(actions, n_steps)

    def set_policy(self, policy) -> None:
        """Register the actor of rollout_policy: a gym_macm.policy.MlpPolicy, or None (World.set_policy)."""
        self.world.set_policy(policy)

    def set_critic(self, critic) -> None:
        """Register the critic of rollout_policy(..., values=, boot=): a gym_macm.policy.MlpCritic, or None
        (World.set_critic)."""
        self.world.set_critic(critic)

    @property
    def first_row(self) -> int:
        """The job's flat row of this shard's row 0, ``env_offset * N``: what set_sampling registers by
        default, and what the first actions take (``pol.act(vec.obs, seed=seed, decision=0,
        first_row=vec.first_row)``). ValueError where it is negative or row 0 has no 32-bit row word."""
        row = self.env_offset * self.N
        if not (0 <= row and row + self.num_envs * self.N <= 1 << 32):
            raise ValueError(f"env_offset * N = {row} does not name this shard's rows in [0, 2**32): "
                             "pass an explicit first_row to set_sampling")
        return row

    def set_sampling(self, seed, decision: int = 0, first_row=None) -> None:
        """Sample the actions of rollout_policy inside the launch (World.set_sampling): no noise tensor,
        reproducible from (seed, decision index) however the steps are cut into launches and however the job's
        envs are split over ranks: ``first_row=None`` registers ``env_offset * N``, so every shard draws the
        whole job's noise for its envs (ValueError where that is negative or does not fit: name a first_row).
        ``seed=None``: off."""
        if seed is None:
            return self.world.set_sampling(None)
        self.world.set_sampling(seed, decision, self.first_row if first_row is None else first_row)

    @property
    def sampling(self):
        """(seed, next decision index) with sampling on, else None (World.sampling)."""
        return self.world.sampling

    def rollout_policy(self, actions, n_steps, noise=None, trajectory=False, traj=None, logits=None, values=None,
                       boot=None):
        """n_steps of the closed loop step -> policy -> step in one launch, beside rollout_bots: the
        registered MlpPolicy acts on the observation each step wrote (World.rollout_policy). ``noise``
        [n_steps, E, N, 9] samples (None: argmax, or after ``set_sampling`` the launch's own draw);
        ``logits`` keeps what the policy computed. With
        ``autoreset`` an env that ends restarts inside the launch and acts on its new initial obs.
        ``values`` / ``boot``: the registered critic's V of every row and the bootstrap value of every
        step, from the same launch."""
        return self.world.rollout_policy(actions, n_steps, noise=noise, trajectory=trajectory, traj=traj, logits=logits,
                                         values=values, boot=boot)

    def reset_envs(self, mask=None):
        """New episodes in the masked envs (see World.reset_envs)."""
        return self.world.reset_envs(mask)

    def observe(self):
        return self.world.observe()

    def get_state(self):
        return self.world.get_state()

    def set_state(self, state):
        self.world.set_state(state)

    def status(self):
        return self.world.status()

    def check_status(self):
        """Raise MacmOverflowError if any env overflowed a capacity (synchronises)."""
        self.world.check_status()

    def spilled(self):
        """Env-steps taken by the spill step (dense envs) since creation."""
        return self.world.spilled()

    def counters(self):
        return self.world.counters()

    def reward_sums(self):
        """(per-env reward totals [E] float64, their sum in env order); World.reward_sums."""
        return self.world.reward_sums()
