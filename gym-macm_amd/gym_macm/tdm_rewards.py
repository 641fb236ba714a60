"""Rewards for cm-tdm-v0 composed from the combat events (TdmWorld.set_events, macm_tdm_set_events).

Not from the reference: its TDM has no reward (combat.py:203-204, ``get_rewards`` is ``pass``) and
``step`` returns only the observation. The device exports the facts, who damaged whom in each step
(``hit_id``), next to health, alive, done and winner; this module turns them into per-agent terms and
a weighted sum in plain torch, on whatever device the tensors live on (CPU tensors included), so that
a user can swap in a reward of their own without touching device code.

Shapes: ``[..., E, N]`` per agent and ``[..., E]`` per env; leading dimensions broadcast, so the
``[K, E, N]`` rows of a trajectory rollout work as they are. ``team`` is ``[N]`` (TdmWorld.team).
"""
from __future__ import annotations

import torch


def _team(team, ref: torch.Tensor) -> torch.Tensor:
    return torch.as_tensor(team, device=ref.device).to(torch.int64)


def combat_events(hit_id: torch.Tensor, team, alive_before: torch.Tensor):
    """(hit_enemy, hit_ally, hurt), int32 ``[..., E, N]``, of the step(s) ``hit_id`` describes:

    hit_enemy[i] = 1 when agent i's attack damaged a body of another team (v = hit_id[i] >= 0 and
    team[v] != team[i]); hit_ally[i] = 1 when it damaged a body of its own team, itself included (the
    literal listener sends most damage to the last body any cast hit); hurt[j] = the number of
    attackers whose attack damaged j. All three are zero for agents dead at the step's start
    (``alive_before`` 0): such an agent cannot attack, and the damage a stale listener still books on a
    dead body is no signal for anyone."""
    team = _team(team, hit_id)
    N = hit_id.shape[-1]
    live = alive_before.to(torch.bool)
    valid = hit_id >= 0
    v = hit_id.clamp(min=0).to(torch.int64)
    same = team[v] == team  # team of the victim against the attacker's own
    hit_enemy = (valid & ~same & live).to(torch.int32)
    hit_ally = (valid & same & live).to(torch.int32)
    hurt = torch.zeros(hit_id.shape[:-1] + (N + 1,), dtype=torch.int32, device=hit_id.device)
    hurt.scatter_add_(-1, torch.where(valid, v, torch.full_like(v, N)), torch.ones_like(hit_id, dtype=torch.int32))
    hurt = hurt[..., :N] * live.to(torch.int32)
    return hit_enemy, hit_ally, hurt


def combat_rewards(hit_id: torch.Tensor, alive_before: torch.Tensor, alive: torch.Tensor, done: torch.Tensor,
                   done_before: torch.Tensor, winner: torch.Tensor, team, hit_enemy: float = 1.0,
                   hit_ally: float = -1.0, hurt: float = -1.0, death: float = -1.0, win: float = 4.0,
                   loss: float = -4.0) -> torch.Tensor:
    """float32 ``[..., E, N]``:

        r = hit_enemy * hit_enemy_i + hit_ally * hit_ally_i + hurt * hurt_i + death * died_i
            + win * won_i + loss * lost_i

    as float32 terms added in that order. died = alive_before & ~alive. won / lost apply only on the
    step where ``done`` first becomes set (done & ~done_before) and only with winner >= 0 (a time
    limit has no winner): won for every member of the winning team, alive or not, lost for every
    member of the other teams. ``done``, ``done_before`` and ``winner`` are ``[..., E]``."""
    teamt = _team(team, hit_id)
    he, ha, hu = combat_events(hit_id, teamt, alive_before)
    died = alive_before.to(torch.bool) & ~alive.to(torch.bool)
    ended = (done.to(torch.bool) & ~done_before.to(torch.bool) & (winner >= 0)).unsqueeze(-1)
    mine = teamt == winner.to(torch.int64).unsqueeze(-1)
    f = torch.float32
    r = torch.tensor(hit_enemy, dtype=f, device=hit_id.device) * he.to(f)
    for wgt, term in ((hit_ally, ha), (hurt, hu), (death, died), (win, ended & mine), (loss, ended & ~mine)):
        r = r + torch.tensor(wgt, dtype=f, device=hit_id.device) * term.to(f)
    return r


def trajectory_alive_before(alive0: torch.Tensor, alive: torch.Tensor, done: torch.Tensor,
                            autoreset: bool = False) -> torch.Tensor:
    """``alive_before`` [K, E, N] (uint8) of a trajectory: row 0 is ``alive0`` [E, N] (the world's
    ``alive`` before the rollout), row k is ``alive[k - 1]``; with ``autoreset``, row k is all ones
    where ``done[k - 1]``: the env was reset before step k, and the trajectory's alive row keeps the
    terminal step's."""
    before = torch.cat([alive0.to(alive.dtype).unsqueeze(0), alive[:-1]], dim=0)
    if autoreset and alive.shape[0] > 1:
        reset = done[:-1].to(torch.bool).unsqueeze(-1)
        before[1:] = torch.where(reset, torch.ones_like(before[1:]), before[1:])
    return before
