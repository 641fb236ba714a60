"""The clipped PPO loss on device (include/macm.h, macm_ppo_loss): log-probabilities from stored logits, the
loss under torch.autograd, and the loss fused into the gradient launches.

    # the rows of a trajectory launch, each decision beside its own reward: views, nothing copied or launched
    t = ppo.transitions(traj, acts, lg, vals, boot)        # row j: obs[j], logits[j] -> acts[j + 1], reward[j + 1]
    adv, ret = gae(t["reward"], t["values"], t["boot"], t["done"], 0.99, 0.95)
    obs, actions, old_values = t["obs"], t["actions"], t["values"]
    old_logp = ppo.log_prob(t["logits"], actions)          # once, from the logits rollout_policy stored
    pol.params.requires_grad_(True); crit.params.requires_grad_(True)
    # composed with the forward kernels: logits and dL/dlogits exist, nothing else per row is kept
    loss, stats = ppo.ppo_loss(pol.forward(obs), crit.forward(obs), actions, old_logp, adv, ret)
    loss.backward()
    # or fused: neither the logits nor dL/dlogits exist in memory, one launch per net
    stats = ppo.ppo_grads(pol, crit, obs, actions, old_logp, adv, ret)   # accumulates into params.grad
    opt.step()
    # epochs over shuffled minibatches with normalised advantages: nothing is gathered, nothing synchronises
    for mb in ppo.minibatches(obs.numel() // 4, 32, device=obs.device):      # int32 index lists, block-shuffled
        norm = ppo.adv_moments(adv, mb)                                    # float64 [4]: mean, rstd, std, n
        ppo.ppo_grads(pol, crit, obs, actions, old_logp, adv, ret, index=mb, adv_norm=norm)
        opt.step(); opt.zero_grad()
    # the optimiser on the device too: Adam, the global-norm clip and a KL gate in one launch per step ...
    opt = ppo.Adam(pol, crit, lr=3e-4, max_grad_norm=0.5, target_kl=0.03)   # opt.step(stats) in the loop above
    # ... and the whole update (moments -> fused gradients -> step, per minibatch) as one call, no synchronise
    epochs = [mb for _ in range(4) for mb in ppo.minibatches(obs.numel() // 4, 32, device=obs.device)]
    stats = ppo.update(opt, obs, actions, old_logp, adv, ret, minibatches=epochs)     # float64 [128, 8]

``stats`` is a float64 [8] device tensor: loss, policy_loss, value_loss, entropy, approx_kl, clip_frac,
ratio_max, rows. In the first epoch, with ``old_logp`` from ``log_prob`` on the rollout's own logits, the
ratio is exactly 1, approx_kl 0 and clip_frac 0. The means are over the rows of the call. A minibatch of
``ppo_grads`` is a contiguous slice of the leading dimension or, with ``index``, any list of rows
(macm_ppo_grad_rows), and ``adv_norm`` normalises its advantages on the way in with the moments
``adv_moments`` computed on the device. The autograd path (``ppo_loss`` with ``pol.forward``) keeps its
contiguous rows: a user of that path gathers and normalises with torch as before.

The per-row definition is float64 on the float32 inputs (include/macm.h). There is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch

from . import _abi
from .policy import N_LOGITS, _overlap, _stream

STATS = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_frac", "ratio_max", "rows")

_ws = {}  # device -> the workspace of ppo_loss on that device, grown on demand: calls belong on one stream


def config(clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.01, vf_clip: float = None):
    """The macm_ppo_config of these coefficients (vf_clip None: 0, read only where old values are given)."""
    return _abi.MacmPpoConfig(float(clip), float(vf_coef), float(ent_coef), 0.0 if vf_clip is None else float(vf_clip),
                              (ctypes.c_int32 * 4)(0, 0, 0, 0))


def workspace_bytes(rows: int) -> int:
    n = ctypes.c_int64(0)
    _abi.check(_abi.lib().macm_ppo_workspace(int(rows), ctypes.byref(n)), "macm_ppo_workspace")
    return int(n.value)


def _workspace(owner, rows, device):
    """The workspace for `rows` rows: the owner's (a net's, shared with param_grad) or this module's."""
    need = workspace_bytes(rows)
    ws = _ws.get(device) if owner is None else getattr(owner, "_grad_ws", None)
    if ws is None or ws.numel() < need:
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=device)
        if owner is None:
            _ws[device] = ws
        else:
            owner._grad_ws = ws
    return ws


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check(name, t, dev, dtype, shape):
    if t.device != dev or not t.is_contiguous() or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} {tuple(shape)} tensor on {dev}")


def _check_rows(dev, lead, actions, old_logp, adv, ret, old_values, policy: bool, value: bool):
    """The per-row inputs behind the logits / values (or the obs rows): what each half reads must be there."""
    if policy:
        for name, t in (("actions", actions), ("old_logp", old_logp), ("adv", adv)):
            if t is None:
                raise ValueError(f"{name} is needed with the policy's logits")
        _check("actions", actions, dev, torch.uint8, lead + (3,))
        _check("old_logp", old_logp, dev, torch.float32, lead)
        _check("adv", adv, dev, torch.float32, lead)
    if value:
        if ret is None:
            raise ValueError("ret is needed with the critic's values")
        _check("ret", ret, dev, torch.float32, lead)
        if old_values is not None:
            _check("old_values", old_values, dev, torch.float32, lead)
    for name, t in (("old_logp", old_logp), ("adv", adv), ("ret", ret), ("old_values", old_values)):
        if t is not None and t.requires_grad:
            raise ValueError(f"{name} must not require grad (the loss is differentiable in logits and values only)")
    if dev.type != "cuda":
        raise ValueError("the PPO loss runs on a GPU device (no CPU fallback)")


def _check_cfg(clip, vf_coef, ent_coef, vf_clip, old_values):
    if not clip > 0 or not vf_coef >= 0 or not ent_coef >= 0:
        raise ValueError("clip must be > 0, vf_coef and ent_coef >= 0")
    if old_values is not None and (vf_clip is None or not vf_clip > 0):
        raise ValueError("old_values needs vf_clip > 0")
    if old_values is None and vf_clip is not None:
        raise ValueError("vf_clip needs old_values")


def transitions(traj: dict, actions: torch.Tensor, logits: torch.Tensor, values: torch.Tensor,
                boot: torch.Tensor) -> dict:
    """The aligned rows of one trajectory launch of ``rollout_policy(..., trajectory=True, logits=, values=,
    boot=)``: a dict of obs, actions, logits, values, reward, done and boot whose row j holds one decision and
    what came of it, for the K - 1 decisions j = 0 .. K-2 that the launch both took and stepped.

    The launch's buffers are staggered (include/macm.h): step k executes action row k and writes reward[k],
    done[k], boot[k] and obs row k; the decision taken from obs row k, with noise row k, leaves its logits in
    logits row k, its action in actions row k + 1 and the value of the obs it saw in values row k + 1, and step
    k + 1 executes it. So decision j is

        obs[j], logits[j]  ->  actions[j + 1], values[j + 1]  ->  reward[j + 1], done[j + 1], boot[j + 1]

    and the result is ``traj["obs"][:K-1]``, ``actions[1:K]``, ``logits[:K-1]``, ``values[1:K]``,
    ``traj["reward"][1:]``, ``traj["done"][1:]`` and ``boot[1:]``: leading-dimension slices, so every entry is a
    contiguous view of its buffer. Nothing is copied, gathered or launched. ``gae`` on the result's reward,
    values, boot and done gives the advantage and return of each row's own action; ``log_prob`` on its logits
    and actions gives the old log-probabilities (the ratio of the first epoch is then exactly 1).

    Two decisions per launch are not among the rows. The decision of action row 0 is the caller's: it was taken
    before the launch (``pol.act(vec.obs)``), and its logits and its obs are not in the launch's buffers. The
    decision of action row K (from obs row K - 1, logits row K - 1) is taken by this launch but stepped by the
    next one, whose action row 0 it is: its reward is not known yet.

    traj holds obs [K, E, N, OD], reward [K, E, N] and done [K, E]; actions is [K + 1, E, N, 3], logits
    [K, E, N, 9], values [K + 1, E, N] and boot [K, E, N]. ValueError: leading sizes that do not agree on one K,
    K < 2, a tensor that is not contiguous, or the overwrite form's shapes ([E, N, ...] with no step dimension)."""
    for f in ("obs", "reward", "done"):
        if traj.get(f) is None:
            raise ValueError(f"traj must hold obs, reward and done: {f} is missing")
    reward = traj["reward"]
    if reward.dim() != 3:
        raise ValueError("traj['reward'] must be [K, E, N]: the trajectory form (the overwrite form keeps no rows)")
    K, E, N = (int(d) for d in reward.shape)
    want = (("obs", traj["obs"], (K, E, N, None)), ("reward", reward, (K, E, N)), ("done", traj["done"], (K, E)),
            ("actions", actions, (K + 1, E, N, 3)), ("logits", logits, (K, E, N, N_LOGITS)),
            ("values", values, (K + 1, E, N)), ("boot", boot, (K, E, N)))
    for name, t, shape in want:
        if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
            raise ValueError(f"{name} is {list(t.shape)}: with reward [{K}, {E}, {N}] the trajectory form is "
                             f"{[s if s is not None else 'OD' for s in shape]} (obs, reward, done, logits and boot "
                             "have K rows, actions and values K + 1)")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: the rows are views of the launch's buffers")
    if K < 2:
        raise ValueError(f"K = {K}: a launch of fewer than 2 steps both takes and steps no decision")
    return dict(obs=traj["obs"][:K - 1], actions=actions[1:K], logits=logits[:K - 1], values=values[1:K],
                reward=reward[1:], done=traj["done"][1:], boot=boot[1:])


def log_prob(logits: torch.Tensor, actions: torch.Tensor, entropy: torch.Tensor = None) -> torch.Tensor:
    """logp (float32 [...]): the log-probability of actions (uint8 [..., 3]) under logits (float32 [..., 9]),
    in one launch (macm_policy_logp); entropy: float32 [...] or None, written with each row's entropy."""
    dev = logits.device
    if dev.type != "cuda":
        raise ValueError("log_prob runs on a GPU device (no CPU fallback)")
    if logits.dim() < 1 or logits.shape[-1] != N_LOGITS:
        raise ValueError(f"logits rows must have {N_LOGITS} values")
    lead = tuple(logits.shape[:-1])
    _check("logits", logits, dev, torch.float32, lead + (N_LOGITS,))
    _check("actions", actions, dev, torch.uint8, lead + (3,))
    if entropy is not None:
        _check("entropy", entropy, dev, torch.float32, lead)
        if _overlap(entropy, logits) or _overlap(entropy, actions):
            raise ValueError("entropy must not alias an input")
    logp = torch.empty(lead, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _abi.check(_abi.lib().macm_policy_logp(_p(logits.detach()), _p(actions), logits.numel() // N_LOGITS, _p(logp),
                                               _p(entropy), _stream(logits)), "macm_policy_logp")
    return logp


def _launch_loss(cfg, rows, dev, logits, actions, old_logp, adv, values, ret, old_values, scale, dlogits, dvalues,
                 stats):
    ws = _workspace(None, rows, dev)
    with torch.cuda.device(dev):
        _abi.check(_abi.lib().macm_ppo_loss(ctypes.byref(cfg), rows, _p(logits), _p(actions), _p(old_logp), _p(adv),
                                            _p(values), _p(ret), _p(old_values), _p(scale), _p(dlogits), _p(dvalues),
                                            _p(stats), _p(ws), ws.numel(),
                                            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "macm_ppo_loss")


class _PpoLoss(torch.autograd.Function):
    """(loss, stats) as a function of logits and values: the forward is a stats-only launch, the backward one
    launch that writes dL/dlogits and dL/dvalues with `scale` pointing at the incoming gradient. Only the
    inputs are kept."""

    @staticmethod
    def forward(ctx, logits, values, actions, old_logp, adv, ret, old_values, cfg):
        first = logits if logits is not None else values
        dev = first.device
        rows = first.numel() // (N_LOGITS if logits is not None else 1)
        stats = torch.empty((8,), dtype=torch.float64, device=dev)
        _launch_loss(cfg, rows, dev, logits, actions, old_logp, adv, values, ret, old_values, None, None, None, stats)
        ctx.cfg, ctx.rows, ctx.dev = cfg, rows, dev
        ctx.has = (logits is not None, values is not None, old_values is not None)
        ctx.save_for_backward(*[t for t in (logits, values, actions, old_logp, adv, ret, old_values) if t is not None])
        ctx.mark_non_differentiable(stats)
        return stats[0].to(torch.float32), stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss, _gstats):
        saved = list(ctx.saved_tensors)
        has_l, has_v, has_o = ctx.has
        logits = saved.pop(0) if has_l else None
        values = saved.pop(0) if has_v else None
        actions, old_logp, adv = (saved.pop(0), saved.pop(0), saved.pop(0)) if has_l else (None, None, None)
        ret = saved.pop(0) if has_v else None
        old_values = saved.pop(0) if has_o else None
        want_l = has_l and ctx.needs_input_grad[0]
        want_v = has_v and ctx.needs_input_grad[1]
        dlogits = torch.empty_like(logits) if want_l else None
        dvalues = torch.empty_like(values) if want_v else None
        if (want_l or want_v) and ctx.rows > 0:
            scale = gloss.to(torch.float32).reshape(1).contiguous()  # stays on the device: no synchronise
            _launch_loss(ctx.cfg, ctx.rows, ctx.dev, logits if want_l else None, actions, old_logp, adv,
                         values if want_v else None, ret, old_values if want_v else None, scale, dlogits, dvalues, None)
        return dlogits, dvalues, None, None, None, None, None, None


def ppo_loss(logits: torch.Tensor, values: torch.Tensor, actions: torch.Tensor, old_logp: torch.Tensor,
             adv: torch.Tensor, ret: torch.Tensor, old_values: torch.Tensor = None, clip: float = 0.2,
             vf_coef: float = 0.5, ent_coef: float = 0.01, vf_clip: float = None):
    """(loss, stats): the clipped PPO loss of logits (float32 [..., 9]) and values (float32 [...]) over actions
    (uint8 [..., 3]), old_logp, adv and ret (float32 [...]); old_values with vf_clip selects the clipped value
    loss. loss is a float32 scalar, differentiable in logits and values (it composes with MlpPolicy.forward /
    MlpCritic.forward); stats is float64 [8] (STATS). Either of logits and values may be None: that half of the
    loss is left out."""
    if logits is None and values is None:
        raise ValueError("logits and values are both None")
    _check_cfg(clip, vf_coef, ent_coef, vf_clip, old_values if values is not None else None)
    if logits is not None:
        if logits.dim() < 1 or logits.shape[-1] != N_LOGITS:
            raise ValueError(f"logits rows must have {N_LOGITS} values")
        dev, lead = logits.device, tuple(logits.shape[:-1])
        _check("logits", logits, dev, torch.float32, lead + (N_LOGITS,))
    else:
        dev, lead = values.device, tuple(values.shape)
    if values is not None:
        _check("values", values, dev, torch.float32, lead)
    _check_rows(dev, lead, actions, old_logp, adv, ret, old_values, logits is not None, values is not None)
    if actions is not None and actions.requires_grad:
        raise ValueError("actions must not require grad")
    cfg = config(clip, vf_coef, ent_coef, vf_clip)
    if values is None:
        ret = old_values = None
    if logits is None:
        actions = old_logp = adv = None
    return _PpoLoss.apply(logits, values, actions, old_logp, adv, ret, old_values, cfg)


def _check_index(index, dev):
    """index as the library takes it: int32, 1-D, contiguous, on dev (an int64 index is converted: a copy)."""
    if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64) or index.device != dev:
        raise ValueError(f"index must be a 1-D int32 (or int64) tensor on {dev}")
    return index.to(torch.int32).contiguous()


def minibatches(n_rows: int, n_minibatches: int, generator: torch.Generator = None, block: int = 64,
                device=None) -> list:
    """n_minibatches int32 index tensors on `device` that together hold every row of range(n_rows) exactly
    once: one epoch's minibatches for ``ppo_grads(index=...)`` and ``adv_moments``. The shuffle is over blocks of
    `block` consecutive rows (aligned to multiples of block; a short last block leads the first minibatch) and
    keeps the rows of a block in order; the minibatches' lengths differ by at most one block. block=1 is a full
    shuffle of the rows.

    Why 64 by default: 64 consecutive rows are one tile of the gradient kernel, and with 64 agents per env
    they are one env's agents at one step, so the minibatches still mix steps and envs freely. A
    block-shuffled gather loads whole cache lines; a row shuffle fetches a 128-byte line for each 16-byte
    obs row (and for each 4-byte old_logp, adv and ret), which is what ``ppo_grads`` pays with block=1.
    Plain torch: `generator` and `device` may be the CPU's."""
    n_rows, m, block = int(n_rows), int(n_minibatches), int(block)
    if n_rows < 0 or m < 1 or block < 1:
        raise ValueError("minibatches: n_rows >= 0, n_minibatches >= 1 and block >= 1")
    if n_rows >= 2 ** 31:
        raise ValueError("minibatches: an int32 index names at most 2^31 - 1 rows")
    n_blocks = -(-n_rows // block)
    gdev = generator.device if generator is not None else torch.device("cpu")
    order = torch.randperm(n_blocks, generator=generator, device=gdev)
    if n_rows % block:  # the short block goes first, to a minibatch with the most blocks: lengths stay within a block
        at = int((order == n_blocks - 1).nonzero()[0, 0])
        order[at], order[0] = order[0].clone(), order[at].clone()
    if device is not None:
        order = order.to(device)
    within = torch.arange(block, device=order.device)
    out = []
    for i in range(m):  # blocks i, i + m, i + 2 m, ... of the shuffled order: counts differ by at most one
        rows = (order[i::m, None] * block + within[None, :]).reshape(-1)
        out.append(rows[rows < n_rows].to(torch.int32))
    return out


def adv_moments(adv: torch.Tensor, index: torch.Tensor = None, eps: float = 1e-8) -> torch.Tensor:
    """{mean, rstd, std, n} (a float64 [4] device tensor) of adv (float32, any shape, flattened) at the rows of
    index (int32 1-D, None: all rows): the mean, 1 / (std + eps) with the unbiased std that ``tensor.std()``
    gives, that std, and the number of positions whose index is inside adv (macm_adv_moments: two passes,
    float64, deterministic). The result is what ``ppo_grads(adv_norm=...)`` takes, and nothing synchronises
    in between. The workspace is this module's, as ppo_loss's is: calls belong on one stream."""
    dev = adv.device
    _check("adv", adv, dev, torch.float32, adv.shape)
    if index is not None:
        index = _check_index(index, dev)
    if not 0 <= eps < float("inf"):
        raise ValueError("eps must be finite and >= 0")
    if dev.type != "cuda":
        raise ValueError("adv_moments runs on a GPU device (no CPU fallback)")
    rows = index.numel() if index is not None else adv.numel()
    out = torch.empty((4,), dtype=torch.float64, device=dev)
    ws = _workspace(None, rows, dev)
    with torch.cuda.device(dev):
        _abi.check(_abi.lib().macm_adv_moments(_p(adv), _p(index), adv.numel() if index is not None else 0, rows,
                                               float(eps), _p(out), _p(ws), ws.numel(), _stream(adv)),
                   "macm_adv_moments")
    return out


def ppo_grads(pol, crit, obs: torch.Tensor, actions: torch.Tensor, old_logp: torch.Tensor, adv: torch.Tensor,
              ret: torch.Tensor, old_values: torch.Tensor = None, clip: float = 0.2, vf_coef: float = 0.5,
              ent_coef: float = 0.01, vf_clip: float = None, index: torch.Tensor = None,
              adv_norm: torch.Tensor = None) -> torch.Tensor:
    """stats (float64 [8]) of the clipped PPO loss of pol (an MlpPolicy) and crit (an MlpCritic) over obs
    [..., in_dim], with dL/dparams accumulated into pol.params.grad and crit.params.grad exactly as
    ``ppo_loss(pol.forward(obs), crit.forward(obs), ...)[0].backward()`` would, bit for bit, but with the loss
    inside the gradient launches (macm_ppo_grad): no logits, values or their gradients in memory. Either net
    may be None. The workspace is the first net's and grows on demand: calls on one object belong on one
    stream.

    index (an int32 1-D device tensor, e.g. one of ``minibatches(...)``) makes the call a minibatch of those
    rows (macm_ppo_grad_rows): obs and the per-row tensors are taken as [n_src, ...] with their leading
    dimensions flattened, position r of the call reads row index[r] of each, and the means are over
    len(index). The results have the bits of the call on ``index_select``-ed copies, which are never made. An
    index outside [0, n_src) is skipped (it adds nothing and is never followed), where ``index_select`` would
    fault. An int64 index is accepted and converted, which costs a copy per call. adv_norm (float64 [2] or [4]
    on the device: mean and rstd, what ``adv_moments`` returns) normalises each advantage as it is loaded,
    (adv - mean) * rstd in float64 rounded once to float32; it works without index too. Measured on the
    flagship trajectory ("PPO over shuffled minibatches": an epoch of 32 minibatches of 2^20 rows):
    23.2 ms with the block=64 index of ``minibatches`` against 22.6 ms for contiguous slices and 30.7 ms for
    ``index_select`` copies; a full row shuffle (block=1) fetches a cache line per row and costs 24.6 ms, 6%
    more than block=64 and still less than the copies. With both None the call is macm_ppo_grad exactly as
    before. The autograd path (``ppo_loss``, ``pol.forward``) takes no index: gather with torch there."""
    if pol is None and crit is None:
        raise ValueError("pol and crit are both None")
    first = pol if pol is not None else crit
    if pol is not None and crit is not None and (pol.device != crit.device or pol.in_dim != crit.in_dim):
        raise ValueError("the policy and the critic must share a device and in_dim (they read the same obs rows)")
    _check_cfg(clip, vf_coef, ent_coef, vf_clip, old_values if crit is not None else None)
    first._check_rows(obs)
    dev, lead = first.device, tuple(obs.shape[:-1])
    _check_rows(dev, lead, actions, old_logp, adv, ret, old_values, pol is not None, crit is not None)
    n_src = rows = obs.numel() // first.in_dim
    if index is not None:
        index = _check_index(index, dev)
        rows = index.numel()
    if adv_norm is not None:
        if adv_norm.device != dev or adv_norm.dtype != torch.float64 or adv_norm.dim() != 1 or \
                adv_norm.numel() not in (2, 4) or not adv_norm.is_contiguous():
            raise ValueError(f"adv_norm must be a contiguous float64 [2] or [4] tensor on {dev} (adv_moments' result)")
    cfg = config(clip, vf_coef, ent_coef, vf_clip)
    ws = _workspace(first, rows, dev)
    gp = torch.empty_like(pol.params, requires_grad=False) if pol is not None else None
    gv = torch.empty_like(crit.params, requires_grad=False) if crit is not None else None
    stats = torch.empty((8,), dtype=torch.float64, device=dev)
    head = (ctypes.byref(cfg), ctypes.byref(pol.struct()) if pol is not None else None,
            ctypes.byref(crit.struct()) if crit is not None else None, _p(obs), 1 if obs.dtype == torch.float64 else 0,
            rows)
    tail = (_p(actions) if pol is not None else None, _p(old_logp) if pol is not None else None,
            _p(adv) if pol is not None else None, _p(ret) if crit is not None else None,
            _p(old_values) if crit is not None else None, _p(gp), _p(gv), _p(stats), _p(ws), ws.numel(), _stream(obs))
    with torch.cuda.device(dev):
        if index is None and adv_norm is None:
            _abi.check(_abi.lib().macm_ppo_grad(*head, *tail), "macm_ppo_grad")
        else:
            _abi.check(_abi.lib().macm_ppo_grad_rows(*head, _p(index), n_src, _p(adv_norm), *tail),
                       "macm_ppo_grad_rows")
    for net, g in ((pol, gp), (crit, gv)):
        if net is not None:
            if net.params.grad is None:
                net.params.grad = g
            else:
                net.params.grad.add_(g)
    return stats


ADAM_HEAD = ("t", "beta1_pow", "beta2_pow", "stopped", "grad_norm", "clip_coef", "skipped_nonfinite", "reserved")


class Adam:
    """Adam over pol.params and crit.params (either net may be None) as one launch per step (macm_ppo_adam):
    the global-norm clip of ``clip_grad_norm_`` (max_grad_norm, None: none), a KL gate (target_kl, None: none;
    compared as given with ``stats[4]``: a user of the 1.5 x convention passes 1.5 x) and a guard that skips
    a step whose gradient norm is not finite, all inside it. The definition is include/macm.h's: float64
    arithmetic on float32 params, gradients and moments, checked bit for bit.

    ``state`` is a zero-filled uint8 device tensor in the header's layout: eight doubles (``ADAM_HEAD``), then
    m and v of the policy, then of the critic (float32). ``lr`` is a plain attribute, read at every step: a
    schedule assigns to it. Once the gate has stopped the optimiser (approx_kl above target_kl, or NaN) every
    later step is a no-op until ``resume()``. Calls on one object belong on one stream."""

    def __init__(self, pol, crit, lr: float = 3e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = None, target_kl: float = None):
        inf = float("inf")
        if not 0 <= lr < inf:
            raise ValueError("lr must be finite and >= 0")
        if len(betas) != 2 or not all(0 <= b < 1 for b in betas):
            raise ValueError("betas must be two values in [0, 1)")
        if not 0 < eps < inf:
            raise ValueError("eps must be finite and > 0")
        if max_grad_norm is not None and not 0 <= max_grad_norm < inf:
            raise ValueError("max_grad_norm must be finite and >= 0 (None or 0: no clipping)")
        if target_kl is not None and not 0 <= target_kl < inf:
            raise ValueError("target_kl must be finite and >= 0 (None or 0: no gate)")
        if pol is None and crit is None:
            raise ValueError("pol and crit are both None")
        if target_kl and pol is None:
            raise ValueError("target_kl needs the policy (approx_kl is the policy's)")
        first = pol if pol is not None else crit
        if pol is not None and crit is not None and pol.device != crit.device:
            raise ValueError("the policy and the critic must share a device")
        self.pol, self.crit, self.device = pol, crit, first.device
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.target_kl = 0.0 if target_kl is None else float(target_kl)
        n = ctypes.c_int64(0)
        _abi.check(_abi.lib().macm_ppo_adam_state_bytes(self._net(pol), self._net(crit), ctypes.byref(n)),
                   "macm_ppo_adam_state_bytes")
        self.state = torch.zeros((int(n.value),), dtype=torch.uint8, device=self.device)
        self._ws = None  # update()'s workspace, grown on demand

    @staticmethod
    def _net(net):
        return ctypes.byref(net.struct()) if net is not None else None

    def config(self):
        """The macm_adam_config of the hyperparameters as they stand."""
        return _abi.MacmAdamConfig(self.lr, self.betas[0], self.betas[1], self.eps, self.max_grad_norm, self.target_kl,
                                   (ctypes.c_int32 * 4)(0, 0, 0, 0))

    def step(self, stats: torch.Tensor = None):
        """One step from pol.params.grad and crit.params.grad, which ``ppo_grads`` or ``loss.backward()`` left
        there; stats (float64 [8], what ``ppo_grads`` returned) feeds the KL gate and is needed with target_kl."""
        grads = []
        for net, what in ((self.pol, "pol"), (self.crit, "crit")):
            g = net.params.grad if net is not None else None
            if net is not None:
                if g is None:
                    raise ValueError(f"{what}.params.grad is None: nothing to step from")
                _check(f"{what}.params.grad", g, self.device, torch.float32, net.params.shape)
            grads.append(g)
        if stats is not None:
            _check("stats", stats, self.device, torch.float64, (8,))
        elif self.target_kl > 0:
            raise ValueError("target_kl needs the stats of the gradient call")
        cfg = self.config()
        with torch.cuda.device(self.device):
            _abi.check(_abi.lib().macm_ppo_adam(ctypes.byref(cfg), self._net(self.pol), self._net(self.crit),
                                                _p(grads[0]), _p(grads[1]), _p(stats), _p(self.state),
                                                self.state.numel(), _stream(self.state)), "macm_ppo_adam")

    def zero_grad(self):
        """Drops both nets' .grad (as torch's zero_grad(set_to_none=True)): the next ``ppo_grads`` sets it."""
        for net in (self.pol, self.crit):
            if net is not None:
                net.params.grad = None

    def head(self) -> torch.Tensor:
        """The state's eight doubles (ADAM_HEAD) as a float64 [8] device view: no copy, no synchronise."""
        return self.state[:64].view(torch.float64)

    def moments(self, which: str):
        """(m, v) of "pol" or "crit": float32 views into the state."""
        n_p = self.pol.params.numel() if self.pol is not None else 0
        n_c = self.crit.params.numel() if self.crit is not None else 0
        f = self.state[64:].view(torch.float32)
        at, n = (0, n_p) if which == "pol" else (2 * n_p, n_c)
        return f[at:at + n], f[at + n:at + 2 * n]

    def resume(self):
        """Clears the stopped word with a fill on the current stream: the steps behind it apply again."""
        self.head()[3:4].zero_()

    def info(self) -> dict:
        """The head as a dict of Python floats. This copies to the host: it synchronises the stream."""
        return dict(zip(ADAM_HEAD, self.head().cpu().tolist()))


def update_workspace_bytes(max_rows: int) -> int:
    n = ctypes.c_int64(0)
    _abi.check(_abi.lib().macm_ppo_update_workspace(int(max_rows), ctypes.byref(n)), "macm_ppo_update_workspace")
    return int(n.value)


def update(opt: Adam, obs: torch.Tensor, actions: torch.Tensor, old_logp: torch.Tensor, adv: torch.Tensor,
           ret: torch.Tensor, old_values: torch.Tensor = None, minibatches=(), normalize_adv: bool = True,
           adv_eps: float = 1e-8, clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.01,
           vf_clip: float = None, out: torch.Tensor = None) -> torch.Tensor:
    """stats (float64 [len(minibatches), 8], STATS per row; `out` if given) of a whole PPO update in one call (macm_ppo_update):
    for each index tensor of `minibatches` (int32 1-D device tensors, e.g. the lists of ``minibatches(...)`` of
    one epoch or of several, one after the other) the moments of its advantages (normalize_adv), the fused
    gradients of opt's nets at those rows and opt's step, gated by that minibatch's approx_kl, all enqueued on
    the current stream with nothing synchronising in between. The params, opt.state and the stats have the
    bits of the loop ``adv_moments -> ppo_grads(index=, adv_norm=) -> opt.step(stats) -> opt.zero_grad()``.
    ``.grad`` is not touched: the gradients live in opt's workspace, which grows on demand.

    An empty minibatch is skipped whole (a zero stats row, no step). After a KL stop the remaining minibatches'
    gradients are still computed and their stats rows written (they describe the unchanged params): ending
    early on the host would need a synchronise per minibatch. ``opt.head()`` tells afterwards, on the device,
    whether and ``opt.info()`` (which synchronises) how it ended."""
    if not isinstance(opt, Adam):
        raise ValueError("opt must be a gym_macm.ppo.Adam")
    pol, crit = opt.pol, opt.crit
    first = pol if pol is not None else crit
    if pol is not None and crit is not None and pol.in_dim != crit.in_dim:
        raise ValueError("the policy and the critic must share in_dim (they read the same obs rows)")
    _check_cfg(clip, vf_coef, ent_coef, vf_clip, old_values if crit is not None else None)
    first._check_rows(obs)
    dev, lead = first.device, tuple(obs.shape[:-1])
    _check_rows(dev, lead, actions, old_logp, adv, ret, old_values, pol is not None, crit is not None)
    if not 0 <= adv_eps < float("inf"):
        raise ValueError("adv_eps must be finite and >= 0")
    index = [_check_index(mb, dev) for mb in minibatches]
    n_mb, n_src = len(index), obs.numel() // first.in_dim
    need = update_workspace_bytes(max([mb.numel() for mb in index], default=0))
    if opt._ws is None or opt._ws.numel() < need:
        opt._ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    stats = out if out is not None else torch.empty((n_mb, 8), dtype=torch.float64, device=dev)
    _check("out", stats, dev, torch.float64, (n_mb, 8))
    ptrs = (ctypes.c_void_p * max(n_mb, 1))(*[mb.data_ptr() for mb in index])
    rows = (ctypes.c_int64 * max(n_mb, 1))(*[mb.numel() for mb in index])
    cfg, acfg = config(clip, vf_coef, ent_coef, vf_clip), opt.config()
    with torch.cuda.device(dev):
        _abi.check(_abi.lib().macm_ppo_update(
            ctypes.byref(cfg), ctypes.byref(acfg), Adam._net(pol), Adam._net(crit), _p(obs),
            1 if obs.dtype == torch.float64 else 0, n_src, _p(actions) if pol is not None else None,
            _p(old_logp) if pol is not None else None, _p(adv) if pol is not None else None,
            _p(ret) if crit is not None else None, _p(old_values) if crit is not None else None, n_mb, ptrs, rows,
            1 if normalize_adv else 0, float(adv_eps), _p(opt.state), opt.state.numel(), _p(stats), _p(opt._ws),
            opt._ws.numel(), _stream(obs)), "macm_ppo_update")
    return stats
