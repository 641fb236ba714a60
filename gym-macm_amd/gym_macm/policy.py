"""A learned policy as the actor of Flock's closed loop: a float32 MLP over every agent's obs row.

    pol = MlpPolicy.from_linear_layers([net.l1, net.l2, net.head], device="cuda:0")
    acts[0] = pol.act(vec.obs, seed=seed, decision=0, first_row=vec.first_row)   # the first actions, uint8 [E, N, 3], sampled
    vec.set_policy(pol); vec.set_sampling(seed, decision=1)
    out = vec.rollout_policy(acts, 128, trajectory=True)   # one launch on the wave path; it draws its own noise

The definition is include/macm.h's (macm_policy_mlp): ``y[j] = b[j] + sum_k W[k][j] x[k]`` as the
k-ordered float32 fmaf chain, relu on the hidden layers, 9 logits (head h of MultiDiscrete([3, 3, 3])
at ``logits[3h + c]``), ``action[h] = argmax_c(logits[3h + c] + noise[3h + c])``, the lowest index on
ties. Gumbel noise samples from the softmax; None is the argmax. A world with sampling on
(``set_sampling``) and ``act(seed=, decision=)`` draw it inside the launch from a counter-based generator
(macm_sample_config: Philox4x32-10 over (seed, decision index, row, head), g = -log(-log(u)) in float64),
reproducible however the steps are cut into launches and, the row being the job's (``first_row``: a shard's
``env_offset * N``), however the envs are split over ranks; ``gumbel_noise`` gives the same numbers as a tensor
for a caller who wants to pass ``noise`` explicitly. The learner recomputes log-probabilities from the
stored logits.

``params`` is one flat device tensor, W[in][out] row-major then the bias, layer after layer. The
library reads it at every launch, so a learner that writes new values into it in place
(``pack`` / ``load_linear_layers`` / ``params.copy_``) needs no second registration.

The critic beside the actor (macm_value_mlp) is a second MLP of the same arithmetic with one output,
and ``gae`` turns a trajectory into advantages and returns in one launch:

    crit = MlpCritic.from_linear_layers([v.fc1, v.fc2, v.head], device="cuda:0"); vec.set_critic(crit)
    vals = torch.empty((K + 1, E, N), device=dev); vals[0] = crit.value(vec.obs)
    boot = torch.empty((K, E, N), device=dev)
    traj = vec.rollout_policy(acts, K, trajectory=True, logits=lg, values=vals, boot=boot)
    t = ppo.transitions(traj, acts, lg, vals, boot)   # gym_macm.ppo: each decision beside its own step, as views
    adv, ret = gae(t["reward"], t["values"], t["boot"], t["done"], 0.99, 0.95)

The launch's rows are staggered: step k executes action row k and writes reward, done, boot and obs row k; the
decision taken from obs row k goes to action row k + 1, with its logits in logits row k and the value of the obs
it saw in values row k + 1. ``values[:K]`` therefore belongs to the decisions of action rows 0 .. K-1, each taken
from the obs before its step, and ``transitions`` pairs obs[j], logits[j] with acts[j + 1], vals[j + 1],
reward[j + 1], done[j + 1] and boot[j + 1] for the K - 1 decisions the launch both took and stepped.

Learning on those rows stays in the library too: ``forward`` is the same kernel under torch.autograd,
and its backward is one launch per net (macm_policy_grad / macm_value_grad), with no nn.Module copy
of the net and no per-row activation kept:

    pol.params.requires_grad_(True); crit.params.requires_grad_(True)
    opt = torch.optim.Adam([pol.params, crit.params], lr=3e-4)
    lg = pol.forward(t["obs"])             # [..., 9], the bits rollout_policy stored at these params
    v = crit.forward(t["obs"])             # [...]
    loss = ppo_loss(lg, t["logits"], t["actions"], adv, ret, v)   # the caller's torch code, any loss
    loss.backward(); opt.step()            # params change in place: the next launch reads them

The clipped PPO loss itself on the device, composed with ``forward`` or fused into the gradient launches,
is in gym_macm.ppo (``log_prob``, ``ppo_loss``, ``ppo_grads``).
"""
from __future__ import annotations

import ctypes

import torch

from . import _abi

N_LOGITS = 9
GRAD_TILE_ROWS = 64  # macm_policy_grad / macm_value_grad: one wave sums tiles of this many rows ...
GRAD_MAX_PARTIALS = 2048  # ... and at most this many waves write a partial (csrc/policy_mlp.hpp, kGradMaxPartials)


def layer_shapes(in_dim: int, hidden: int, n_hidden: int, n_out: int = N_LOGITS) -> list:
    """[(in, out)] of the layers: n_hidden hidden layers, then the n_out outputs (the 9 logits; a critic: 1)."""
    dims = [int(in_dim)] + [int(hidden)] * int(n_hidden) + [int(n_out)]
    return list(zip(dims[:-1], dims[1:]))


def n_params(in_dim: int, hidden: int, n_hidden: int, n_out: int = N_LOGITS) -> int:
    return sum(i * o + o for i, o in layer_shapes(in_dim, hidden, n_hidden, n_out))


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _Mlp:
    """What MlpPolicy and MlpCritic share: the flat params tensor, its layout and the C-ABI struct."""
    N_OUT, STRUCT, WHAT = None, None, None  # the subclass's outputs, _abi struct and name in messages

    def __init__(self, in_dim: int, hidden: int, n_hidden: int, device=None):
        if int(in_dim) not in (4, 6) or int(hidden) not in (16, 32) or int(n_hidden) not in (1, 2):
            raise ValueError(f"{type(self).__name__}: in_dim must be 4 or 6, hidden 16 or 32, n_hidden 1 or 2")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"the {self.WHAT}'s params live on a GPU device (no CPU fallback)")
        self.in_dim, self.hidden, self.n_hidden = int(in_dim), int(hidden), int(n_hidden)
        self.shapes = layer_shapes(in_dim, hidden, n_hidden, self.N_OUT)
        self.params = torch.zeros((n_params(in_dim, hidden, n_hidden, self.N_OUT),), dtype=torch.float32,
                                  device=self.device)
        assert self.params.data_ptr() % 16 == 0
        self._struct = self.STRUCT(self.in_dim, self.hidden, self.n_hidden, 0, ctypes.c_void_p(self.params.data_ptr()))

    def struct(self):
        """The C-ABI struct (it points into ``params``: this object must outlive its uses)."""
        return self._struct

    def pack(self, weights, biases):
        """weights[l]: [in, out] (already transposed), biases[l]: [out]; written into params in place."""
        if len(weights) != len(self.shapes) or len(biases) != len(self.shapes):
            raise ValueError(f"expected {len(self.shapes)} layers")
        flat = []
        for (i, o), w, b in zip(self.shapes, weights, biases):
            w = torch.as_tensor(w, dtype=torch.float32)
            b = torch.as_tensor(b, dtype=torch.float32)
            if tuple(w.shape) != (i, o) or tuple(b.shape) != (o,):
                raise ValueError(f"layer shapes must be W [{i}, {o}] and b [{o}]; got {tuple(w.shape)}, {tuple(b.shape)}")
            flat += [w.detach().reshape(-1).to(self.device), b.detach().reshape(-1).to(self.device)]
        with torch.no_grad():  # (params may be a leaf that requires grad: a learner's in-place write)
            self.params.copy_(torch.cat(flat))
        return self

    def unpack(self):
        """(weights, biases): views into params, W [in, out] and b [out] per layer."""
        ws, bs, at = [], [], 0
        for i, o in self.shapes:
            ws.append(self.params[at:at + i * o].view(i, o))
            at += i * o
            bs.append(self.params[at:at + o])
            at += o
        return ws, bs

    def load_linear_layers(self, layers):
        """The weights of torch.nn.Linear layers ([out, in] each), transposed to [in][out], into params."""
        return self.pack([l.weight.detach().t().contiguous() for l in layers], [l.bias.detach() for l in layers])

    def _check_rows(self, obs: torch.Tensor):
        if obs.device != self.device or not obs.is_contiguous() or obs.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"obs must be a contiguous float32/float64 tensor on the {self.WHAT}'s device")
        if obs.shape[-1] != self.in_dim:
            raise ValueError(f"obs rows must have {self.in_dim} values")
        if obs.requires_grad:
            raise ValueError(f"obs must not require grad (the {self.WHAT} has no gradient with respect to obs)")

    def _outputs(self, obs: torch.Tensor) -> torch.Tensor:
        """The net's outputs for obs through the one-shot kernel (the subclass's)."""
        raise NotImplementedError

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        """The net's outputs for obs [..., in_dim] with the bits of the one-shot kernels and the rollouts;
        where ``params.requires_grad`` is set (and grad mode is on) the result is differentiable with respect
        to params: its backward is one launch of the gradient kernel, which recomputes the activations."""
        self._check_rows(obs)
        if self.params.requires_grad and torch.is_grad_enabled():
            return _MlpForward.apply(self.params, obs, self)
        return self._outputs(obs)

    def grad_workspace_bytes(self, rows: int) -> int:
        n = ctypes.c_int64(0)
        _abi.check(_abi.lib().macm_mlp_grad_workspace(int(rows), ctypes.byref(n)), "macm_mlp_grad_workspace")
        return int(n.value)

    def param_grad(self, obs: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
        """dL/dparams (float32 [n_params], a new tensor) from dout = dL/doutputs (float32 [..., 9]; a critic:
        [...]) over obs [..., in_dim], on the current stream (macm_policy_grad / macm_value_grad). The
        workspace is this object's and grows on demand: calls on one object belong on one stream."""
        self._check_rows(obs)
        lead = tuple(obs.shape[:-1])
        want = lead + ((self.N_OUT,) if self.N_OUT != 1 else ())
        if (dout.device != self.device or not dout.is_contiguous() or dout.dtype != torch.float32
                or tuple(dout.shape) != want):
            raise ValueError(f"dout must be a contiguous float32 {want} tensor on the {self.WHAT}'s device")
        rows = obs.numel() // self.in_dim
        need = self.grad_workspace_bytes(rows)
        ws = getattr(self, "_grad_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._grad_ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=self.device)
        grad = torch.empty_like(self.params, requires_grad=False)
        with torch.cuda.device(self.device):
            _abi.check(getattr(_abi.lib(), self.GRAD_FN)(
                ctypes.byref(self._struct), ctypes.c_void_p(obs.data_ptr()), 1 if obs.dtype == torch.float64 else 0,
                rows, ctypes.c_void_p(dout.data_ptr()), ctypes.c_void_p(grad.data_ptr()),
                ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream(obs)), self.GRAD_FN)
        return grad

    @classmethod
    def from_linear_layers(cls, layers, device=None):
        """layers: the hidden torch.nn.Linear layers (relu between them) and the head (9 logits; a critic: 1)."""
        layers = list(layers)
        if len(layers) not in (2, 3) or layers[-1].out_features != cls.N_OUT:
            raise ValueError(f"expected 1 or 2 hidden nn.Linear layers and a head with {cls.N_OUT} output"
                             + ("s" if cls.N_OUT != 1 else ""))
        if device is None:
            device = layers[0].weight.device
        return cls(layers[0].in_features, layers[0].out_features, len(layers) - 1, device).load_linear_layers(layers)


class _MlpForward(torch.autograd.Function):
    """net.forward(obs) as a function of net.params: the one-shot kernel forward, the gradient kernel backward.
    Only obs is kept for the backward (and params, for autograd's check that they were not overwritten
    between the two): the backward recomputes the activations from the params as they stand."""

    @staticmethod
    def forward(ctx, params, obs, net):
        ctx.net = net
        ctx.save_for_backward(params, obs)
        return net._outputs(obs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        _, obs = ctx.saved_tensors
        return ctx.net.param_grad(obs, gout.to(torch.float32).contiguous()), None, None


class MlpPolicy(_Mlp):
    """in_dim: the world's obs_dim (4 polar, 6 cartesian); hidden 16 or 32; n_hidden 1 or 2."""
    N_OUT, STRUCT, WHAT = N_LOGITS, _abi.MacmPolicyMlp, "policy"
    GRAD_FN = "macm_policy_grad"

    def _outputs(self, obs: torch.Tensor) -> torch.Tensor:
        logits = torch.empty(tuple(obs.shape[:-1]) + (N_LOGITS,), dtype=torch.float32, device=self.device)
        self.act(obs, logits=logits)
        return logits

    def act(self, obs: torch.Tensor, noise: torch.Tensor = None, logits: torch.Tensor = None,
            out: torch.Tensor = None, seed: int = None, decision: int = 0, first_row: int = 0) -> torch.Tensor:
        """The policy's actions (uint8 [..., 3]) for obs [..., in_dim] (macm_policy_flock); noise and
        logits: float32 [..., 9] or None (logits is written). With ``seed`` the launch draws the noise itself
        (macm_policy_flock_sampled_at): flat row r of obs at decision index ``decision``, as the job's row
        ``first_row + r`` (a shard's obs: ``FlockVec.first_row``), the numbers of
        ``gumbel_noise(seed, decision, 1, obs.shape[:-1], first_row=first_row)``; ``noise`` must then be None.
        ``first_row`` is only meaningful with ``seed``."""
        if obs.device != self.device or not obs.is_contiguous() or obs.dtype not in (torch.float32, torch.float64):
            raise ValueError("obs must be a contiguous float32/float64 tensor on the policy's device")
        if obs.shape[-1] != self.in_dim:
            raise ValueError(f"obs rows must have {self.in_dim} values")
        lead = tuple(obs.shape[:-1])
        for name, t in (("noise", noise), ("logits", logits)):
            if t is not None and (t.device != self.device or not t.is_contiguous() or t.dtype != torch.float32
                                  or tuple(t.shape) != lead + (N_LOGITS,)):
                raise ValueError(f"{name} must be a contiguous float32 {lead + (N_LOGITS,)} tensor on the policy's device")
        if out is None:
            out = torch.empty(lead + (3,), dtype=torch.uint8, device=self.device)
        elif (out.device != self.device or not out.is_contiguous() or out.dtype != torch.uint8
              or tuple(out.shape) != lead + (3,)):
            raise ValueError(f"out must be a contiguous uint8 {lead + (3,)} tensor on the policy's device")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        L = _abi.lib()
        if seed is None and first_row != 0:
            raise ValueError("first_row names the rows of the draw: it needs seed")
        if seed is not None:
            if noise is not None:
                raise ValueError("noise and seed exclude each other: with seed the launch draws its own noise")
            cfg = sample_config(seed, decision)
            first_row = sample_first_row(first_row)
            with torch.cuda.device(self.device):
                _abi.check(L.macm_policy_flock_sampled_at(ctypes.byref(self._struct), p(obs),
                                                          1 if obs.dtype == torch.float64 else 0, first_row,
                                                          obs.numel() // self.in_dim, ctypes.byref(cfg), p(out), p(logits),
                                                          _stream(obs)),
                           "macm_policy_flock_sampled_at")
            return out
        with torch.cuda.device(self.device):
            _abi.check(L.macm_policy_flock(ctypes.byref(self._struct), p(obs), 1 if obs.dtype == torch.float64 else 0,
                                           obs.numel() // self.in_dim, p(noise), p(out), p(logits), _stream(obs)),
                       "macm_policy_flock")
        return out


class MlpCritic(_Mlp):
    """The critic beside the actor (macm_value_mlp): the same MLP with a trunk of its own and one output,
    V(obs). Its shape (hidden 16 or 32, n_hidden 1 or 2) is independent of the actor's."""
    N_OUT, STRUCT, WHAT = 1, _abi.MacmValueMlp, "critic"
    GRAD_FN = "macm_value_grad"

    def _outputs(self, obs: torch.Tensor) -> torch.Tensor:
        return self.value(obs)

    def value(self, obs: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """V (float32 [...]) of obs [..., in_dim] (macm_value_flock)."""
        if obs.device != self.device or not obs.is_contiguous() or obs.dtype not in (torch.float32, torch.float64):
            raise ValueError("obs must be a contiguous float32/float64 tensor on the critic's device")
        if obs.shape[-1] != self.in_dim:
            raise ValueError(f"obs rows must have {self.in_dim} values")
        lead = tuple(obs.shape[:-1])
        if out is None:
            out = torch.empty(lead, dtype=torch.float32, device=self.device)
        elif (out.device != self.device or not out.is_contiguous() or out.dtype != torch.float32
              or tuple(out.shape) != lead):
            raise ValueError(f"out must be a contiguous float32 {lead} tensor on the critic's device")
        with torch.cuda.device(self.device):
            _abi.check(_abi.lib().macm_value_flock(ctypes.byref(self._struct), ctypes.c_void_p(obs.data_ptr()),
                                                   1 if obs.dtype == torch.float64 else 0, obs.numel() // self.in_dim,
                                                   ctypes.c_void_p(out.data_ptr()), _stream(obs)), "macm_value_flock")
        return out


def gae(reward: torch.Tensor, values: torch.Tensor, boot: torch.Tensor, done: torch.Tensor, gamma: float, lam: float,
        adv: torch.Tensor = None, ret: torch.Tensor = None):
    """(adv, ret), float32 [K, E, N]: generalised advantage estimation over a trajectory in one launch
    (macm_gae). reward, values and boot are float32 [K, E, N], done uint8 [K, E]; values[k] is V of the
    observation the action of step k was taken from and boot[k] V of the observation step k produced, so
    every end bootstraps from its own terminal observation, and a done row cuts the recursion. adv[k] is the
    advantage of the action step k executed. On the rows of ``gym_macm.ppo.transitions`` that action is the
    row's own; on a launch's raw buffers (values: the first K rows of its [K + 1, E, N] buffer) it is action
    row k, taken from the obs before step k, not from obs row k."""
    dev = reward.device
    if reward.dim() != 3:
        raise ValueError("reward must be a [K, E, N] tensor")
    K, E, N = (int(d) for d in reward.shape)
    if adv is None:
        adv = torch.empty((K, E, N), dtype=torch.float32, device=dev)
    if ret is None:
        ret = torch.empty((K, E, N), dtype=torch.float32, device=dev)
    for name, t in (("reward", reward), ("values", values), ("boot", boot), ("adv", adv), ("ret", ret)):
        if (t.device != dev or not t.is_contiguous() or t.dtype != torch.float32 or tuple(t.shape) != (K, E, N)):
            raise ValueError(f"{name} must be a contiguous float32 {[K, E, N]} tensor on {dev}")
    if done.device != dev or not done.is_contiguous() or done.dtype != torch.uint8 or tuple(done.shape) != (K, E):
        raise ValueError(f"done must be a contiguous uint8 {[K, E]} tensor on {dev}")
    ins = (reward, values, boot, done)
    for name, o in (("adv", adv), ("ret", ret)):
        if any(_overlap(o, i) for i in ins) or (name == "ret" and _overlap(o, adv)):
            raise ValueError(f"{name} must not alias an input or the other output")
    if dev.type != "cuda":
        raise ValueError("gae runs on a GPU device (no CPU fallback)")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        _abi.check(_abi.lib().macm_gae(p(reward), p(values), p(boot), p(done), K, E, N, float(gamma), float(lam),
                                       p(adv), p(ret), _stream(reward)), "macm_gae")
    return adv, ret


def sample_config(seed: int, decision: int = 0) -> "_abi.MacmSampleConfig":
    """macm_sample_config from Python ints; ValueError outside [0, 2**64)."""
    seed, decision = int(seed), int(decision)
    if not (0 <= seed < 1 << 64) or not (0 <= decision < 1 << 64):
        raise ValueError("seed and decision must be in [0, 2**64)")
    return _abi.MacmSampleConfig(seed, decision, (ctypes.c_int32 * 4)(0, 0, 0, 0))


def sample_first_row(first_row: int) -> int:
    """first_row as the C-ABI takes it (an int64 that ctypes would truncate silently); ValueError outside
    [0, 2**32]. The library checks first_row + rows <= 2**32."""
    first_row = int(first_row)
    if not (0 <= first_row <= 1 << 32):
        raise ValueError("first_row must be in [0, 2**32]")
    return first_row


def gumbel_noise(seed: int, decision: int, n_dec: int, rows_shape, device=None, words: bool = False,
                 first_row: int = 0):
    """The Gumbel noise that decisions ``decision .. decision + n_dec - 1`` draw under ``seed`` for the rows of
    ``rows_shape`` (e.g. (E, N); row r is the flat index), float32 [n_dec, *rows_shape, 9], in one launch
    (macm_policy_noise_at): what a sampling world adds to its logits, bit for bit, so
    ``rollout_policy(noise=gumbel_noise(seed, d, K, (E, N)))`` on a world without sampling is the twin of the
    launch a world with ``set_sampling(seed, d)`` makes. ``first_row``: row r is the job's row ``first_row + r``,
    so the result is rows [first_row, first_row + rows) of the job's noise (a shard with env_offset e0:
    ``first_row=e0 * N``, the twin of ``set_sampling(seed, d, first_row=e0 * N)``). With ``words`` also the generator's raw output:
    (noise, words), words int32 [n_dec, *rows_shape, 3, 4] holding the uint32 bits (``.cpu().numpy().view(np.uint32)``)."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("gumbel_noise runs on a GPU device (no CPU fallback)")
    shape = tuple(int(d) for d in (rows_shape if hasattr(rows_shape, "__iter__") else (rows_shape,)))
    rows = 1
    for d in shape:
        rows *= d
    n_dec = int(n_dec)
    cfg = sample_config(seed, decision)
    first_row = sample_first_row(first_row)
    noise = torch.empty((n_dec,) + shape + (N_LOGITS,), dtype=torch.float32, device=device)
    w = torch.empty((n_dec,) + shape + (3, 4), dtype=torch.int32, device=device) if words else None
    with torch.cuda.device(device):
        _abi.check(_abi.lib().macm_policy_noise_at(ctypes.byref(cfg), first_row, n_dec, rows,
                                                   ctypes.c_void_p(noise.data_ptr()),
                                                   ctypes.c_void_p(w.data_ptr()) if words else None, _stream(noise)),
                   "macm_policy_noise_at")
    return (noise, w) if words else noise


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a.numel() > 0 and b.numel() > 0 and a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()
