"""A learned policy as the actor of TDM's closed loop: a permutation-invariant float32 net over every
agent's [N-1, 4] observation slots, with its health beside the pooled set.

    pol = TdmSetPolicy.from_linear_layers([net.phi, net.rho, net.head], device="cuda:0")
    w = TdmWorld(tdm_config([16, 16]), E); w.reset(seed)
    acts = torch.empty((K + 1, E, N, 4), dtype=torch.uint8, device=dev)
    bots.combat_actions(w.obs, w.mask, out=acts[0])                 # team 1: the scripted bot
    pol.act(w.obs, w.mask, w.health, out=acts[0], agents=w.policy_agents([0]))   # team 0: the policy, over it
    w.set_policy(pol, teams=[0])
    traj = w.rollout_policy_traj(acts, K, noise=noise, logits=lg)   # one launch on the wave path

The definition is include/macm.h's (macm_tdm_policy), all float32 fmaf chains with k ascending:

    e_k = relu(b1 + W1^T o[k])            for every slot k with mask[k] != 0
    g   = max(0, max_k e_k)               (an empty set pools to zeros)
    t   = relu(b2 + W2^T (g, health))     (the health is the last input)
    z   = b3 + W3^T t                     11 logits of MultiDiscrete([3, 3, 3, 2]): heads 0..2 at z[3h + c],
                                          the attack head at z[9], z[10]
    action[h] = argmax_c(z + noise), the lowest index on ties

``params`` is one flat device tensor, W[in][out] row-major then the bias, layer after layer:
W1[4][H], b1[H], W2[H + 1][H], b2[H], W3[H][11], b3[11]. The library reads it at every launch, so a
learner that writes new values into it in place needs no second registration.

A learner's update runs under torch autograd without a copy of the net: with ``pol.params.requires_grad_()``,
``pol.forward(obs, mask, health)`` returns the logits with the bits the rollout stored, and its backward is
one launch of the gradient kernel (macm_tdm_policy_grad) into ``params.grad``; it keeps obs, mask and health
and no per-slot activation. ``torch_logits`` states the same function in plain differentiable torch: the
portable statement, with no bit claim.
"""
from __future__ import annotations

import ctypes

import torch

from . import _abi

N_LOGITS = 11
HEADS = (3, 3, 3, 2)


def layer_shapes(hidden: int) -> list:
    """[(in, out)] of the three layers: the slot encoder, the trunk over (pool, health), the head."""
    H = int(hidden)
    return [(4, H), (H + 1, H), (H, N_LOGITS)]


def n_params(hidden: int) -> int:
    return sum(i * o + o for i, o in layer_shapes(hidden))


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class TdmSetPolicy:
    """hidden: 16 or 32. ``params``: the flat float32 device tensor the library reads."""

    def __init__(self, hidden: int, device=None):
        if int(hidden) not in (16, 32):
            raise ValueError("TdmSetPolicy: hidden must be 16 or 32")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("the policy's params live on a GPU device (no CPU fallback)")
        self.hidden = int(hidden)
        self.shapes = layer_shapes(hidden)
        self.params = torch.zeros((n_params(hidden),), dtype=torch.float32, device=self.device)
        assert self.params.data_ptr() % 16 == 0
        self._struct = _abi.MacmTdmPolicy(self.hidden, (ctypes.c_int32 * 3)(0, 0, 0),
                                          ctypes.c_void_p(self.params.data_ptr()))

    def struct(self):
        """The C-ABI struct (it points into ``params``: this object must outlive its uses)."""
        return self._struct

    def pack(self, weights, biases):
        """weights[l]: [in, out] (already transposed), biases[l]: [out]; written into params in place."""
        if len(weights) != 3 or len(biases) != 3:
            raise ValueError("expected 3 layers")
        flat = []
        for (i, o), w, b in zip(self.shapes, weights, biases):
            w = torch.as_tensor(w, dtype=torch.float32)
            b = torch.as_tensor(b, dtype=torch.float32)
            if tuple(w.shape) != (i, o) or tuple(b.shape) != (o,):
                raise ValueError(f"layer shapes must be W [{i}, {o}] and b [{o}]; got {tuple(w.shape)}, {tuple(b.shape)}")
            flat += [w.detach().reshape(-1).to(self.device), b.detach().reshape(-1).to(self.device)]
        with torch.no_grad():
            self.params.copy_(torch.cat(flat))
        return self

    def unpack(self, params: torch.Tensor = None):
        """(weights, biases): views into params (or a tensor of its layout), W [in, out] and b [out] per layer."""
        p = self.params if params is None else params
        ws, bs, at = [], [], 0
        for i, o in self.shapes:
            ws.append(p[at:at + i * o].view(i, o))
            at += i * o
            bs.append(p[at:at + o])
            at += o
        return ws, bs

    def load_linear_layers(self, layers):
        """The weights of torch.nn.Linear layers ([out, in] each), transposed to [in][out], into params."""
        return self.pack([l.weight.detach().t().contiguous() for l in layers], [l.bias.detach() for l in layers])

    @classmethod
    def from_linear_layers(cls, layers, device=None):
        """layers: [phi, rho, head] = nn.Linear(4, H), nn.Linear(H + 1, H), nn.Linear(H, 11)."""
        layers = list(layers)
        if len(layers) != 3:
            raise ValueError("expected [phi, rho, head]: nn.Linear(4, H), nn.Linear(H + 1, H), nn.Linear(H, 11)")
        H = layers[0].out_features
        got = [(l.in_features, l.out_features) for l in layers]
        if got != [(4, H), (H + 1, H), (H, N_LOGITS)]:
            raise ValueError(f"expected layers of shapes {[(4, H), (H + 1, H), (H, N_LOGITS)]}; got {got}")
        if device is None:
            device = layers[0].weight.device
        return cls(H, device).load_linear_layers(layers)

    def _check_inputs(self, obs, mask, health):
        if obs.device != self.device or not obs.is_contiguous() or obs.dtype not in (torch.float32, torch.float64):
            raise ValueError("obs must be a contiguous float32/float64 tensor on the policy's device")
        if obs.dim() < 3 or obs.shape[-1] != 4 or obs.shape[-2] != obs.shape[-3] - 1:
            raise ValueError("obs must be [..., N, N-1, 4]")
        lead = tuple(obs.shape[:-2])
        if (mask.device != self.device or not mask.is_contiguous() or mask.dtype != torch.uint8
                or tuple(mask.shape) != lead + (obs.shape[-2],)):
            raise ValueError(f"mask must be a contiguous uint8 {lead + (obs.shape[-2],)} tensor on the policy's device")
        if (health.device != self.device or not health.is_contiguous() or health.dtype != torch.float64
                or tuple(health.shape) != lead):
            raise ValueError(f"health must be a contiguous float64 {lead} tensor on the policy's device")
        return lead

    def act(self, obs: torch.Tensor, mask: torch.Tensor, health: torch.Tensor, noise: torch.Tensor = None,
            logits: torch.Tensor = None, out: torch.Tensor = None, agents: torch.Tensor = None) -> torch.Tensor:
        """The policy's actions (uint8 [..., N, 4]) for obs [..., N, N-1, 4], mask [..., N, N-1] and health
        [..., N] (macm_policy_tdm); noise and logits: float32 [..., N, 11] or None (logits is written).
        agents: uint8 [N] on the device or None (every agent); the rows of agents whose entry is 0 keep what
        ``out`` and ``logits`` held, so the bot's actions can be written first and the policy's over them."""
        lead = self._check_inputs(obs, mask, health)
        N = int(lead[-1])
        for name, t in (("noise", noise), ("logits", logits)):
            if t is not None and (t.device != self.device or not t.is_contiguous() or t.dtype != torch.float32
                                  or tuple(t.shape) != lead + (N_LOGITS,)):
                raise ValueError(f"{name} must be a contiguous float32 {lead + (N_LOGITS,)} tensor on the policy's device")
        if agents is not None and (agents.device != self.device or not agents.is_contiguous()
                                   or agents.dtype != torch.uint8 or tuple(agents.shape) != (N,)):
            raise ValueError(f"agents must be a contiguous uint8 [{N}] tensor on the policy's device")
        if out is None:
            if agents is not None:
                raise ValueError("agents leaves rows untouched: pass the action tensor they live in as out")
            out = torch.empty(lead + (4,), dtype=torch.uint8, device=self.device)
        elif (out.device != self.device or not out.is_contiguous() or out.dtype != torch.uint8
              or tuple(out.shape) != lead + (4,)):
            raise ValueError(f"out must be a contiguous uint8 {lead + (4,)} tensor on the policy's device")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            _abi.check(_abi.lib().macm_policy_tdm(ctypes.byref(self._struct), p(obs), p(mask), p(health),
                                                  1 if obs.dtype == torch.float64 else 0, N, health.numel(), p(agents),
                                                  p(noise), p(out), p(logits), _stream(obs)), "macm_policy_tdm")
        return out

    def _check_agents(self, agents, N):
        if agents is not None and (agents.device != self.device or not agents.is_contiguous()
                                   or agents.dtype != torch.uint8 or tuple(agents.shape) != (N,)):
            raise ValueError(f"agents must be a contiguous uint8 [{N}] tensor on the policy's device")

    def _logits(self, obs, mask, health, agents=None):
        """macm_policy_tdm's logits [..., N, 11] (the actions go to a scratch tensor); zeros in the rows of
        the agents outside ``agents``."""
        lead = tuple(health.shape)
        alloc = torch.zeros if agents is not None else torch.empty
        logits = alloc(lead + (N_LOGITS,), dtype=torch.float32, device=self.device)
        scratch = torch.empty(lead + (4,), dtype=torch.uint8, device=self.device)
        self.act(obs, mask, health, logits=logits, out=scratch, agents=agents)
        return logits

    def forward(self, obs: torch.Tensor, mask: torch.Tensor, health: torch.Tensor,
                agents: torch.Tensor = None) -> torch.Tensor:
        """The logits [..., N, 11] for obs [..., N, N-1, 4], mask [..., N, N-1] and health [..., N] with the
        bits of macm_policy_tdm and the rollouts; where ``params.requires_grad`` is set (and grad mode is on) the
        result is differentiable with respect to params: its backward is one launch of the gradient kernel,
        which recomputes the activations. agents: uint8 [N] on the device or None; the rows of agents whose
        entry is 0 are zeros and take no part in the gradient."""
        self._check_inputs(obs, mask, health)
        self._check_agents(agents, int(health.shape[-1]))
        if obs.requires_grad or health.requires_grad:
            raise ValueError("obs and health must not require grad (the policy has no gradient with respect to them)")
        if self.params.requires_grad and torch.is_grad_enabled():
            return _TdmForward.apply(self.params, obs, mask, health, agents, self)
        return self._logits(obs, mask, health, agents)

    def grad_workspace_bytes(self, rows: int) -> int:
        n = ctypes.c_int64(0)
        _abi.check(_abi.lib().macm_tdm_grad_workspace(int(rows), ctypes.byref(n)), "macm_tdm_grad_workspace")
        return int(n.value)

    def param_grad(self, obs: torch.Tensor, mask: torch.Tensor, health: torch.Tensor, dlogits: torch.Tensor,
                   agents: torch.Tensor = None) -> torch.Tensor:
        """dL/dparams (float32 [n_params], a new tensor) from dlogits = dL/dlogits (float32 [..., N, 11]) over
        the rows of ``forward``, on the current stream (macm_tdm_policy_grad). The rows of agents whose entry in
        ``agents`` is 0 are not read. The workspace is this object's, one per row count: calls on one object
        belong on one stream."""
        lead = self._check_inputs(obs, mask, health)
        N = int(lead[-1])
        self._check_agents(agents, N)
        if (dlogits.device != self.device or not dlogits.is_contiguous() or dlogits.dtype != torch.float32
                or tuple(dlogits.shape) != lead + (N_LOGITS,)):
            raise ValueError(f"dlogits must be a contiguous float32 {lead + (N_LOGITS,)} tensor on the policy's device")
        rows = health.numel()
        cache = self.__dict__.setdefault("_grad_ws", {})
        ws = cache.get(rows)
        if ws is None:
            ws = cache[rows] = torch.empty((max(self.grad_workspace_bytes(rows), 16),), dtype=torch.uint8,
                                           device=self.device)
        grad = torch.empty_like(self.params, requires_grad=False)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            _abi.check(_abi.lib().macm_tdm_policy_grad(
                ctypes.byref(self._struct), p(obs), p(mask), p(health), 1 if obs.dtype == torch.float64 else 0, N, rows,
                p(agents), p(dlogits), p(grad), p(ws), ws.numel(), _stream(obs)), "macm_tdm_policy_grad")
        return grad

    def torch_logits(self, obs: torch.Tensor, mask: torch.Tensor, health: torch.Tensor,
                     params: torch.Tensor = None) -> torch.Tensor:
        """The 11 logits [..., N, 11] as plain differentiable torch, in the dtype of ``params`` (default: this
        policy's float32 params; any tensor of that layout on any device, e.g. a float64 copy that requires
        grad): a masked max over the slots. It lets a learner run its update under torch autograd; it makes no
        bit-exactness claim (torch's matmul does not keep the fmaf order of the kernel).

        The masked-slot rule: a slot whose mask is 0 takes no part, whatever it holds (NaN and inf included:
        it is replaced before the encoder, not multiplied by 0 after it). The empty-set rule: the pool starts
        from +0 and the encoder ends in a relu, so a row without a live slot (a dead agent, the last one
        standing) pools to zeros and its logits are the trunk's on (0, ..., 0, health). The relu is the
        definition's `v > 0 ? v : 0`, so a NaN pre-activation (a NaN or inf in a live slot) gives 0 in the
        forward pass as on the device; the gradient through such a slot is not meaningful (NaN times 0)."""
        P = self.params if params is None else params
        (W1, W2, W3), (b1, b2, b3) = self.unpack(P)
        live = mask.to(torch.bool).unsqueeze(-1)  # [..., N, N-1, 1]
        o = torch.where(live, obs.to(P.dtype), torch.zeros((), dtype=P.dtype, device=obs.device))
        zero = torch.zeros((), dtype=P.dtype, device=obs.device)
        relu = lambda v: torch.where(v > 0, v, zero)  # the definition's: a NaN gives +0 (torch.relu passes it on)
        e = relu(o @ W1 + b1)  # [..., N, N-1, H]
        e = torch.where(live, e, torch.zeros((), dtype=P.dtype, device=obs.device))
        if e.shape[-2] > 0:
            g = e.max(dim=-2).values  # e >= 0: the masked slots' zeros are the pool's start
        else:
            g = e.new_zeros(e.shape[:-2] + e.shape[-1:])
        u = torch.cat([g, health.to(torch.float32).to(P.dtype).unsqueeze(-1)], dim=-1)
        t = relu(u @ W2 + b2)
        return t @ W3 + b3


class _TdmForward(torch.autograd.Function):
    """pol.forward(obs, mask, health) as a function of pol.params: the one-shot kernel forward, the gradient
    kernel backward. Only obs, mask and health (and agents) are kept for the backward, and params for
    autograd's check that they were not overwritten between the two: the backward recomputes the activations
    from the params as they stand."""

    @staticmethod
    def forward(ctx, params, obs, mask, health, agents, pol):
        ctx.pol, ctx.agents = pol, agents
        ctx.save_for_backward(params, obs, mask, health)
        return pol._logits(obs, mask, health, agents)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        _, obs, mask, health = ctx.saved_tensors
        g = ctx.pol.param_grad(obs, mask, health, gout.to(torch.float32).contiguous(), ctx.agents)
        return g, None, None, None, None, None
