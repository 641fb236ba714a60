"""A learned policy as the actor of Flock's closed loop: a float32 MLP over every agent's obs row.

    pol = MlpPolicy.from_linear_layers([net.l1, net.l2, net.head], device="cuda:0")
    act = pol.act(vec.obs)                          # the first actions, uint8 [E, N, 3]
    vec.set_policy(pol)
    out = vec.rollout_policy(act, 128, noise=gumbel, trajectory=True)   # one launch on the wave path

The definition is include/macm.h's (macm_policy_mlp): ``y[j] = b[j] + sum_k W[k][j] x[k]`` as the
k-ordered float32 fmaf chain, relu on the hidden layers, 9 logits (head h of MultiDiscrete([3, 3, 3])
at ``logits[3h + c]``), ``action[h] = argmax_c(logits[3h + c] + noise[3h + c])``, the lowest index on
ties. The caller supplies the noise (Gumbel noise samples from the softmax; None is the argmax) and
recomputes log-probabilities from the stored logits; the device draws nothing.

``params`` is one flat device tensor, W[in][out] row-major then the bias, layer after layer. The
library reads it at every launch, so a learner that writes new values into it in place
(``pack`` / ``load_linear_layers`` / ``params.copy_``) needs no second registration.
"""
from __future__ import annotations

import ctypes

import torch

from . import _abi

N_LOGITS = 9


def layer_shapes(in_dim: int, hidden: int, n_hidden: int) -> list:
    """[(in, out)] of the layers: n_hidden hidden layers, then the 9 logits."""
    dims = [int(in_dim)] + [int(hidden)] * int(n_hidden) + [N_LOGITS]
    return list(zip(dims[:-1], dims[1:]))


def n_params(in_dim: int, hidden: int, n_hidden: int) -> int:
    return sum(i * o + o for i, o in layer_shapes(in_dim, hidden, n_hidden))


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class MlpPolicy:
    """in_dim: the world's obs_dim (4 polar, 6 cartesian); hidden 16 or 32; n_hidden 1 or 2."""

    def __init__(self, in_dim: int, hidden: int, n_hidden: int, device=None):
        if int(in_dim) not in (4, 6) or int(hidden) not in (16, 32) or int(n_hidden) not in (1, 2):
            raise ValueError("MlpPolicy: in_dim must be 4 or 6, hidden 16 or 32, n_hidden 1 or 2")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("the policy's params live on a GPU device (no CPU fallback)")
        self.in_dim, self.hidden, self.n_hidden = int(in_dim), int(hidden), int(n_hidden)
        self.shapes = layer_shapes(in_dim, hidden, n_hidden)
        self.params = torch.zeros((n_params(in_dim, hidden, n_hidden),), dtype=torch.float32, device=self.device)
        assert self.params.data_ptr() % 16 == 0
        self._struct = _abi.MacmPolicyMlp(self.in_dim, self.hidden, self.n_hidden, 0,
                                          ctypes.c_void_p(self.params.data_ptr()))

    def struct(self) -> "_abi.MacmPolicyMlp":
        """The C-ABI struct (it points into ``params``: this object must outlive its uses)."""
        return self._struct

    def pack(self, weights, biases) -> "MlpPolicy":
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

    def load_linear_layers(self, layers) -> "MlpPolicy":
        """The weights of torch.nn.Linear layers ([out, in] each), transposed to [in][out], into params."""
        return self.pack([l.weight.detach().t().contiguous() for l in layers], [l.bias.detach() for l in layers])

    @classmethod
    def from_linear_layers(cls, layers, device=None) -> "MlpPolicy":
        """layers: the hidden torch.nn.Linear layers (relu between them) and the 9-logit head."""
        layers = list(layers)
        if len(layers) not in (2, 3) or layers[-1].out_features != N_LOGITS:
            raise ValueError("expected 1 or 2 hidden nn.Linear layers and a head with 9 outputs")
        if device is None:
            device = layers[0].weight.device
        return cls(layers[0].in_features, layers[0].out_features, len(layers) - 1, device).load_linear_layers(layers)

    def act(self, obs: torch.Tensor, noise: torch.Tensor = None, logits: torch.Tensor = None,
            out: torch.Tensor = None) -> torch.Tensor:
        """The policy's actions (uint8 [..., 3]) for obs [..., in_dim] (macm_policy_flock); noise and
        logits: float32 [..., 9] or None (logits is written)."""
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
        with torch.cuda.device(self.device):
            _abi.check(L.macm_policy_flock(ctypes.byref(self._struct), p(obs), 1 if obs.dtype == torch.float64 else 0,
                                           obs.numel() // self.in_dim, p(noise), p(out), p(logits), _stream(obs)),
                       "macm_policy_flock")
        return out
