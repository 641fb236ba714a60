"""The set policy's gradient launches on a side stream, behind a backlog (tests/stream_order.py):
TdmSetPolicy.param_grad and the autograd pair (forward, then a loss's backward through it), with and without
`agents`. Inputs are written late and overwritten after, the outputs are prefilled, the consumer is not joined;
the results are bit for bit those of a twin on the default stream, on objects of its own: a policy's gradient
workspace sees one stream throughout a case."""
import pytest
import torch

import stream_order as so
import tdm_policy_ref as ref
from stream_order import DEV, Rig

pytestmark = pytest.mark.gpu

from gym_macm.tdm_policy import N_LOGITS, TdmSetPolicy  # noqa: E402

SHAPES = [(13, 5), (241, 17)]  # 65 and 4097 agent rows: a tile and a row; several waves and a row


@pytest.fixture(scope="module", autouse=True)
def _controls_hold():
    so.require_controls()


def floats(shape, seed, scale=1.0, dtype=torch.float32):
    return ((torch.rand(tuple(shape), device=DEV, generator=so.generator(seed), dtype=dtype) * 2 - 1) * scale)


def late(real, decoy):
    return (torch.empty_like(real), real, decoy)


def bits_of(shape, seed):
    return (torch.rand(tuple(shape), device=DEV, generator=so.generator(seed)) < 0.7).to(torch.uint8)


def inputs(E, N):
    return {"obs": late(floats((E, N, N - 1, 4), 3, 3.0), floats((E, N, N - 1, 4), 1003, 3.0)),
            "mask": late(bits_of((E, N, N - 1), 5), bits_of((E, N, N - 1), 1005)),
            "health": late(floats((E, N), 7, dtype=torch.float64).abs(), floats((E, N), 1007, dtype=torch.float64).abs()),
            "dlogits": late(floats((E, N, N_LOGITS), 9), floats((E, N, N_LOGITS), 1009))}


def policy(grad):
    pol = TdmSetPolicy(32, DEV)
    pol.params.copy_(torch.from_numpy(ref.seeded_params(32)))
    if grad:
        pol.params.requires_grad_()
    return pol


def agents_of(N, some):
    return (torch.arange(N, device=DEV) % 3 != 1).to(torch.uint8) if some else None


def run(name, build):
    """build() -> Rig with .fn; the twin's objects are built and warmed on the default stream, the ones under test
    on the side stream."""
    def made():
        rig = build()
        rig.load("decoy")
        rig.fn(rig)
        return rig

    def made_on(S):
        with torch.cuda.stream(S):
            return made()

    return so.run_ordered(name, made, lambda rig: rig.fn(rig), make_side=made_on)


@pytest.mark.parametrize("some", [False, True], ids=["all", "agents"])
@pytest.mark.parametrize("E,N", SHAPES)
def test_param_grad(E, N, some):
    def build():
        pol, ins, agents = policy(False), inputs(E, N), agents_of(N, some)
        r = Rig(None, ins, {})

        def fn(r):
            so.poison(pol.params.shape, torch.float32)
            r.outs["grad"] = pol.param_grad(ins["obs"][0], ins["mask"][0], ins["health"][0], ins["dlogits"][0],
                                            agents=agents)
        r.fn = fn
        return r
    A, _ = run(f"tdm param_grad {E}x{N}", build)
    assert float(A["out"]["grad"].abs().max()) > 0


@pytest.mark.parametrize("some", [False, True], ids=["all", "agents"])
@pytest.mark.parametrize("E,N", SHAPES)
def test_forward_then_backward(E, N, some):
    """pol.forward and a loss's backward entirely on the side stream: the one-shot kernel, torch's own kernels
    of the loss, the gradient launch and its reduction."""
    def build():
        pol, ins, agents = policy(True), inputs(E, N), agents_of(N, some)
        r = Rig(None, ins, {})

        def fn(r):
            pol.params.grad = None
            so.poison((E, N, N_LOGITS), torch.float32)
            z = pol.forward(ins["obs"][0], ins["mask"][0], ins["health"][0], agents=agents)
            so.poison(pol.params.shape, torch.float32)
            (torch.tanh(z) * ins["dlogits"][0]).sum().backward()
            r.outs.update(logits=z.detach(), grad=pol.params.grad)
        r.fn = fn
        return r
    A, _ = run(f"tdm forward/backward {E}x{N}", build)
    assert float(A["out"]["grad"].abs().max()) > 0
