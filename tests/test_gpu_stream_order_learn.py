"""The one-shot kernels and the autograd layer on a side stream, behind a backlog (tests/stream_order.py):
MlpPolicy.act, MlpCritic.value, the scripted bots, gae, log_prob, both nets' param_grad, macm_ppo_loss through
ctypes with every output, ppo_grads, the composed loss's backward (whose incoming gradient reaches the kernel
through a device pointer with no synchronisation), and a gradient workspace that grows while the launch
before is still queued. The reference is the same call on the default stream between full synchronisations,
on objects of its own: each net, and the module workspace of ppo_loss, sees one stream throughout a case."""
import ctypes

import pytest
import torch

import stream_order as so
from stream_order import DEV, Rig

pytestmark = pytest.mark.gpu

from gym_macm import _abi, bots, ppo  # noqa: E402
from gym_macm.policy import MlpCritic, MlpPolicy, gae  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _controls_hold():
    so.require_controls()


ROWS = (65, 4097)      # a wave and a row; several blocks and a row
BIG = 131137           # the gradient paths: more 64-row tiles than waves that write a partial, reduced in a second launch
OD = 4


def floats(shape, seed, scale=1.0):
    return (torch.rand(tuple(shape), device=DEV, generator=so.generator(seed)) * 2 - 1) * scale


def late(real, decoy):
    return (torch.empty_like(real), real, decoy)


def late_floats(shape, seed, scale=1.0):
    return late(floats(shape, seed, scale), floats(shape, seed + 1000, scale))


def late_actions(shape, seed):
    return late(so.flock_actions(shape, seed), so.flock_actions(shape, seed + 1000))


def nets(seed=1):
    pol, crit = MlpPolicy(OD, 16, 2, device=DEV), MlpCritic(OD, 32, 1, device=DEV)
    pol.params.copy_(floats(pol.params.shape, seed, 0.7))
    crit.params.copy_(floats(crit.params.shape, seed + 1, 0.7))
    return pol, crit


def run(name, build, warm=True):
    """build() -> Rig with .fn; the twin's objects are built and warmed on the default stream, the ones under
    test on the side stream (warm=False: not warmed at all, the measured call is the objects' first)."""
    def made():
        rig = build()
        if warm:
            rig.load("decoy")
            rig.fn(rig)
        return rig

    def made_on(S):
        # ppo_loss keeps one workspace per device in the module global ppo._ws, and its docstring makes "one
        # stream per workspace" the caller's duty. The twin's calls own it on the default stream, so the side
        # stream's calls get a dict of their own, swapped in around each of them (made_on, call). There is no
        # public hook for this; the backward is synchronous inside rig.fn, so the swap covers it.
        ws = {}
        keep, ppo._ws = ppo._ws, ws
        try:
            with torch.cuda.stream(S):
                rig = made()
        finally:
            ppo._ws = keep
        rig.ws = ws
        return rig

    def call(rig):
        if hasattr(rig, "ws"):
            keep, ppo._ws = ppo._ws, rig.ws
            try:
                rig.fn(rig)
            finally:
                ppo._ws = keep
        else:
            rig.fn(rig)

    return so.run_ordered(name, made, call, make_side=made_on)


@pytest.mark.parametrize("rows", ROWS)
def test_policy_act(rows):
    def build():
        pol, _ = nets()
        ins = {"obs": late_floats((rows, OD), 3), "noise": late_floats((rows, 9), 5, 2.0),
               "params": (pol.params, floats(pol.params.shape, 7, 0.7), floats(pol.params.shape, 8, 0.7))}
        outs = {"actions": torch.empty((rows, 3), dtype=torch.uint8, device=DEV),
                "logits": torch.empty((rows, 9), dtype=torch.float32, device=DEV)}
        r = Rig(None, ins, outs)
        r.fn = lambda r: pol.act(ins["obs"][0], noise=ins["noise"][0], logits=outs["logits"], out=outs["actions"])
        return r
    run(f"policy.act {rows}", build)


@pytest.mark.parametrize("rows", ROWS)
def test_critic_value(rows):
    def build():
        _, crit = nets()
        ins = {"obs": late_floats((rows, OD), 3)}
        outs = {"values": torch.empty((rows,), dtype=torch.float32, device=DEV)}
        r = Rig(None, ins, outs)
        r.fn = lambda r: crit.value(ins["obs"][0], out=outs["values"])
        return r
    run(f"critic.value {rows}", build)


@pytest.mark.parametrize("rows", ROWS)
def test_bots_flock(rows):
    def build():
        ins = {"obs": late_floats((rows, OD), 11, 3.0)}
        outs = {"actions": torch.empty((rows, 3), dtype=torch.uint8, device=DEV)}
        r = Rig(None, ins, outs)
        r.fn = lambda r: bots.flock_actions(ins["obs"][0], out=outs["actions"])
        return r
    run(f"bots.flock {rows}", build)


@pytest.mark.parametrize("E,N", [(13, 5), (241, 17)])  # 65 and 4097 agent rows
def test_bots_combat(E, N):
    def build():
        bit = lambda seed: (torch.rand((E, N, N - 1), device=DEV, generator=so.generator(seed)) < 0.7).to(torch.uint8)
        ins = {"obs": late_floats((E, N, N - 1, 4), 13, 3.0), "mask": late(bit(15), bit(16))}
        for t, seed in zip(ins["obs"][1:], (17, 18)):  # the ally flag: the bot acts on the slots where it is 0
            t[..., 3] = bit(seed).to(torch.float32)
        outs = {"actions": torch.empty((E, N, 4), dtype=torch.uint8, device=DEV)}
        r = Rig(None, ins, outs)
        r.fn = lambda r: bots.combat_actions(ins["obs"][0], ins["mask"][0], out=outs["actions"])
        return r
    run(f"bots.combat {E * N}", build)


@pytest.mark.parametrize("E,N", [(13, 5), (241, 17)])
def test_gae(E, N):
    K = 7

    def build():
        bit = lambda seed: (torch.rand((K, E), device=DEV, generator=so.generator(seed)) < 0.2).to(torch.uint8)
        ins = {"reward": late_floats((K, E, N), 21), "values": late_floats((K, E, N), 23),
               "boot": late_floats((K, E, N), 25), "done": late(bit(27), bit(28))}
        outs = {"adv": torch.empty((K, E, N), dtype=torch.float32, device=DEV),
                "ret": torch.empty((K, E, N), dtype=torch.float32, device=DEV)}
        r = Rig(None, ins, outs)
        r.fn = lambda r: gae(ins["reward"][0], ins["values"][0], ins["boot"][0], ins["done"][0], 0.99, 0.95,
                             adv=outs["adv"], ret=outs["ret"])
        return r
    run(f"gae {K}x{E * N}", build)


@pytest.mark.parametrize("rows", ROWS)
def test_log_prob(rows):
    def build():
        ins = {"logits": late_floats((rows, 9), 31, 3.0), "actions": late_actions((rows,), 33)}
        outs = {"entropy": torch.empty((rows,), dtype=torch.float32, device=DEV)}
        r = Rig(None, ins, outs)

        def fn(r):
            so.poison((rows,), torch.float32)  # logp is allocated inside
            r.outs["logp"] = ppo.log_prob(ins["logits"][0], ins["actions"][0], entropy=outs["entropy"])
        r.fn = fn
        return r
    run(f"log_prob {rows}", build)


@pytest.mark.parametrize("which", ["policy", "critic"])
@pytest.mark.parametrize("rows", ROWS + (BIG,))
def test_param_grad(rows, which):
    def build():
        net = nets()[0 if which == "policy" else 1]
        ins = {"obs": late_floats((rows, OD), 41), "dout": late_floats((rows, 9) if which == "policy" else (rows,), 43)}
        r = Rig(None, ins, {})

        def fn(r):
            so.poison(net.params.shape, torch.float32)
            r.outs["grad"] = net.param_grad(ins["obs"][0], ins["dout"][0])
        r.fn = fn
        return r
    run(f"param_grad {which} {rows}", build)


def loss_inputs(rows, seed=51):
    """The per-row inputs of the loss; old_logp around the log-probability of other logits (finite ratios)."""
    other = floats((rows, 9), seed + 7, 1.5)
    acts = late_actions((rows,), seed + 1)
    old = lambda a, s: (ppo.log_prob(other, a) + floats((rows,), s, 0.3)).contiguous()
    ins = {"actions": acts, "old_logp": late(old(acts[1], seed + 2), old(acts[2], seed + 3)),
           "adv": late_floats((rows,), seed + 4), "ret": late_floats((rows,), seed + 5)}
    torch.cuda.current_stream().synchronize()
    return ins


@pytest.mark.parametrize("rows", ROWS)
def test_ppo_loss_c_abi(rows):
    """macm_ppo_loss with every output (dlogits, dvalues, stats), the stream handle passed directly."""
    def build():
        ins = {"logits": late_floats((rows, 9), 61, 1.5), "values": late_floats((rows,), 63), **loss_inputs(rows),
               "scale": late(torch.full((1,), 0.5, device=DEV), torch.full((1,), 2.0, device=DEV))}
        outs = {"dlogits": torch.empty((rows, 9), dtype=torch.float32, device=DEV),
                "dvalues": torch.empty((rows,), dtype=torch.float32, device=DEV),
                "stats": torch.empty((8,), dtype=torch.float64, device=DEV)}
        ws = torch.empty((max(ppo.workspace_bytes(rows), 16),), dtype=torch.uint8, device=DEV)
        cfg = ppo.config()
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        r = Rig(None, ins, outs)
        r.ws_buf = ws
        r.fn = lambda r: _abi.check(_abi.lib().macm_ppo_loss(
            ctypes.byref(cfg), rows, p(ins["logits"][0]), p(ins["actions"][0]), p(ins["old_logp"][0]), p(ins["adv"][0]),
            p(ins["values"][0]), p(ins["ret"][0]), None, p(ins["scale"][0]), p(outs["dlogits"]), p(outs["dvalues"]),
            p(outs["stats"]), p(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "macm_ppo_loss")
        return r
    run(f"macm_ppo_loss {rows}", build)


def grads_rig(rows):
    pol, crit = nets()
    ins = {"obs": late_floats((rows, OD), 71), **loss_inputs(rows)}
    r = Rig(None, ins, {})

    def fn(r):
        pol.params.grad = crit.params.grad = None
        so.poison(pol.params.shape, torch.float32)
        r.outs["stats"] = ppo.ppo_grads(pol, crit, ins["obs"][0], ins["actions"][0], ins["old_logp"][0], ins["adv"][0],
                                        ins["ret"][0])
        r.outs["grad_policy"], r.outs["grad_value"] = pol.params.grad, crit.params.grad
    r.fn = fn
    return r


@pytest.mark.parametrize("rows", ROWS + (BIG,))
def test_ppo_grads(rows):
    run(f"ppo_grads {rows}", lambda: grads_rig(rows))


@pytest.mark.parametrize("rows", ROWS)
def test_composed_loss_backward(rows):
    """ppo_loss(pol.forward(obs), crit.forward(obs), ...)[0].backward() entirely on the side stream: the forward
    kernels, the loss's stats launch, the loss's backward launch scaled through a device pointer, both nets'
    gradient launches."""
    def build():
        pol, crit = nets()
        pol.params.requires_grad_(True)
        crit.params.requires_grad_(True)
        ins = {"obs": late_floats((rows, OD), 81), **loss_inputs(rows)}
        r = Rig(None, ins, {})

        def fn(r):
            pol.params.grad = crit.params.grad = None
            loss, stats = ppo.ppo_loss(pol.forward(ins["obs"][0]), crit.forward(ins["obs"][0]), ins["actions"][0],
                                       ins["old_logp"][0], ins["adv"][0], ins["ret"][0])
            (loss * 0.75).backward()  # the incoming gradient is a device value, not 1
            r.outs.update(loss=loss.detach(), stats=stats, grad_policy=pol.params.grad, grad_value=crit.params.grad)
        r.fn = fn
        return r
    A, _ = run(f"composed backward {rows}", build)
    assert float(A["out"]["grad_policy"].abs().max()) > 0 and float(A["out"]["grad_value"].abs().max()) > 0


@pytest.mark.parametrize("how", ["param_grad", "ppo_grads"])
def test_workspace_growth_in_flight(how):
    """A gradient call at 65 rows directly followed by one at 131,137 rows on the same object, behind one
    backlog with no synchronisation between: the object's workspace is replaced while the first launch that
    uses the old one is still queued. Both results equal their default-stream bits."""
    def build():
        pol, crit = nets()
        small, big = 65, BIG
        if how == "param_grad":
            ins = {f"{k}{n}": late_floats(shape, seed + len(k)) for n, seed in ((small, 91), (big, 93))
                   for k, shape in (("obs", (n, OD)), ("dout", (n, 9)))}
        else:
            ins = {f"{k}{n}": v for n, seed in ((small, 91), (big, 93))
                   for k, v in {"obs": late_floats((n, OD), seed + 40), **loss_inputs(n, seed)}.items()}
        r = Rig(None, ins, {})

        def fn(r):
            assert getattr(pol, "_grad_ws", None) is None, "the workspace must start absent and grow twice"
            for n in (small, big):
                x = lambda k: ins[f"{k}{n}"][0]
                if how == "param_grad":
                    r.outs[f"grad{n}"] = pol.param_grad(x("obs"), x("dout"))
                else:
                    pol.params.grad = crit.params.grad = None
                    r.outs[f"stats{n}"] = ppo.ppo_grads(pol, crit, x("obs"), x("actions"), x("old_logp"), x("adv"),
                                                        x("ret"))
                    r.outs[f"grad_policy{n}"], r.outs[f"grad_value{n}"] = pol.params.grad, crit.params.grad
                r.sizes = getattr(r, "sizes", []) + [pol._grad_ws.numel()]
            assert r.sizes[-1] > r.sizes[-2], "the workspace did not grow between the two calls"
        r.fn = fn
        return r
    run(f"workspace growth {how}", build, warm=False)
