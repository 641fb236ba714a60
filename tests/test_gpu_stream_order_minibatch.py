"""A minibatch update on a side stream, behind a backlog (tests/stream_order.py): adv_moments and then
ppo_grads(index=, adv_norm=) reading the moments through their device pointer with nothing synchronised in
between, with the index, the advantages and every other input written late on the side stream and overwritten
right after. Bit for bit against a twin on the default stream; the rig and its inputs are
test_gpu_stream_order_learn.py's."""
import pytest
import torch

import stream_order as so
from stream_order import DEV, Rig
from test_gpu_stream_order_learn import OD, late, late_floats, loss_inputs, nets, run

pytestmark = pytest.mark.gpu

from gym_macm import ppo  # noqa: E402

N_SRC, ROWS = 4097, 2049  # several blocks of the moments' sums, tiles of the gradient's; a last tile of one row


@pytest.fixture(scope="module", autouse=True)
def _controls_hold():
    so.require_controls()


def minibatch_rig():
    pol, crit = nets()
    pick = lambda seed: torch.randperm(N_SRC, device=DEV, generator=so.generator(seed))[:ROWS].to(torch.int32)
    ins = {"obs": late_floats((N_SRC, OD), 91), **loss_inputs(N_SRC, seed=93), "index": late(pick(95), pick(96))}
    r = Rig(None, ins, {})

    def fn(r):
        x = lambda k: ins[k][0]
        pol.params.grad = crit.params.grad = None
        so.poison((4,), torch.float64)
        so.poison(pol.params.shape, torch.float32)
        r.outs["norm"] = ppo.adv_moments(x("adv"), x("index"))
        r.outs["stats"] = ppo.ppo_grads(pol, crit, x("obs"), x("actions"), x("old_logp"), x("adv"), x("ret"),
                                        index=x("index"), adv_norm=r.outs["norm"])
        r.outs["grad_policy"], r.outs["grad_value"] = pol.params.grad, crit.params.grad
    r.fn = fn
    return r


def test_minibatch_update_behind_its_moments():
    A, _ = run("adv_moments -> ppo_grads(index, adv_norm)", minibatch_rig)
    assert float(A["out"]["norm"][3]) == ROWS and float(A["out"]["stats"][7]) == ROWS
