"""A whole PPO update on a side stream, behind a backlog (tests/stream_order.py): gym_macm.ppo.update enqueues
three minibatches (moments -> fused gradients -> step, each reading what the launch before it wrote through
device pointers: the moments, the gradients, the stats row, the params and the optimiser state) with nothing
synchronised in between. The indices, the advantages and every other input, the params and the state
included, are written late on the side stream and overwritten right after; the params, the state and the stats
are read by an unsynchronised consumer. Bit for bit against a twin on the default stream; the rig and its
inputs are test_gpu_stream_order_learn.py's."""
import pytest
import torch

import stream_order as so
from stream_order import DEV, Rig
from test_gpu_stream_order_learn import OD, floats, late, late_floats, loss_inputs, nets, run

pytestmark = pytest.mark.gpu

from gym_macm import ppo  # noqa: E402

N_SRC, ROWS, N_MB = 4097, 1345, 3  # several blocks of the moments' sums, tiles of the gradient's; a last tile of one row


@pytest.fixture(scope="module", autouse=True)
def _controls_hold():
    so.require_controls()


def update_rig():
    pol, crit = nets()
    opt = ppo.Adam(pol, crit, lr=1e-2, max_grad_norm=0.5, target_kl=1e3)  # (the gate reads its stats row and stays open)
    pick = lambda seed: torch.randperm(N_SRC, device=DEV, generator=so.generator(seed))[:ROWS].to(torch.int32)
    moved = torch.zeros_like(opt.state)  # the decoy of the state: a fresh head over moments that are not zero
    moved[64:].view(torch.float32).fill_(0.01)
    ins = {"obs": late_floats((N_SRC, OD), 91), **loss_inputs(N_SRC, seed=93),
           **{f"index{i}": late(pick(95 + 2 * i), pick(96 + 2 * i)) for i in range(N_MB)},
           "params_p": (pol.params, floats(pol.params.shape, 7, 0.7), floats(pol.params.shape, 8, 0.7)),
           "params_v": (crit.params, floats(crit.params.shape, 9, 0.7), floats(crit.params.shape, 10, 0.7)),
           "state": (opt.state, torch.zeros_like(opt.state), moved)}
    outs = {"stats": torch.empty((N_MB, 8), dtype=torch.float64, device=DEV), "params_p": pol.params,
            "params_v": crit.params, "state": opt.state}
    r = Rig(None, ins, outs, inout=("params_p", "params_v", "state"))

    def fn(r):
        x = lambda k: ins[k][0]
        ppo.update(opt, x("obs"), x("actions"), x("old_logp"), x("adv"), x("ret"),
                   minibatches=[x(f"index{i}") for i in range(N_MB)], out=outs["stats"])
    r.fn = fn
    r.opt = opt
    return r


def test_update_behind_a_backlog():
    A, B = run("ppo.update of three minibatches", update_rig)
    stats, head = A["out"]["stats"], A["out"]["state"][:64].view(torch.float64)
    assert stats[:, 7].tolist() == [float(ROWS)] * N_MB and bool((stats[1:, 4] > 0).all())
    assert float(head[0]) == N_MB and float(head[3]) == 0.0 and float(head[4]) > 0
    assert so.same_bits(B["out"]["params_p"], A["out"]["params_p"]) and so.same_bits(B["out"]["state"], A["out"]["state"])
