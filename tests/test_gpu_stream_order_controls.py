"""The stream-order harness (tests/stream_order.py) tested on itself, with torch operations only: on this
machine, does a mistake of the kinds the harness is after change what the consumer sees?

* a copy of the real inputs issued on the default stream, behind the plug, is NOT seen by the side
  stream's consumer: it sees the decoy;
* a consumer on a second side stream that does not wait for the first sees the prefill;
* the same two setups, correctly ordered on the side stream, see the real values.

The runtime maps streams onto a few hardware queues, and two streams on one queue run in submission order
whatever the program says; the harness therefore measures which of torch's side streams run beside the
default stream and beside each other (stream_order.runs_beside) and uses those. If even so the first two do
not hold (side streams that synchronise with the null stream, one hardware queue for everything), the plug
or the backlog proves nothing here, and the stream-order case files, which ask
stream_order.require_controls(), fail with that message instead of passing for no reason."""
import pytest

import stream_order as so

pytestmark = pytest.mark.gpu


def test_a_copy_on_the_default_stream_behind_the_plug_is_not_seen():
    c = so.controls()
    assert c["misstreamed_unseen"], (
        "a copy issued on the default stream behind the plug WAS seen by the side stream's consumer: the plug "
        "proves nothing on this machine (do torch's side streams synchronise with the null stream here?)")
    print(f"the mis-streamed copy landed {c['misstreamed_margin_ms']:.1f} ms after the consumer's clone")
    assert c["misstreamed_margin_ms"] >= so.MIN_MARGIN_MS / 2, c


def test_a_consumer_that_does_not_wait_sees_the_prefill():
    c = so.controls()
    assert c["unjoined_unseen"], (
        "a consumer on a second side stream that does not wait for the first saw the written values: the backlog "
        "proves nothing on this machine (do the two side streams share one in-order queue?)")
    print(f"the unjoined consumer read {c['unjoined_margin_ms']:.1f} ms before the write")
    assert c["unjoined_margin_ms"] >= so.MIN_BACKLOG_MS / 2, c


def test_correctly_ordered_runs_see_the_real_values():
    assert so.controls()["ordered_seen"], "a copy and a consumer both ordered on the side stream did not see the real values"


def test_require_controls_passes_here():
    so.require_controls()


def test_prefill_and_its_detection():
    import torch
    for dt in (torch.float32, torch.float64, torch.uint8, torch.int32):
        t = torch.zeros((5, 3), dtype=dt, device=so.DEV)
        assert not bool(so.prefilled(t).any())
        so.prefill(t)
        assert bool(so.prefilled(t).all()), dt
    assert not so.same_bits(torch.zeros(2, device=so.DEV), -torch.zeros(2, device=so.DEV)), "bits, not values"
