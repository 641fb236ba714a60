"""Stream-order harness (a helper, not a test): run one library call on a side stream so that an
ordering mistake inside the library changes bits.

include/macm.h: "Everything is ordered on `stream`". Behind that the library forks onto streams of its
own (the workgroup rollout's env slices, the B -> C handoff, the split TDM observation) and issues
memsets and copies that must name the caller's stream. On torch's default stream, with the device
synchronised around every call, none of that can go wrong visibly. Here a call runs like this:

    default stream:  [plug: spin T_p ....................................]
    side stream S:   [backlog: spin T_b][late inputs][prefill][the call][clones][late overwrite][getters]

* the backlog keeps everything on S from starting for T_b, while the host has long issued it all;
* the call's inputs hold a valid *decoy* until the late copy on S puts the real values in: a library read
  that runs ahead of S reads the decoy. The decoy is copied back right behind the consumer's clones, all
  queued while the backlog still spins: a library read on an internal stream that was not joined back
  into S races that copy (a missing join shows first in the clones, which then run early too; the
  overwrite adds the reads that no cloned output depends on);
* every output is prefilled on S (NaN for floats, 0xA5 bytes otherwise): an output the library wrote
  from a stream that S does not wait for, or too early, shows the pattern or stale values;
* the consumer clones every output on S with no synchronisation, and then reads the world's state,
  counters, reward sums and status through the library's own getters, which synchronise S themselves;
* the plug holds the default (null) stream for T_p > T_b: torch's side streams do not synchronise with
  it, so whatever the library wrongly issued on stream 0 runs after the consumer has cloned.

The clones are compared bit for bit (uint8 views) with a twin that ran the same call on the default
stream between full synchronisations. Every case asserts that the decoy inputs lead the twin elsewhere
and that the prefill pattern occurs nowhere in the twin's outputs; tests/test_gpu_stream_order_controls.py
shows with torch operations alone that the plug and the backlog work on the machine at hand, and the
case files ask `require_controls()` before they rely on them.

The runtime maps its streams onto a few hardware queues (4 by default), and streams that share a queue run
in submission order, so a delay on one holds the other. S is therefore a side stream that was measured to
run beside the default stream (side_stream()). Which queue a stream created inside the library lands on is
the runtime's choice: where it shares S's queue, a join left out would not show on that run.

Forms in which one kernel waits for another kernel's progress (the handoff, the tail observation, a
pooled spill working set) run without the plug: a foreign kernel resident beside those is another matter.
The backlog stays: it sits ahead in S and has finished before any library kernel may start.
"""
import numpy as np
import torch

from action_gen import DEV, generator  # noqa: F401 (generator: the case files' seeded draws)
from action_gen import random_flock_actions as flock_actions  # noqa: F401
from action_gen import random_tdm_actions as tdm_actions  # noqa: F401

MIN_BACKLOG_MS = 20.0   # T_b >= max(this, 10 x the twin's call)
MIN_MARGIN_MS = 20.0    # T_p >= T_b + max(this, 10 x the twin's call)
MAX_DELAYS_MS = 500.0   # T_b + T_p stays below this: well under the ~1 s clocks of the handoff watcher and the spill wait
PREFILL_BYTE = 0xA5

_rate = None  # spin cycles per millisecond


def spin_rate():
    """Cycles of torch.cuda._sleep per millisecond, measured once with events (the spin kernel's clock is
    the device's)."""
    global _rate
    if _rate is None:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        e0.record()
        torch.cuda._sleep(10 ** 7)
        e1.record()
        torch.cuda.synchronize()
        _rate = 10 ** 7 / max(e0.elapsed_time(e1), 1e-3)
    return _rate


def spin(ms):
    """A kernel that spins for ~ms milliseconds, on the current stream."""
    torch.cuda._sleep(int(ms * spin_rate()))


PROBE_MS = 3.0
_side = None  # the side stream of this process's cases


def runs_beside(x, y):
    """Does work on stream y run while stream x is busy? The runtime maps its streams onto a few hardware
    queues (GPU_MAX_HW_QUEUES, 4 by default), and two streams that share one run in the order of their
    submission: a delay on one then holds the other, and the harness would prove nothing between them.
    Measured: a spin on x, then an empty event pair on y; y's must complete before x's spin ends."""
    torch.cuda.synchronize()
    x_end, y_done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(x):
        spin(PROBE_MS)
        x_end.record()
    with torch.cuda.stream(y):
        torch.cuda._sleep(100)
        y_done.record()
    torch.cuda.synchronize()
    return y_done.elapsed_time(x_end) > PROBE_MS / 2


def stream_beside(*others, tries=32):
    """A torch side stream that runs beside each of `others` (torch's pool hands out 32 in turn), or None."""
    for _ in range(tries):
        s = torch.cuda.Stream(device=DEV)
        if all(s.cuda_stream != o.cuda_stream and runs_beside(o, s) and runs_beside(s, o) for o in others):
            return s
    return None


def side_stream():
    """The side stream S of the cases: one that runs beside the default (null) stream, found once."""
    global _side
    if _side is None:
        _side = stream_beside(torch.cuda.default_stream(DEV))
        assert _side is not None, ("none of torch's side streams runs beside the default stream on this machine: the "
                                   "plug would hold the side stream too, and the stream-order cases prove nothing")
    return _side


def timed(fn):
    """fn() on the default stream between full synchronisations; (its result, milliseconds by events)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return r, e0.elapsed_time(e1)


def delays(t_call_ms, name=""):
    """(T_b, T_p) in ms for a call the twin took t_call_ms for; printed, and bounded as the module says."""
    t_b = max(MIN_BACKLOG_MS, 10.0 * t_call_ms)
    t_p = t_b + max(MIN_MARGIN_MS, 10.0 * t_call_ms)
    print(f"stream-order {name}: twin call {t_call_ms:.3f} ms, T_b {t_b:.1f} ms, T_p {t_p:.1f} ms")
    assert t_b + t_p < MAX_DELAYS_MS, (f"{name}: T_b + T_p = {t_b + t_p:.0f} ms is not below {MAX_DELAYS_MS:.0f} ms: "
                                       "the case's shape is too large for this harness")
    return t_b, t_p


def bits(t):
    """The tensor's bytes."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y))


def prefill(t):
    """NaN for floats, 0xA5 bytes for everything else; on the current stream."""
    if t.is_floating_point():
        t.fill_(float("nan"))
    else:
        t.view(torch.uint8).fill_(PREFILL_BYTE)


def prefilled(t):
    """Per element: does it hold the prefill pattern?"""
    if t.is_floating_point():
        return torch.isnan(t)
    pat = torch.full((1,), PREFILL_BYTE, dtype=torch.uint8, device=t.device).repeat(t.element_size()).view(t.dtype)
    return t == pat


def poison(shape, dtype):
    """Best-effort prefill of an output the call allocates itself: a block of the same size is filled with the
    pattern on the current stream and released, so that the allocator hands the call's allocation that block."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    prefill(t)
    del t


class Rig:
    """One instance of a case: the object under test and the buffers of the call.

    obj:     a FlockVec / World / TdmWorld (its state, counters, reward sums and status are part of the
             comparison), or None for the one-shot kernels
    inputs:  name -> (buf, real, decoy): the call reads `buf`; real and decoy are device staging tensors
    outs:    name -> tensor the call writes (world-owned ones such as vec.obs included)
    inout:   names of `outs` the call also reads (no prefill: the late input carries them)
    rows:    name -> callable(twin's outputs) -> bool tensor over the leading dimension(s): the rows the call
             writes; the others must still hold the prefill afterwards (reset_envs, final outputs)
    keep:    ("state",) where the call leaves a state that does not depend on its inputs (a step that ends every
             episode under autoreset): the decoy must then change the outputs only
    The call may add tensors it allocates itself to `outs` (a returned gradient): they are cloned like the rest.
    """

    def __init__(self, obj=None, inputs=None, outs=None, inout=(), rows=None, keep=()):
        self.obj, self.inputs, self.outs = obj, dict(inputs or {}), dict(outs or {})
        self.inout, self.rows, self.keep = set(inout), dict(rows or {}), keep

    def load(self, which):
        i = 1 if which == "real" else 2
        for v in self.inputs.values():
            v[0].copy_(v[i])


def snapshot(rig, between=None):
    """What a call left behind: clones of the outputs on the current stream (no synchronisation), then
    the world's state, counters, reward sums and status through the library's synchronising getters.
    `between()` runs after the clones are queued and before the first getter synchronises the stream."""
    snap = {"out": {k: t.clone() for k, t in rig.outs.items()}}
    if between is not None:
        between()
    o = rig.obj
    if o is not None:
        snap["state"] = o.get_state()
        snap["counters"] = o.counters()
        if hasattr(o, "reward_sums"):
            per_env, total = o.reward_sums()
            snap["reward_sums"] = np.append(per_env, total)
        snap["status"] = o.status()
    return snap


def _np_bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def differences(x, y, rows=None):
    """The names at which two snapshots differ in bits (outputs restricted to the rows a partial call writes)."""
    diff = []
    for k in x["out"]:
        a, b = x["out"][k], y["out"][k]
        if rows and k in rows:
            a, b = a[rows[k]], b[rows[k]]
        if not same_bits(a, b):
            diff.append(f"out[{k}]")
    for k in x.get("state", {}):
        if not np.array_equal(_np_bits(x["state"][k]), _np_bits(y["state"][k])):
            diff.append(f"state[{k}]")
    for k in ("counters", "reward_sums"):
        if k in x and not np.array_equal(_np_bits(x[k]), _np_bits(y[k])):
            diff.append(k)
    return diff


def run_ordered(name, make, call, plug=True, calls=1, pre=None, make_side=None):
    """The harness's one run (the module docstring). make() -> Rig builds a warmed instance on the default
    stream (three are built: the twin, the decoy twin and the one under test); call(rig) makes the call on
    the current stream with the rig's buffers. `calls` > 1 repeats the call back to back on S with no
    synchronisation between (the twin repeats it too). `pre(rig)` is a call that synchronises the stream
    itself (set_state) and so cannot sit behind a backlog with late inputs: on S it runs behind the backlog,
    which it waits out, and a second backlog follows it, behind which the inputs are written and the call is
    made; the plug is lengthened by that second backlog. The twin runs pre and the call in turn. make_side(S) builds the instance under test
    instead of make(), for objects that must see one stream only (a net's gradient workspace): it warms
    them on S. Returns the two snapshots."""
    S = side_stream()
    a, d = make(), make()
    b = make() if make_side is None else make_side(S)
    S.synchronize()
    torch.cuda.synchronize()

    def whole(rig):
        if pre is not None:
            pre(rig)
        for _ in range(calls):
            call(rig)

    # the twin: real inputs, default stream, full synchronisation; its call is the measure of the delays
    a.load("real")
    _, t_call = timed(lambda: whole(a))
    A = snapshot(a)
    torch.cuda.synchronize()
    assert A.get("status", 0) == 0, f"{name}: the twin's status is {A.get('status')}"
    rows = {k: f(A["out"]) for k, f in a.rows.items()}
    for k, t in A["out"].items():
        if k in a.inout:
            continue
        t = t[rows[k]] if k in rows else t
        assert t.numel() > 0, f"{name}: the twin wrote no row of {k}: the case proves nothing about it"
        assert not bool(prefilled(t).any()), f"{name}: the prefill pattern occurs in the twin's {k}"
    # the decoy must lead elsewhere, or a late-input race could not show
    if a.inputs:
        d.load("decoy")
        whole(d)
        D = snapshot(d)
        torch.cuda.synchronize()
        diff = differences(A, D, rows)
        assert any(s.startswith("out[") for s in diff), f"{name}: the decoy inputs give the real inputs' outputs"
        if a.obj is not None and "state" not in a.keep:
            assert any(s.startswith("state[") for s in diff), f"{name}: the decoy inputs give the real inputs' state"
    t_b, t_p = delays(t_call, name)
    if pre is not None:  # two backlogs on S: the plug outlasts both
        t_p += t_b
        assert 2 * t_b + t_p < MAX_DELAYS_MS, f"{name}: the delays add up to {2 * t_b + t_p:.0f} ms"

    b.load("decoy")
    torch.cuda.synchronize()
    if plug:
        spin(t_p)  # the default stream is held past the consumer
    with torch.cuda.stream(S):
        spin(t_b)
        if pre is not None:
            pre(b)  # synchronises S: the backlog is over when it returns
            spin(t_b)
        b.load("real")
        for k, t in b.outs.items():
            if k not in b.inout:
                prefill(t)
        for _ in range(calls):
            call(b)
        # the late overwrite is queued right behind the clones, before the getters synchronise S: issued after
        # them it would find S drained and could race nothing
        B = snapshot(b, between=lambda: b.load("decoy"))
    S.synchronize()
    torch.cuda.synchronize()

    assert B.get("status", 0) == 0, f"{name}: status {B.get('status')} on the side stream"
    for k, t in b.outs.items():  # a write that lands behind the consumer (from behind the plug, say) shows here
        assert k in b.inout or same_bits(t, B["out"][k]), f"{name}: {k} was written again after the consumer had read it"
    diff = differences(A, B, rows)
    assert not diff, f"{name}: on a side stream behind a backlog these differ from the twin's bits: {diff}"
    for k, r in rows.items():  # a partial call leaves the other rows alone
        rest = B["out"][k][~r]
        assert bool(prefilled(rest).all()), f"{name}: {k} was written outside the rows of the call"
    return A, B


# -- the controls' verdict, shared by the case files ---------------------------------------------------

_controls = None


def controls():
    """What the plug and the backlog prove on this machine, measured once with torch operations only:
    a dict with `misstreamed_unseen` (a copy issued on the default stream behind the plug is not seen by
    S's consumer), `unjoined_unseen` (a consumer on a second side stream that does not wait for S sees the
    prefill), `ordered_seen` (both, correctly ordered, see the real values) and the margins in ms."""
    global _controls
    if _controls is not None:
        return _controls
    n = 1 << 16
    g = torch.Generator(device=DEV)
    g.manual_seed(1234)
    real = torch.rand((n,), device=DEV, generator=g)
    decoy = torch.rand((n,), device=DEV, generator=g)
    res = {}
    _, t_call = timed(lambda: torch.empty_like(real).copy_(real))
    t_b, t_p = delays(t_call, "controls")
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def run(wrong):
        # 1: the input's late copy, on S (right) or on the default stream behind the plug (wrong)
        buf = decoy.clone()
        torch.cuda.synchronize()
        S = side_stream()
        start, cloned, landed = ev(), ev(), ev()
        start.record()  # default stream, ahead of the plug
        spin(t_p)
        if wrong:
            buf.copy_(real)
            landed.record()
        with torch.cuda.stream(S):
            spin(t_b)
            if not wrong:
                buf.copy_(real)
            seen = buf.clone()
            cloned.record()
        S.synchronize()
        torch.cuda.synchronize()
        margin = start.elapsed_time(landed) - start.elapsed_time(cloned) if wrong else None
        return seen, margin

    def run2(wrong):
        # 2: the output's consumer, on S (right) or on a second side stream that does not wait for S (wrong)
        out = torch.empty_like(real)
        torch.cuda.synchronize()
        S = side_stream()
        # a second side stream that runs beside S (streams that share a hardware queue run in submission order)
        S2 = stream_beside(S) if wrong else S
        if S2 is None:
            return real, float("nan")
        start, cloned, written = ev(), ev(), ev()
        start.record()
        with torch.cuda.stream(S):
            prefill(out)
        S.synchronize()
        with torch.cuda.stream(S):
            spin(t_b)
            out.copy_(real)
            written.record()
        with torch.cuda.stream(S2 if wrong else S):
            seen = out.clone()
            cloned.record()
        S.synchronize()
        S2.synchronize()
        torch.cuda.synchronize()
        margin = start.elapsed_time(written) - start.elapsed_time(cloned) if wrong else None
        return seen, margin

    seen, m1 = run(True)
    res["misstreamed_unseen"] = same_bits(seen, decoy)
    res["misstreamed_margin_ms"] = m1
    seen, m2 = run2(True)
    res["unjoined_unseen"] = bool(prefilled(seen).all())
    res["unjoined_margin_ms"] = m2
    res["ordered_seen"] = same_bits(run(False)[0], real) and same_bits(run2(False)[0], real)
    print(f"stream-order controls: a copy mis-issued on the default stream landed {m1:.1f} ms after the consumer's "
          f"clone (unseen: {res['misstreamed_unseen']}); an unjoined consumer read {m2:.1f} ms before the write "
          f"(saw the prefill: {res['unjoined_unseen']}); ordered runs saw the real values: {res['ordered_seen']}")
    _controls = res
    return res


def require_controls():
    """The case files' module-level check: without the controls a pass of theirs would mean nothing."""
    c = controls()
    assert c["misstreamed_unseen"] and c["unjoined_unseen"] and c["ordered_seen"], (
        "the stream-order controls do not hold on this machine (tests/test_gpu_stream_order_controls.py): "
        f"the plug or the backlog proves nothing here, so the stream-order cases cannot pass: {c}")


# -- the decoy of an actions tensor (the real draws are tests/action_gen.py's, as in the other GPU tests) -----

def noop_like(a):
    """The decoy of an actions tensor: all no-op (discrete: 1 is 'no force / no turn', TDM's attack flag 0;
    continuous: zero force)."""
    if a.is_floating_point():
        return torch.zeros_like(a)
    d = torch.ones_like(a)
    if a.shape[-1] == 4:
        d[..., 3] = 0
    return d
