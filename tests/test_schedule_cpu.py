"""CPU test of graphed.ahead_schedule, the slot arithmetic of GraphedTrainStep's side-stream schedule at (G, A, P): it reproduces
the formulas the two hand-written schedules used (lookahead=L: (1, L, L); trunk_pairs=G: (G, 1, 2 or RING_SLOTS)), and a simulation
shows that no trunk slot or staging set is overwritten before the last reader of what it held has run - for the waiting schedule
and, with the class's RING_* constants, for the ring, where one slot or one set fewer must show a hazard."""
import pytest

from __graft_entry__ import load_package

load_package()
from drn_wsod_pytorch_amd.graphed import GraphedTrainStep, ahead_arity, ahead_schedule  # noqa: E402

LAG, SETS, SLOTS = GraphedTrainStep.RING_LAG, GraphedTrainStep.RING_SETS, GraphedTrainStep.RING_SLOTS


@pytest.mark.parametrize("L", [2, 3, 4])
def test_lookahead_formulas(L):
    assert ahead_arity(1, L) == L - 1
    for t in range(64):
        s = ahead_schedule(t, 1, L, L)
        upcoming = list(range(t + 2, t + L + 1))  # the L-1 batches after next_batch
        assert s.launch == (t + L) % L
        assert (s.pool_slot, s.pool_part) == ((t + 1) % L, 0)
        assert upcoming[s.stage] == [upcoming[-1]]
        assert ahead_arity(1, L) == len(upcoming)
        assert s.nb == 0


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("G", [2, 3, 4, 8])
def test_group_formulas(G, P):
    assert ahead_arity(G, 1) == 2 * G - 2
    for t in range(64):
        s = ahead_schedule(t, G, 1, P, SETS)
        assert s.launch == ((t // G + 1) % P if t % G == 0 else None)
        assert s.stage == slice(G - 2, 2 * G - 2)
        assert (s.pool_slot, s.pool_part) == (((t + 1) // G) % P, (t + 1) % G)
        assert s.nb == (t + 1) % SETS
        assert ahead_schedule(t, G, 1, P).nb == 0  # one staging set where the ring is off


def hazards(G, A, P, sets, lag, steps=200):
    """Simulate `steps` steps.  Step t writes batch t+1's proposals / labels into staging set `nb` and, when a chain is launched,
    group t // G + A into trunk slot `launch`; the pooling at its end reads batch t+1 from the set and group (t+1) // G from slot
    `pool_slot`.  Priming left groups 0 .. A-1 in slots 0 .. A-1 and runs step 0 eagerly on one staging set, then waits for the
    device.  For every write at step t, t' is the last step at whose end the content it destroys is read.  What orders the write
    behind that read: lag = 0, the side stream's wait for the main stream at the start of step t, which covers the steps up to
    t-1; lag > 0 (ring), the host's wait for the heads of step t - lag, which run behind the read at the end of step t' when
    t' + 1 <= t - lag.  -> the list of violations, and of reads that do not find what they want (it must be empty too)."""
    content = {("slot", q): ("group", q) for q in range(A)}
    last_read = {}  # content -> last step at whose end it is read
    writes, bad = [], []
    for t in range(steps):
        s = ahead_schedule(t, G, A, P, sets if lag and t else 1)
        new = [(("set", s.nb), ("batch", t + 1))]
        if s.launch is not None:
            new.append((("slot", s.launch), ("group", t // G + A)))
        for res, what in new:
            writes.append((t, res, content.get(res)))
            content[res] = what
        for res, want in ((("set", s.nb), ("batch", t + 1)), (("slot", s.pool_slot), ("group", (t + 1) // G))):
            if content.get(res) != want:
                bad.append(("stale read", t, res, want, content.get(res)))
            last_read[want] = t
    for t, res, old in writes:
        t_read = last_read.get(old)
        if old is None or t_read is None:
            continue
        if t_read >= t:
            bad.append(("destroyed before its last read", t, res, old, t_read))
        elif lag and t >= 1 and t_read >= 1 and not t_read + 1 <= t - lag:  # (t' <= 0: priming ends with a device-wide wait)
            bad.append(("ring: not behind the heads the host waited for", t, res, old, t_read))
    return bad


@pytest.mark.parametrize("G", [2, 3, 4, 8])
def test_no_slot_or_set_is_overwritten_early(G):
    assert hazards(G, 1, 2, 1, 0) == []              # the waiting schedule: every last reader is at t' <= t-1
    assert hazards(G, 1, SLOTS, SETS, LAG) == []     # the ring: t' + 1 <= t - RING_LAG


@pytest.mark.parametrize("L", [2, 3, 4])
def test_lookahead_slots_are_not_overwritten_early(L):
    assert hazards(1, L, L, 1, 0) == []


def test_the_check_can_fail():
    assert any(h[0].startswith("ring") and h[2][0] == "slot" for h in hazards(2, 1, SLOTS - 1, SETS, LAG))
    assert any(h[0].startswith("ring") and h[2][0] == "set" for h in hazards(2, 1, SLOTS, SETS - 1, LAG))
    assert hazards(2, 1, 1, 1, 0) and hazards(1, 3, 2, 1, 0)  # waiting schedule: one slot for groups, two slots at lookahead 3


# ---- launch order of _run_ahead, per stream, against the record of the two schedules it replaced ------------------------------------
class _Recorder:
    """stands in for torch.cuda's streams and events: every wait, record and host-side event wait goes into `log` in program
    order, with the stream it was issued on; an event is known by the position of its record"""

    def __init__(self):
        self.log, self.cur, self.n = [], [], 0
        rec = self

        class Stream:
            def __init__(self, name=None):
                rec.n += 1
                self.name = name or "side%d" % rec.n

            def wait_stream(self, other):
                rec.log.append((self.name, "wait_stream", other.name))

            def wait_event(self, ev):
                rec.log.append((self.name, "wait_event", ev.tag))

        class Event:
            def __init__(self, tag=None):
                self.tag = tag

            def record(self, stream=None):
                stream = stream or rec.cur[-1]
                self.tag = ("rec", stream.name, len(rec.log))
                rec.log.append((stream.name, "record"))

            def synchronize(self):
                rec.log.append(("host", "sync", self.tag))

        self.Stream, self.Event = Stream, Event
        self.cur.append(Stream("main"))

    def stream(self, s):
        import contextlib

        @contextlib.contextmanager
        def ctx():
            self.cur.append(s)
            try:
                yield
            finally:
                self.cur.pop()
        return ctx()

    def say(self, *what):
        self.log.append((self.cur[-1].name,) + what)


def _launch_order(monkeypatch, G, A, P, ring, split_tail, stage_ahead, steps=13, inputs_ready=None, hook_event=True):
    """_run_ahead for `steps` steps (step 0 eager, as at priming, then replays) on a GraphedTrainStep whose pieces only log.
    inputs_ready: "none" passes step()'s default explicitly, "event" one event per replayed step (tagged ("ready", step));
    hook_event=False: the fc6 tail leaves no small_ready_event behind (no pipelined optimizer's hook)"""
    import torch

    rec = _Recorder()
    monkeypatch.setattr(torch.cuda, "Stream", rec.Stream)
    monkeypatch.setattr(torch.cuda, "Event", rec.Event)
    monkeypatch.setattr(torch.cuda, "stream", rec.stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: rec.cur[-1])
    ids = lambda items: tuple(x["id"] for x in items)
    o = GraphedTrainStep.__new__(GraphedTrainStep)
    o.split_tail, o.stage_ahead, o.iter_size, o._t, o._nb, o._ring_on, o._ring_evs = split_tail, stage_ahead, 1, 0, 0, ring, []

    class Opt:
        small_ready_event = None

    class Engine:
        kshard = None

        def run_fc1_tail(self):
            rec.say("tail")
            if hook_event:
                o.opt.small_ready_event = rec.Event()
                o.opt.small_ready_event.record()

    class Graph:
        def __init__(self, slot):
            self.slot = slot

        def replay(self):
            rec.say("bb", self.slot, "replay")

    o.opt, o.engine = Opt(), Engine()
    o._heads = lambda eager: rec.say("heads", eager) or {}
    o._stage_props = lambda b: rec.say("props", ids(b), o._nb)
    o._stage_labels_ahead = lambda b, via_stage=False: rec.say("labels", ids(b), via_stage, o._nb)
    o._stage_image = lambda items, slot: rec.say("images", ids(items), slot)
    o._bb_body = lambda slot: rec.say("bb", slot, "eager")
    o._pool_body = lambda slot, part: rec.say("pool", slot, part, o._nb)
    o._opt_step = lambda: rec.say("opt_step")
    o._GAP = (G, A, P)
    o._sides = [rec.Stream("side0")] + [rec.Stream() for _ in range(A - 2)]
    o._done = [rec.Event("prime%d" % q) if q < A else None for q in range(P)]
    o.g_pbb = [Graph(slot) for slot in range(P)]
    seq = [[{"id": k}] for k in range(steps + 2 + ahead_arity(G, A))]
    for i in range(steps):
        args = (i == 0, seq[i + 1], tuple(seq[i + 2: i + 2 + ahead_arity(G, A)]))
        if inputs_ready is None:
            o._run_ahead(*args)
        else:
            o._run_ahead(*args, () if inputs_ready == "none" or i == 0 else (rec.Event(("ready", i)),))
    return rec.log


@pytest.fixture(scope="module")
def recorded_order():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graphed_launch_order.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("stage_ahead", [True, False])
@pytest.mark.parametrize("split_tail", [True, False])
def test_launch_order_is_the_recorded_one(monkeypatch, recorded_order, split_tail, stage_ahead):
    """tests/golden/graphed_launch_order.json was recorded with this recorder from the two hand-written schedules that _run_ahead
    replaced (lookahead 2 / 3 / 4; groups of 2 / 3 / 4 / 8, waiting and ring), 13 steps each: every launch, copy, event record,
    stream wait, event wait and host-side wait, with its stream, slot, part, staging set and batches, in program order.  The one
    schedule has to issue exactly that at each of their parameters."""
    import json

    cases = [("L%d" % L, 1, L, L, False) for L in (2, 3, 4)]
    cases += [("G%d ring%d" % (G, ring), G, 1, SLOTS if ring else 2, ring) for G in (2, 3, 4, 8) for ring in (False, True)
              if split_tail or not ring]
    for name, G, A, P, ring in cases:
        got = _launch_order(monkeypatch, G, A, P, ring, split_tail, stage_ahead)
        want = recorded_order["%s split%d ahead%d" % (name, split_tail, stage_ahead)]
        assert json.loads(json.dumps(got)) == want, name


def _cases(split_tail):
    cases = [("L%d" % L, 1, L, L, False) for L in (2, 3, 4)]
    return cases + [("G%d ring%d" % (G, ring), G, 1, SLOTS if ring else 2, ring) for G in (2, 3, 4, 8) for ring in (False, True)
                    if split_tail or not ring]


@pytest.mark.parametrize("stage_ahead", [True, False])
@pytest.mark.parametrize("split_tail", [True, False])
def test_inputs_ready_none_enqueues_nothing_and_an_event_only_its_waits(monkeypatch, recorded_order, split_tail, stage_ahead):
    """step(inputs_ready=None) - bench.py's call - issues the recorded order, entry for entry.  With an event per step the order
    is the same but for wait_event entries on that event: one on the side stream in front of its first staging copy of the step
    (proposals with stage_ahead, else the images of a launched chain), and with stage_ahead off one on the main stream in front
    of the proposals staged there."""
    import json

    for name, G, A, P, ring in _cases(split_tail):
        want = recorded_order["%s split%d ahead%d" % (name, split_tail, stage_ahead)]
        none = _launch_order(monkeypatch, G, A, P, ring, split_tail, stage_ahead, inputs_ready="none")
        assert json.loads(json.dumps(none)) == want, name
        got = _launch_order(monkeypatch, G, A, P, ring, split_tail, stage_ahead, inputs_ready="event")
        is_wait = lambda e: e[1] == "wait_event" and isinstance(e[2], tuple) and e[2][0] == "ready"
        # (events are known by the position of their record: compare with the waits' own positions taken out)
        strip = lambda log: [tuple(x for x in e if not (isinstance(x, tuple) and x and x[0] == "rec")) for e in log]
        assert strip([e for e in got if not is_wait(e)]) == strip(none), name
        waits = [(k, e) for k, e in enumerate(got) if is_wait(e)]
        assert {e[2][1] for _, e in waits} <= set(range(1, 13)) and waits, name
        for k, e in waits:
            nxt = got[k + 1]
            if e[0] == "main":
                assert not stage_ahead and nxt[:2] == ("main", "props"), (name, e, nxt)
            else:
                assert nxt[0] == e[0] and nxt[1] == ("props" if stage_ahead else "images"), (name, e, nxt)
        for i in range(1, 13):  # every step that stages caller tensors on a stream has that stream wait first
            mine = [e for _, e in waits if e[2][1] == i]
            assert len(mine) >= 1, (name, i)
            assert len(mine) == len({e[0] for e in mine}), (name, i)


class _Hooks:
    def on_ready(self, what):
        pass


def _gated(hook_owner, pipelined, ring=True):
    o = GraphedTrainStep.__new__(GraphedTrainStep)

    class Engine:
        kshard = None

    o.opt = _Hooks()
    o.opt._pipelined = pipelined
    o.engine = Engine()
    o.engine.grad_ready_hook = {"opt": o.opt.on_ready, "dp": _Hooks().on_ready, "none": None}[hook_owner]
    o.trunk_pairs, o.split_tail, o._ring_want = True, True, ring
    return o


def test_ring_needs_this_optimizers_pipelined_hook_and_one_rank(monkeypatch):
    """The ring's throttle is the event FusedSGD's hook leaves behind the heads.  Another object's hook alone (DataParallel's
    without enable_pipelined) or a job of several ranks gets the waiting schedule - and the step runs: it used to raise "the ring
    schedule needs the pipelined optimizer's hook" at the first replay."""
    import torch.distributed as dist

    assert _gated("opt", True)._ring_allowed() is True
    assert _gated("opt", True, ring=False)._ring_allowed() is False
    assert _gated("dp", False)._ring_allowed() is False
    assert _gated("dp", True)._ring_allowed() is False
    assert _gated("none", True)._ring_allowed() is False
    o = _gated("opt", True)
    o.opt._dp = type("Dp", (), {"world": 2})()
    assert o._ring_allowed() is False
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    assert _gated("opt", True)._ring_allowed() is False
    monkeypatch.undo()
    # DataParallel's hook only, ring=True asked for: _ring_on is False and thirteen steps run, in the waiting schedule's order
    ring_on = _gated("dp", False)._ring_allowed()
    assert ring_on is False
    got = _launch_order(monkeypatch, 2, 1, 2, ring_on, True, True, hook_event=False)
    want = _launch_order(monkeypatch, 2, 1, 2, False, True, True)
    want = [e for k, e in enumerate(want) if not (e == ("main", "record") and want[k - 1] == ("main", "tail"))]  # (the hook's event)
    strip = lambda log: [tuple(x for x in e if not (isinstance(x, tuple) and x and x[0] == "rec")) for e in log]
    assert strip(got) == strip(want) and len(got) > 13 * 8
    assert ("side0", "wait_stream", "main") in got and not any(e[:2] == ("host", "sync") for e in got)
