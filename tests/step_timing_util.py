"""Delay injection for GraphedTrainStep: run one schedule with one of its streams made the laggard, and compare with the same
schedule serialised.

A training step is spread over the main stream, one or more side streams and the optimizer stream; only events (and, under the
ring, a host throttle) order them.  On the tiny fixture the host is the bottleneck, so every stream has drained before the next
piece is enqueued and a missing edge is never needed.  Here a finite busy kernel (`delay`) holds one stream back while the host
enqueues the step behind it: what the step enqueues on the OTHER streams then really has to wait, and it only does if an event
says so.  All kernels are bit-reproducible, so a schedule is correct if and only if the run equals its own serialisation
(`serial`: a device-wide wait after every step) bit for bit.

  delay(stream, ms)          busy kernel on `stream` (at most MAX_DELAY_MS), returns the event recorded behind it
  run(schedule, injection)   model + optimizer + step object, `steps` steps enqueued without a host sync
  serial(schedule)           the reference: no injection, a sync after every step; also measures the wall time of one step

The batches are DEVICE-resident (images, proposal boxes, objectness; gt_classes stay on the host, where _stage_labels reads them),
so the is_cuda branches of _stage_image / _stage_props run: the ones with the record_stream calls.

Step 0 primes the step object (an eager step, a device-wide wait, the captures): no delay can be outstanding across it, so the
injections start at step 1.  `premise[i]` says for step i + 1 that none of the delays injected in front of it had finished when
step() returned - the dependent work was enqueued while the laggard was busy.  The other half of the premise is independent():
streams that the runtime put on the main stream's hardware queue run in submission order, which orders them without any event;
run() replaces such a draw of pool streams before it injects anything."""
import time

import torch

import golden_util as G
from __graft_entry__ import load_package

MAX_DELAY_MS = 50.0
NAME = "model_r50c4_tiny"
PRECISION = "bf16"  # the mode bench.py runs: the optimizer stream also writes the bf16 shadow the next heads read
# tests/test_model_gpu.py::test_hipgraph_step_equals_eager's sequence (not periodic in 2, 3 or 4), as
# test_ring_schedule_equals_waiting_schedule extends it
PATTERN = [0, 1, 2, 0, 1, 1, 0, 2, 1, 0, 2, 2, 0, 1, 0, 2, 2, 1, 1, 0]

# kw: GraphedTrainStep's arguments; pipelined: FusedSGD.enable_pipelined's (None: the plain optimizer step, captured)
SCHEDULES = {
    "lookahead1": dict(kw=dict(lookahead=1), pipelined=None),
    "lookahead2": dict(kw=dict(lookahead=2), pipelined=None),
    "lookahead3": dict(kw=dict(lookahead=3), pipelined=None),
    "lookahead2_split": dict(kw=dict(lookahead=2, split_tail=True), pipelined={}),
    # stage_ahead=False: proposals are staged on the main stream, so nothing but main.wait_event(self._done[slot]) orders the
    # pooling behind the conv chain (with stage_ahead the wait for the proposals' event, later on the same side stream, implies it)
    "lookahead2_late_staging": dict(kw=dict(lookahead=2, stage_ahead=False), pipelined=None),
    "pairs_waiting": dict(kw=dict(trunk_pairs=True, split_tail=True, eager_fc6=True, ring=False), pipelined={}),
    "pairs_ring": dict(kw=dict(trunk_pairs=True, split_tail=True, eager_fc6=True, ring=True), pipelined={}),
    "group4_ring": dict(kw=dict(trunk_pairs=4, split_tail=True, eager_fc6=True, ring=True), pipelined={}),
    # tests/test_accum_gpu.py::test_graphed_step_accumulates_like_the_eager_loop's "ring_group2", ITER_SIZE 2
    "accum2_pairs_ring": dict(kw=dict(trunk_pairs=True, split_tail=True, ring=True), pipelined=dict(iter_size=2)),
}
INJECTIONS = ("side", "main", "optimizer", "inflight", "reuse")


def wants_ring(schedule):
    kw = SCHEDULES[schedule]["kw"]
    return bool(kw.get("trunk_pairs")) and kw.get("ring", True)


def _ga(schedule):
    """(G, A) of the ahead schedule, None at lookahead 1"""
    kw = SCHEDULES[schedule]["kw"]
    g = kw.get("trunk_pairs", False)
    if g:
        return (2 if g is True else int(g)), 1
    L = kw.get("lookahead", 1)
    return None if L == 1 else (1, L)


def width(schedule):
    """how many batches one step() call takes"""
    from drn_wsod_pytorch_amd.graphed import ahead_arity

    ga = _ga(schedule)
    return 2 if ga is None else 2 + ahead_arity(*ga)


def staged_images(schedule, i):
    """positions of the batches whose IMAGES step i reads (on a side stream): the next batch at lookahead 1, else the group whose
    conv chain the step launches"""
    from drn_wsod_pytorch_amd.graphed import ahead_arity, ahead_schedule

    ga = _ga(schedule)
    if ga is None:
        return [i + 1]
    s = ahead_schedule(i, ga[0], ga[1], 2)  # (which batches, and whether a chain starts, do not depend on the slot count)
    if i % ga[0]:
        return []
    return [i + 2 + k for k in range(*s.stage.indices(ahead_arity(*ga)))]


# ---- the delay kernel ---------------------------------------------------------------------------------------------------------------
_cycles_per_ms = None


def _timed_sleep(cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(int(cycles))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate():
    """cycles of torch.cuda._sleep per millisecond, measured once with events.  The count is raised from a small one until the
    kernel takes 2 ms, so nothing longer than 4 ms is ever issued to find it out"""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda.synchronize()
        _timed_sleep(1000)  # (the first launch loads the kernel)
        n, t = 10000, 0.0
        while True:
            t = min(_timed_sleep(n) for _ in range(3))
            if t >= 2.0:
                break
            n *= 2
            assert n < 1 << 40, "torch.cuda._sleep does not get longer with its argument"
        half = min(_timed_sleep(n // 2) for _ in range(3))
        _cycles_per_ms = (n - n // 2) / max(t - half, 1e-3)  # (the difference: launch overhead drops out)
        got = _timed_sleep(10.0 * _cycles_per_ms)
        assert 5.0 <= got <= 20.0, "a 10-ms delay measured %.2f ms: the calibration is off" % got
    return _cycles_per_ms


def independent(stream, main, ms=2.0):
    """does work on `stream` run while `main` is busy?  The runtime multiplexes streams onto a few hardware queues, and two streams
    that share one run in the order of submission - an ordering no event asked for, which would hide a missing one.  A delay on
    `main`, a minimal kernel on `stream`: independent if that kernel is done while the delay is still running"""
    torch.cuda.synchronize()
    ev = delay(main, ms)
    mark = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100)
        mark.record(stream)
    mark.synchronize()  # (at the worst behind the delay: finite)
    free = not ev.query()
    torch.cuda.synchronize()
    return free


def delay(stream, ms):
    """enqueue a busy kernel of `ms` milliseconds (at most MAX_DELAY_MS: finite, far from anything like a hang) on `stream`;
    -> the event recorded behind it"""
    assert 0.0 < ms <= MAX_DELAY_MS, ms
    cycles = int(ms * calibrate())
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev.record(stream)
    return ev


# ---- device-resident batches --------------------------------------------------------------------------------------------------------
_KEYS = ("image", "proposal_boxes", "objectness_logits")
_lib = None


def library():
    """(the three host batches b0, b1, b2 of test_hipgraph_step_equals_eager, their device tensors).  The device copies are the
    source of every true content and of every decoy; nothing writes them"""
    global _lib
    if _lib is None:
        d = G.load(NAME)
        ocfg = G.MODEL_CASES[NAME]
        base = G.batch_from(d)
        alt = dict(base[0])
        alt["image"] = (255.0 - base[0]["image"]).contiguous()
        alt["objectness_logits"] = base[0]["objectness_logits"].flip(0).contiguous()
        alt2 = dict(base[0])
        alt2["image"] = base[0]["image"].flip(2).contiguous()
        alt2["proposal_boxes"] = base[0]["proposal_boxes"].flip(0).contiguous()
        alt2["gt_classes"] = (base[0]["gt_classes"] + 1) % ocfg.num_classes
        raws = [dict(base[0]), alt, alt2]
        dev = [{k: r[k].float().contiguous().cuda() for k in _KEYS} for r in raws]
        torch.cuda.synchronize()
        for a in range(3):
            for b in range(a):  # a decoy must be WRONG data: every pair differs in what the step reads
                assert any(not torch.equal(dev[a][k], dev[b][k]) for k in _KEYS)
        _lib = (raws, dev)
    return _lib


def decoy_of(k):
    """whose contents stand in for batch k's before the true ones arrive: another batch's, valid and of the same shape, so a
    lost race reads wrong data and no kernel is sent out of range"""
    return (k + 1) % 3


def device_batch(labels, content):
    """one batch with the host labels of b<labels> and fresh device tensors holding the contents of b<content>"""
    raws, dev = library()
    b = {k: dev[content][k].clone() for k in _KEYS}
    b["gt_classes"] = raws[labels]["gt_classes"]
    b["gt_boxes"] = raws[labels]["gt_boxes"]
    return G.drn_inputs([b])


def _fill(batch, k, props=False, image=False):
    """copy b<k>'s true contents into the batch's device tensors, on the current stream (device to device: the host goes on)"""
    dev = library()[1][k]
    x = batch[0]
    if props:
        x["proposals"].proposal_boxes.tensor.copy_(dev["proposal_boxes"], non_blocking=True)
        x["proposals"].objectness_logits.copy_(dev["objectness_logits"], non_blocking=True)
    if image:
        x["image"].copy_(dev["image"], non_blocking=True)


# ---- one run ------------------------------------------------------------------------------------------------------------------------
def build(schedule, first_batch):
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer

    spec = SCHEDULES[schedule]
    d = G.load(NAME)
    cfg, model = G.drn_model(G.MODEL_CASES[NAME], int(d["seed"]), "cuda", 5, PRECISION)
    model.roi_heads.box_head.dropout_p = 0.0
    model.train()
    opt = build_optimizer(cfg, model)
    if spec["pipelined"] is not None:
        opt.enable_pipelined(None, **spec["pipelined"])
    return model, opt, GraphedTrainStep(model, opt, first_batch, **spec["kw"])


REUSE_CLAIMS = 8


def named_streams(stepper, opt):
    """every stream of the step but the main one (after priming)"""
    out = [("side%d" % k, s) for k, s in enumerate(getattr(stepper, "_sides", None) or [stepper._side])]
    if getattr(opt, "_opt_stream", None) is not None and getattr(opt, "_pipelined", False):
        out.append(("optimizer", opt._opt_stream))
    return out


def lagging_streams(stepper, opt, injection):
    if injection == "main":
        return [torch.cuda.current_stream()]
    if injection in ("side", "reuse"):
        return list(getattr(stepper, "_sides", None) or [stepper._side])
    if injection == "optimizer":
        out = [opt._opt_stream]
        comm = getattr(stepper, "_comm", None)
        return out + ([comm] if comm is not None else [])
    return []


class _Aliased(Exception):
    pass


MAX_ATTEMPTS = 16


def run(schedule, injection=None, steps=12, delay_ms=None, sync_each=False, inputs_ready="ring"):
    """_run_once() on streams that are independent of the main stream (independent()): the step object and the optimizer draw
    theirs from torch's pool, so a draw that shares the main stream's hardware queue is thrown away (with a varying number of pool
    streams, so that the next draw lands elsewhere) and the run built again; after MAX_ATTEMPTS the result says so
    (res["aliased"]) and assert_premise fails"""
    burnt = []
    for attempt in range(MAX_ATTEMPTS):
        try:
            res = _run_once(schedule, injection, steps, delay_ms, sync_each, inputs_ready, attempt == MAX_ATTEMPTS - 1)
            res["draws"] = attempt + 1
            return res
        except _Aliased:
            burnt.append([torch.cuda.Stream() for _ in range(attempt + 1)])


def _run_once(schedule, injection, steps, delay_ms, sync_each, inputs_ready, last_attempt):
    """`steps` steps of `schedule` over the non-periodic sequence, enqueued without a host sync (sync_each: the serialisation).
    injection, applied in front of every step from step 1 on:
      "side" / "main" / "optimizer"  a delay on every side stream / the current stream / the optimizer stream
      "inflight"   the device tensors this step is the first to be handed hold a decoy; a delay and then the copies of the true
                   contents are enqueued on the caller's stream right before step().  inputs_ready: "ring" = under the ring an
                   event recorded behind those copies is passed as step(inputs_ready=); "never" = no event for any schedule
      "reuse"      a delay on every side stream; after step() returns, the tensors of the batch it staged are dropped and tensors
                   of the same sizes, filled with the decoy, are allocated on the main stream at once
    -> dict(losses [steps, n] / weights / momentum / shadow (host copies), premise, wall (seconds per step), ring_on, delay_ms)"""
    assert injection is None or injection in INJECTIONS
    assert not (sync_each and injection)
    w = width(schedule)
    truth = [PATTERN[p % len(PATTERN)] for p in range(steps + w)]
    inflight = injection == "inflight"
    seq = [device_batch(k, decoy_of(k) if inflight else k) for k in truth]
    if inflight:  # what priming reads is complete before the first call
        for p in range(w):
            _fill(seq[p], truth[p], props=p < 2, image=True)
    torch.cuda.synchronize()
    model, opt, stepper = build(schedule, seq[0])
    eng = model.roi_heads._engine
    main = torch.cuda.current_stream()
    out, premise, wall, keep, aliased = [], [], [], [], []
    try:
        for i in range(steps):
            evs, kw = [], {}
            t0 = time.perf_counter()
            if i and injection:
                evs = [delay(s, delay_ms) for s in lagging_streams(stepper, opt, injection)]
                if inflight:
                    evs.append(delay(main, delay_ms))
                    _fill(seq[i + 1], truth[i + 1], props=True, image=w == 2)
                    if w > 2:
                        _fill(seq[i + w - 1], truth[i + w - 1], image=True)
                    if inputs_ready == "ring" and stepper._ring_on:
                        kw["inputs_ready"] = torch.cuda.Event()
                        kw["inputs_ready"].record(main)
            losses = stepper.step(*seq[i: i + w], **kw)
            if evs:
                premise.append(all(not ev.query() for ev in evs))
            out.append(torch.stack([losses[k].detach().clone().reshape(()).float() for k in sorted(losses)]))  # (a device copy: no sync)
            if i == 0 and injection:
                aliased = [n for n, s in named_streams(stepper, opt) if not independent(s, main)]
                if aliased and not last_attempt:
                    raise _Aliased()
            if i and injection == "reuse":
                # what step i read of the caller's tensors - the proposals of batch i + 1, the images it staged - is enqueued on a
                # lagging side stream and is read by no later step: free it and claim the same sizes again, several times over
                # (whichever block the allocator hands out first), with wrong data in them.  The main stream waits for the
                # proposals' copy before it pools, so only the images' reads can really lose here (lookahead >= 2, groups)
                drop = [(seq[i + 1][0], "proposals", ("proposal_boxes", "objectness_logits"), truth[i + 1])]
                drop += [(seq[p][0], "image", ("image",), truth[p]) for p in staged_images(schedule, i)]
                for x, field, keys, k in drop:
                    x[field] = None
                    dec = library()[1][decoy_of(k)]
                    keep.append([dec[key].clone() for key in keys for _ in range(REUSE_CLAIMS)])
            if sync_each:
                torch.cuda.synchronize()
                wall.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        res = dict(losses=torch.stack(out).cpu(), weights=eng.arena_w.detach().cpu().clone(),
                   momentum=None if opt._mom is None else opt._mom.detach().cpu().clone(),
                   shadow=None if eng.arena_s is None else eng.arena_s.detach().cpu().clone(),
                   premise=premise, wall=wall, ring_on=bool(stepper._ring_on), delay_ms=delay_ms, aliased=aliased)
    finally:
        torch.cuda.synchronize()
        stepper.release()
        load_package().set_precision("fp32")
    assert res["ring_on"] == wants_ring(schedule), (schedule, res["ring_on"])
    return res


_serial, DELAYS = {}, {}


def serial(schedule, steps=12):
    """the reference of `schedule`: the same run with torch.cuda.synchronize() after every step and no injection (computed once)"""
    if (schedule, steps) not in _serial:
        _serial[schedule, steps] = run(schedule, None, steps, sync_each=True)
    return _serial[schedule, steps]


def step_ms(schedule):
    """measured wall time of one serialised, replayed step of the schedule (the median; step 0 primes and is left out)"""
    wall = sorted(serial(schedule)["wall"][1:])
    return 1e3 * wall[len(wall) // 2]


def run_with_premise(schedule, injection, **kw):
    """run() at the schedule's delay length: 4 x the measured serial step to start with, doubled (up to MAX_DELAY_MS) while a run
    does not meet the premise at every step - such a run is a dry run and is thrown away.  The length found stays with the
    schedule (DELAYS); it is printed"""
    ms = DELAYS.get(schedule) or min(MAX_DELAY_MS, 4.0 * step_ms(schedule))
    while True:
        res = run(schedule, injection, delay_ms=ms, **kw)
        if all(res["premise"]) or ms >= MAX_DELAY_MS:
            break
        ms = min(MAX_DELAY_MS, 2.0 * ms)
    DELAYS[schedule] = ms
    print("%s / %s: serial step %.2f ms, delay %.2f ms, premise held at %d of %d steps, streams independent of main at draw %d"
          % (schedule, injection, step_ms(schedule), ms, sum(res["premise"]), len(res["premise"]), res["draws"]))
    return res


def assert_equals_serial(res, ref, what):
    """losses at every step, final weights, momentum and bf16 shadow, bit for bit"""
    assert torch.isfinite(ref["losses"]).all(), what
    steps = ref["losses"].shape[0]
    # the sequence really changes the losses from step to step: otherwise a stale slot would show nothing
    assert len({tuple(r.tolist()) for r in ref["losses"]}) > steps // 2, what
    bad = [i for i in range(steps) if not torch.equal(res["losses"][i], ref["losses"][i])]
    assert not bad, "%s: losses differ from the serialised run at steps %s" % (what, bad)
    for k in ("weights", "momentum", "shadow"):
        assert (res[k] is None) == (ref[k] is None), (what, k)
        if ref[k] is not None:
            assert torch.equal(res[k], ref[k]), "%s: %s differs from the serialised run" % (what, k)


def assert_premise(res, what):
    assert not res["aliased"], ("%s: the premise does not hold - %s shared the main stream's hardware queue in every one of %d draws, "
                                "so submission order, not an event, may have ordered them" % (what, res["aliased"], MAX_ATTEMPTS))
    late = [i + 1 for i, ok in enumerate(res["premise"]) if not ok]
    assert res["premise"] and not late, (
        "%s: the premise does not hold - at steps %s a %.1f-ms delay had already finished when step() returned, so nothing shows "
        "that an event ordered the streams there" % (what, late, res["delay_ms"]))
