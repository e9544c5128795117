"""GraphedTrainStep under adverse stream timing, bit for bit against its own serialisation (tests/step_timing_util.py).

Every schedule - lookahead 1 / 2 / 3, lookahead 2 with the split tail and the pipelined optimizer, lookahead 2 with
stage_ahead=False (the one order in which nothing but main.wait_event(self._done[slot]) puts the pooling behind the conv chain),
trunk pairs waiting and ring, groups of 4 under the ring, ITER_SIZE 2 on the ring - runs twelve steps of the tiny fixture over device-resident batches with each
stream made the laggard in turn; each injection is a case of its own, so a failure names the missing edge:

  side        a delay on every side stream in front of each step: main.wait_event(done) / main.wait_event(self._done[slot])
  main        a delay on the current stream: the side stream's ordering behind the last readers of its slot / staging set
              (wait_stream in the waiting schedules, the host throttle under the ring)
  optimizer   a delay on the optimizer stream (schedules with the pipelined optimizer): the join in front of the next heads
  inflight    the next batch's device tensors hold another batch's contents until a delayed copy on the caller's stream
              delivers the true ones right before step(): the waiting schedules order the side stream behind the caller's
              stream; the ring is handed step(inputs_ready=event)
  reuse       the staged batch's tensors are dropped when step() returns and their sizes claimed again, filled with another
              batch's contents, while the side stream lags: the record_stream calls of _stage_props / _stage_image

Asserted in every case: the losses of every step, the final weights, momentum and bf16 shadow torch.equal to the serialised run;
the losses differ between steps on more than half of the steps; and the PREMISE - none of the delays injected in front of a step
had finished when that step() returned (the dependent work was enqueued while the laggard was busy: an event ordered the two, not
luck).  Part of the premise: the side and optimizer streams do not share the main stream's hardware queue (two streams on one
queue run in submission order and would hide a missing event; step_timing_util.independent probes it, and a draw of pool streams
that fails the probe is replaced).  A case whose premise fails fails, with a message that says so.

What a removed edge does (each tried once on a scratch copy; all are bit mismatches):
  main.wait_event(self._done[s.pool_slot])  laggard side fails at lookahead2_late_staging (elsewhere the proposals' event implies it)
  side.wait_stream(main) in _run_ahead      laggard main and inflight fail at lookahead 2 / 3 / 2_late_staging and pairs_waiting
  self._side.wait_stream(main) in _run      laggard main and inflight fail at lookahead1;  main.wait_event(done): laggard side
  the optimizer join in FusedSGD.step       laggard optimizer fails at every schedule with the pipelined optimizer
  the inputs_ready wait                     inflight fails at the three ring schedules (as it does on the code before
                                            inputs_ready existed: losses differ from step 2 on)
  the record_stream calls                   reuse fails at lookahead2_late_staging

The delay starts at 4 x the measured wall time of one serialised step of the schedule and is doubled, up to the 50-ms cap, until
a run meets the premise at every step.  On the MI355X (serial step / delay used, milliseconds; premise held at all 11 injected
steps of every case):
  lookahead1 0.39 / 1.54   lookahead2 0.36 / 1.46   lookahead3 0.36 / 1.45   lookahead2_split 0.47 / 1.88
  lookahead2_late_staging 0.44 / 1.75   pairs_waiting 0.48 / 1.91   pairs_ring 0.47 / 1.89   group4_ring 0.38 / 1.51
  accum2_pairs_ring 0.36 / 1.45
4 x the serial step sufficed everywhere: no case needed a doubling.  Streams independent of the main one were found at the first
to fifth draw.  (Before FusedSGD.refresh_tables stopped rewriting an unchanged table on every step - a copy from pageable memory,
which holds the host until the stream has drained - the laggard-main and inflight premise failed at all 11 steps of the schedules
with the plain optimizer, at the 50-ms cap too.)
"""
import pytest
import torch

import step_timing_util as T
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
load_package()

PIPELINED = [s for s in T.SCHEDULES if T.SCHEDULES[s]["pipelined"] is not None]
RING = [s for s in T.SCHEDULES if T.wants_ring(s)]
WAITING = [s for s in T.SCHEDULES if not T.wants_ring(s)]


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    load_package().set_precision("fp32")


def _case(schedule, injection, **kw):
    ref = T.serial(schedule)
    res = T.run_with_premise(schedule, injection, **kw)
    what = "%s, laggard %s" % (schedule, injection)
    T.assert_premise(res, what)
    T.assert_equals_serial(res, ref, what)


def test_delay_is_finite_and_calibrated():
    """a 5-ms delay takes 2.5 .. 10 ms by the device's own clock, its event is pending while it runs and done after a sync, and
    nothing above the cap is accepted"""
    main = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    T.calibrate()
    torch.cuda.synchronize()
    e0.record()
    ev = T.delay(main, 5.0)
    pending = not ev.query()
    e1.record()
    torch.cuda.synchronize()
    assert pending and ev.query()
    assert 2.5 <= e0.elapsed_time(e1) <= 10.0, e0.elapsed_time(e1)
    with pytest.raises(AssertionError):
        T.delay(main, T.MAX_DELAY_MS + 1.0)


@pytest.mark.parametrize("schedule", list(T.SCHEDULES))
def test_unsynchronised_run_equals_serial(schedule):
    """no injection: twelve steps enqueued without a host sync against the same steps with a sync after each"""
    T.assert_equals_serial(T.run(schedule), T.serial(schedule), schedule)


@pytest.mark.parametrize("schedule", list(T.SCHEDULES))
def test_laggard_side_stream(schedule):
    _case(schedule, "side")


@pytest.mark.parametrize("schedule", list(T.SCHEDULES))
def test_laggard_main_stream(schedule):
    _case(schedule, "main")


@pytest.mark.parametrize("schedule", PIPELINED)
def test_laggard_optimizer_stream(schedule):
    _case(schedule, "optimizer")


@pytest.mark.parametrize("schedule", WAITING)
def test_inputs_in_flight_waiting_schedules_need_no_event(schedule):
    """plain order on the caller's stream suffices: the side stream waits for that stream at the start of the step"""
    _case(schedule, "inflight", inputs_ready="never")


@pytest.mark.parametrize("schedule", RING)
def test_inputs_in_flight_ring_with_inputs_ready(schedule):
    """the ring's side stream waits for nothing the caller enqueued: step(inputs_ready=) orders it behind the producer"""
    _case(schedule, "inflight", inputs_ready="ring")


@pytest.mark.parametrize("schedule", list(T.SCHEDULES))
def test_allocator_reuse_behind_a_lagging_side_stream(schedule):
    _case(schedule, "reuse")
