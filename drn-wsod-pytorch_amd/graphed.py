"""The training step as replayed hipGraphs (what sits around the hot path in projects/WSL/tools/train_net.py:65-117).

  GraphedTrainStep   frozen trunk (FREEZE_AT = 5, every shipped config): heads graph on the main stream, the conv chain of FUTURE
                     batches on a side stream, pooling piece + fc6 forward + fc6 weight-gradient tail issued eagerly around it
                     (bench.py's step)
  GraphedFullStep    trainable trunk: forward, losses, backward, optimizer as one graph (two with a gradient exchange between)
Both stage their inputs into the static buffers of _StaticInputs.  ahead_schedule() is the slot arithmetic of the frozen-trunk
step: no torch in it, tests/test_schedule_cpu.py simulates it.

Split out of engine.py in round 5; `engine` re-exports both names."""

import weakref
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist

from . import ops
from ._cabi import DrnError


class Ahead(NamedTuple):
    """what step t of the ahead schedule touches (ahead_schedule)"""
    launch: Optional[int]  # trunk slot the conv chain launched at this step writes; None: no chain starts at this step
    stage: slice           # the batches of that chain, as a slice of step()'s `upcoming` (upcoming[0] is batch t+2)
    pool_slot: int         # the pooling at the end of the step (batch t+1) reads this trunk slot ...
    pool_part: int         # ... and this batch of the slot's group
    nb: int                # staging set the step stages batch t+1 into, and its pooling reads


def ahead_arity(G, A):
    """how many batches step() takes after next_batch: up to the last one of the group launched A groups ahead (it depends on
    neither t nor P, and step() checks it before P is settled)"""
    return A * G + G - 2


def ahead_schedule(t, G, A, P, sets=1):
    """The side-stream schedule of GraphedTrainStep at step t: one conv chain per group of G consecutive batches, launched A groups
    ahead (on the steps with t % G == 0), group q living in trunk slot q % P; `sets` staging sets for proposals / labels (A G >= 2).
      lookahead=L    is (G, A, P) = (1, L, L);
      trunk_pairs=G  is (G, 1, 2), and (G, 1, RING_SLOTS) with RING_SETS staging sets under the ring.
    The chain launched at step t is that of group t // G + A = batches t + A G .. t + A G + G - 1; the pooling at the end of step t
    is that of batch t + 1, part (t + 1) % G of group (t + 1) // G."""
    lo = A * G - 2
    return Ahead((t // G + A) % P if t % G == 0 else None, slice(lo, lo + G), ((t + 1) // G) % P, (t + 1) % G, (t + 1) % sets)


def _captured(body, *args):
    """-> (hipGraph of body(*args), what body returned).  thread_local: with N > 1 the RCCL watchdog thread polls its events while
    we capture; only this thread's calls belong to the capture"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out = body(*args)
    return g, out


class _StaticInputs:
    """What both graphed steps share: the static device buffers a captured graph reads its inputs from (proposals, objectness,
    image-level labels, images) and the staging of labels and images into them."""

    def __init__(self, model, optimizer, example_batch):
        if getattr(model, "cpg", False):
            raise DrnError("CSCROIHeads decides per step, on the host, which class maps to compute: eager steps only")
        self.model, self.opt = model, optimizer
        self.heads = model.roi_heads
        self.engine = self.heads._engine
        dev = model.device
        K = self.heads.num_classes
        self.nper = [len(x["proposals"]) for x in example_batch]
        n_img, M = len(example_batch), sum(self.nper)
        self.n_img, self.K = n_img, K
        self.image = [x["image"].to(dev).float().clone() for x in example_batch]
        self._images = [self.image]  # image sets by trunk slot (the ahead schedule of GraphedTrainStep allocates its own)
        self._off = [0]
        for n in self.nper:
            self._off.append(self._off[-1] + n)
        self.rois = self._new_rois()
        self.obj = torch.zeros((M,), dtype=torch.float32, device=dev)
        self.props = torch.zeros((M, 4), dtype=torch.float32, device=dev)
        self._layout_labels()
        self.img_off = torch.tensor(self._off, dtype=torch.int32, device=dev)
        self.losses = None
        self.engine.pool_sets_pinned = None  # a new step captures anew: the previous owner's pin (if any) is void
        self.engine.pool_sets_pin_owner = None
        self.engine.captured_by = None  # weakref to the step whose captured graphs hold the engine's launch sequence

    def _annot_max_gt(self):
        """annotated boxes per image in the label buffer: max_gt of the metrics ring's annotated-box block and / or the capacity
        of a regressing PCL head (ONE block; ROIHeads._annot_capacity), 0 without either"""
        cap = getattr(self.heads, "_annot_capacity", None)
        if cap is not None:
            return cap()
        m = self.engine.metrics
        return m.max_gt if m is not None and m.annotated else 0

    def _annot_setter(self):
        f = getattr(self.heads, "_annot_setter", None)
        return (f(),) if f is not None else ()

    def _layout_labels(self):
        """image-level labels live in ONE device block (one H2D copy per step): [onehot f32 | classes i32 | count i32], and - only
        with the metrics ring's annotated-box block (ROIHeads.enable_metrics(annotated=True)) - behind them the annotated boxes
        [boxes f32 | classes i32 | count i32] (roi_heads.pack_annotated).  Settled before the step is primed."""
        from .modeling.roi_heads import annotated_views, annotated_words

        n_img, K = self.n_img, self.K
        self._ann_gt = self._annot_max_gt()
        nk = n_img * K
        self._gt_words = 2 * nk + n_img
        extra = annotated_words(n_img, self._ann_gt) if self._ann_gt else 0
        self._gt_block = torch.zeros((self._gt_words + extra,), dtype=torch.int32, device=self.model.device)
        self.gt = dict(onehot=self._gt_block[:nk].view(torch.float32).view(n_img, K),
                       classes=self._gt_block[nk: 2 * nk].view(n_img, K), count=self._gt_block[2 * nk: self._gt_words],
                       props=self.props, max_rows=max(self.nper), rows=list(self.nper))
        if self._ann_gt:
            self.gt.update(annotated_views(self._gt_block[self._gt_words:], n_img, self._ann_gt))
        if hasattr(self, "_gt_nb"):
            self._gt_nb = [torch.zeros_like(self._gt_block) for _ in self._gt_nb]
        if hasattr(self, "_ring"):
            del self._ring

    def _check_label_layout(self):
        """the annotated-box option may be switched until the step is primed (enable_metrics() is refused afterwards): the block is
        laid out anew while nothing was captured; a captured step keeps the layout its graphs read"""
        if self._annot_max_gt() != self._ann_gt:
            own = self.engine.captured_by
            if own is None or own() is not self:
                self._layout_labels()

    @property
    def metrics(self):
        """the head engine's MetricsRing (ROIHeads.enable_metrics(), BEFORE this step is primed: the two launches are captured
        with the heads like any other), or None"""
        return self.engine.metrics

    def _anchor_metrics(self, start_iter):
        """the ring counts records; the next one is iteration start_iter (one small D2H read, at construction)"""
        if self.metrics is not None:
            self.metrics.iter0 = int(start_iter) - int(self.metrics.state[0])

    def _mark_captured(self):
        self.engine.captured_by = weakref.ref(self)
        self._metrics_keep = self.metrics  # the captured launches write into its buffers: they live as long as the graphs

    def _new_rois(self):
        """[M, 5] rows (image index, box): the index column is written once, here"""
        t = torch.zeros((self._off[-1], 5), dtype=torch.float32, device=self.model.device)
        for i in range(self.n_img):
            t[self._off[i]: self._off[i + 1], 0] = float(i)
        return t

    def _stage_labels(self, batch, dst=None):
        """Image-level labels of the CURRENT batch.  They are built on the host and go through a ring of PINNED
        staging buffers so the H2D copies are truly asynchronous - a pageable source would block the host until the
        previous replay has drained and leave the GPU idle between replays."""
        self._check_label_layout()
        ints = [torch.unique(x["instances"].gt_classes.cpu(), sorted=True) for x in batch]
        nk = self.n_img * self.K
        if not hasattr(self, "_ring"):
            self._ring = [dict(buf=torch.zeros_like(self._gt_block, device="cpu").pin_memory(), ev=None) for _ in range(8)]
            self._ring_i = 0
        slot = self._ring[self._ring_i]
        self._ring_i = (self._ring_i + 1) % len(self._ring)
        if slot["ev"] is not None:
            slot["ev"].synchronize()  # only blocks when the host is a full ring ahead of the GPU
        buf = slot["buf"]
        buf.zero_()
        oh = buf[:nk].view(torch.float32).view(self.n_img, self.K)
        cl = buf[nk: 2 * nk].view(self.n_img, self.K)
        for i, g in enumerate(ints):
            oh[i, g] = 1
            cl[i, : len(g)] = g.to(torch.int32)
            buf[2 * nk + i] = len(g)
        if self._ann_gt:  # the annotated boxes ride in the same pinned buffer and the same copy
            from .modeling.roi_heads import pack_annotated

            buf[self._gt_words:].copy_(pack_annotated([x["instances"] for x in batch], self._ann_gt, *self._annot_setter()))
        (self._gt_block if dst is None else dst).copy_(buf, non_blocking=True)
        slot["ev"] = torch.cuda.Event()
        slot["ev"].record()

    def _stage_image(self, items, slot):
        """images of `items` (one batch, or the batches of a group end to end) -> the image set of a trunk slot"""
        for i, x in enumerate(items):
            self._images[slot][i].copy_(x["image"], non_blocking=True)
            if x["image"].is_cuda:  # (a device mapper's image lives in another stream's pool: DatasetMapper.finish)
                x["image"].record_stream(torch.cuda.current_stream())

    @property
    def last_state(self):
        """intermediate values (MIL scores, image scores, pseudo-GT rows, labels) of the step that ran last"""
        return self._captured_state if getattr(self, "_replayed", False) else self._eager_state

    def _keep_state(self, st):
        # static buffers: after a replay the CAPTURED state holds that step's MIL scores / pseudo-GT / labels; the priming
        # step ran eagerly (its state is the one built before the capture)
        if torch.cuda.is_current_stream_capturing():
            self._captured_state = st
        else:
            self._eager_state = st


class GraphedTrainStep(_StaticInputs):
    """One training step as hipGraphs captured once and replayed: a step is ~100 kernel launches of 2-450 us, so
    the eager Python host needs ~2.4 ms to enqueue what the GPU executes in ~2.1 ms; a replay costs the host ~9 us per
    node and nothing else.

      g_main (main stream) : heads forward (fc6 GEMM first, on the pooled operand prepared by the PREVIOUS step), MIL /
                             OICR losses, explicit backward up to the fc6 weight gradient
      tail   (eager)       : fc6 dW row-slab GEMMs on the main stream; per bucket, (all-reduce +) SGD on the optimizer
                             stream (`split_tail`, the default of bench.py; with split_tail=False the tail is part of
                             g_main - measured 1.3 % slower, the executor schedules forked branches late)
      trunk  (side stream) : preprocess + frozen backbone of FUTURE batches (latency-bound convs under the GEMMs), one graph per slot
      pool   (main stream) : ROIPool(+objectness) -> A and A^T of the next batch, behind this step's last reader of A^T
    Legal because every shipped config freezes the whole backbone (FREEZE_AT=5).

    Two schedules.  lookahead=1 (_run): g_bb runs the trunk of the NEXT batch into feat_next during the step and the captured g_pool
    pools it; one buffer set suffices.  Everything else is the AHEAD schedule (_run_ahead) at parameters (G, A, P) - one conv chain
    per group of G batches, launched A groups ahead into one of P trunk slots (g_pbb: one graph per slot); ahead_schedule() is its
    whole index arithmetic, and tests/test_schedule_cpu.py shows by simulation that no slot or staging set is overwritten before
    its last reader ran:
      lookahead=L >= 2  (1, L, L) on L-1 alternating side streams: measured with HIP events, the conv chain of ONE image takes
                        ~1.7 ms beside the GEMMs (0.6 ms alone) and the main stream idled 0.26 ms per step waiting for it; with the
                        trunk of batch t+L running during step t the pooling of batch t+1 never waits, L-1 chains are in flight at
                        once and each may take L-1 steps.  step(batch, next_batch, batches t+2 .. t+L): only their images are read.
      trunk_pairs=G     (G, 1, 2) on one side stream (True = 2): the chain is latency-bound, so G images cost what one costs and the
                        per-image chain time shrinks G-fold - for trunks whose chain is as long as the step or longer (WS-R101: ~100
                        launches, 0.7 ms of every 1.5-ms step spent waiting for it).  step() takes batches t .. t+2G-1.
      the RING          (G, 1, RING_SLOTS) with RING_SETS staging sets (round 6; trunk groups on one GPU with the split tail and the
                        pipelined optimizer's hook, ring=True): the side stream does NOT wait for the main stream at all - any such
                        wait, even on an event that completed two steps ago, costs ~1 % of the step
                        (profiles/r6_40_side_wait_experiments.txt).  What the wait guaranteed - the previous reader of a set / slot
                        is done before the side stream overwrites it - the HOST guarantees instead: before it enqueues step t it
                        waits (a no-op in steady state: it runs ~1 step ahead) for the event the optimizer stream already waits on,
                        recorded behind the heads of step t - RING_LAG.
    The pooling piece of the ahead schedule - one staging launch + the pooling kernel - is issued eagerly: a graph's hand-over to the
    next launch costs more than an eager launch gap (+0.65 %, profiles/r2_39_eager_pool_ab.txt).

    Static shapes only (fixed image size, proposals per image, images per GPU: the benchmark's case and the common
    fixed-R training case); anything else runs the eager path.

    N > 1 (`split_tail`): the captured heads graph stops in front of the fc6 weight-gradient GEMMs.  That tail - the
    announcement of the small gradients, the dW row-slab GEMMs and, from the optimizer's hooks, one RCCL all-reduce +
    SGD launch per bucket on the optimizer stream - is issued eagerly after the replay (~10 launches), so no
    collective is ever captured into a hipGraph, while the next image's backbone graph and pooling graph run under
    the exchange.  The optimizer stream is joined at the start of the next step."""

    RING_LAG, RING_SETS, RING_SLOTS = 3, 4, 3

    def __init__(self, model, optimizer, example_batch, split_tail=False, lookahead=1, trunk_pairs=False,
                 eager_fc6=False, stage_ahead=True, ring=True, start_iter=0):
        super().__init__(model, optimizer, example_batch)
        if any(p.requires_grad for p in model.backbone.parameters()):
            raise DrnError("GraphedTrainStep runs the trunk of FUTURE batches on a side stream, which needs a frozen "
                           "backbone (FREEZE_AT = 5); use GraphedFullStep for a trainable trunk")
        assert 1 <= lookahead <= 4
        self.lookahead = lookahead
        # eager_fc6 (bench.py): the fc6 forward GEMM - first launch of the heads and the step's dominant kernel - is
        # issued eagerly in front of the captured heads graph, like the fc6 dW tail behind it, so HIP events on the
        # launch stream can bracket it inside the timed region (ops.GEMM_TIMING)
        self.eager_fc6 = bool(eager_fc6)
        # stage_ahead: the next batch's labels are staged behind this step's heads graph and its proposals on the side
        # stream (False = the round-2 order, kept for A/B runs: proposals in front of the pooling graph on the main
        # stream, labels at the start of their own step, i.e. between the pooling kernel and the fc6 forward)
        self.stage_ahead = bool(stage_ahead)
        self.trunk_pairs = bool(trunk_pairs)
        self.G = (2 if trunk_pairs is True else int(trunk_pairs)) if trunk_pairs else 0
        if self.trunk_pairs and self.G < 2:
            raise DrnError("trunk_pairs: True (two batches per conv chain) or an int >= 2")
        # (G, A) of the ahead schedule; None: lookahead=1.  P and the ring are settled at priming (_prime_ahead)
        self._GA = (self.G, 1) if self.trunk_pairs else (1, lookahead) if lookahead >= 2 else None
        self._t = 0
        # Proposals / objectness / labels of the NEXT batch are staged on the side stream (the labels by an H2D copy) and read by
        # the pooling piece at the end of the step, which hands boxes and labels on to the buffers the heads graph reads - a node
        # inside a graph / one launch instead of eager copies with launch gaps on the main stream.  One set, RING_SETS under the ring
        self._rois_nb = [self._new_rois() for _ in range(self.RING_SETS)]
        self._obj_nb = [torch.zeros_like(self.obj) for _ in range(self.RING_SETS)]
        self._gt_nb = [torch.zeros_like(self._gt_block) for _ in range(self.RING_SETS)]
        self._ring_want = bool(ring)  # (False: the side stream waits for the main stream at the start of every step, as before round 6)
        self._ring_on = False  # (set by _prime_ahead)
        self._nb = 0          # the staging set in use (0 for every schedule but the ring)
        self._ring_evs = []   # events behind the heads of the last steps (oldest first)
        self._side = torch.cuda.Stream()
        self._primed = False
        self.split_tail = bool(split_tail)
        # WSL.ITER_SIZE = N > 1 (the pipelined optimizer's iter_size): the captured heads graph back-propagates loss / N with
        # the small tensors' accumulate flags on, and is the same for every micro-iteration; what differs by window position -
        # where the fc6 weight gradient goes, whether the optimizer stream gets work, whether the step ends with opt.step() -
        # is the eager tail, so the tail is always split off.  Micro-iterations count from start_iter (a resumed run).
        self.iter_size = int(getattr(optimizer, "iter_size", 1))
        self._iter = int(start_iter)
        self._start_iter = int(start_iter)
        if self.iter_size > 1:
            if not getattr(optimizer, "_pipelined", False):
                raise DrnError("GraphedTrainStep with WSL.ITER_SIZE > 1 needs FusedSGD.enable_pipelined(iter_size=N)")
            self.split_tail = True
        if self.engine.kshard is not None and not (self.split_tail and self.eager_fc6 and (lookahead >= 2 or trunk_pairs)):
            raise DrnError("K-sharded fc6 holds collectives in the pooling piece, behind the fc6 GEMM and in the dW tail: "
                           "GraphedTrainStep(split_tail=True, eager_fc6=True, lookahead >= 2 or trunk_pairs)")
        self.engine.defer_fc1_tail = self.split_tail
        # the anomaly guard (FusedSGD(nonfinite=...)): its check and the guard pointer of every update are captured with the
        # heads graph.  ITER_SIZE 1: every step opens its window.  N > 1: ONE captured graph serves every position of the window,
        # so the position cannot be a captured argument - the host opens the window instead (LossGuard.open_window)
        self._guard = getattr(optimizer, "_guard", None)
        if self._guard is not None:
            self._guard.window_first = self.iter_size == 1
            self._guard.iter0 = self._start_iter - self._guard.read()["calls"]
        self._anchor_metrics(self._start_iter)

    def release(self):
        """give the fc6 operand sets back (they may grow again); the captured graphs of this object must not be replayed
        afterwards"""
        own = self.engine.pool_sets_pin_owner
        if own is not None and own() is self:
            self.engine.pool_sets_pinned = None
            self.engine.pool_sets_pin_owner = None
        own = self.engine.captured_by
        if own is not None and own() is self:
            self.engine.captured_by = None
        self._primed = False

    # ---- host side of one step: stage inputs into the static buffers (tiny async copies) -----------------------
    @property
    def rois_next(self):
        return self._rois_nb[self._nb]

    @property
    def obj_next(self):
        return self._obj_nb[self._nb]

    @property
    def _gt_stage(self):
        return self._gt_nb[self._nb]

    def _stage_labels_ahead(self, next_batch, via_stage=False):
        """Labels of the NEXT batch, issued during this step instead of at the start of their own (where a 4-us H2D copy
        and its two launch gaps sat between the pooling kernel and the fc6 forward).  via_stage (the ahead schedule,
        called on the side stream next to the proposals): into `_gt_stage`, from where the pooling piece - which runs
        behind this step's heads graph, the label block's reader - copies them into the block; otherwise straight into
        the block on the current stream, behind the heads graph.  step() skips its own staging when it is handed this
        very batch."""
        if next_batch is not None and self.stage_ahead:
            self._stage_labels(next_batch, self._gt_stage if via_stage else None)
            self._labels_for = next_batch

    def _stage_labels_now(self, batch):
        if getattr(self, "_labels_for", None) is not batch:
            self._stage_labels(batch)
        self._labels_for = None

    def _stage_next(self, batch):
        """image + proposals of the NEXT batch (device tensors: async D2D copies)"""
        self._stage_props(batch)
        self._stage_image(batch, 0)

    def _stage_props(self, batch):
        off = 0
        for i, x in enumerate(batch):
            n = self.nper[i]
            assert len(x["proposals"]) == n, "graphed step: proposals per image must stay fixed"
            bx, ob = x["proposals"].proposal_boxes.tensor, x["proposals"].objectness_logits
            self.rois_next[off: off + n, 1:].copy_(bx, non_blocking=True)
            self.obj_next[off: off + n].copy_(ob, non_blocking=True)
            for src in (bx, ob):
                if src.is_cuda:  # the caller's tensors may be read on a side stream: keep the allocator from reusing them
                    src.record_stream(torch.cuda.current_stream())
            off += n

    # ---- the pieces of a trunk slot (lookahead=1: slot 0 = the staged image set and feat_next) ------------------------------------
    def _backbone(self, slot=0):
        m = self.model
        imgs = m.preprocess_image([{"image": im} for im in self._images[slot]])
        feats = m.backbone(imgs.tensor)
        f = feats[self.heads.box_in_features[0]].permute(0, 2, 3, 1)
        assert f.is_contiguous()
        return f

    def _bb_body(self, slot=0):
        with torch.no_grad():
            self._feats[slot].copy_(self._backbone(slot))

    def _pool_body(self, slot=0, part=0):
        """pooled fc6 operand (A, A^T) of the staged next batch - batch `part` of the slot's group - + hand its proposals over to
        the heads"""
        n = self.n_img
        feat = self._feats[slot][part * n: (part + 1) * n]
        via = self._GA is not None and self.stage_ahead
        with torch.no_grad():
            # the heads only need the pooled operand and the proposal boxes (pseudo-GT mining / IoU labelling) of a batch; the
            # small copy goes IN FRONT of the pooling kernel (its last reader, the previous heads graph, is long done) so that
            # nothing sits between the pooling and the fc6 forward
            # one launch: proposal boxes -> props, and (via: the ahead schedule) the next batch's labels, staged on the side stream
            # (_stage_labels_ahead), -> the label block
            ops.stage_heads_inputs(self.rois_next, self.props, self._gt_stage if via else None, self._gt_block if via else None)
            if self.engine.kshard is not None:  # K-sharded fc6: this rank's channel slice of every rank's image (collectives, eager)
                self.pooled = self.engine.pool_kshard(feat, self.rois_next, self.obj_next)
                return
            self.pooled = self.engine.pool(feat, self.rois_next, self.obj_next, True, slot=0)
            self._check_pooled()

    def _check_pooled(self):
        """The captured heads graph reads the fc6 operand pair (A, A^T) at the addresses it saw when it was captured; the
        pooling piece is issued eagerly (eager_pool) and asks the head engine for its buffers on every step.  Once primed,
        the two must agree - a re-allocation in between (an inference pass used to replace the sets) would
        make the replayed graph read freed memory without any error."""
        ptrs = (self.pooled["A"].data_ptr(), self.pooled["AT"].data_ptr())
        if not getattr(self, "_primed", False):
            self._pool_ptrs = ptrs
            self.engine.pool_sets_pinned = (self.pooled["A"].dtype, True)
            # the pin belongs to THIS step object: it lapses when the object dies or another step is built on the model
            # (it used to outlive its owner and made the re-creation the error message asks for fail)
            self.engine.pool_sets_pin_owner = weakref.ref(self)
        elif ptrs != self._pool_ptrs:
            raise DrnError("the fc6 operand buffers moved after the step was captured (%s -> %s): re-create the "
                           "GraphedTrainStep" % (self._pool_ptrs, ptrs))

    # ---- the heads -----------------------------------------------------------------------------------------------
    def _heads(self, eager):
        """fc6 forward (eager, when timed) + the heads graph of the current batch on the current stream"""
        self._fc6_eager()
        return self._main_body() if eager else (self.g_main.replay(), self.losses)[1]

    def _fc6_eager(self):
        if self.eager_fc6:
            self._fc6_part = self.engine.fc6_partials(self.pooled, self.rois.shape[0], True)

    def _main_body(self):
        losses, st = self.engine.forward(None, self.rois, self.obj, True, self.img_off, self.n_img, self.gt,
                                         pooled=self.pooled, fc6_part=self._fc6_part if self.eager_fc6 else None)
        self._keep_state(st)
        # = sum(losses.values()).backward() without autograd's scalar adds / ones / stack launches
        # (ITER_SIZE N > 1: the common upstream gradient is 1 / N, train_net.py:100-107)
        self.engine.backward(st, None if self.iter_size == 1 else 1.0 / self.iter_size)   # pipelined SGD buckets fork onto the optimizer stream in here
        if not self.split_tail:
            self.opt.step(1.0)           # joins the optimizer stream
        return losses

    def _opt_step(self):
        """end of the eager tail: join the optimizer stream - on closing micro-iterations only when gradients accumulate (the
        others gave that stream nothing to do, and optimizer.step() is not called for them)"""
        if self.iter_size == 1 or self._win.closing:
            self.opt.step(1.0)

    # ---- the ahead schedule: lookahead L >= 2, trunk groups, the ring ---------------------------------------------------------------
    def _run_ahead(self, eager, next_batch, upcoming, ready=()):
        """Step t at (G, A, P): see ahead_schedule for the indices.
          side : proposals / labels of batch t+1 -> the staging set; when t % G == 0, the images of the group A ahead -> its slot
                 and the conv chain of that slot.  The slot's and the set's last readers are pooling launches of earlier steps: one
                 wait on the main stream orders the side stream behind them, under the ring the host's throttle does.  With A >= 3
                 the A-1 side streams take turns.  `ready` (step()'s inputs_ready): events behind the producers of the caller's
                 tensors - the stream that stages them waits for each first; empty, nothing is enqueued
          main : heads graph of batch t (+ eager tail), wait for the trunk of batch t+1's group, pooling piece of batch t+1"""
        main = torch.cuda.current_stream()
        t = self._t
        ring = self._ring_on and not eager
        s = ahead_schedule(t, *self._GAP, self.RING_SETS if ring else 1)
        side = self._sides[t % len(self._sides)]
        if ring:
            while len(self._ring_evs) > self.RING_LAG - 1:
                self._ring_evs.pop(0).synchronize()  # heads(t - RING_LAG) are done: every earlier reader of the set / slot written below
        else:
            side.wait_stream(main)
        self._nb = s.nb
        losses = self._heads(eager)
        if self.split_tail:
            self.engine.run_fc1_tail()
        if ring:
            ev = getattr(self.opt, "small_ready_event", None)  # FusedSGD._on_grad_ready("small"): between the heads graph and the dW launch
            if ev is None:
                raise DrnError("the ring schedule needs the pipelined optimizer's hook on the fc6 tail")
            self.opt.small_ready_event = None
            self._ring_evs.append(ev)
        evp = None
        with torch.cuda.stream(side):
            if self.stage_ahead or s.launch is not None:
                for ev in ready:
                    side.wait_event(ev)
            # proposals of batch t+1 on the side stream (behind the last reader of their staging set, in front of the conv chain):
            # three small launches that sat between the last dW slab and the pooling piece on the main stream (22 us in the timeline)
            if self.stage_ahead:
                self._stage_props(next_batch)
                self._stage_labels_ahead(next_batch, via_stage=True)  # -> _gt_stage; the pooling piece hands them on
                evp = torch.cuda.Event()
                evp.record(side)
            if s.launch is not None:
                self._stage_image([x for b in upcoming[s.stage] for x in b], s.launch)
                self._bb_body(s.launch) if eager else self.g_pbb[s.launch].replay()
                self._done[s.launch] = torch.cuda.Event()
                self._done[s.launch].record(side)
        if evp is not None:
            main.wait_event(evp)
        else:
            for ev in ready:
                main.wait_event(ev)
            self._stage_props(next_batch)
        main.wait_event(self._done[s.pool_slot])
        self._pool_body(s.pool_slot, s.pool_part)
        if self.split_tail:
            self._opt_step()
        self._t = t + 1
        return losses

    def _ring_allowed(self):
        """the ring: trunk groups on ONE GPU, the eager fc6 tail with THIS optimizer's pipelined hook (its event is the throttle's).
        Any other hook on the head engine (DataParallel's alone) or a job of several ranks gets the waiting schedule"""
        hook = self.engine.grad_ready_hook
        own = bool(getattr(self.opt, "_pipelined", False)) and hook is not None and getattr(hook, "__self__", None) is self.opt
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        dp = getattr(self.opt, "_dp", None)
        if dp is not None:
            world = max(world, int(dp.world))
        return bool(self.trunk_pairs and self.engine.kshard is None and self.split_tail and own and world == 1
                    and self._ring_want)

    def _prime_ahead(self, first_batch, next_batch, upcoming):
        """The trunks of groups 0 .. A-1 and the pooling of batch 0, step 0 eagerly (_run_ahead launches group A's chain), then the
        captures: the heads graph and one chain graph per slot."""
        self.heads.train()
        main = torch.cuda.current_stream()
        G, A = self._GA
        self._ring_on = self._ring_allowed()
        P = A if not self.trunk_pairs else self.RING_SLOTS if self._ring_on else 2
        self._GAP = (G, A, P)
        self._sides = [self._side] + [torch.cuda.Stream() for _ in range(A - 2)]
        self._images = [[im.clone() for _ in range(G) for im in self.image] for _ in range(P)]
        self._done = [None] * P
        batches = [first_batch, next_batch] + list(upcoming)
        with torch.no_grad():
            self._stage_image([x for b in batches[:G] for x in b], 0)
            f0 = self._backbone(0).clone()
            self._feats = [f0] + [torch.zeros_like(f0) for _ in range(P - 1)]
            self._stage_props(first_batch)
            self._pool_body(0, 0)
            for q in range(A):
                if q:
                    self._stage_image([x for b in batches[q * G: (q + 1) * G] for x in b], q)
                    self._bb_body(q)
                self._done[q] = torch.cuda.Event()
                self._done[q].record(main)
        self._stage_labels(first_batch)
        self.opt.zero_grad()
        self._t = 0
        first = {k: v.detach().clone() for k, v in self._run_ahead(True, next_batch, upcoming).items()}
        self.opt.zero_grad()
        torch.cuda.synchronize()
        self.g_pbb = [_captured(self._bb_body, slot)[0] for slot in range(P)]
        self.g_main, self.losses = _captured(self._main_body)
        self._primed = True
        self._mark_captured()
        return first

    # ---- lookahead = 1 ------------------------------------------------------------------------------------------------------------
    def _run(self, eager, next_batch=None, ready=()):
        """One step = three pieces on two torch streams, ordered by events exactly like eager multi-stream code.  (A
        single graph with the backbone as an internal branch was measured first: the HIP graph executor starts that
        branch late whatever the capture order, so the 49 latency-bound conv nodes ended up on the critical path.)
          side : backbone graph of the NEXT image     - may start once the previous step's pooling has read feat_next
          main : heads / losses / backward / SGD graph - reads the operand pooled by the previous step
          main : pooling graph of the NEXT batch       - behind this step's last reader of A^T, after the backbone"""
        main = torch.cuda.current_stream()
        self._side.wait_stream(main)  # staged image is in place; previous pooling has consumed feat_next
        # submit the heads graph FIRST: submitting a graph costs the host ~9 us per node, and the backbone graph has
        # 49 nodes - issued first it would leave the main stream idle for ~0.45 ms in front of the fc6 GEMM
        losses = self._heads(eager)
        if self.split_tail:
            self.engine.run_fc1_tail()  # eager: dW slabs on this stream, all-reduce + SGD per bucket on the optimizer stream
        with torch.cuda.stream(self._side):
            if next_batch is not None:
                for ev in ready:  # (step()'s inputs_ready)
                    self._side.wait_event(ev)
                # the next batch's image / proposals are consumed by this stream's backbone graph and by the pooling graph
                # behind it: staging them here keeps five small copies off the front of the heads graph
                self._stage_next(next_batch)
            self._bb_body() if eager else self.g_bb.replay()
            done = torch.cuda.Event()
            done.record(self._side)
        self._stage_labels_ahead(next_batch)
        main.wait_event(done)
        self._pool_body() if eager else self.g_pool.replay()
        if self.split_tail:
            self._opt_step()  # join the optimizer stream: the exchange ran under the backbone + pooling above
        return losses

    def prime(self, first_batch, next_batch):
        """Step 0, eagerly (so every workspace exists and the captured SGD is not the momentum-initialising first
        step), then the captures.  Returns step 0's losses."""
        self.heads.train()
        self._stage_next(first_batch)
        with torch.no_grad():
            self.feat_next = self._backbone().clone()
            self._feats = [self.feat_next]
            self._pool_body()
        self._stage_labels(first_batch)
        self._stage_next(next_batch)
        self.opt.zero_grad()
        first = {k: v.detach().clone() for k, v in self._run(eager=True).items()}
        self.opt.zero_grad()
        torch.cuda.synchronize()
        self.g_bb = _captured(self._bb_body)[0]
        self.g_main, self.losses = _captured(self._main_body)
        self.g_pool = _captured(self._pool_body)[0]
        self._primed = True
        self._mark_captured()
        return first

    def step(self, batch, next_batch, *upcoming, inputs_ready=None):
        """run the step for `batch` (which must be the batch passed as `next_batch` to the previous call); the same
        step prepares `next_batch` (backbone on the side stream, pooling behind the last dW GEMM).  The ahead schedule also takes
        the ahead_arity(G, A) batches after that, of which only the images are read: lookahead=L, batches t+2 .. t+L (the backbone
        of the last one runs now); trunk_pairs=G, batches t+2 .. t+2G-1 (when t % G == 0 the chain of the last G starts now).

        When the inputs must be ready.  The step reads the caller's DEVICE tensors - proposal boxes and objectness of `next_batch`,
        the images of `next_batch` (lookahead=1) or of `upcoming` - on a side stream, and keeps the allocator from reusing them
        (record_stream) until it has.  What that read is ordered behind depends on the schedule:
          the waiting schedules (lookahead=L, trunk groups with ring=False or wherever the ring does not apply) : the side stream
              waits for the stream current at the call, so whatever the caller enqueued THERE before step() - a non-blocking
              copy, preprocessing - is done first.  Plain stream order suffices
          the ring : the side stream waits for nothing the caller enqueued.  The tensors must be complete from the HOST's point
              of view (the producer synchronised, as DatasetMapper.finish does), or the caller passes
        inputs_ready = an event, or a sequence of events, recorded behind the producers of these tensors (on any stream): every
        stream that stages caller tensors in this step waits for each of them first (wait_event: the host never blocks).  It is
        honoured by every schedule; with None nothing is enqueued.  Image-level labels (gt_classes) are read on the host during
        the call and are outside this contract."""
        ready = () if inputs_ready is None else (inputs_ready,) if isinstance(inputs_ready, torch.cuda.Event) \
            else tuple(inputs_ready)
        self._replayed = self._primed
        if not self._primed:
            self._check_label_layout()  # (in front of the first staging: the staging sets follow the block)
        if self._primed:
            # the captured (or eagerly issued) SGD launches read lr / weight decay from device tables: follow the schedule
            self.opt.refresh_tables()
        if self.iter_size > 1:
            from .engine import window_position

            self._win = window_position(self._iter, self.iter_size, self._start_iter)
            self.opt.set_window(self._win)
            self._iter += 1
            if self._guard is not None and self._win.first:
                self._guard.open_window()
        if self._GA is None:
            if not self._primed:
                self._await(ready)
                return self.prime(batch, next_batch)
            self._stage_labels_now(batch)
            return self._run(eager=False, next_batch=next_batch, ready=ready)
        if len(upcoming) != ahead_arity(*self._GA):
            if self.trunk_pairs:
                raise DrnError("GraphedTrainStep(trunk_pairs=%d).step needs batches t+2 .. t+%d" % (self.G, 2 * self.G - 1))
            raise DrnError("GraphedTrainStep(lookahead=%d).step needs the %d batches after next_batch"
                           % (self.lookahead, self.lookahead - 1))
        if not self._primed:
            self._await(ready)
            return self._prime_ahead(batch, next_batch, upcoming)
        self._stage_labels_now(batch)
        return self._run_ahead(False, next_batch, upcoming, ready)

    @staticmethod
    def _await(ready):
        """priming stages on the current stream and the streams it forks wait for that one: the events go in front of it all"""
        for ev in ready:
            torch.cuda.current_stream().wait_event(ev)


class GraphedFullStep(_StaticInputs):
    """The training step of a TRAINABLE trunk (MODEL.BACKBONE.FREEZE_AT < 5) as ONE hipGraph on one stream: preprocess,
    trunk forward with saved activations, ROIPool (with arg-max), heads, losses, the explicit backward through the
    heads, fc6 dX, RoIPool / ROIAlign backward and every trainable trunk block (conv dgrad / wgrad straight into the
    trunk's gradient arena), then the fused SGD step of both arenas and the re-pack of the updated conv weights at the
    top of the next replay.  ~250 launches of 5-60 us that the eager Python host cannot enqueue as fast as the GPU runs
    them; a replay costs one graph launch.  Nothing of a future batch can run ahead here - the trunk's weights change
    every step - so there is no side stream and no lookahead: step(batch) stages `batch` and replays.
    Static shapes (image size, proposals per image, images per GPU), ITER_SIZE 1.
    N > 1 (`parallel` = the model's DataParallel, round 3): no collective is ever captured - the step becomes TWO graphs
    around an eager exchange: [forward + backward] -> all-reduce of the head engine's gradient arena (everything up to the
    end of fc1.weight: the unused bbox_pred tail never travels) and of the trunk's flat gradient arena -> [SGD of both
    arenas with 1 / world + zero_grad].  DataParallel's per-bucket hooks stay silent (`sync_gradients` off): the buckets
    only pay when the optimizer can update one while the next is still being produced, which the plain optimizer step of a
    trainable trunk does not do."""

    def __init__(self, model, optimizer, example_batch, parallel=None, start_iter=0):
        if getattr(optimizer, "_pipelined", False):
            raise DrnError("GraphedFullStep uses the plain optimizer step (the pipelined mode assumes a frozen trunk)")
        super().__init__(model, optimizer, example_batch)
        self.engine.defer_fc1_tail = False
        self.g_step = None
        self.g_trunk = None
        self.g_opt = None
        if parallel is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            #  without the DataParallel object the step would run with NO gradient exchange and no error
            raise DrnError("GraphedFullStep in a %d-rank job needs parallel=DataParallel(model): without it the replicas "
                           "train on their local gradients and diverge" % dist.get_world_size())
        self.dp = parallel if (parallel is not None and parallel.exchange) else None
        self._comm = None
        # the anomaly guard: the check (heads forward) and the guard pointer of both arenas' updates are captured; ITER_SIZE 1
        # here, so every step opens its window
        self._guard = getattr(optimizer, "_guard", None)
        if self._guard is not None:
            if self.dp is not None:
                optimizer._refuse_guard_multi_rank("a gradient exchange")
            self._guard.window_first = True
        self._anchor_metrics(start_iter)  # (start_iter: the training iteration of the first step, for the metrics ring alone)

    def _stage(self, batch):
        self._stage_labels(batch)
        off = 0
        for i, x in enumerate(batch):
            n = self.nper[i]
            assert len(x["proposals"]) == n, "graphed step: proposals per image must stay fixed"
            self.rois[off: off + n, 1:].copy_(x["proposals"].proposal_boxes.tensor, non_blocking=True)
            self.obj[off: off + n].copy_(x["proposals"].objectness_logits, non_blocking=True)
            off += n
        self.props.copy_(self.rois[:, 1:])
        self._stage_image(batch, 0)

    def _fwd_bwd(self):
        m, eng = self.model, self.engine
        imgs = m.preprocess_image([{"image": im} for im in self._images[0]])
        feats = m.backbone(imgs.tensor)  # training mode + trainable blocks: activations are kept for backward_nhwc()
        f = feats[self.heads.box_in_features[0]].permute(0, 2, 3, 1)
        assert f.is_contiguous()
        # N > 1: the trunk's backward is a piece of its own (_trunk_bwd), so that the all-reduce of the heads' gradient arena -
        # final when the heads' backward ends - runs under it; the hook only keeps what that piece needs
        eng.feature_grad_hook = m._backbone_backward if self.dp is None else self._keep_feature_grad
        losses, st = eng.forward(f, self.rois, self.obj, True, self.img_off, self.n_img, self.gt)
        self._keep_state(st)
        # the per-bucket hooks of DataParallel (eager trainer) are replaced by _exchange_* below: off while THIS step's
        # backward runs, restored right after (the flag used to stay off on the shared object for good)
        flag = None if self.dp is None else self.dp.sync_gradients
        if self.dp is not None:
            self.dp.sync_gradients = False
        try:
            eng.backward(st, None)
        finally:
            if self.dp is not None:
                self.dp.sync_gradients = flag
        return losses

    def _keep_feature_grad(self, dfeat, acc):
        self._dfeat = (dfeat, acc)

    def _trunk_bwd(self):
        dfeat, acc = self._dfeat
        self.model._backbone_backward(dfeat, acc)

    def _opt_body(self):
        self.opt.step(1.0 if self.dp is None else self.dp.grad_scale)
        self.opt.zero_grad()

    def _exchange_heads(self):
        """all-reduce of the heads' gradient arena (the SGD kernels apply 1 / world) on the exchange stream, started the
        moment the heads' backward is queued: it runs under the trunk's backward (round 4; one eager call between two
        graphs with nothing beside it before)"""
        e = self.engine
        o, n = e._seg["fc1.weight"]
        main = torch.cuda.current_stream()
        if self._comm is None:
            self._comm = torch.cuda.Stream()
        self._comm.wait_stream(main)
        with torch.cuda.stream(self._comm):
            dist.all_reduce(e.arena_g[: o + n], group=self.dp.group)

    def _exchange_trunk(self):
        """all-reduce of the trunk's gradient arena behind the heads' one (same stream: RCCL runs one collective of a
        communicator at a time anyway), then the main stream joins"""
        main = torch.cuda.current_stream()
        bg = getattr(self.model, "_bb_grad_arena", None)
        if bg is not None:
            self._comm.wait_stream(main)
            with torch.cuda.stream(self._comm):
                dist.all_reduce(bg, group=self.dp.group)
        main.wait_stream(self._comm)

    def _full_body(self):
        losses = self._fwd_bwd()
        if self.dp is not None:
            self._exchange_heads()
            self._trunk_bwd()
            self._exchange_trunk()
        self._opt_body()
        return losses

    def step(self, batch):
        self.heads.train()
        self._replayed = self.g_step is not None
        self._stage(batch)
        if self.g_step is None:
            # step 0 eagerly (workspaces exist, momentum buffers initialised, packs invalidated by the update), then the
            # capture: the captured forward starts with the re-pack of the freshly updated conv weights
            self.opt.zero_grad()
            first = {k: v.detach().clone() for k, v in self._full_body().items()}
            torch.cuda.synchronize()
            # the capture pass RUNS nothing: the gradient arenas and weights are exactly as step 0 left them
            if self.dp is None:
                self.g_step, self.losses = _captured(self._full_body)
            else:
                self.g_step, self.losses = _captured(self._fwd_bwd)
                self.g_trunk = _captured(self._trunk_bwd)[0]
                self.g_opt = _captured(self._opt_body)[0]
            self._mark_captured()
            return first
        self.opt.refresh_tables()
        self.g_step.replay()
        if self.dp is not None:
            self._exchange_heads()   # exchange stream: under the trunk's backward
            self.g_trunk.replay()
            self._exchange_trunk()
            self.g_opt.replay()
        return self.losses
