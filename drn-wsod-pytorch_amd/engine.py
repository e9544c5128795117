"""Trainer-side pieces the hot path sits inside:

  build_optimizer / FusedSGD   torch.optim.SGD with the per-parameter groups of detectron2/solver/build.py:93-137
                               (bias lr x BIAS_LR_FACTOR, bias wd = WEIGHT_DECAY_BIAS), as ONE HIP kernel over the
                               head engine's flat parameter arena (fp32 master + momentum).
  WarmupMultiStepLR            detectron2/solver/lr_scheduler.py:16-49
  DataParallel                 replaces DistributedDataParallel(broadcast_buffers=False, find_unused_parameters=True)
                               of detectron2/engine/defaults.py:279-282: one process per GPU, gradients of the flat
                               arena are all-reduced (RCCL over xGMI) on a side stream, bucketed so that the small
                               tensors and then each fc6-gradient slab are on the wire while the next dW slab is
                               still being computed; unused bbox_pred parameters never enter a bucket.
  Trainer.run_step             projects/WSL/tools/train_net.py:65-117 (ITER_SIZE accumulation, loss dict keys) without
                               the per-iteration host syncs (metric gather is deferred; the anomaly check of
                               train_loop.py:252-258 is either deferred - check_finite() - or, with
                               FusedSGD(nonfinite="raise" | "skip"), made on the device in front of every update: LossGuard)."""
import bisect
import collections
import math

import torch
import torch.distributed as dist

from . import ops
from ._cabi import DrnError
from .events import EventStorage


class Window(collections.namedtuple("Window", "first closing")):
    """Position of a micro-iteration inside its gradient-accumulation window (WSL.ITER_SIZE = N > 1): `first` - nothing has been
    accumulated yet, the gradients are overwritten; `closing` - the optimizer steps behind this backward.  A micro-iteration
    that is neither is a middle one; the window {0} after start_iter = 0 is both."""
    __slots__ = ()


def window_position(it, iter_size, start_iter=0):
    """projects/WSL/tools/train_net.py:100-113: the optimizer steps and the gradients are cleared when it % N == 0, so the first
    window after start_iter = 0 is the single iteration 0 and the later ones are kN+1 .. (k+1)N; a run resumed at `start_iter`
    starts from cleared gradients whatever its position (zero_grad at iter == start_iter)."""
    n = int(iter_size)
    return Window(first=(it == start_iter or (it - 1) % n == 0), closing=(it % n == 0))


NONFINITE_MODES = ("off", "raise", "skip")
_NONFINITE_MSG = "Loss became infinite or NaN at iteration={}!"  # detectron2/engine/train_loop.py:252-258


class LossGuard:
    """Device side of the anomaly guard (FusedSGD(nonfinite=...)): the int32 state drn_loss_guard keeps - [0] the skip flag every
    guarded update kernel reads, [1] checks seen, [2] first bad check or -1, [3] bad checks - and what the head engine needs to
    issue the check behind its loss tail.  window_first: whether the NEXT check opens a WSL.ITER_SIZE window (mode "skip": a bad
    micro-step discards its whole window and nothing more); iter0: the training iteration of check 0, for the message."""

    def __init__(self, mode, device):
        self.mode = mode
        self.code = ops.GUARD_RAISE if mode == "raise" else ops.GUARD_SKIP
        self.state = ops.loss_guard_state(device)
        self.window_first = True
        self.iter0 = 0

    def check(self, loss_list):
        ops.loss_guard(loss_list, self.code, self.window_first, self.state)

    def open_window(self):
        """a captured check has its window_first frozen: clear the flag on the stream in front of the window's first replay
        instead (mode "skip"; the flag of "raise" is sticky) and capture every check with window_first = 0 - the same rule,
        flag = bad_now or (flag and not window_first)"""
        if self.mode == "skip":
            self.state[:1].zero_()

    def read(self):
        flag, calls, first_bad, bad = self.state.cpu().tolist()  # the one small D2H read
        return {"mode": self.mode, "skip": bool(flag), "calls": calls, "first_bad": first_bad, "bad": bad,
                "first_bad_iteration": None if first_bad < 0 else self.iter0 + first_bad}


class FusedSGD:
    def __init__(self, model, base_lr, momentum, weight_decay, bias_lr_factor=1.0, weight_decay_bias=None,
                 weight_decay_norm=0.0, nesterov=False, clip_type=None, clip_value=1.0, norm_type=2.0, nonfinite="off"):
        """clip_type / clip_value / norm_type: SOLVER.CLIP_GRADIENTS (detectron2/solver/build.py:19-90) - every parameter is
        clipped on its own right before the update, on the gradient the update sees (g * grad_scale): "value" clamps to
        +-clip_value, "norm" scales by min(clip_value / (||g||_norm_type + 1e-6), 1); None = no clipping (every launch as before).
        nonfinite: the anomaly guard (detectron2/engine/train_loop.py:252-258 checks every iteration's summed loss in front of
        the optimizer).  "off" (default): every launch as before.  "raise" / "skip": a one-wave kernel behind the loss tail tests
        isfinite(sum of the losses) on the device, and every update kernel of the step - the fused fc6 dW + SGD launch included -
        leaves weights, momentum and shadow bit-unchanged when it is not.  "raise": the flag is sticky, so the state stays that of
        the last finite iteration until Trainer.check_finite() / state_dict() raise the reference's FloatingPointError with the
        first bad iteration.  "skip": the bad window is dropped and training goes on; guard_state() reports the counts."""
        if nonfinite not in NONFINITE_MODES:
            raise ValueError("nonfinite=%r: one of %s" % (nonfinite, ", ".join(repr(m) for m in NONFINITE_MODES)))
        self.nonfinite = nonfinite
        if nesterov:
            raise DrnError("nesterov SGD is not used by any DRN-WSOD config")
        if clip_type not in (None, "value", "norm"):
            raise ValueError("%r is not a valid GradientClipType (SOLVER.CLIP_GRADIENTS.CLIP_TYPE: 'value' or 'norm')" % (clip_type,))
        self.clip_type, self.clip_value, self.norm_type = clip_type, float(clip_value), float(norm_type)
        if clip_type == "norm":
            ops.norm_type_code(norm_type)  # 1, 2 and inf are built; DrnError naming the key otherwise
        if clip_type is not None and not self.clip_value >= 0.0:
            raise DrnError("SOLVER.CLIP_GRADIENTS.CLIP_VALUE must be >= 0 (got %r)" % (clip_value,))
        self._norms = None  # clip_type "norm": per-parameter norms of the last plain step (heads' segments, then the trunk's)
        self._norm_ws = None
        self.model = model
        self.engine = model.roi_heads._engine
        self.momentum = momentum
        wdb = weight_decay if weight_decay_bias is None else weight_decay_bias
        self.engine.ensure(next(model.roi_heads.parameters()).device)
        # (the guard lives on the engine that issues its check; off = the attribute is None and no launch changes)
        self._guard = LossGuard(nonfinite, self.engine.arena_w.device) if nonfinite != "off" else None
        self.engine.loss_guard = self._guard
        self.param_groups = []
        for name, p, off, n, used in self.engine.segments:
            is_bias = name.endswith(".bias")
            self.param_groups.append({"params": [p], "name": name, "off": off, "cnt": n, "used": used,
                                      "lr": base_lr * (bias_lr_factor if is_bias else 1.0),
                                      "initial_lr": base_lr * (bias_lr_factor if is_bias else 1.0),
                                      "weight_decay": wdb if is_bias else weight_decay, "momentum": momentum})
        self._mom = None
        self._segs_key = None
        self._segs_dev = None
        self._steps = 0
        # MODEL.BACKBONE.FREEZE_AT < 5: trainable trunk parameters get a flat arena of their own (weights, gradients,
        # momentum; nn.Parameters and their .grad are views in the state_dict layout, which is also the layout the
        # weight-gradient GEMMs write)
        self._bb = None
        extra = [(n, p) for n, p in model.named_parameters() if p.requires_grad and not n.startswith("roi_heads.")]
        if extra:
            dev = extra[0][1].device
            tot = sum((p.numel() + 7) // 8 * 8 for _, p in extra)
            bw = torch.zeros((tot,), dtype=torch.float32, device=dev)
            bg = torch.zeros_like(bw)
            off, groups = 0, []
            for n, p in extra:
                cnt = p.numel()
                bw[off: off + cnt].copy_(p.data.reshape(-1))
                p.data = bw[off: off + cnt].view(p.shape)
                p.grad = bg[off: off + cnt].view(p.shape)
                is_bias = n.endswith(".bias")
                groups.append({"params": [p], "name": n, "off": off, "cnt": cnt, "used": True, "bb": True,
                               "lr": base_lr * (bias_lr_factor if is_bias else 1.0),
                               "initial_lr": base_lr * (bias_lr_factor if is_bias else 1.0),
                               "weight_decay": wdb if is_bias else weight_decay, "momentum": momentum})
                off += (cnt + 7) // 8 * 8
            self._bb = dict(w=bw, g=bg, mom=None, groups=groups, segs_key=None, segs_dev=None)
            self.param_groups += groups
            model._bb_grad_arena = bg  # the data-parallel engine sums this buffer
            for m in model.backbone.modules():
                if hasattr(m, "invalidate_packs"):
                    m.invalidate_packs()

    @property
    def _gs(self):
        """guard= argument of every update launch: the guard's device state, or None (the unguarded entry points)"""
        return None if self._guard is None else self._guard.state

    def guard_state(self):
        """The anomaly guard's device state as a dict (one small D2H read, which waits for the work queued so far): mode, skip
        (the flag now), calls, first_bad (check index or -1), bad, first_bad_iteration.  None with nonfinite="off"."""
        return None if self._guard is None else self._guard.read()

    def raise_if_nonfinite(self):
        """nonfinite="raise": FloatingPointError with the reference's message if a loss has been non-finite since the guard was
        enabled - naming the FIRST such iteration, whose update and every later one were skipped.  Returns guard_state()."""
        st = self.guard_state()
        if st is not None and st["mode"] == "raise" and st["first_bad"] >= 0:
            raise FloatingPointError(_NONFINITE_MSG.format(st["first_bad_iteration"]))
        return st

    def _refuse_guard_multi_rank(self, what):
        raise DrnError("FusedSGD(nonfinite=%r) with %s: the ranks would have to agree on the skip flag before any of them "
                       "updates, which is not built (single process only; use nonfinite='off' and Trainer.check_finite())"
                       % (self.nonfinite, what))

    def _segs_bb(self):
        bb = self._bb
        key = tuple((g["lr"], g["weight_decay"]) for g in bb["groups"])
        if key != bb["segs_key"]:
            bb["segs_dev"] = ops.sgd_segments(((g["off"], g["cnt"], g["lr"], g["weight_decay"]) for g in bb["groups"]),
                                              out=bb["segs_dev"], device=bb["w"].device)
            bb["segs_key"] = key
        return bb["segs_dev"], len(bb["groups"])

    def _step_bb(self, grad_scale):
        bb = self._bb
        if bb["mom"] is None:
            bb["mom"] = torch.zeros_like(bb["w"])
        segs, nseg = self._segs_bb()
        ops.sgd_step(bb["w"], bb["mom"], bb["g"], segs, nseg, self.momentum, self._steps == 0, grad_scale,
                     clip=self._clip(bb["g"], segs, nseg, grad_scale, self._nseg), guard=self._gs)
        for m in self.model.backbone.modules():
            if hasattr(m, "invalidate_packs"):
                m.invalidate_packs()  # updated in place: the packed compute copies of the conv weights are stale

    def _clip(self, grads, segs, nseg, grad_scale, first):
        """clip argument of the plain step's ops.sgd_step over one arena (None without clipping).  "norm": the per-segment norms
        are computed here, on the device, into elements first .. first + nseg of ONE buffer that is allocated once (as is the
        workspace), so a captured step keeps writing what last_grad_norms() hands out."""
        if self.clip_type is None:
            return None
        if self.clip_type == "value":
            return (ops.CLIP_VALUE, self.clip_value, None)
        if self._norms is None:
            tot = self._nseg + (len(self._bb["groups"]) if self._bb is not None else 0)
            self._norms = torch.zeros((tot,), dtype=torch.float32, device=grads.device)
            self._norm_ws = torch.empty((ops.grad_norms_ws_bytes(tot),), dtype=torch.uint8, device=grads.device)
        norms = self._norms[first: first + nseg]
        ops.grad_norms(grads, segs, nseg, self.norm_type, grad_scale, out=norms, workspace=self._norm_ws)
        return (ops.CLIP_NORM, self.clip_value, norms)

    def last_grad_norms(self):
        """(names, norms): the per-parameter gradient norms ||g * grad_scale||_NORM_TYPE the last plain step() clipped by, as the
        device tensor the step wrote (no synchronisation: float() it only when you need to look), in the order of `names` -
        the heads' parameters, then a trainable trunk's.  clip_type "norm" only; (names, None) before the first step."""
        if self.clip_type != "norm":
            raise DrnError("last_grad_norms(): SOLVER.CLIP_GRADIENTS.CLIP_TYPE is %r, norms are computed for 'norm' only"
                           % (self.clip_type,))
        names = [g["name"] for g in self.param_groups if g["used"] and not g.get("bb")]
        if self._bb is not None:
            names += [g["name"] for g in self._bb["groups"]]
        return names, self._norms

    def _segs(self):
        groups = [g for g in self.param_groups if g["used"] and not g.get("bb")]
        key = tuple((g["lr"], g["weight_decay"]) for g in groups)
        if key != self._segs_key:
            # (out=: in place from the second time on - a captured hipGraph keeps reading this table)
            self._segs_dev = ops.sgd_segments(((g["off"], g["cnt"], g["lr"], g["weight_decay"]) for g in groups),
                                              out=self._segs_dev, device=self.engine.arena_w.device)
            self._segs_key, self._nseg = key, len(groups)
        return self._segs_dev, self._nseg

    # ---- pipelined mode: the update of a gradient bucket starts as soon as the bucket is final ----------------
    @property
    def iter_size(self):
        """WSL.ITER_SIZE the pipelined mode was enabled for (1: no accumulation; also for the plain step(), which the Trainer
        drives by its own window rule)"""
        return getattr(self, "_iter_size", 1)

    def set_window(self, win):
        """iter_size > 1: position (Window) of the micro-iteration whose backward comes next.  The head engine's fc6 tail and this
        optimizer's hooks issue by it: gradients accumulate in the fp32 arena, buckets are announced and updated on closing
        micro-iterations only."""
        if self.iter_size == 1:
            raise DrnError("set_window(): the pipelined mode was enabled without gradient accumulation (iter_size = 1)")
        self._window = win
        self.engine.accum_window = win

    def enable_pipelined(self, dp=None, slab_rows=None, comm_dtype=None, exchange=None, kshard_wire=None, fused_tn=None,
                         iter_size=1):
        """The explicit backward finishes gradients in a known order: first every small tensor
        (predictors, fc7, fc6 bias), then fc6.weight in row slabs.  In pipelined mode each bucket is (all-reduced when
        N > 1 and then) updated by the SGD kernel on a second stream the moment its dW GEMM is queued, so the HBM-bound
        optimizer pass hides under the MFMA-bound remaining dW GEMMs; `step()` then only joins the streams.
        Same arithmetic as the plain step (the kernel, the per-group lr/wd and the 1/W scale are identical).
        comm_dtype: dtype of the fc6 weight-gradient buckets.  torch.bfloat16 = the dW GEMM rounds its fp32 accumulators
        once and writes bf16 straight into a bucket buffer that RCCL sums (N > 1) and the SGD kernel reads: half the
        xGMI bytes (the dominant cost of the 8-GPU step: 411 MB fp32 per step for R50-C4) and 0.4 GB less HBM traffic
        per step on every GPU.  Default = bf16 in the bf16 compute mode - the same rounding torch.autocast(bf16) applies
        to a Linear's weight gradient; master weights and momentum stay fp32 - and fp32 (the reference's DDP
        arithmetic) in the fp32 parity mode.  With an exchange the small tensors cross the wire in the same dtype (cast
        into a wire buffer; their local fp32 gradient stays in the arena); without one they are read in fp32.
        exchange (N > 1): "sharded" (default) = SURVEY 8(e)'s target - every fc6 row slab is REDUCE-SCATTERED (rank k
        receives the sum of rows k*q .. (k+1)*q of the slab), the fused SGD kernel updates only those rows (the 2.05-GB
        optimizer pass shrinks to 1/N per GPU; momentum is sharded the same way), and the updated compute copy of the
        rows - the bf16 shadow, or the fp32 master in the parity mode - is ALL-GATHERED into every rank's arena under the
        next image's trunk / pooling graphs.  Same wire bytes as an all-reduce (2 (N-1)/N of the bucket), identical
        arithmetic (sum over ranks, 1/N in the kernel).  "allreduce" = one all-reduce per bucket and the replicated
        update on every rank (detectron2/engine/defaults.py:279-282's DDP, restated).  The small tensors (38 MB) are
        all-reduced and updated on every rank in both modes.
        iter_size = WSL.ITER_SIZE (default 1: every launch as before).  N > 1, single process, frozen trunk: the micro-iterations
        of a window (window_position; set_window() before every backward) accumulate in the fp32 gradient arena - the small
        tensors through the accumulate flags of their GEMMs / column sums (always on: the arena's small-tensor region is
        cleared behind the closing update instead, so ONE captured heads graph serves every position), fc1.weight through
        drn_gemm_tn / drn_gemm_nt with fp32 C - and only the closing one announces buckets: the small tensors are updated in
        fp32 from the arena, fc1.weight is rounded to the bf16 bucket ONCE per window, by drn_gemm_tn_acc_sgd together with
        its update (fused_tn) or by drn_cast2d + drn_sgd_step_block.  In the fp32 parity mode the arena is the gradient."""
        iter_size = int(iter_size)
        if iter_size < 1:
            raise DrnError("iter_size must be >= 1")
        if self._guard is not None:
            if dp is not None and dp.exchange:
                self._refuse_guard_multi_rank("a gradient exchange")
            if exchange == "fc6_kshard":
                self._refuse_guard_multi_rank("the K-sharded fc6")
        self._bucket_clip = None
        if self.clip_type is not None:
            # SOLVER.CLIP_GRADIENTS on this schedule: value clipping, single process, iter_size 1, fc6 dW unfused (the fused
            # launches' epilogues carry no clamp); everything else is the plain step()'s
            why = None
            if self.clip_type == "norm":
                why = "CLIP_TYPE 'norm' needs a whole tensor's norm before any of it is updated, and fc6.weight arrives in slabs"
            elif dp is not None and dp.exchange:
                why = "clipping acts on the gradient summed over the ranks, which this schedule updates bucket by bucket"
            elif exchange == "fc6_kshard":
                why = "the K-sharded fc6 updates its columns in the fused fc6 dW + SGD launch"
            elif iter_size > 1:
                why = "the closing micro-iteration of a WSL.ITER_SIZE > 1 window rounds and updates fc6.weight in one fused launch"
            elif fused_tn:
                why = "fused_tn=True: the fused fc6 dW + SGD launch has no clamp in its epilogue (leave fused_tn unset)"
            if why is not None:
                raise DrnError("SOLVER.CLIP_GRADIENTS is not built for this pipelined optimizer schedule (%s); use the "
                               "plain step()" % why)
            fused_tn = False
            self._bucket_clip = (ops.CLIP_VALUE, self.clip_value, None)
        if iter_size > 1:
            if self._bb is not None:
                raise DrnError("WSL.ITER_SIZE > 1 in the pipelined optimizer mode needs a frozen backbone (FREEZE_AT=5)")
            if (dp is not None and dp.exchange) or exchange == "fc6_kshard":
                raise DrnError("WSL.ITER_SIZE > 1 in the pipelined optimizer mode is a single-process schedule: no gradient "
                               "exchange, no K-sharded fc6 (use the plain step())")
        if self._bb is not None:
            raise DrnError("the pipelined optimizer mode assumes a frozen backbone (FREEZE_AT=5); use the plain step()")
        e = self.engine
        d1 = self.model.roi_heads.box_head.fc1.weight.shape[0]
        world = dp.world if dp is not None else 1
        if slab_rows is None:
            # 256-row tile granularity of the dW GEMM: two equal slabs (measured: 3+ forked buckets make the HIP graph
            # executor schedule the branches badly, 395 -> 310 img/s).  N > 1 used 5/8 + 3/8 of the rows until the end of
            # round 2 (980 + 588 tiles = 4 + 3 rounds of the 256 CUs where two equal slabs took 4 + 4); with tail
            # balancing and the joint peel (run_fc1_tail) two equal slabs are 3 + 3 exact rounds + one small launch -
            # 36 us less GEMM time, the first bucket is final earlier and both exchanges move the same bytes
            t = (d1 + 255) // 256
            slab_rows = [min(d1, ((t + 1) // 2) * 256)]
            slab_rows = sorted(set(r for r in slab_rows if 0 < r < d1)) + [d1]
        if exchange not in (None, "sharded", "allreduce", "fc6_kshard"):
            raise DrnError("exchange must be 'sharded', 'allreduce' or 'fc6_kshard'")
        # "fc6_kshard" (round 4, opt-in): fc6 is sharded along K over the ranks instead of replicated - rank k keeps the
        # columns k of fc1.weight, pools that channel slice of every rank's image, and a reduce-scatter of the partial H1
        # (forward) / an all-gather of dP1 (backward) replace the exchange of the 205-MB weight gradient; the optimizer
        # updates only the owned columns (_HeadEngine.kshard).  The small tensors keep the all-reduce.  Fixed-shape batches,
        # eager steps.
        self._kshard = exchange == "fc6_kshard" and dp is not None and dp.exchange
        e.kshard, e.fc1_fused_cols = None, None  # (re-entrant: bench.py falls back from one exchange to the next)
        if self._kshard:
            import weakref

            me = weakref.ref(self)
            e.kshard = dict(group=dp.group, world=world, rank=dist.get_rank(dp.group), wire=kshard_wire,
                            sync=lambda: me() is not None and me().sync_master())
            e.fc1_fused_cols = self._fused_fc1_cols if (fused_tn is None or fused_tn) else None
            slab_rows = [d1]
        self._sharded = world > 1 and exchange not in ("allreduce", "fc6_kshard")
        if self._sharded:
            r0 = 0
            for r1 in slab_rows:
                if (r1 - r0) % world:
                    if exchange == "sharded":
                        raise DrnError("sharded exchange: every fc6 row slab must split evenly over the %d ranks "
                                       "(slab %d:%d)" % (world, r0, r1))
                    self._sharded = False  # default mode: fall back to the all-reduce for shapes that do not divide
                    self._fallback = "fc6 row slab %d:%d does not split evenly over %d ranks" % (r0, r1, world)
                r0 = r1
            # the all-gather lands in the flat bf16 shadow arena, which is the forward's fc6 operand only when a row of
            # fc1.weight needs no K padding (C*P*P a multiple of the 128-byte slab); a padded operand is its own buffer,
            # re-cast from the fp32 master - stale for the rows other ranks own
            k1 = self.model.roi_heads.box_head.fc1.weight.shape[1]
            if self._sharded and ops.kpad(k1, torch.bfloat16) != k1:
                if exchange == "sharded":
                    raise DrnError("sharded exchange: fc1.weight rows of %d elements are K-padded in the bf16 compute copy; "
                                   "use exchange='allreduce'" % k1)
                self._sharded = False
                self._fallback = "fc1.weight rows of %d elements are K-padded in the bf16 compute copy" % k1
        if world > 1 and exchange is None and not self._sharded:
            # (this used to be silent) the default exchange for N > 1 is the sharded one
            import warnings

            warnings.warn("FusedSGD.enable_pipelined: the sharded gradient exchange does not apply (%s); using the "
                          "all-reduce exchange - every rank runs the full optimizer pass" % getattr(self, "_fallback", "?"))
        self._master_stale = False
        if self._sharded or self._kshard:
            self._install_state_dict_hook()
        self._slab_ends = slab_rows
        e.fc1_slab_ends = slab_rows
        e.grad_ready_hook = self._on_grad_ready
        self._iter_size, self._window = iter_size, None
        e.accum_window = None
        e.accum_small = iter_size > 1
        # (iter_size > 1: the column sums finish inside the backward with their accumulate flag - as the plain step's do - instead
        # of as partials that the optimizer stream adds up: nothing of a non-closing micro-iteration runs on that stream)
        e.defer_colsum = iter_size == 1
        if iter_size > 1:
            e.ensure(next(self.model.roi_heads.parameters()).device)
            e.arena_g.zero_()
        self._dp, self._pipelined = dp, True
        self._opt_stream = torch.cuda.Stream() if torch.cuda.is_available() else None
        self._bucket_segs = {}
        # with an exchange the optimizer stream carries only the link-bound all-reduces (one event per bucket); the
        # HBM-bound SGD launches are issued by step() on the caller's stream, each behind its bucket's event, so the
        # update of bucket i runs under the all-reduce of bucket i+1 without a fifth stream (HIP multiplexes streams
        # onto 4 hardware queues by default; a fifth aliased the main stream's queue and cost 20 %)
        self._deferred = []
        self._exchange_on = dp is not None and dp.exchange
        if comm_dtype is None:
            from . import get_precision

            comm_dtype = torch.bfloat16 if get_precision() == "bf16" else torch.float32
        self._comm_dtype = comm_dtype
        e.fc1_grad_bucket = None
        if self._comm_dtype == torch.bfloat16:
            k1 = self.model.roi_heads.box_head.fc1.weight.shape[1]
            e.ensure(next(self.model.roi_heads.parameters()).device)
            e.fc1_grad_bucket = torch.zeros((d1, k1), dtype=torch.bfloat16, device=e.arena_w.device)
        # fused_tn (single process, bf16 bucket; default on): fc6 dW + its optimizer step as ONE launch, the update of every
        # tile inside the next tile's mainloop (enable_fused_fc1_tn; +0.8 .. +2.4 % same-box, bit-identical).  Shapes outside
        # the kernel's class fall back per call.
        e.fc1_fused_tn = None
        if fused_tn is None:
            # the fused launch holds every CU with two 248-register waves per SIMD: a trunk conv workgroup (~100 registers)
            # no longer fits beside it, and a trunk whose conv chain is as long as the step (WS-R101: ~100 launches) loses more
            # than the fusion gains (647 vs 658 img/s, profiles/r4_19_side_workloads.txt); R50 / VGG16 trunks gain
            try:
                fused_tn = len(self.model.backbone.conv_modules()) <= 64
            except Exception:  # noqa: BLE001
                fused_tn = True
        if fused_tn and not self._exchange_on and e.fc1_grad_bucket is not None:
            self.enable_fused_fc1_tn()
            if iter_size > 1:
                e.fc1_fused_tn = self._fused_fc1_tn_acc

    def enable_fused_fc1_tn(self):
        """Single process, bf16 mode, on top of the pipelined mode (round 4; iter_size > 1: _fused_fc1_tn_acc takes its place): the fc6 weight gradient's main
        columns - exact rounds of the persistent kernel - go through drn_gemm_tn_sgd, which applies the optimizer step of
        every tile inside the NEXT tile's mainloop of the same launch (steady HBM traffic under the MFMA work, gradient read
        back from L2, no optimizer launches for fc6 on the other stream).  The trailing columns keep the small-tile launch +
        drn_sgd_step_block.  Bit-identical to the unfused step (same bf16 rounding of the gradient, same update)."""
        if not getattr(self, "_pipelined", False):
            raise DrnError("enable_pipelined() first")
        if self._exchange_on:
            raise DrnError("the fused fc6 dW + SGD launch is a single-process schedule")
        if self.clip_type is not None:
            raise DrnError("SOLVER.CLIP_GRADIENTS: the fused fc6 dW + SGD launch has no clamp in its epilogue; the clipped "
                           "pipelined schedule runs fc6 dW unfused")
        self.engine.fc1_fused_tn = self._fused_fc1_tn

    def _fused_fc1_tn(self, dPT, A, D1, n_main, Mp, M, gw):
        e = self.engine
        if e.arena_s is None or gw.dtype != torch.bfloat16:
            return False
        if self._mom is None:
            self._mom = torch.zeros_like(e.arena_w)
        segs, _ = self._bucket_table(("fc1", 0, D1))
        o, n = e._seg["fc1.weight"]
        k1 = n // D1
        view = lambda t: t[o: o + n].view(D1, k1)[:, :n_main]
        return ops.gemm_tn_sgd(dPT, A[:, :n_main], D1, n_main, Mp, M, gw[:, :n_main], view(e.arena_w), view(self._mom),
                               view(e.arena_s), segs, self.momentum, self._steps == 0, 1.0, guard=self._gs)

    def _fused_fc1_tn_acc(self, dPT, A, D1, n_main, Mp, M, ga, gw):
        """closing micro-iteration of a window: bucket = bf16(fp32 accumulator + dW) and the update, one launch
        (drn_gemm_tn_acc_sgd); False -> the caller runs drn_gemm_tn (accumulate) + drn_cast2d + drn_sgd_step_block"""
        e = self.engine
        if e.arena_s is None or gw.dtype != torch.bfloat16:
            return False
        if self._mom is None:
            self._mom = torch.zeros_like(e.arena_w)
        segs, _ = self._bucket_table(("fc1", 0, D1))
        o, n = e._seg["fc1.weight"]
        k1 = n // D1
        view = lambda t: t[o: o + n].view(D1, k1)[:, :n_main]
        return ops.gemm_tn_acc_sgd(dPT, A[:, :n_main], D1, n_main, Mp, M, ga[:, :n_main], gw[:, :n_main], view(e.arena_w),
                                   view(self._mom), view(e.arena_s), segs, self.momentum, self._steps == 0, 1.0,
                                   guard=self._gs)

    def _fused_fc1_cols(self, dPT, A, D1, k0, k1, Kp, kb, gw):
        """K-sharded fc6: dW of the owned columns k0:k1 and their update as one launch (drn_gemm_tn_sgd; N = 2 / 4: the
        column count is a multiple of 256); False -> the caller runs the unfused pair"""
        e = self.engine
        if e.arena_s is None or gw.dtype != torch.bfloat16 or not getattr(self, "_kshard", False):
            return False
        if self._mom is None:
            self._mom = torch.zeros_like(e.arena_w)
        segs, _ = self._bucket_table(("fc1", 0, D1))
        o, n = e._seg["fc1.weight"]
        kk = n // D1
        view = lambda t: t[o: o + n].view(D1, kk)[:, k0:k1]
        ok = ops.gemm_tn_sgd(dPT, A, D1, k1 - k0, Kp, kb, gw[:, k0:k1], view(e.arena_w), view(self._mom), view(e.arena_s),
                             segs, self.momentum, self._steps == 0, 1.0 / self._dp.world)
        if ok:
            self._master_stale = True
        return ok

    def _bucket_table(self, what):
        groups = [g for g in self.param_groups if g["used"]]
        key = (what, tuple((g["lr"], g["weight_decay"]) for g in groups))
        hit = self._bucket_segs.get(what)
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        rows = []
        for g in groups:
            if what == "small" and g["name"] != "fc1.weight":
                rows.append((g["off"], g["cnt"], g["lr"], g["weight_decay"]))
            elif what != "small" and g["name"] == "fc1.weight":
                r0, r1 = what[1], what[2]
                k1 = self.model.roi_heads.box_head.fc1.weight.shape[1]
                rows.append((g["off"] + r0 * k1, (r1 - r0) * k1, g["lr"], g["weight_decay"]))
        # (out=: in place from the second time on - captured graphs keep reading this table)
        dev = ops.sgd_segments(rows, out=hit[1] if hit is not None else None, device=self.engine.arena_w.device)
        self._bucket_segs[what] = (key, dev, len(rows))
        return dev, len(rows)

    def _exchange(self, what):
        """sum one gradient bucket over the ranks (in place; on the current stream).  Returns the exchange buffer the
        optimizer must read when this bucket lives there instead of the fp32 arena."""
        e = self.engine
        bucket = e.fc1_grad_bucket if what != "small" else None
        if what[0] == "fc1b":
            return bucket  # K-sharded fc6: this rank's columns are already the sum over every rank's image
        if self._exchange_on:
            if what == "small":
                o_fc1, _ = e._seg["fc1.weight"]  # arena order: everything else precedes fc1.weight
                if self._comm_dtype == torch.bfloat16:
                    # bf16 on the wire for the small tensors too (38 -> 19 MB, the first all-reduce of every step):
                    # one cast pass into a bucket buffer; the fp32 arena keeps the local gradient
                    if getattr(self, "_small_bucket", None) is None or self._small_bucket.numel() != o_fc1:
                        self._small_bucket = torch.zeros((o_fc1,), dtype=torch.bfloat16, device=e.arena_g.device)
                    bucket = self._small_bucket
                    bucket.copy_(e.arena_g[:o_fc1])  # wire staging (torch plumbing, like the all-reduce itself)
                    dist.all_reduce(bucket, group=self._dp.group)
                else:
                    dist.all_reduce(e.arena_g[:o_fc1], group=self._dp.group)
            else:
                _, r0, r1 = what
                o, _ = e._seg["fc1.weight"]
                k1 = self.model.roi_heads.box_head.fc1.weight.shape[1]
                src = bucket[r0:r1] if bucket is not None else e.arena_g[o + r0 * k1: o + r1 * k1].view(r1 - r0, k1)
                if self._sharded:
                    # reduce-scatter: this rank receives the summed gradient of ITS rows of the slab
                    q = (r1 - r0) // self._dp.world
                    bufs = self._shard_bufs()
                    out = bufs.get(what)
                    if out is None or out.shape != (q, k1) or out.dtype != src.dtype:
                        out = bufs[what] = torch.empty((q, k1), dtype=src.dtype, device=src.device)
                    dist.reduce_scatter_tensor(out, src, group=self._dp.group)
                    return out
                dist.all_reduce(src, group=self._dp.group)
        return bucket

    def _shard_bufs(self):
        if getattr(self, "_rs_out", None) is None:
            self._rs_out = {}
        return self._rs_out

    def _own_rows(self, what):
        """rows of slab `what` = ("fc1", r0, r1) that this rank updates in the sharded exchange"""
        _, r0, r1 = what
        q = (r1 - r0) // self._dp.world
        rank = dist.get_rank(self._dp.group)
        return r0 + rank * q, r0 + (rank + 1) * q

    def _gather_rows(self, what, master_too=False):
        """all-gather the rows every rank updated: into the compute copy the next forward reads (bf16 shadow, or the fp32
        master when there is no shadow); master_too also gathers the fp32 master and the momentum (checkpoint time)"""
        e = self.engine
        _, r0, r1 = what
        a, b = self._own_rows(what)
        o, _ = e._seg["fc1.weight"]
        k1 = self.model.roi_heads.box_head.fc1.weight.shape[1]
        arenas = [e.arena_s if e.arena_s is not None else e.arena_w]
        if master_too:
            arenas = [t for t in (e.arena_w, self._mom) if t is not None]
        inplace = dist.get_backend(self._dp.group) == "nccl"  # RCCL's in-place form: input = output[rank * count ...]
        for t in arenas:
            full, mine = t[o + r0 * k1: o + r1 * k1], t[o + a * k1: o + b * k1]
            dist.all_gather_into_tensor(full, mine if inplace else mine.clone(), group=self._dp.group)

    def sync_master(self):
        """Sharded exchange, bf16 mode: every rank's fp32 master weights and momentum are current only for the rows it
        updates (the forward reads the all-gathered bf16 shadow).  Before a checkpoint / state_dict() the owners' rows
        are gathered so that every rank holds the full fp32 state again."""
        if not (getattr(self, "_sharded", False) or getattr(self, "_kshard", False)) or not self._master_stale:
            return
        self._rendezvous("sync_master() / state_dict() / DetectionCheckpointer.save()")
        if self._opt_stream is not None:
            torch.cuda.current_stream().wait_stream(self._opt_stream)
        if getattr(self, "_kshard", False):
            # K-sharded fc6: every rank owns a column block of fc1.weight (master, momentum, compute copy)
            e = self.engine
            o, n = e._seg["fc1.weight"]
            d1, k1 = self.model.roi_heads.box_head.fc1.weight.shape
            world = self._dp.world
            q = k1 // world
            rank = dist.get_rank(self._dp.group)
            for t in (e.arena_w, self._mom, e.arena_s):
                if t is None:
                    continue
                full = t[o: o + n].view(d1, k1)
                mine = full[:, rank * q: (rank + 1) * q].contiguous()
                allc = torch.empty((world, d1, q), dtype=t.dtype, device=t.device)
                dist.all_gather_into_tensor(allc.view(-1), mine.view(-1), group=self._dp.group)
                full.view(d1, world, q).copy_(allc.permute(1, 0, 2))
            self._master_stale = False
            return
        r0 = 0
        for r1 in self._slab_ends:
            self._gather_rows(("fc1", r0, r1), master_too=True)
            r0 = r1
        self._master_stale = False

    sync_timeout = 120.0  # seconds sync_master() waits for the other ranks before it raises instead of hanging

    def _rendezvous(self, what):
        """The gather of the owners' rows is a COLLECTIVE, while the reference checkpoints on rank 0 only
        (detectron2/engine/defaults.py:352 registers PeriodicCheckpointer under comm.is_main_process()).  A driver ported
        line by line would therefore block forever inside the all-gather; this one-word all-reduce is issued
        asynchronously first and polled with a deadline, so a lone caller gets a DrnError that says what to do
        (ADVICE r2).  After the error the process group is unusable - the run must stop, which is the point."""
        import time

        dev = self.engine.arena_w.device
        flag = torch.ones(1, dtype=torch.float32, device=dev)
        work = dist.all_reduce(flag, group=self._dp.group, async_op=True)
        t0 = time.monotonic()
        nccl = dist.get_backend(self._dp.group) == "nccl"
        if not nccl:
            # gloo completes some operations only inside wait() (DataParallel.selftest notes the same): a bounded wait
            # instead of polling is_completed()
            import datetime

            try:
                work.wait(timeout=datetime.timedelta(seconds=self.sync_timeout))
                return
            except Exception as ex:  # noqa: BLE001 - timeout / peer failure: the group is unusable either way
                raise DrnError("%s is a collective in the sharded exchange: the rendezvous on rank %d failed or timed out "
                               "after %.0f s (%s).  Call it on EVERY rank, or train with exchange='allreduce'"
                               % (what, dist.get_rank(self._dp.group), self.sync_timeout, ex)) from ex
        while not work.is_completed():
            if time.monotonic() - t0 > self.sync_timeout:
                raise DrnError("%s is a collective in the sharded exchange (every rank holds the fp32 master / momentum "
                               "of its own fc6 rows only): rank %d waited %.0f s for the other ranks.  Call it on EVERY "
                               "rank - DetectionCheckpointer.save() writes the file on the rank with save_to_disk only - or "
                               "call optimizer.sync_master() on all ranks right before a rank-0-only save, or train with "
                               "exchange='allreduce'" % (what, dist.get_rank(self._dp.group), self.sync_timeout))
            time.sleep(0.002)

    def _install_state_dict_hook(self):
        """Staleness lives with the model, not with whoever happens to hold the optimizer: a bare model.state_dict(), or a
        checkpointer built without the optimizer, gathers the owners' rows first (it is then a collective as well, with
        the same fail-fast rendezvous) instead of silently writing the other ranks' stale fp32 rows."""
        heads = self.model.roi_heads
        if getattr(heads, "_drn_sync_hook", None) is None:
            import weakref

            ref = weakref.ref(self)

            def hook(module, prefix, keep_vars):
                opt = module.__dict__.get("_drn_sync_owner")
                opt = opt() if opt is not None else None
                if opt is not None:
                    opt.sync_master()

            # (model.state_dict() reaches this hook when it recurses into roi_heads; the tensors it returns are views of the
            # arena, which the gather fills in place)
            heads._drn_sync_hook = heads.register_state_dict_pre_hook(hook)
            heads.__dict__["_drn_sync_owner"] = ref
        else:
            import weakref

            heads.__dict__["_drn_sync_owner"] = weakref.ref(self)

    def _on_grad_ready(self, what):
        e = self.engine
        if self._mom is None:
            self._mom = torch.zeros_like(e.arena_w)
        if what[0] == "fc1b":
            if self._exchange_on and not getattr(self, "_kshard", False):
                raise DrnError("block updates of the fc6 weight gradient are a single-process / K-sharded schedule; with a "
                               "gradient exchange the slabs are row ranges")
            # the block kernel takes the whole tensor's table entry (lr / wd on the device) + the block's bounds
            segs, nseg = self._bucket_table(("fc1", 0, self.model.roi_heads.box_head.fc1.weight.shape[0]))
        else:
            segs, nseg = self._bucket_table(what)
        world = self._dp.world if self._dp is not None else 1
        cur = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(cur)
        self._opt_stream.wait_event(ev)
        if what == "small":
            self.small_ready_event = ev  # (graphed.py: recorded behind the step's heads; the graphed step's host-side throttle waits on old ones)
        if self.iter_size > 1:
            if self._window is None:
                raise DrnError("WSL.ITER_SIZE > 1: set_window() must precede every backward (Trainer / GraphedTrainStep do)")
            if not self._window.closing:
                return  # the gradients stay in the fp32 arena; nothing for the optimizer stream
        with torch.cuda.stream(self._opt_stream):
            if what == "small":
                e.flush_colsums()  # bias gradients: second stage of their column sums, off the backward's critical path
            bucket = self._exchange(what)
            if self._exchange_on:
                evc = torch.cuda.Event()
                evc.record(self._opt_stream)
                self._deferred.append((what, bucket, segs, nseg, evc))
                return
            self._update(what, bucket, segs, nseg)
            if what == "small" and self.iter_size > 1:
                # the next window accumulates from zero (the heads' accumulate flags are always on); step() joins this stream
                e.arena_g[: e._seg["fc1.weight"][0]].zero_()

    def _update(self, what, bucket, segs, nseg):
        e = self.engine
        world = self._dp.world if self._dp is not None else 1
        clip = self._bucket_clip  # value clipping is element-wise: every bucket's launch clamps its own elements
        if what[0] == "fc1b":
            # a rectangular block of fc1.weight (the trailing columns of the fused dW launch; the K-sharded fc6's owned columns)
            _, r0, r1, c0, c1 = what
            k1 = self.model.roi_heads.box_head.fc1.weight.shape[1]
            ops.sgd_step_block(e.arena_w, self._mom, bucket if bucket is not None else e.arena_g, segs, r0, r1 - r0, c0,
                               c1 - c0, k1, self.momentum, self._steps == 0, 1.0 / world, shadow=e.arena_s,
                               grad_off=e._seg["fc1.weight"][0] if bucket is not None else 0, clip=clip, guard=self._gs)
            if getattr(self, "_kshard", False):
                self._master_stale = True  # the other ranks' columns of fc1.weight / momentum / shadow live on those ranks
            return
        if what != "small" and getattr(self, "_sharded", False) and self._exchange_on:
            # `bucket` = this rank's reduce-scattered rows: update them alone
            a, b = self._own_rows(what)
            k1 = self.model.roi_heads.box_head.fc1.weight.shape[1]
            segs, nseg = self._bucket_table(("fc1", a, b))
            ops.sgd_step(e.arena_w, self._mom, bucket, segs, nseg, self.momentum, self._steps == 0, 1.0 / world,
                         shadow=e.arena_s, grad_off=e._seg["fc1.weight"][0] + a * k1, clip=clip, guard=self._gs)
            self._master_stale = True  # momentum (and, with a bf16 shadow, the fp32 master) of the other ranks' rows
            return
        if bucket is not None:
            ops.sgd_step(e.arena_w, self._mom, bucket, segs, nseg, self.momentum, self._steps == 0, 1.0 / world,
                         shadow=e.arena_s, grad_off=0 if what == "small" else e._seg["fc1.weight"][0], clip=clip,
                         guard=self._gs)
        else:
            ops.sgd_step(e.arena_w, self._mom, e.arena_g, segs, nseg, self.momentum, self._steps == 0, 1.0 / world,
                         shadow=e.arena_s, clip=clip, guard=self._gs)
        if what == "small" and e.sh is not None:
            e.refresh_transposes()  # fc7 / predictor weights are final for this step: rebuild their K-major twins here
            e._transposes_fresh = True

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            if g.get("bb"):
                continue  # trunk gradients stay views of their arena; the next backward overwrites them
            for p in g["params"]:
                p.grad = None
        self.engine._grads_valid = False

    def step(self, grad_scale=1.0):
        e = self.engine
        if not e._grads_valid:
            raise DrnError("optimizer.step() before any backward()")
        if getattr(self, "_pipelined", False):
            cur = torch.cuda.current_stream()
            if self._deferred:
                # exchanged buckets: update each one here as soon as its all-reduce (optimizer stream) has finished
                gathered = []
                for what, bucket, segs, nseg, evc in self._deferred:
                    cur.wait_event(evc)
                    self._update(what, bucket, segs, nseg)
                    if what != "small" and what[0] != "fc1b" and getattr(self, "_sharded", False):
                        # the rows this rank just updated go to every other rank (optimizer stream: link-bound, beside
                        # the next bucket's update on this stream); the next forward waits for the last gather below
                        ev = torch.cuda.Event()
                        ev.record(cur)
                        self._opt_stream.wait_event(ev)
                        with torch.cuda.stream(self._opt_stream):
                            self._gather_rows(what)
                            g = torch.cuda.Event()
                            g.record(self._opt_stream)
                        gathered.append(g)
                for g in gathered:
                    cur.wait_event(g)
                self._deferred = []
            else:
                # every bucket was already updated on the optimizer stream during backward(): join it
                cur.wait_stream(self._opt_stream)
            self._steps += 1
            e.mark_dirty(shadow_fresh=e.arena_s is not None)
            return
        if self._mom is None:
            self._mom = torch.zeros_like(e.arena_w)
        segs, nseg = self._segs()
        ops.sgd_step(e.arena_w, self._mom, e.arena_g, segs, nseg, self.momentum, self._steps == 0, grad_scale,
                     shadow=e.arena_s, clip=self._clip(e.arena_g, segs, nseg, grad_scale, 0), guard=self._gs)
        if self._bb is not None:
            self._step_bb(grad_scale)
        self._steps += 1
        e.mark_dirty(shadow_fresh=e.arena_s is not None)

    def state_dict(self):
        """torch.optim.SGD's checkpoint content in this optimizer's flat form: the momentum arena of the heads, the
        momentum arena of a trainable trunk (FREEZE_AT < 5), the step count and the per-group hyper-parameters."""
        bb = self._bb
        self.raise_if_nonfinite()  # nonfinite="raise": a run whose loss went non-finite is not saved as healthy
        self.sync_master()  # sharded exchange: collect the rows the other ranks own
        return {"momentum_buffer": None if self._mom is None else self._mom.detach().cpu(),
                "bb_momentum_buffer": None if bb is None or bb["mom"] is None else bb["mom"].detach().cpu(),
                "steps": self._steps,
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        """Resume (detectron2/engine/defaults.py:304-319 hands the optimizer to the checkpointer).  Checkpoints are read
        with map_location='cpu': the saved momentum is COPIED into device buffers shaped like the weight arenas."""
        e = self.engine
        mom = sd.get("momentum_buffer")
        if mom is None:
            self._mom = None
        else:
            if mom.numel() != e.arena_w.numel():
                raise DrnError("optimizer checkpoint does not match this model: momentum arena of %d elements, "
                               "parameter arena of %d" % (mom.numel(), e.arena_w.numel()))
            if self._mom is None:
                self._mom = torch.zeros_like(e.arena_w)
            self._mom.copy_(mom.to(torch.float32).reshape(-1))
        bmom = sd.get("bb_momentum_buffer")
        if self._bb is not None:
            if bmom is None:
                self._bb["mom"] = None
            else:
                if bmom.numel() != self._bb["w"].numel():
                    raise DrnError("optimizer checkpoint does not match this model's trainable trunk")
                if self._bb["mom"] is None:
                    self._bb["mom"] = torch.zeros_like(self._bb["w"])
                self._bb["mom"].copy_(bmom.to(torch.float32).reshape(-1))
        elif bmom is not None:
            raise DrnError("optimizer checkpoint carries trunk momentum but this model's trunk is frozen")
        self._steps = int(sd["steps"])
        saved = sd["param_groups"]
        if len(saved) != len(self.param_groups):
            raise DrnError("optimizer checkpoint has %d parameter groups, this optimizer %d"
                           % (len(saved), len(self.param_groups)))
        for g, s in zip(self.param_groups, saved):
            if s.get("name") != g["name"]:
                raise DrnError("optimizer checkpoint group %r does not match %r" % (s.get("name"), g["name"]))
            g.update({k: v for k, v in s.items() if k in ("lr", "initial_lr", "weight_decay", "momentum")})
        self.refresh_tables()

    def refresh_tables(self):
        """Re-evaluate every per-segment (lr, weight decay) table that already lives on the device, IN PLACE: kernels
        captured into a hipGraph keep reading those buffers, so a replay follows scheduler.step() only if the tables
        are rewritten before it (GraphedTrainStep.step does this).  A table is rewritten only when an lr or weight decay in it
        changed: the rewrite is a copy from pageable memory, which holds the host until the current stream has drained - done
        on every step it kept the host of the graphed steps with the plain optimizer from ever running ahead of the device."""
        if self._segs_dev is not None:
            self._segs()
        for what in list(getattr(self, "_bucket_segs", {})):
            self._bucket_table(what)
        if self._bb is not None and self._bb["segs_dev"] is not None:
            self._segs_bb()


def build_optimizer(cfg, model, nonfinite="off"):
    """detectron2/solver/build.py:93-137, with maybe_add_gradient_clipping (:62-90) folded into the optimizer's own kernels.
    nonfinite: FusedSGD's anomaly guard ("off" / "raise" / "skip"); an argument, not a config key - the merged configs are the
    reference's."""
    clip = cfg.SOLVER.CLIP_GRADIENTS
    kw = {"nonfinite": nonfinite}
    if clip.ENABLED:
        kw.update(clip_type=clip.CLIP_TYPE, clip_value=clip.CLIP_VALUE, norm_type=clip.NORM_TYPE)
    return FusedSGD(model, cfg.SOLVER.BASE_LR, cfg.SOLVER.MOMENTUM, cfg.SOLVER.WEIGHT_DECAY, cfg.SOLVER.BIAS_LR_FACTOR,
                    cfg.SOLVER.WEIGHT_DECAY_BIAS, cfg.SOLVER.WEIGHT_DECAY_NORM, cfg.SOLVER.NESTEROV, **kw)


class WarmupMultiStepLR:
    """detectron2/solver/lr_scheduler.py:16-49 + _get_warmup_factor_at_iter :83-113."""

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=0.001, warmup_iters=1000, warmup_method="linear",
                 last_epoch=-1):
        if not list(milestones) == sorted(milestones):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(milestones))
        self.optimizer, self.milestones, self.gamma = optimizer, list(milestones), gamma
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        self.base_lrs = [g["initial_lr"] for g in optimizer.param_groups]
        self.last_epoch = last_epoch
        self.step()

    def _warm(self, it):
        if it >= self.warmup_iters:
            return 1.0
        if self.warmup_method == "constant":
            return self.warmup_factor
        alpha = it / self.warmup_iters
        return self.warmup_factor * (1 - alpha) + alpha

    def get_lr(self):
        f = self._warm(self.last_epoch)
        return [b * f * self.gamma ** bisect.bisect_right(self.milestones, self.last_epoch) for b in self.base_lrs]

    def step(self):
        self.last_epoch += 1
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g["lr"] = lr

    def state_dict(self):
        """torch.optim.lr_scheduler._LRScheduler.state_dict minus the optimizer (what the reference checkpoints)"""
        return {"milestones": list(self.milestones), "gamma": self.gamma, "warmup_factor": self.warmup_factor,
                "warmup_iters": self.warmup_iters, "warmup_method": self.warmup_method,
                "base_lrs": list(self.base_lrs), "last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        self.milestones, self.gamma = list(sd["milestones"]), sd["gamma"]
        self.warmup_factor, self.warmup_iters = sd["warmup_factor"], sd["warmup_iters"]
        self.warmup_method, self.base_lrs = sd["warmup_method"], list(sd["base_lrs"])
        self.last_epoch = sd["last_epoch"]
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g["lr"] = lr
        if hasattr(self.optimizer, "refresh_tables"):
            self.optimizer.refresh_tables()


def build_lr_scheduler(cfg, optimizer):
    assert cfg.SOLVER.LR_SCHEDULER_NAME == "WarmupMultiStepLR"
    return WarmupMultiStepLR(optimizer, cfg.SOLVER.STEPS, cfg.SOLVER.GAMMA, warmup_factor=cfg.SOLVER.WARMUP_FACTOR,
                             warmup_iters=cfg.SOLVER.WARMUP_ITERS, warmup_method=cfg.SOLVER.WARMUP_METHOD)


class DataParallel:
    """Gradient exchange of the data-parallel step.  Images shard across ranks (rank g takes elements g, g+W, ...
    of the stream, detectron2/data/samplers/distributed_sampler.py:43-45); nothing crosses GPUs in forward; per
    optimizer step the trainable gradients are summed over ranks and the SGD kernel applies 1/W (= DDP's mean).
    Buckets follow the order gradients become final in the explicit backward: [all small tensors] then the fc6
    weight gradient in `slabs` row slabs, each launched on a side stream as soon as its dW GEMM has been queued."""

    def __init__(self, model, process_group=None, slabs=4, backend_stream=True, force_exchange=False):
        self.model = model
        self.engine = model.roi_heads._engine
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        # force_exchange: run the collectives even in a 1-rank group (exercises the RCCL path on a single-GPU box)
        self.exchange = self.world > 1 or (force_exchange and dist.is_available() and dist.is_initialized())
        self.engine.fc1_grad_slabs = slabs if self.world > 1 else 1
        if self.world > 1:
            if self.engine.grad_ready_hook is not None:
                raise DrnError("the head engine already has a gradient hook (FusedSGD.enable_pipelined ran first): build "
                               "DataParallel before the optimizer's pipelined mode and pass it as enable_pipelined(dp)")
            self.engine.grad_ready_hook = self._on_ready
        # world == 1: nothing to exchange - an existing hook (the pipelined optimizer's) is left alone
        self._use_stream = backend_stream and torch.cuda.is_available()
        self._comm = None
        self._pending = []
        # DistributedDataParallel.no_sync(): with WSL.ITER_SIZE > 1 the micro-steps accumulate LOCALLY and only the last
        # backward of the window announces its buckets.  (The reference's DDP averages on every backward, which is
        # idempotent; summing an already-summed buffer again is not.)  Trainer.run_step sets this per micro-step.
        self.sync_gradients = True

    def broadcast_parameters(self, src=0):
        """DistributedDataParallel's construction-time sync (detectron2/engine/defaults.py:279-282): every parameter AND
        buffer of the module comes from rank `src` - the head arena in one piece, then the trunk's weights and FrozenBN
        statistics (they never change afterwards when frozen, but the ranks must start from the same ones)."""
        if not self.exchange:
            return
        self.engine.ensure(next(self.model.roi_heads.parameters()).device)
        dist.broadcast(self.engine.arena_w, src, group=self.group)
        lo = self.engine.arena_w.data_ptr()
        hi = lo + self.engine.arena_w.numel() * 4
        with torch.no_grad():
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                if lo <= t.data_ptr() < hi:
                    continue  # lives in the arena: already done
                dist.broadcast(t.data, src, group=self.group)
        # packed conv weights / folded FrozenBN affines cached before the broadcast are stale on the non-source ranks
        # (`.data` has its own version counter, so the keys those caches use did not move): drop them explicitly
        for m in self.model.modules():
            if hasattr(m, "invalidate_packs"):
                m.invalidate_packs()
        self.engine.mark_dirty()

    def _reduce(self, t):
        if self._use_stream and t.is_cuda:
            if self._comm is None:
                self._comm = torch.cuda.Stream()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self._comm.wait_event(ev)
            with torch.cuda.stream(self._comm):
                dist.all_reduce(t, group=self.group)
        else:
            dist.all_reduce(t, group=self.group)

    def _on_ready(self, what):
        e = self.engine
        if not self.sync_gradients:
            return  # inside an accumulation window: the gradient stays local until the window's last backward
        if what == "backbone":  # trainable trunk (FREEZE_AT < 5): its flat gradient arena, once its backward is done
            bg = getattr(self.model, "_bb_grad_arena", None)
            if bg is not None:
                self._reduce(bg)
        elif what == "small":
            o_fc1, _ = e._seg["fc1.weight"]
            self._reduce(e.arena_g[:o_fc1])  # arena order: heads, fc2, fc1.bias come before fc1.weight
        else:
            _, r0, r1 = what
            o, n = e._seg["fc1.weight"]
            k1 = self.model.roi_heads.box_head.fc1.weight.shape[1]
            self._reduce(e.arena_g[o + r0 * k1: o + r1 * k1])

    def selftest(self, buckets, iters=3, timeout=120.0, wire_dtype=torch.bfloat16):
        """Run the collectives of the training step ONCE on scratch buffers of the real bucket sizes before any warm-up:
        all-reduce of the small bucket, reduce-scatter + all-gather of every fc6 row slab (and the all-reduce form of the
        slab).  Every collective is issued asynchronously and polled against `timeout`, so a wedged RCCL bootstrap, a
        missing peer mapping (HSA_ENABLE_IPC_MODE_LEGACY) or a rank that never arrives raises a DrnError that names the
        collective and the rank instead of hanging the job.  Checks the arithmetic too (every rank
        contributes rank + 1).  Returns {collective: {"bytes", "ms", "algbw_GBps", "busbw_GBps"}} with the NCCL-tests
        bus-bandwidth convention (all-reduce 2 (N-1)/N, reduce-scatter / all-gather (N-1)/N of the buffer).
        buckets: {"small": elements, "slabs": [(rows, cols), ...], "kshard": None | {"pack_bytes", "M", "D1", "wire_dtype",
        "dp1_dtype"}}"""
        import time

        if not (dist.is_available() and dist.is_initialized()):
            raise DrnError("DataParallel.selftest needs an initialised process group")
        g, W = self.group, self.world
        rank = dist.get_rank(g)
        dev = self.engine.arena_w.device if self.engine.arena_w is not None else \
            next(self.model.roi_heads.parameters()).device
        es = torch.empty((), dtype=wire_dtype).element_size()

        polled = dist.get_backend(g) == "nccl"  # gloo completes some ops only inside wait(): use its own timeout there

        def wait(work, what):
            t0 = time.monotonic()
            if not polled:
                import datetime

                try:
                    work.wait(timeout=datetime.timedelta(seconds=timeout))
                except RuntimeError as ex:
                    raise DrnError("collective self-test: %s failed or timed out on rank %d of %d (backend %s): %s" % (
                        what, rank, W, dist.get_backend(g), ex)) from ex
                return
            while not work.is_completed():
                if time.monotonic() - t0 > timeout:
                    raise DrnError("RCCL self-test: %s did not complete within %.0f s on rank %d of %d (backend %s) - a rank "
                                   "is missing, or the peer-to-peer mapping failed (is HSA_ENABLE_IPC_MODE_LEGACY=0 set "
                                   "in every rank's environment?)" % (what, timeout, rank, W, dist.get_backend(g)))
                time.sleep(0.001)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)

        def timed(fn, what, nbytes, bus_factor):
            try:
                wait(fn(), what)  # first call: communicator setup, untimed
                t0 = time.perf_counter()
                for _ in range(iters):
                    wait(fn(), what)
                ms = (time.perf_counter() - t0) / iters * 1e3
            except RuntimeError as ex:  # torch surfaces RCCL errors as RuntimeError (DistBackendError)
                if isinstance(ex, DrnError):
                    raise
                raise DrnError("RCCL self-test: %s failed on rank %d of %d: %s" % (what, rank, W, ex)) from ex
            alg = nbytes / ms / 1e6
            return {"bytes": int(nbytes), "ms": ms, "algbw_GBps": alg, "busbw_GBps": alg * bus_factor}

        out = {}
        n = int(buckets["small"])
        small = torch.empty((n,), dtype=wire_dtype, device=dev)

        def ar_small():
            small.fill_(rank + 1.0)
            return dist.all_reduce(small, group=g, async_op=True)

        out["all_reduce small bucket"] = timed(ar_small, "all_reduce of the small bucket (%d elements)" % n, n * es, 2.0 * (W - 1) / W)
        exp = W * (W + 1) / 2.0
        if float(small[0]) != exp or float(small[-1]) != exp:
            raise DrnError("RCCL self-test: all_reduce returned %r, expected %r" % (float(small[0]), exp))
        for i, (rows, cols) in enumerate(buckets["slabs"]):
            if rows % W:
                continue  # the step falls back to the all-reduce for such a slab
            full = torch.empty((rows, cols), dtype=wire_dtype, device=dev)
            mine = torch.empty((rows // W, cols), dtype=wire_dtype, device=dev)

            def rs():
                full.fill_(rank + 1.0)
                return dist.reduce_scatter_tensor(mine, full, group=g, async_op=True)

            out["reduce_scatter fc6 slab %d" % i] = timed(rs, "reduce_scatter of fc6 slab %d [%d x %d]" % (i, rows, cols),
                                                          rows * cols * es, (W - 1.0) / W)
            if float(mine[0, 0]) != exp:
                raise DrnError("RCCL self-test: reduce_scatter returned %r, expected %r" % (float(mine[0, 0]), exp))

            def ag():
                mine.fill_(rank + 1.0)
                return dist.all_gather_into_tensor(full, mine, group=g, async_op=True)

            out["all_gather fc6 slab %d" % i] = timed(ag, "all_gather of fc6 slab %d" % i, rows * cols * es, (W - 1.0) / W)
            if float(full[rows - 1, cols - 1]) != float(W):
                raise DrnError("RCCL self-test: all_gather returned %r in the last rank's rows, expected %r" % (
                    float(full[rows - 1, cols - 1]), float(W)))
            del full, mine
        ks = buckets.get("kshard")
        if ks:
            # the K-sharded fc6's own collectives at their real sizes: all-gather of the packed feature map /
            # proposals, reduce-scatter of the partial pre-activation [N*M x D1] in the wire dtype, all-gather of dP1 [M x D1]
            nb, M, D1 = int(ks["pack_bytes"]), int(ks["M"]), int(ks["D1"])
            pk, pk_all = torch.empty((nb,), dtype=torch.uint8, device=dev), torch.empty((W, nb), dtype=torch.uint8, device=dev)

            def ag_pack():
                pk.fill_(rank + 1)
                return dist.all_gather_into_tensor(pk_all.view(-1), pk, group=g, async_op=True)

            out["all_gather feature pack (fc6_kshard)"] = timed(ag_pack, "all_gather of the packed feature map / proposals (%d bytes)" % nb,
                                                                 W * nb, (W - 1.0) / W)
            if int(pk_all[W - 1, nb - 1]) != W:
                raise DrnError("RCCL self-test: all_gather of the feature pack returned %r, expected %r" % (int(pk_all[W - 1, nb - 1]), W))
            wdt = ks.get("wire_dtype", torch.float32)
            part, h1 = torch.empty((W * M, D1), dtype=wdt, device=dev), torch.empty((M, D1), dtype=wdt, device=dev)

            def rs_h1():
                part.fill_(rank + 1.0)
                return dist.reduce_scatter_tensor(h1.view(-1), part.view(-1), group=g, async_op=True)

            out["reduce_scatter H1 partials (fc6_kshard)"] = timed(rs_h1, "reduce_scatter of the fc6 partial pre-activation [%d x %d] (%s)"
                                                                   % (W * M, D1, str(wdt).replace("torch.", "")),
                                                                   part.numel() * part.element_size(), (W - 1.0) / W)
            if float(h1[0, 0]) != exp:
                raise DrnError("RCCL self-test: reduce_scatter of H1 returned %r, expected %r" % (float(h1[0, 0]), exp))
            ddt = ks.get("dp1_dtype", torch.bfloat16)
            dp1, dp1_all = torch.empty((M, D1), dtype=ddt, device=dev), torch.empty((W, M, D1), dtype=ddt, device=dev)

            def ag_dp1():
                dp1.fill_(rank + 1.0)
                return dist.all_gather_into_tensor(dp1_all.view(-1), dp1.view(-1), group=g, async_op=True)

            out["all_gather dP1 (fc6_kshard)"] = timed(ag_dp1, "all_gather of dP1 [%d x %d]" % (M, D1),
                                                        dp1_all.numel() * dp1_all.element_size(), (W - 1.0) / W)
            if float(dp1_all[W - 1, M - 1, D1 - 1]) != float(W):
                raise DrnError("RCCL self-test: all_gather of dP1 returned %r, expected %r" % (float(dp1_all[W - 1, M - 1, D1 - 1]), float(W)))
        return out

    def finish(self):
        """make the optimizer stream wait for the exchanged gradients"""
        if self.world > 1 and self._comm is not None:
            torch.cuda.current_stream().wait_stream(self._comm)

    @property
    def grad_scale(self):
        return 1.0 / self.world


class Trainer:
    """projects/WSL/tools/train_net.py:41-117 (run_step) over detectron2/engine/train_loop.py:170-289."""

    def __init__(self, cfg, model, data_loader_iter, optimizer=None, scheduler=None, parallel=None, start_iter=0,
                 metrics_period=0, metrics_slots=256, metrics_annotated=False, metrics_max_gt=64):
        """metrics_period N > 0: every step's losses and the OICR branches' label statistics are recorded on the device
        (ROIHeads.enable_metrics, metrics.MetricsRing); every N iterations the ring is drained - a stream-ordered copy, no sync -
        and the PREVIOUS drain, long complete by then, is decoded into self.storage at the records' own iterations, with `lr`
        from the host when a scheduler is present.  flush_metrics() collects what is still under way.  0 (default): off, every
        launch as before.  More than one rank: each rank logs its own records (no cross-rank average).
        metrics_annotated: also the six un-suffixed scalars against the annotated boxes (enable_metrics(annotated=True))."""
        self.cfg, self.model = cfg, model
        self._it = data_loader_iter
        self.optimizer = optimizer or build_optimizer(cfg, model)
        self.scheduler = scheduler
        self.dp = parallel or DataParallel(model)
        self.iter_size = cfg.WSL.ITER_SIZE
        if getattr(self.optimizer, "_pipelined", False) and self.optimizer.iter_size != self.iter_size:
            raise DrnError("the pipelined optimizer updates each bucket during backward: its iter_size (%d) must equal "
                           "WSL.ITER_SIZE (%d) - enable_pipelined(iter_size=cfg.WSL.ITER_SIZE)"
                           % (self.optimizer.iter_size, self.iter_size))
        # resume: `start_iter` = checkpoint["iteration"] + 1 (DefaultTrainer.resume_or_load, defaults.py:304-319)
        self.iter = self.start_iter = int(start_iter)
        self.storage = EventStorage(self.start_iter)
        self.last_losses = None
        self._guard = getattr(self.optimizer, "_guard", None)
        if self._guard is not None:
            if getattr(self.dp, "exchange", False):
                self.optimizer._refuse_guard_multi_rank("a gradient exchange")
            self._anchor_guard()
        self.metrics_period = int(metrics_period)
        self.metrics, self._lr_log = None, {}
        if self.metrics_period > 0:
            if self.metrics_period > metrics_slots:
                raise DrnError("metrics_period %d exceeds the ring's %d slots: records would be lost between drains"
                               % (self.metrics_period, metrics_slots))
            if metrics_annotated:
                self.metrics = model.roi_heads.enable_metrics(metrics_slots, annotated=True, max_gt=metrics_max_gt)
            else:
                self.metrics = model.roi_heads.enable_metrics(metrics_slots)
            self.metrics.iter0 = self.iter

    def _feed_metrics(self, wait):
        """decode the last drain into the storage (wait: synchronise its event - and nothing else - first)"""
        recs, lost = self.metrics.collect(wait=wait)
        for it, scalars in recs:
            if it in self._lr_log:
                scalars = dict(scalars, lr=self._lr_log.pop(it))
            for k, v in scalars.items():
                self.storage.put_scalar_at(k, v, it, smoothing_hint=k != "lr")
        return lost

    def flush_metrics(self):
        """drain now and wait for that one copy: everything recorded so far is in self.storage afterwards.  Returns the
        number of records lost (overwritten in the ring before a drain reached them).  A CSC head's weight statistics
        (CSCROIHeads.enable_csc_stats) are flushed as well: CscStats.flush() drains the open period and waits for its copy."""
        stats = getattr(getattr(getattr(self.model, "roi_heads", None), "_engine", None), "csc_stats", None)
        if stats is not None:
            stats.flush()
        if self.metrics is None:
            return 0
        lost = self._feed_metrics(True)
        self.metrics.drain()
        return lost + self._feed_metrics(True)

    def _anchor_guard(self):
        """the guard counts checks; the next one is iteration self.iter"""
        self._guard.iter0 = self.iter - self._guard.read()["calls"]

    def resume_or_load(self, checkpointer, path="", resume=True):
        """DefaultTrainer.resume_or_load (detectron2/engine/defaults.py:304-319): load `path` or, with resume=True and a
        last_checkpoint in the checkpointer's directory, that checkpoint including optimizer / scheduler state; training
        continues at the iteration after the saved one."""
        extra = checkpointer.resume_or_load(path, resume=resume) or {}
        if resume and checkpointer.has_checkpoint():
            self.iter = self.start_iter = int(extra.get("iteration", -1)) + 1
            self.storage = EventStorage(self.start_iter)
            if self._guard is not None:
                self._anchor_guard()
            if self.metrics is not None:
                self.metrics.iter0 = self.iter - int(self.metrics.state[0])
        return extra

    def run_step(self):
        assert self.model.training, "[Trainer] model was changed to eval mode!"
        def draw():
            while True:  # train_net.py:74-81: re-draw batches that contain an image without GT
                d = next(self._it)
                if all(len(x["instances"]) > 0 for x in d):
                    return d

        data = self._lookahead if getattr(self, "_lookahead", None) is not None else draw()
        self._lookahead = draw()
        if self._guard is not None:  # the check is issued behind the loss tail, inside the forward
            self._guard.window_first = window_position(self.iter, self.iter_size, self.start_iter).first
        with self.storage:
            loss_dict = self.model(data)
        if hasattr(self.model, "prefetch_features"):
            # frozen backbone + pooling of the NEXT batch on a side stream, issued between this batch's forward and its
            # backward: the trunk then runs beside the backward's GEMMs and the optimizer pass.  Issued in front of the
            # forward (round 1) it ran beside the fc6 forward GEMM and its activations interleaved with the forward's in
            # the caching allocator: measured on VOC-like shapes 2.78 vs 2.25 ms per step over 16 rotating shapes, 3.61
            # vs 2.81 ms at 1000x1464 (tools/eager_shapes_bench.py, tools/eager_one_shape.py, profiles/r2_15_*)
            self.model.prefetch_features(self._lookahead)
        if self.iter == self.start_iter:
            self.optimizer.zero_grad()
        last_micro = self.iter % self.iter_size == 0  # train_net.py:105: the optimizer steps on these iterations
        self.dp.sync_gradients = last_micro           # DDP no_sync() for the other micro-steps of the window
        if self.iter_size > 1 and getattr(self.optimizer, "_pipelined", False):
            self.optimizer.set_window(window_position(self.iter, self.iter_size, self.start_iter))
        if not (hasattr(self.model, "backward_losses") and self.model.backward_losses(1.0 / self.iter_size)):
            (sum(loss_dict.values()) / self.iter_size).backward()  # train_net.py:100-107; the line above = the same without autograd
        if last_micro:
            self.dp.finish()
            self.optimizer.step(self.dp.grad_scale)
            self.optimizer.zero_grad()
        if self.metrics is not None:
            if self.scheduler is not None:  # hooks.LRScheduler.after_step (hooks.py:228-231): the lr this iteration ran with, of
                # the largest parameter group
                self._lr_log[self.iter] = max(self.optimizer.param_groups, key=lambda g: g["cnt"])["lr"]
            if (self.iter - self.start_iter + 1) % self.metrics_period == 0:
                self._feed_metrics(True)  # the previous drain: metrics_period steps old
                self.metrics.drain()
        if self.scheduler is not None:
            # hooks.LRScheduler.after_step (detectron2/engine/hooks.py:232-235) runs after EVERY iteration: SOLVER.STEPS,
            # WARMUP_ITERS and MAX_ITER count micro-iterations also when WSL.ITER_SIZE > 1
            self.scheduler.step()
        self.last_losses = loss_dict  # device scalars; float() them only when you need to look (no per-iter sync)
        self.iter += 1
        self.storage.step()
        return loss_dict

    def check_finite(self):
        """SimpleTrainer._detect_anomaly (train_loop.py:252-258), on demand instead of every iteration.  With the optimizer's
        anomaly guard on (FusedSGD(nonfinite=...)) the device state is read instead of the last losses: "raise" raises the
        reference's message with the FIRST bad iteration (whose update, and every later one, was skipped); "skip" never raises.
        Returns the guard's state (None with the guard off)."""
        if self._guard is not None:
            return self.optimizer.raise_if_nonfinite()
        if self.last_losses is not None:
            tot = float(sum(v.detach() for v in self.last_losses.values()))
            if not math.isfinite(tot):
                raise FloatingPointError("Loss became infinite or NaN at iteration={}!".format(self.iter))


from .graphed import GraphedFullStep, GraphedTrainStep  # noqa: E402,F401  (the step objects live in graphed.py)
