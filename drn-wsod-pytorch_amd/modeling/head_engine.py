"""The fused schedule of the DAN / WSDDN / OICR / PCL / CSC heads (`_HeadEngine`) and its autograd hook (`_TrainFn`).

One engine per OICRROIHeads module: the flat parameter arena shared with the fused SGD kernel and the gradient exchange, the
compute-dtype shadows of the weights, the activation workspaces, the two fc6 operand sets per (dtype, training)
(`_OperandSets`), one forward trunk (fc6, fc7, all predictor Linears as three MFMA GEMM groups) with one loss tail per head
family, and the explicit backward down to the fc6 weight-gradient tail.  No host synchronisation happens inside a step.

The engine's state is closed: `__slots__` names every attribute, `__init__` gives each its default and says who sets it.  A
misspelt switch (bench.py --engine-opt, a tool, a test) is an AttributeError instead of a new attribute that changes nothing."""
import math
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist

from .. import ops
from .._cabi import DrnError

# Counter-based dropout of the training step (drn_drop_rule, csrc/drn_common.h): fc6 draws its mask with seed + counter,
# fc7 with seed + FC7_SEED_OFFSET + counter, and the logits pass advances the device-side counter by DROP_COUNTER_STEP.
# (The two are the same number, so fc7's mask of one step is fc6's mask of the next wherever both layers have the same
# width; changing either changes every step's masks.)
FC7_SEED_OFFSET = 0x9E3779B1
DROP_COUNTER_STEP = 0x9E3779B1


def dropout_seeds(seed):
    """(fc6 seed, fc7 seed) of one training step; the device-side counter is added to both inside the kernels"""
    return seed, seed + FC7_SEED_OFFSET


class _TrainFn(torch.autograd.Function):
    """Hooks the fused schedule into autograd: `sum(loss_dict.values()).backward()` (the reference trainer,
    projects/WSL/tools/train_net.py:92-107) lands here with one upstream gradient per loss."""

    @staticmethod
    def forward(ctx, anchor, engine, state):
        ctx.engine, ctx.state = engine, state
        return tuple(state["loss_list"])

    @staticmethod
    def backward(ctx, *gouts):
        ctx.engine.backward(ctx.state, gouts)
        return None, None, None


class _Fc1Tail(NamedTuple):
    """what backward() hands run_fc1_tail(): the operands and shape of the fc6 weight gradient dW = dP1^T . A"""
    dP1T: torch.Tensor              # [D1, kpad(M)]
    AT: Optional[torch.Tensor]      # [K1, kpad(M)]: rows from at_row0 on were written by the pooling launch
    D1: int
    K1: int
    Mp: int
    acc: bool
    A: torch.Tensor                 # [M, kpad(K1)]
    M: int
    at_row0: int


class _Step(NamedTuple):
    """what the forward trunk of a training step hands its loss tail and _finish()"""
    w: dict                         # workspace views of this batch (+ A, AT, AT_row0)
    col: dict                       # predictor name -> first logits column
    M: int
    dtype: torch.dtype
    masks: Optional[list]
    drop_p: float
    gt: dict
    img_off: torch.Tensor
    n_img: int
    logit_part: Optional[torch.Tensor]  # split-K partials of the predictor GEMM: the fused MIL + OICR tail reduces them
    logit_seed: int
    seed_dev: Optional[torch.Tensor]
    fg_hook: Optional[object]       # feature_grad_hook (trainable backbone)
    fg: Optional[dict]              # what the gradient of the feature map needs (trainable backbone, CSC)


class _OperandSets:
    """The two fc6 operand sets of one (dtype, training): A [cap, kpad(K1)] (+ A^T [K1, kpad(cap)] when training), so that the
    NEXT batch can be pooled on a side stream while the current batch's forward / backward still reads its own set.  A set is
    'pending' from its prefetch until a forward consumes it, 'current' from then until the next forward; a new batch never
    takes a pending set, and takes the current one only when no set is free AND the current batch's backward has been issued
    (the trainer's order: prefetch of batch t+1 in front of forward t).  Allocation is for a capacity (the largest M seen,
    rounded up to 64; grow-only) and the sets hand out views.  One object per key: an inference pass between two training steps
    (EvalHook) never replaces - i.e. frees - the training sets, whose addresses a captured heads graph and the eagerly issued
    pooling piece of GraphedTrainStep both hold."""

    __slots__ = ("key", "sets", "cap", "current_done")

    def __init__(self, key):
        self.key = key            # (dtype, training)
        self.sets = None          # two dicts: A_buf, AT_buf, state, M and the views A, AT of the batch they hold
        self.cap = 0
        self.current_done = True  # the last reader of the current batch's A^T (run_fc1_tail) has been issued

    def reserve(self, M, K1, device, pinned):
        """make room for M proposals; `pinned`: a captured step holds the addresses, so growing is refused"""
        if self.sets is not None and M <= self.cap:
            return
        if pinned and self.sets is not None:
            raise DrnError("the fc6 operand sets of %s are pinned by a captured step (GraphedTrainStep) and cannot "
                           "grow from %d to %d proposals" % (self.key, self.cap, M))
        dtype, training = self.key
        cap = (M + 63) // 64 * 64
        z = lambda r_, c_: torch.zeros((r_, c_), dtype=dtype, device=device)
        self.sets = [dict(A_buf=z(cap, ops.kpad(K1, dtype)), AT_buf=z(K1, ops.kpad(cap, dtype)) if training else None,
                          state="free", M=None) for _ in range(2)]
        self.cap = cap
        self.current_done = True

    def take(self, M, slot=None, prefetch=False):
        """the set the batch of M proposals is pooled into (`slot` pins the choice: GraphedTrainStep), with its views"""
        dtype, training = self.key
        if slot is None:
            free = [i for i, q in enumerate(self.sets) if q["state"] == "free"]
            cur = [i for i, q in enumerate(self.sets) if q["state"] == "current"]
            if free:
                slot = free[0]
            elif cur and (not training or self.current_done):
                slot = cur[0]
            else:
                raise DrnError("no free fc6-operand buffer set: at most one batch can be pooled ahead of the one in flight")
        s = self.sets[slot]
        if s["M"] != M:
            Mp = ops.kpad(M, dtype)
            s["A"] = s["A_buf"][:M]
            s["AT"] = s["AT_buf"][:, :Mp] if s["AT_buf"] is not None else None
            if s["AT"] is not None and Mp > M and s["M"] is not None:
                s["AT_buf"][:, M:Mp].zero_()  # K-role pad of the dW GEMM: never a previous batch's columns
            s["M"] = M
        if prefetch:
            s["state"] = "pending"
        else:
            self.mark_current(s)
        return s

    def owns(self, s):
        return self.sets is not None and any(q is s for q in self.sets)

    def mark_current(self, s):
        """a forward consumes `s`: the set of the batch before it is free again"""
        for q in self.sets:
            if q["state"] == "current" and q is not s:
                q["state"] = "free"
        s["state"] = "current"
        self.current_done = False


class _HeadEngine:
    """Flat parameter arena + the fused fwd/bwd kernel schedule of the DAN / WSDDN / OICR heads."""

    __slots__ = (
        "h", "anchor",
        # switches for A/B runs
        "fc1_tn", "fused_fc7_fwd", "fused_loss_tail", "fused_pred_dx", "fc7_dx_split", "fc7_bwd_pair", "fc7_pair_dx_splits",
        "fc1_joint_peel", "fc1_fused_all", "fc1_grad_slabs", "fc1_slab_ends",
        # what other objects install
        "grad_ready_hook", "feature_grad_hook", "loss_guard", "metrics", "csc_stats", "fc1_fused_tn", "fc1_fused_cols", "fc1_grad_bucket",
        "kshard", "accum_window", "accum_small", "defer_colsum", "defer_fc1_tail", "pcl_image_batches", "pool_sets_pinned",
        "pool_sets_pin_owner", "captured_by",
        # layout made by ensure()
        "arena_w", "arena_g", "segments", "cols", "NH", "_seg", "_fc1_off",
        # caches and per-step hand-overs
        "sh", "arena_s", "_shadow_key", "_dirty", "_shadow_from_sgd", "_transposes_fresh", "_ws", "_pools", "seed_dev",
        "_scale_vecs", "_colidx", "_colidx_key", "_w1t", "_dA", "_w1t_key", "_pending_colsum", "_tail", "_tail_w",
        "_last_state", "_grads_valid", "_ncu")

    _tn_ok = None  # drn_gemm_tn's first-use self-check (_tn_selfcheck): once per process, so on the class

    def __init__(self, heads):
        self.h = heads
        self.anchor = None               # scalar leaf the losses hang on in autograd (made by ensure())
        # ---- switches for A/B runs (bench.py flags / --engine-opt, tools/, tests); the defaults are the shipped path ----
        self.fc1_tn = True               # bf16: fc6 dW = dP1^T . A through drn_gemm_tn (no materialised A^T); False: NT form on A^T
        self.fused_fc7_fwd = True        # fc7 GEMM + bias + ReLU + dropout + transposed copy as one launch (drn_linear_act_fwd)
        self.fused_loss_tail = True      # predictor reduce + bias, WSDDN and the OICR cascade in six launches (drn_mil_oicr_losses)
        self.fused_pred_dx = True        # predictor dX + fc7's activation backward as one launch (drn_gemm_nt_act_bwd)
        self.fc7_dx_split = True         # split K of the fc7 dX GEMM like the forward GEMMs
        self.fc7_bwd_pair = True         # fc7 dW and fc7 dX as ONE persistent launch (drn_gemm_nt_pair)
        self.fc7_pair_dx_splits = 0      # K-splits of the dX half of that launch; 0: as many as fill half the CUs
        self.fc1_joint_peel = 1          # one small-tile launch peels the trailing fc6 dW columns of all row slabs
        self.fc1_fused_all = 1           # the trailing tile columns ride in the fused dW + SGD launch as a partial last round
        self.fc1_grad_slabs = 1          # row slabs of the fc6 dW (DataParallel: one exchange bucket each)
        self.fc1_slab_ends = None        # explicit slab ends in rows (FusedSGD.enable_pipelined); None: fc1_grad_slabs equal ones
        # ---- what other objects install ----
        self.grad_ready_hook = None      # FusedSGD.enable_pipelined / DataParallel: called per finished gradient bucket
        self.feature_grad_hook = None    # GeneralizedRCNNWSL.forward / GraphedFullStep: takes the feature-map gradient (FREEZE_AT < 5)
        self.loss_guard = None           # FusedSGD(nonfinite=...): the LossGuard whose check follows the loss tail
        self.metrics = None              # ROIHeads.enable_metrics / disable_metrics: the MetricsRing
        self.csc_stats = None            # CSCROIHeads.enable_csc_stats / disable_csc_stats: the metrics.CscStats
        self.fc1_fused_tn = None         # FusedSGD.enable_pipelined / enable_fused_fc1_tn: fc6 dW + SGD as one launch
        self.fc1_fused_cols = None       # FusedSGD.enable_pipelined(exchange="fc6_kshard"): the same for the owned columns
        self.fc1_grad_bucket = None      # FusedSGD.enable_pipelined: [D1, K1] bf16 exchange buffer instead of the arena
        self.kshard = None               # FusedSGD.enable_pipelined(exchange="fc6_kshard"): dict(group, world, rank, wire, sync)
        self.accum_window = None         # FusedSGD.set_window: engine.Window of the next backward (WSL.ITER_SIZE > 1)
        self.accum_small = False         # FusedSGD.enable_pipelined(iter_size > 1): the small tensors always accumulate
        self.defer_colsum = False        # FusedSGD.enable_pipelined(iter_size = 1): bias column sums finish on the optimizer stream
        self.defer_fc1_tail = False      # GraphedTrainStep(split_tail) / GraphedFullStep / bench.py: the step calls run_fc1_tail itself
        self.pcl_image_batches = False   # PCLROIHeads.enable_image_batches
        self.pool_sets_pinned = None     # GraphedTrainStep._check_pooled: key of the operand sets its graphs hold
        self.pool_sets_pin_owner = None  # GraphedTrainStep._check_pooled: weakref to that step
        self.captured_by = None          # graphed steps (_mark_captured): weakref to the step whose graphs hold the launch sequence
        # ---- layout made by ensure() (cols, NH, _seg and _fc1_off stay unset until it has run: bench.py asks hasattr(_seg)) ----
        self.arena_w = None
        self.arena_g = None
        self.segments = []               # (name, param, offset, numel, used)
        # ---- caches and per-step hand-overs ----
        self.sh = None                   # compute-dtype shadows of the weights (refresh_shadows)
        self.arena_s = None              # bf16 shadow of the arena (same flat layout), refreshed by the fused SGD kernel
        self._shadow_key = None
        self._dirty = True
        self._shadow_from_sgd = False
        self._transposes_fresh = False   # FusedSGD._update: refresh_transposes() already ran behind the small-tensor update
        self._ws = {}                    # (dtype, training) -> workspaces (ws)
        self._pools = {}                 # (dtype, training) -> _OperandSets (pool)
        self.seed_dev = None             # device-side dropout counter
        self._scale_vecs = {}            # (losses, value, device) -> upstream-gradient vector (backward)
        self._colidx = None
        self._colidx_key = None
        self._w1t = None                 # K-major copy of W1 and the fc6 dX (trainable backbone, CSC)
        self._dA = None
        self._w1t_key = None
        self._pending_colsum = ()        # deferred bias column sums of the last backward (flush_colsums)
        self._tail = None                # _Fc1Tail of the last backward (run_fc1_tail)
        self._tail_w = None
        self._last_state = None          # state of the last training forward (GeneralizedRCNNWSL.backward_losses consumes it)
        self._grads_valid = False        # FusedSGD.zero_grad clears it
        self._ncu = None

    # ---- layout --------------------------------------------------------------------------------
    def _layout(self):
        h = self.h
        K = h.num_classes
        cols, off = [], 0
        cols.append(("cls", h.box_predictor.cls, off, K)); off += K
        cols.append(("det", h.box_predictor.det, off, K)); off += K
        for k in range(h.refine_K):
            cols.append(("r%d" % k, h.box_refinery[k].cls_score, off, K + 1)); off += K + 1
        for k in range(h.refine_K):
            if h.refine_reg[k]:
                cols.append(("b%d" % k, h.box_refinery[k].bbox_pred, off, 4 * K)); off += 4 * K
        return cols, off

    def ensure(self, device):
        h = self.h
        fc1 = h.box_head.fc1
        if (self.arena_w is not None and self.arena_w.device == device and
                fc1.weight.data_ptr() == self.arena_w.data_ptr() + 4 * self._fc1_off):
            return
        cols, NH = self._layout()
        self.cols, self.NH = cols, NH
        order = [(n + ".weight", m.weight, True) for n, m, _, _ in cols]
        order += [(n + ".bias", m.bias, True) for n, m, _, _ in cols]
        order += [("fc2.weight", h.box_head.fc2.weight, True), ("fc2.bias", h.box_head.fc2.bias, True),
                  ("fc1.bias", fc1.bias, True), ("fc1.weight", fc1.weight, True)]
        for k in range(h.refine_K):
            if not h.refine_reg[k]:  # unused parameters: kept in the arena, never touched
                order += [("u%d.weight" % k, h.box_refinery[k].bbox_pred.weight, False),
                          ("u%d.bias" % k, h.box_refinery[k].bbox_pred.bias, False)]
        # the concatenated head weights / biases must stay contiguous (they are ONE GEMM operand); every other
        # segment starts on a 64-element boundary = one 128-byte line of the bf16 shadow arena (256 B of the fp32 one):
        # the GEMMs fetch operands in 128-byte K-slabs per row, and a row that starts mid-line makes every slab straddle
        # two lines (measured on the fc6 forward GEMM: 392 us with a 16-byte aligned W1 vs 340 us line-aligned)
        contiguous = {n + ".weight" for n, _, _, _ in cols[1:]} | {n + ".bias" for n, _, _, _ in cols[1:]}
        offs, off = [], 0
        for name, p, used in order:
            if name not in contiguous:
                off = (off + 63) // 64 * 64
            offs.append(off)
            off += p.numel()
        total = (off + 63) // 64 * 64
        w = torch.zeros((total,), dtype=torch.float32, device=device)
        g = torch.zeros((total,), dtype=torch.float32, device=device)
        self.segments = []
        for (name, p, used), off in zip(order, offs):
            n = p.numel()
            w[off: off + n].copy_(p.detach().reshape(-1).to(device))
            p.data = w[off: off + n].view(p.shape)
            p.grad = None
            self.segments.append((name, p, off, n, used))
            if name == "fc1.weight":
                self._fc1_off = off
        self.arena_s = None
        self._shadow_from_sgd = False
        self.arena_w, self.arena_g = w, g
        self._seg = {name: (o, n) for name, _, o, n, _ in self.segments}
        self._dirty = True
        self._ws = {}
        self._grads_valid = False
        self.anchor = torch.zeros((), device=device, requires_grad=True)

    def _gview(self, name, shape=None):
        o, n = self._seg[name]
        v = self.arena_g[o: o + n]
        return v.view(shape) if shape is not None else v

    def mark_dirty(self, shadow_fresh=False):
        """weights changed; shadow_fresh: the fused SGD kernel already rewrote the flat bf16 shadow"""
        self._dirty = True
        self._shadow_from_sgd = shadow_fresh

    def refresh_transposes(self):
        """K-major twins of fc7 / predictor weights for the dX GEMMs.  The pipelined optimizer calls this on its own
        stream right behind the small-tensor SGD bucket (under the fc6 dW GEMMs) and sets `_transposes_fresh`, which
        takes the two launches off the front of the next forward."""
        h, sh = self.h, self.sh
        fc1, fc2 = h.box_head.fc1, h.box_head.fc2
        D1, D2, NH = fc1.weight.shape[0], fc2.weight.shape[0], self.NH
        o, _ = self._seg[self.cols[0][0] + ".weight"]
        # a shadow that is a view of the flat compute-dtype arena is refreshed by the SGD kernel itself (or by
        # refresh_shadows just before this call): transposing IT is a bf16 -> bf16 copy with 16-B accesses (~10 us)
        # instead of a scalar fp32 -> bf16 pass over the master weights (100 us beside the dW GEMM, on the optimizer
        # stream's chain small SGD -> transposes -> fc6 SGD slabs that ends the step)
        src2 = fc2.weight.data if sh.get("W2_own", True) else sh["W2"]
        srch = self.arena_w[o: o + NH * D2].view(NH, D2) if sh.get("Wh_own", True) else sh["Wh"]
        ops.transpose2d(src2, D2, D1, out=sh["W2T"])
        ops.transpose2d(srch, NH, D2, out=sh["WhT"])

    # ---- compute-dtype shadows of the weights -----------------------------------------------------
    def refresh_shadows(self, dtype):
        key = (dtype,) + tuple(p._version for _, p, _, _, u in self.segments if u)
        if not self._dirty and key == self._shadow_key:
            return
        h = self.h
        dev = self.arena_w.device
        fc1, fc2 = h.box_head.fc1, h.box_head.fc2
        D1, K1 = fc1.weight.shape
        D2 = fc2.weight.shape[0]
        NH = self.NH
        kp = lambda k: ops.kpad(k, dtype)
        o, _ = self._seg[self.cols[0][0] + ".weight"]
        wh = self.arena_w[o: o + NH * D2].view(NH, D2)
        if self.sh is None or self.sh.get("dtype") != dtype:
            z = lambda r, c: torch.zeros((r, c), dtype=dtype, device=dev)
            self.sh = dict(dtype=dtype, W2T=z(D1, kp(D2)), WhT=z(D2, kp(NH)))
            # operands whose padded layout equals the master layout live in the flat shadow arena (bf16) or ARE the
            # master (fp32); only padded ones get their own buffer
            self.arena_s = torch.zeros_like(self.arena_w, dtype=torch.bfloat16) if dtype == torch.bfloat16 else None
            self._shadow_from_sgd = False
            flat = self.arena_s if dtype == torch.bfloat16 else self.arena_w
            for nm, pnt, rows, cols_ in (("W1", fc1.weight, D1, K1), ("W2", fc2.weight, D2, D1), ("Wh", wh, NH, D2)):
                if kp(cols_) == cols_:
                    so = (pnt.data_ptr() - self.arena_w.data_ptr()) // 4
                    self.sh[nm], self.sh[nm + "_own"] = flat[so: so + rows * cols_].view(rows, cols_), False
                else:
                    self.sh[nm], self.sh[nm + "_own"] = z(rows, kp(cols_)), True
        sh = self.sh
        for nm, src, rows, cols_ in (("W1", fc1.weight.data, D1, K1), ("W2", fc2.weight.data, D2, D1), ("Wh", wh, NH, D2)):
            if sh[nm + "_own"] or (dtype == torch.bfloat16 and not self._shadow_from_sgd):
                ops.cast2d(src, rows, cols_, sh[nm])
        sh["W1v"] = sh["W1"]
        if not self._transposes_fresh:
            self.refresh_transposes()
        self._transposes_fresh = False
        self._shadow_key, self._dirty, self._shadow_from_sgd = key, False, False

    # ---- workspaces ---------------------------------------------------------------------------------
    def ws(self, M, dtype, training):
        """Activation / gradient workspaces for M proposals.  The buffers are allocated for a CAPACITY (the largest M seen,
        rounded up to 64; grow-only) and handed out as views for the M of this batch: real data has another proposal count
        every step, and re-allocating (and zero-filling) ~150 MB of workspaces per step made the eager step allocator-
        bound.  K-role buffers - the transposed twins, whose columns M .. kpad(M) are read by a GEMM as zero padding -
        get that pad re-zeroed whenever M changes (a narrow strided fill), so a view never shows a previous batch's
        columns."""
        key = (dtype, training)
        base = self._ws.get(key)
        kp = lambda k: ops.kpad(k, dtype)
        if base is None or M > base["cap"]:
            h = self.h
            dev = self.arena_w.device
            D1, K1 = h.box_head.fc1.weight.shape
            D2 = h.box_head.fc2.weight.shape[0]
            cap = (M + 63) // 64 * 64
            z = lambda r, c, dt=dtype: torch.zeros((r, c), dtype=dt, device=dev)
            NHp = kp(self.NH)
            b = dict(H1=z(cap, kp(D1)), H2=z(cap, kp(D2)), logits=z(cap, NHp, torch.float32))
            if training:
                Cp = kp(cap)
                b.update(H1T=z(D1, Cp), H2T=z(D2, Cp), dlogits=z(cap, NHp, torch.float32), dS=z(cap, NHp),
                         dST=z(self.NH, Cp), dH2=z(cap, D2, torch.float32), dP2=z(cap, kp(D2)), dP2T=z(D2, Cp),
                         dH1=torch.zeros((1, cap, D1), dtype=torch.float32, device=dev), dP1T=z(D1, Cp),
                         colpart=z((cap + 63) // 64, max(D1, D2, self.NH), torch.float32),
                         # one scratch per layer for the deferred mode (the three reductions then run later, together)
                         colpart3=[z((cap + 63) // 64, n_, torch.float32) for n_ in (self.NH, D2, D1)])
            base = self._ws[key] = dict(cap=cap, bufs=b, M=None, views=None)
        if base["M"] != M:
            b, Mp = base["bufs"], kp(M)
            v = {}
            for name, t in b.items():
                if name in self._WS_T:          # [X, kpad(cap)] transposed twins: columns of this batch + zero pad
                    v[name] = t[:, :Mp]
                    if Mp > M and base["M"] is not None:
                        t[:, M:Mp].zero_()
                elif name == "dH1":             # [splits, cap, D1]
                    v[name] = t[:, :M]
                elif name == "colpart":
                    v[name] = t[: (M + 63) // 64]
                elif name == "colpart3":
                    v[name] = [c[: (M + 63) // 64] for c in t]
                else:                           # [cap, X] row-major
                    v[name] = t[:M]
            base["M"], base["views"] = M, v
        return base["views"]

    _WS_T = ("H1T", "H2T", "dST", "dP2T", "dP1T")

    # ---- fc6 operand: pooled proposals ------------------------------------------------------------------
    def pool(self, feat_nhwc, rois, objectness, training, slot=None, want_argmax=False, prefetch=False):
        """ROIPool/ROIAlign fused with the objectness scaling -> fc6 operand A [M, C*P*P] (+ A^T for the dW GEMM when
        training), into one of the two buffer sets of this (dtype, training) (_OperandSets), so that the NEXT batch can be
        pooled on a side stream (prefetch=True) while the current batch's forward/backward still reads its own set.
        `slot` pins the set (GraphedTrainStep)."""
        h = self.h
        dev, dtype = feat_nhwc.device, feat_nhwc.dtype
        self.ensure(dev)
        M = rois.shape[0]
        D1, K1 = h.box_head.fc1.weight.shape
        key = (dtype, training)
        sets = self._pools.get(key)
        if sets is None:
            sets = self._pools[key] = _OperandSets(key)
        own = self.pool_sets_pin_owner
        sets.reserve(M, K1, dev, pinned=self.pool_sets_pinned == key and (own is None or own() is not None))
        s = sets.take(M, slot, prefetch)
        ka = h.box_pooler.kernel_args()
        # round 3: in the bf16 mode the fc6 weight gradient reads A itself (drn_gemm_tn); of A^T only the rows of the columns
        # its tail-balancing launch peels off are still needed (run_fc1_tail) - the pooling launch skips the rest
        s["t_row0"] = self._fc1_tail_row0(dtype, D1, K1) if s["AT"] is not None else 0
        pp = ka["P"] * ka["P"] if "P" in ka else 49
        res = ops.roi_pool_nhwc(feat_nhwc, rois, objectness, out=s["A"], out_t=s["AT"],
                                want_argmax=want_argmax and ka["mode"] == 0, t_first_channel=s["t_row0"] // pp, **ka)
        s["argmax"] = res[1] if (want_argmax and ka["mode"] == 0) else None
        return s

    def _mark_current(self, s):
        """a prefetched set is consumed by this forward"""
        for sets in self._pools.values():
            if sets.owns(s):
                sets.mark_current(s)

    # ---- fc6 weight gradient: row slabs, tail balancing, TN operand -------------------------------------------------
    def _fc1_slabs(self, D1):
        ends = self.fc1_slab_ends
        if ends is None:
            nslab = self.fc1_grad_slabs
            rows = (D1 + nslab - 1) // nslab
            ends = [min(D1, (s_ + 1) * rows) for s_ in range(nslab)]
        return [(a, b) for a, b in zip([0] + list(ends[:-1]), ends) if a < b]

    def _fc1_use_tn(self, dtype):
        return (self.fc1_tn and dtype == torch.bfloat16
                and self._tn_selfcheck())

    @classmethod
    def _tn_selfcheck(cls):
        """First use, once per process: drn_gemm_tn's transposing LDS reads are inline asm with hand-counted
        `lgkmcnt` waits that the compiler does not see; another hipcc version or register allocation could read a fragment
        before it has landed and produce silently wrong gradients.  One small TN launch (the persistent ping-pong kernel:
        288 tiles, ragged K rows) against drn_gemm_nt on the materialised transpose - bit-identical by construction -
        decides whether the TN form is used; on a mismatch the NT form on A^T takes over, loudly."""
        if cls._tn_ok is None:
            if torch.cuda.is_current_stream_capturing():
                return True  # decided by the eager priming step that precedes every capture
            g = torch.Generator(device="cpu").manual_seed(11)
            M, N, K, kb = 2304, 2048, 192, 150
            a = torch.randn((M, K), generator=g).to("cuda", torch.bfloat16)
            bt = torch.randn((kb, N), generator=g).to("cuda", torch.bfloat16)
            b = torch.zeros((N, K), dtype=torch.bfloat16, device="cuda")
            b[:, :kb] = bt.t()
            a[:, kb:] = 1.0  # the K padding of Bt reads as zeros whatever A holds there
            ok = torch.equal(ops.gemm_tn(a, bt, M, N, K, kb), ops.gemm_nt(a, b, M, N, K))
            if not ok:
                import warnings

                warnings.warn("drn_gemm_tn failed its first-use self-check against drn_gemm_nt on this toolchain: the fc6 "
                              "weight gradient falls back to the NT form on a materialised A^T (fc1_tn = False)")
            cls._tn_ok = bool(ok)
        return cls._tn_ok

    def _fc1_col_plan(self, dtype, D1, K1):
        """(n_main, slab width in columns) of the fused dW + SGD launch (drn_gemm_tn_sgd), or None when it does not apply: TN
        operand form, a bf16 gradient bucket, whole 256-row tiles.  (Round 4 also ran the unfused dW in column slabs of exact
        rounds with a block update per slab - measured neutral twice, profiles/r4_01_col_slabs_ab.txt - removed in round 5.)"""
        if self.fc1_fused_tn is not None and D1 % 256 == 0:
            # ONE slab of all exact rounds, the rest are the trailing columns
            tiles_m = D1 // 256
            if self._ncu is None:
                self._ncu = torch.cuda.get_device_properties(self.arena_w.device).multi_processor_count
            ncu = self._ncu
            step = ncu // math.gcd(ncu, tiles_m)
            nt = (K1 // 256) // step * step
            if self.fc1_fused_all and K1 % 256 == 0:
                # the trailing tile columns ride in the same launch as a partial last round - it runs while the other
                # workgroups drain - instead of a small-tile launch + block update of their own: no A^T rows at all, the
                # pooling launch loses its 64-ROI tail launch (+2 % same box, profiles/r4_17; fc1_fused_all = 0: A/B)
                nt = K1 // 256
            if nt > 0 and self._fc1_use_tn(dtype):
                return nt * 256, nt * 256
        return None

    def _fc1_tail_row0(self, dtype, D1, K1):
        """first row of A^T the fc6 dW still reads: the smallest main-column count over the row slabs (the columns from
        there on are peeled into the small-tile NT launch, which takes A^T); 0 when the NT form is used throughout"""
        if not self._fc1_use_tn(dtype):
            return 0
        plan = self._fc1_col_plan(dtype, D1, K1)
        if plan is not None:
            return plan[0]
        return min(ops.gemm_nt_main_cols(b - a, K1) for a, b in self._fc1_slabs(D1))

    @staticmethod
    def _splits(M, N, K, dtype):
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        nslab = K * ops.esize(dtype) // 128
        return max(1, min(1024 // max(tiles, 1), max(1, nslab // 8), 16))

    def _linear_fwd(self, A, Wt, M, N, K, bias, relu, out, outT, mask, seed, drop_p, seed_dev=None, fused=False):
        # fused (fc7, bf16): GEMM + bias + ReLU + dropout + the transposed copy as ONE launch of the eight-wave 128x128 kernel
        # (drn_linear_act_fwd) - no split-K partials, no second pass; outside that kernel's class the two-launch form below
        if (fused and A.dtype == torch.bfloat16 and self.fused_fc7_fwd and out is not None and
                out.dtype == torch.bfloat16 and
                ops.linear_act_fwd(A, Wt, M, N, K, bias, relu, mask, seed, drop_p, out=out, outT=outT, seed_dev=seed_dev)):
            return
        s = self._splits(M, N, K, A.dtype)
        part = ops.gemm_nt(A, Wt, M, N, K, splits=s)
        ops.bias_act_fwd(part, M, N, bias, relu, mask, seed, drop_p, out=out, outT=outT, seed_dev=seed_dev)

    def fc6_partials(self, pooled, M, training):
        """The fc6 forward GEMM on its own (split-K partial sums into a static workspace).  GraphedTrainStep issues this
        ONE launch eagerly in front of the captured heads graph, so that the step's dominant kernel can be bracketed
        by HIP events on its stream inside the timed region (a node of a replayed hipGraph cannot); forward() then takes
        the partials through `fc6_part`."""
        h = self.h
        dev, dtype = pooled["A"].device, pooled["A"].dtype
        self.ensure(dev)
        if pooled.get("kshard"):
            return self._fc6_partials_kshard(pooled, M)
        self.refresh_shadows(dtype)
        D1, K1 = h.box_head.fc1.weight.shape
        w = self.ws(M, dtype, training)
        K1p = ops.kpad(K1, dtype)
        s = self._splits(M, D1, K1p, dtype)
        if w.get("part1") is None or w["part1"].shape[0] != s:
            w["part1"] = torch.empty((s, M, D1), dtype=torch.float32, device=dev)
        ops.gemm_nt(pooled["A"], self.sh["W1v"], M, D1, K1p, out=w["part1"], splits=s)
        return w["part1"]

    # ---- fc6 sharded along K over the data-parallel ranks (round 4; FusedSGD.enable_pipelined(exchange="fc6_kshard")) ------
    # Data parallelism exchanges the fc6 weight gradient - 205 MB in bf16 per step and GPU, against 1.3 ms of compute with one
    # image per GPU - and has every rank run the 2-GB optimizer pass (or, sharded, gather 205 MB of updated weights).  fc6
    # is H1 = A . W^T with K = C*49 = 50176: rank k keeps the COLUMNS k of W (channels k*C/N .. (k+1)*C/N of the pooled
    # features - `c*49 + bin` makes a channel range a column range), pools that channel slice of ALL N ranks' images (the
    # ranks all-gather their 0.4-MB feature maps and 40-KB proposal lists, not their 200-MB pooled matrices), multiplies
    # [N*R x K/N] . [D1 x K/N]^T - the same FLOPs as its own [R x K] . [D1 x K]^T - and a reduce-scatter over row blocks hands
    # every rank the complete H1 of its own image.  Backward: all-gather of dP1 (8 MB per rank), dW[:, columns k] =
    # dP1_all^T . A_k - again the same FLOPs - and the optimizer updates only those columns: no gradient exchange and no
    # weight gather for fc6 at all, 1/N of the optimizer traffic.  Wire bytes per step and GPU at N = 8: 2 x 57 MB
    # (fp32 partial sums of H1 out, bf16 dP1 in) instead of 2 x 180 MB.  The arithmetic is the mean-gradient step of DDP
    # (detectron2/engine/defaults.py:279-282) up to the fp32 summation order of the K blocks.
    # `kshard` is dict(group, world, rank, wire, sync) once enabled, plus the buffers the methods below keep in it.
    def _ks_gather(self, t):
        ks = self.kshard
        out = torch.empty((ks["world"],) + tuple(t.shape), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(out.view(-1), t.contiguous().view(-1), group=ks["group"])
        return out

    def pool_kshard(self, feat_nhwc, rois, objectness):
        """pooled operand of the K-sharded fc6: this rank's channel slice of EVERY rank's image -> A_k [N*M, (C/N)*P*P]
        (collectives on the current stream: all-gather of the feature maps, proposals and objectness)"""
        h, ks = self.h, self.kshard
        N, rank = ks["world"], ks["rank"]
        dtype = feat_nhwc.dtype
        M = rois.shape[0]
        n, H, W, C = feat_nhwc.shape
        ka = h.box_pooler.kernel_args()
        pp = ka["P"] * ka["P"] if "P" in ka else 49
        if C % N or ((C // N) * pp * ops.esize(dtype)) % 128:
            raise DrnError("fc6 K-sharding needs the channel count %d to split over %d ranks into whole 128-byte K slabs" % (C, N))
        # equal shapes on all ranks (fixed-size batches; ragged real data keeps the sharded gradient exchange)
        key = (n, H, W, C, M)
        if ks.get("checked") != key:
            shp = torch.tensor(key, dtype=torch.int64, device=feat_nhwc.device)
            allshp = self._ks_gather(shp)
            if not bool((allshp == shp).all()):
                raise DrnError("fc6 K-sharding needs the same image / proposal shapes on every rank (got %s)" % allshp.tolist())
            ks["checked"] = key
        c0, c1 = rank * (C // N), (rank + 1) * (C // N)
        # ONE all-gather: [feature map | proposals | objectness] of every rank as bytes (three small collectives were three
        # launch + rendezvous latencies on the step's dependent chain)
        fb, rb = feat_nhwc.numel() * feat_nhwc.element_size(), rois.numel() * 4
        ob = objectness.numel() * 4 if objectness is not None else 0
        pack = ks.get("pack")
        if pack is None or pack.numel() != fb + rb + ob:
            pack = ks["pack"] = torch.empty((fb + rb + ob,), dtype=torch.uint8, device=feat_nhwc.device)
            ks["pack_all"] = torch.empty((N, fb + rb + ob), dtype=torch.uint8, device=feat_nhwc.device)
        pack[:fb].view(feat_nhwc.dtype).copy_(feat_nhwc.reshape(-1))
        pack[fb: fb + rb].view(torch.float32).copy_(rois.reshape(-1))
        if ob:
            pack[fb + rb:].view(torch.float32).copy_(objectness.reshape(-1))
        allp = ks["pack_all"]
        dist.all_gather_into_tensor(allp.view(-1), pack, group=ks["group"])
        feats = allp[:, :fb].view(feat_nhwc.dtype).view(N, n, H, W, C)[..., c0:c1].reshape(N * n, H, W, c1 - c0).contiguous()
        rois_all = allp[:, fb: fb + rb].view(torch.float32).view(N, M, 5).clone()
        rois_all[:, :, 0] += (torch.arange(N, device=rois.device, dtype=rois.dtype) * n).view(N, 1)
        rois_all = rois_all.view(N * M, 5)
        obj_all = allp[:, fb + rb:].view(torch.float32).reshape(N * M).contiguous() if ob else None
        cols = (c1 - c0) * pp
        MA = N * M
        D1 = h.box_head.fc1.weight.shape[0]
        buf = ks.get("A")
        if buf is None or buf.shape != (MA, cols) or buf.dtype != dtype:
            buf = ks["A"] = torch.zeros((MA, cols), dtype=dtype, device=feat_nhwc.device)
            ks["part"] = torch.empty((1, MA, D1), dtype=torch.float32, device=feat_nhwc.device)
            ks["h1"] = torch.empty((1, M, D1), dtype=torch.float32, device=feat_nhwc.device)
        ops.roi_pool_nhwc(feats, rois_all, obj_all, out=buf, **ka)
        ks["cols"] = (c0 * pp, c1 * pp, MA)
        return dict(A=buf, AT=None, t_row0=0, kshard=True, state="current", M=M)

    def _fc6_partials_kshard(self, pooled, M):
        """[N*M x K/N] . [D1 x K/N]^T on this rank's columns of the compute copy, then the reduce-scatter over row blocks:
        -> the complete fp32 pre-activation of THIS rank's proposals, [1, M, D1]"""
        ks = self.kshard
        k0, k1, MA = ks["cols"]
        dtype = pooled["A"].dtype
        self.refresh_shadows(dtype)
        D1 = self.h.box_head.fc1.weight.shape[0]
        W1k = self.sh["W1v"][:, k0:k1]  # (row pitch K1)
        # few ranks leave too few 256x256 tiles for the CUs (N = 2: 16 x 8): split K like the replicated forward does and
        # add the splits up in split order before the wire
        tiles = ((MA + 255) // 256) * ((D1 + 255) // 256)
        nslab = (k1 - k0) * ops.esize(dtype) // 128
        sp = max(1, min(256 // max(tiles, 1), nslab // 16, 8))
        if sp > 1:
            if ks.get("parts") is None or ks["parts"].shape[0] != sp:
                ks["parts"] = torch.empty((sp, MA, D1), dtype=torch.float32, device=pooled["A"].device)
            ops.gemm_nt(pooled["A"], W1k, MA, D1, k1 - k0, out=ks["parts"], splits=sp)
            torch.sum(ks["parts"], dim=0, keepdim=True, out=ks["part"])
        else:
            ops.gemm_nt(pooled["A"], W1k, MA, D1, k1 - k0, out=ks["part"])
        if ks.get("wire") == torch.bfloat16:
            # optional: the partial sums cross the wire in bf16 (half the bytes of the step's largest collective; RCCL adds
            # them in bf16 - N roundings of 2^-9 in front of an activation that is stored in bf16 anyway)
            if ks.get("part16") is None or ks["part16"].shape != ks["part"].shape:
                ks["part16"] = torch.empty_like(ks["part"], dtype=torch.bfloat16)
                ks["h16"] = torch.empty_like(ks["h1"], dtype=torch.bfloat16)
            ks["part16"].copy_(ks["part"])
            dist.reduce_scatter_tensor(ks["h16"].view(-1), ks["part16"].view(-1), group=ks["group"])
            ks["h1"].copy_(ks["h16"])
        else:
            dist.reduce_scatter_tensor(ks["h1"].view(-1), ks["part"].view(-1), group=ks["group"])
        return ks["h1"]

    def _fc6_tail_kshard(self, w, t, gw, hook):
        """dW[:, own columns] = dP1_all^T . A_k (run_fc1_tail, K-sharded fc6)"""
        ks = self.kshard
        k0, k1, MA = ks["cols"]
        D1, dtype = t.D1, t.dP1T.dtype
        dP1_all = self._ks_gather(w["dP1"][:t.M, :D1].contiguous()).view(MA, D1)
        dPT = ops.transpose2d(dP1_all, MA, D1)            # [D1, kpad(N*M)]: the K-major operand of the dW GEMM
        Kp = dPT.shape[1]
        out = gw[:, k0:k1].unsqueeze(0)
        fused = self.fc1_fused_cols
        if dtype == torch.bfloat16 and fused is not None and fused(dPT, ks["A"], D1, k0, k1, Kp, MA, gw):
            return  # gradient and update of the owned columns in one launch
        if dtype == torch.bfloat16:
            ops.gemm_tn(dPT, ks["A"], D1, k1 - k0, Kp, MA, out=out)
        else:
            AT = ops.transpose2d(ks["A"], MA, k1 - k0)    # fp32 parity mode: the NT form on a transposed copy
            ops.gemm_nt(dPT, AT, D1, k1 - k0, Kp, out=out)
        if hook is not None:
            hook(("fc1b", 0, D1, k0, k1))

    # ---- forward: operand, trunk, one loss tail per head family, one ending ------------------------------------------
    def _operand(self, feat_nhwc, rois, objectness, training, pooled, want_argmax):
        """the fc6 operand of this forward: pooled here (replicated or K-sharded fc6) or taken from a prefetch"""
        if training and self.kshard is not None:
            if want_argmax:
                raise DrnError("fc6 K-sharding needs a frozen trunk (FREEZE_AT = 5) and the OICR / WSDDN / PCL heads")
            if pooled is None:
                pooled = self.pool_kshard(feat_nhwc, rois, objectness)
            elif not pooled.get("kshard"):
                raise DrnError("fc6 K-sharding: the prefetched operand was pooled for the replicated fc6")
        elif pooled is None:
            pooled = self.pool(feat_nhwc, rois, objectness, training, want_argmax=want_argmax)
        elif want_argmax:
            raise DrnError("a trainable backbone / the CSC head cannot use a prefetched pooled operand")
        else:
            self._mark_current(pooled)
        return pooled

    def _dropout(self, training, dev):
        """(p, explicit masks or None, seed, device-side counter or None) of the two dropout layers of this forward"""
        box_head = self.h.box_head
        drop_p = box_head.dropout_p if training else 0.0
        masks = box_head.dropout_masks if training else None
        if not (training and masks is None and drop_p > 0):
            return drop_p, masks, 0, None
        # counter-based masks keyed by (torch seed, device-side step counter, layer): the counter lives on the
        # device and is advanced on the stream, so a replayed hipGraph draws fresh masks every step
        if self.seed_dev is None or self.seed_dev.device != dev:
            self.seed_dev = torch.zeros((1,), dtype=torch.int64, device=dev)
        return drop_p, masks, torch.initial_seed() & 0xFFFFFFFFFFFF, self.seed_dev

    def forward(self, feat_nhwc, rois, objectness, training, img_off=None, n_img=1, gt=None, pooled=None,
                fc6_part=None):
        """fc6, fc7 and all predictor Linears on the pooled operand.  Inference: -> (workspace views, predictor columns).
        Training: the loss tail of the head family, which ends in _finish() -> (loss dict, state)."""
        h = self.h
        fg_hook = self.feature_grad_hook if training else None
        csc = training and h.csc_head
        kshard = training and self.kshard is not None
        if self.kshard is not None and not training:
            # an evaluation forward reads ALL K columns of fc1.weight, and every rank has only updated its own block since
            # the last gather: gather the owners' columns first.  That is a collective - every rank has to run the
            # evaluation, like every rank has to checkpoint - guarded by the optimizer's fail-fast rendezvous.
            sync = self.kshard.get("sync")
            if sync is not None:
                sync()
        pooled = self._operand(feat_nhwc, rois, objectness, training, pooled, want_argmax=fg_hook is not None or csc)
        dev, dtype = pooled["A"].device, pooled["A"].dtype
        self.ensure(dev)
        self.refresh_shadows(dtype)
        M = rois.shape[0]
        w = dict(self.ws(M, dtype, training))
        w["A"], w["AT"], w["AT_row0"] = pooled["A"], pooled["AT"], pooled.get("t_row0", 0)
        sh = self.sh
        fc1, fc2 = h.box_head.fc1, h.box_head.fc2
        D1, K1 = fc1.weight.shape
        D2 = fc2.weight.shape[0]
        K, NH = h.num_classes, self.NH
        kp = lambda k: ops.kpad(k, dtype)
        drop_p, masks, seed, seed_dev = self._dropout(training, dev)
        seed6, seed7 = dropout_seeds(seed)
        if kshard and fc6_part is None:
            fc6_part = self._fc6_partials_kshard(pooled, M)
        if fc6_part is not None:  # the GEMM was issued by fc6_partials() (eagerly, in front of a captured graph)
            ops.bias_act_fwd(fc6_part, M, D1, fc1.bias.data, True, masks[0] if masks else None, seed6, drop_p,
                             out=w["H1"], outT=w["H1T"] if training else None, seed_dev=seed_dev)
        else:
            self._linear_fwd(w["A"], sh["W1v"], M, D1, kp(K1), fc1.bias.data, True, w["H1"],
                             w["H1T"] if training else None, masks[0] if masks else None, seed6, drop_p, seed_dev)
        self._linear_fwd(w["H1"], sh["W2"], M, D2, kp(D1), fc2.bias.data, True, w["H2"], w["H2T"] if training else None,
                         masks[1] if masks else None, seed7, drop_p, seed_dev, fused=True)
        # (the logits pass has no dropout: given the counter it advances it - behind both dropout layers - instead of a
        # counter_add launch of its own on the heads' dependent chain)
        logit_seed = DROP_COUNTER_STEP if seed_dev is not None else 0
        # drn_mil_oicr_losses: the predictor's split-K reduce + bias, WSDDN and the refinement cascade in six launches
        # (nine as separate calls); taken when the heads are exactly cls / det / non-regressing OICR branches
        fuse_tail = (training and not csc and self.fused_loss_tail and h.refine_K > 0 and h.refine_mode != "pcl" and
                     not any(h.refine_reg[: h.refine_K]) and NH == 2 * K + h.refine_K * (K + 1))
        logit_part = None
        if fuse_tail:
            logit_part = ops.gemm_nt(w["H2"], sh["Wh"], M, NH, kp(D2), splits=self._splits(M, NH, kp(D2), dtype))
        else:
            self._linear_fwd(w["H2"], sh["Wh"], M, NH, kp(D2), self._head_bias(), False, w["logits"], None, None,
                             logit_seed, 0.0, seed_dev)
        col = {n: c for n, _, c, _ in self.cols}
        if not training:
            return w, col
        fg = None
        if fg_hook is not None or csc:
            fg = dict(rois=rois, obj=objectness, feat_shape=tuple(feat_nhwc.shape), argmax=pooled.get("argmax"))
        s = _Step(w, col, M, dtype, masks, drop_p, gt, img_off, n_img, logit_part, logit_seed, seed_dev, fg_hook, fg)
        if csc:
            return self._losses_csc(s)
        if h.refine_mode == "pcl" and h.refine_K > 0:
            return self._losses_pcl(s)
        return self._losses_oicr(s)

    def _head_bias(self):
        """the concatenated predictor biases [NH]"""
        bo, _ = self._seg[self.cols[0][0] + ".bias"]
        return self.arena_w[bo: bo + self.NH]

    def _wsddn(self, s):
        """MIL scores and loss_cls fused with their dlogits -> (scores, img_scores, loss_part)"""
        h = self.h
        return ops.wsddn_fwd_bwd(s.w["logits"], s.col["cls"], s.col["det"], h.num_classes, s.img_off, s.n_img, s.gt["onehot"],
                                 dlogits=s.w["dlogits"], mean_loss=h.box_predictor.mean_loss, max_rows=s.gt["max_rows"])

    def _loss_cls(self, loss_part, n_img):
        h = self.h
        for m in [h.box_predictor] + list(h.box_refinery[: h.refine_K]):
            assert m.loss_weight.get("loss_cls", 1.0) == 1.0, "loss_cls weight != 1 is not used by any config"
        return (loss_part if n_img == 1 else ops.sum_small(loss_part)).view(())

    def _losses_oicr(self, s):
        """WSDDN and OICR heads: the MIL loss, then every refinement branch's pseudo-GT cross entropy (+ box regression) - as
        the fused tail, as the four-launch chain (no regressing branch), or branch by branch.  Losses fused with their dlogits."""
        h = self.h
        w, col, gt, dl = s.w, s.col, s.gt, s.w["dlogits"]
        K, RK = h.num_classes, h.refine_K
        thr = h.proposal_matcher.thresholds[1:-1]
        rcols = [col["r%d" % k] for k in range(RK)]
        chain = None
        if s.logit_part is not None:
            scores, img_scores, loss_part, chain = ops.mil_oicr_losses(
                s.logit_part, self._head_bias(), w["logits"], col["cls"], col["det"], K, s.img_off, s.n_img, gt["onehot"],
                rcols, gt["props"], gt["classes"], gt["count"], thr, h.proposal_matcher.labels, dlogits=dl,
                mean_loss=h.box_predictor.mean_loss, max_rows=gt["max_rows"], seed_inc=s.logit_seed, seed_dev=s.seed_dev)
        else:
            scores, img_scores, loss_part = self._wsddn(s)
        loss_names, loss_list = ["loss_cls"], [self._loss_cls(loss_part, s.n_img)]
        head_cols = [("cls", 0), ("det", 0)]
        prev_scores, prev_boxes, prev_zero = scores, gt["props"], False
        aux = dict(scores=scores, img_scores=img_scores, targets=[])
        if chain is None and RK > 0 and not any(h.refine_reg[:RK]):
            # no branch regresses boxes: every branch's targets depend only on the previous branch's softmax of logits
            # that already exist, so the whole cascade is four launches (drn_oicr_refine_chain)
            chain = ops.oicr_refine_chain(w["logits"], rcols, K, scores, gt["props"], s.img_off, s.n_img, gt["classes"],
                                          gt["count"], img_scores, thr, h.proposal_matcher.labels, dlogits=dl)
        for k in range(RK):
            if chain is not None:
                tg, probs, loss = chain[k]
            else:
                tg = ops.oicr_targets(prev_scores, prev_boxes, gt["props"], s.img_off, s.n_img, gt["classes"], gt["count"],
                                      img_scores, K, thr, h.proposal_matcher.labels, zero_delta_decode=prev_zero)
                probs, loss = ops.softmax_ce(w["logits"], col["r%d" % k], K + 1, tg["labels"], tg["weights"], dlogits=dl)
            loss_names.append("loss_cls_r%d" % k)
            loss_list.append(loss.view(()))
            head_cols.append(("r%d" % k, len(loss_list) - 1))
            aux["targets"].append(tg)
            prev_scores = probs
            bw = h.box_refinery[k].box2box_transform.weights
            if h.refine_reg[k]:  # fast_rcnn.py:1146-1211 + :1227-1240: loss_box_reg_r{k}
                lreg = ops.box_reg_loss(w["logits"], col["b%d" % k], K, tg["labels"], gt["props"], tg["gt_boxes"], bw,
                                        dlogits=dl)
                loss_names.append("loss_box_reg_r%d" % k)
                loss_list.append(lreg.view(()))
                head_cols.append(("b%d" % k, len(loss_list) - 1))
                prev_boxes, prev_zero = ops.apply_deltas(w["logits"], gt["props"], K, bw, col0=col["b%d" % k]), False
            else:
                # a non-regressing head passes apply_deltas(0, proposals) on: only the G mined boxes are ever read,
                # so the decode happens inside the next targets kernel instead of materialising [M, 4K] boxes
                prev_boxes, prev_zero = gt["props"], True
        return self._finish(s, loss_names, rcols, loss_list=loss_list, head_cols=head_cols, aux=aux)

    def _losses_pcl(self, s):
        """PCLROIHeads (roi_heads_pcl.py:311-334): the MIL loss, then every branch's targets from the previous branch's
        probabilities through proposal clustering; targets, loss and dlogits of all branches in three launches.  Branches with
        WSL.REFINE_REG add loss_box_reg_r{k} against the annotated boxes (one more launch pair)."""
        h = self.h
        w, col, gt, dl = s.w, s.col, s.gt, s.w["dlogits"]
        K, RK = h.num_classes, h.refine_K
        scores, img_scores, loss_part = self._wsddn(s)
        loss_names, loss_list = ["loss_cls"], [self._loss_cls(loss_part, s.n_img)]
        head_cols = [("cls", 0), ("det", 0)]
        aux = dict(scores=scores, img_scores=img_scores, targets=[])
        batches = self.pcl_image_batches
        if s.n_img != 1 and not batches:
            raise DrnError("PCL clusters the proposals of ONE image per step (third_party/pcl.py:94 asserts it)")
        rcols = [col["r%d" % k] for k in range(RK)]
        if batches:
            # PCLROIHeads.enable_image_batches(): one (branch, image) grid clusters every image; loss_cls_r{k} is the mean
            # over the images of the single-image loss and dlogits carries the 1 / n_img (include/drn_wsod.h)
            max_rows = gt.get("max_rows") or s.M
            adj = ops.pcl_adjacency_batch(gt["props"], s.img_off, s.n_img, max_rows, 0.4)
            per_image, loss_img, loss_b = ops.pcl_refine_batch(w["logits"], rcols, K, scores, gt["props"], adj, gt["onehot"],
                                                               s.img_off, s.n_img, max_rows, dl, rows=gt.get("rows"))
            aux["targets"], aux["pcl_loss_img"] = per_image, loss_img
            branch_loss = [loss_b[k: k + 1] for k in range(RK)]
        else:
            adj = ops.pcl_adjacency(gt["props"], 0.4)
            res = ops.pcl_refine(w["logits"], rcols, K, scores, gt["props"], adj, gt["onehot"].view(-1), dl)
            aux["targets"] = list(res)
            branch_loss = [r["loss"] for r in res]
        # regressing branches (reg/pcl_* recipes; PCLOutputs.box_reg_loss, fast_rcnn.py:1746-1811): the proposals regress onto the
        # matched ANNOTATED box - PCL never relabels against pseudo ground truth - and nothing feeds back into the clustering
        # above.  Labelling, target, loss and dlogits of all such branches and all images: one launch pair (drn_annot_box_reg)
        reg = [k for k in range(RK) if h.refine_reg[k]]
        lreg = None
        if reg:
            if "ann_boxes" not in gt:
                raise DrnError("a regressing PCL branch needs the annotated boxes in this step's labels (PCLROIHeads packs them; a "
                               "graphed step lays its label buffer out before it is primed)")
            pm = h.proposal_matcher
            lreg = ops.annot_box_reg(w["logits"], [col["b%d" % k] for k in reg], K, gt["props"], s.img_off, s.n_img,
                                     gt["ann_boxes"], gt["ann_classes"], gt["ann_count"], pm.thresholds[1:-1], pm.labels,
                                     h.box_refinery[reg[0]].box2box_transform.weights, dlogits=dl, max_rows=gt.get("max_rows"))
        for k in range(RK):
            loss_names.append("loss_cls_r%d" % k)
            loss_list.append(branch_loss[k].view(()))
            head_cols.append(("r%d" % k, len(loss_list) - 1))
            if h.refine_reg[k]:  # (right behind loss_cls_r{k}, as in the reference's dict)
                i = reg.index(k)
                loss_names.append("loss_box_reg_r%d" % k)
                loss_list.append(lreg[i: i + 1].view(()))
                head_cols.append(("b%d" % k, len(loss_list) - 1))
        # (no branch for the metrics: the reference logs no label accuracy for PCL)
        return self._finish(s, loss_names, [], loss_list=loss_list, head_cols=head_cols, aux=aux)

    def _losses_csc(self, s):
        """CSCROIHeads, roi_heads_csc.py:301-352 (training branch): MIL scores, the CSC weights (image-gradient maps through
        input_gradient(), csc.hip), the two weighted image-level losses fused with their dlogits."""
        h = self.h
        w, col, gt = s.w, s.col, s.gt
        K = h.num_classes
        if getattr(h, "image_batches", False):
            return self._losses_csc_batch(s)
        if s.n_img != 1:
            raise DrnError("CSCROIHeads works on ONE image per step (roi_heads_csc.py:433,442 read image_sizes[0] / "
                           "gt_classes_img_oh[0])")
        scores, img_scores, _, rowsm = ops.wsddn_fwd_bwd(w["logits"], col["cls"], col["det"], K, s.img_off, 1, gt["onehot"],
                                                         dlogits=None, mean_loss=h.box_predictor.mean_loss,
                                                         max_rows=gt["max_rows"], return_rowsm=True)
        W, cpgs = h._csc_weights(self, w, col, scores, rowsm, s.M, s.dtype, s.fg, s.masks, s.drop_p)
        if self.csc_stats is not None:
            self._csc_stats_forward(s, scores, W)
        loss = ops.csc_loss(w["logits"], col["cls"], col["det"], K, scores, rowsm, W, gt["onehot"].view(-1),
                            h.box_predictor.mean_loss, dlogits=w["dlogits"])
        return self._finish(s, ["loss_cls_pos", "loss_cls_neg"], [], loss_list=[loss[0].view(()), loss[1].view(())],
                            head_cols=[("cls", 0), ("det", 0)], csc=True,
                            aux=dict(scores=scores, img_scores=img_scores, targets=[], W=W, cpgs=cpgs))

    def _losses_csc_batch(self, s):
        """CSCROIHeads.enable_image_batches(): the MIL scores of all images, one image-gradient pass per class SLOT over the
        whole batch (CSCROIHeads._csc_weights_batch), one weights launch set for every (image, labelled class), one loss launch:
        loss_cls_pos / loss_cls_neg are the mean over the images of the single-image losses and dlogits carries the 1 / n_img
        (include/drn_wsod.h, "CSC on image batches")"""
        h = self.h
        w, col, gt = s.w, s.col, s.gt
        K = h.num_classes
        ops.csc_batch_limits(s.n_img, K)
        mean_loss = h.box_predictor.mean_loss
        scores, img_scores, _, rowsm = ops.wsddn_fwd_bwd(w["logits"], col["cls"], col["det"], K, s.img_off, s.n_img, gt["onehot"],
                                                         dlogits=None, mean_loss=mean_loss, max_rows=gt["max_rows"],
                                                         return_rowsm=True)
        W, cpgs = h._csc_weights_batch(self, s, scores, rowsm)
        if self.csc_stats is not None:
            self._csc_stats_forward(s, scores, W)
        loss_img, loss = ops.csc_loss_batch(w["logits"], col["cls"], col["det"], K, scores, rowsm, W, gt["onehot"], s.img_off,
                                            s.n_img, mean_loss, dlogits=w["dlogits"])
        return self._finish(s, ["loss_cls_pos", "loss_cls_neg"], [], loss_list=[loss[0].view(()), loss[1].view(())],
                            head_cols=[("cls", 0), ("det", 0)], csc=True,
                            aux=dict(scores=scores, img_scores=img_scores, targets=[], W=W, cpgs=cpgs, csc_loss_img=loss_img))

    def _csc_stats_forward(self, s, scores, W):
        """the weight statistics (CSCROIHeads.enable_csc_stats; drn_csc_stats) once W is final, on the stream the losses run on:
        one launch pair for all images of the step while head.iter <= CSC_MAX_ITER - past it W is None and the forward is only
        counted.  Which (image, class) pairs are ACTIVE is the decision the step itself took (CSCROIHeads._csc_sched): an image
        batch's slot rows sit in the plan it uploaded already; the single image's active classes - at most K - go up as one small
        pinned copy, in a step that has just read K image scores back."""
        h = self.h
        launch = h.iter <= h.csc_max_iter
        slots = None
        if launch:
            sched = h._csc_sched
            if isinstance(sched, ops.CscBatchPlan):
                slots = sched.d_slot_rows
            elif sched:
                slots = torch.tensor(sched, dtype=torch.int64)
                if scores.is_cuda:
                    slots = slots.pin_memory().to(scores.device, non_blocking=True)
        self.csc_stats.forward(scores, W, s.img_off, s.n_img, s.gt["onehot"], slots, launch)

    def _finish(self, s, loss_names, col0s, **fields):
        """the one ending of a training forward: the state backward() takes (`fields`: loss_list, head_cols, aux, csc), the
        guard's check and the metrics record behind the loss tail, the autograd hook -> (loss dict, state)"""
        state = dict(w=s.w, M=s.M, dtype=s.dtype, masks=s.masks, drop_p=s.drop_p, **fields)
        if s.fg_hook is not None:  # trainable backbone
            state["fg"] = dict(s.fg, hook=s.fg_hook)
        self._last_state = state
        self._guard_check(state["loss_list"])
        self._metrics_record(loss_names, state, s.n_img, col0s, s.gt, s.img_off)
        outs = _TrainFn.apply(self.anchor, self, state)
        return dict(zip(loss_names, outs)), state

    def _guard_check(self, loss_list):
        """the anomaly guard's check (FusedSGD(nonfinite=...); drn_loss_guard), right behind the loss tail: on the stream that
        computed the losses and in front of the first event an optimizer stream waits on (the backward records those)"""
        if self.loss_guard is not None:
            self.loss_guard.check(loss_list)

    def _metrics_record(self, loss_names, state, n_img, col0s, gt=None, img_off=None):
        """per-step metrics (ROIHeads.enable_metrics; drn_head_metrics + drn_metrics_record) right behind the guard's check, on
        the stream that computed the losses: the label statistics of the OICR branches in `col0s` against the labels their
        losses used, then the step's record.  WSDDN / CSC / PCL heads pass no branch (the reference logs no label accuracy for
        them: PCLOutputs.losses never calls _log_accuracy).  Off = the attribute is None and no launch changes.
        A ring with the annotated-box block (enable_metrics(annotated=True)) gets, for every head class alike, the proposals, the
        annotated boxes of the step's label upload and the MIL scores: two more launches in front of the record."""
        m = self.metrics
        if m is not None:
            annot = None
            if m.annotated:
                if gt is None or "ann_boxes" not in gt:
                    raise DrnError("metrics with the annotated-box block: this step's labels carry no annotated boxes "
                                   "(enable_metrics(annotated=True) comes before the graphed step is primed)")
                pm = self.h.proposal_matcher
                annot = dict(props=gt["props"], img_off=img_off, boxes=gt["ann_boxes"], classes=gt["ann_classes"],
                             count=gt["ann_count"], thresholds=pm.thresholds[1:-1], labels=pm.labels,
                             scores=state["aux"]["scores"], max_rows=gt.get("max_rows"))
            m.record(loss_names, state["loss_list"], n_img, state["M"], state["w"]["logits"], col0s, self.h.num_classes,
                     [t["labels"] for t in state["aux"]["targets"]] if col0s else (), annot=annot)

    def input_gradient(self, w, M, dtype, fg, masks, drop_p, refresh_w1t=True):
        """gradient of the feature map for the logits gradient sitting in w["dlogits"]: the d/dx half of backward()
        alone (predictor -> fc7 -> fc6 -> RoIPool / ROIAlign with the objectness scaling); no weight or bias gradient
        is written, nothing the training backward needs is overwritten except the scratch it rewrites itself."""
        h = self.h
        sh = self.sh
        fc1, fc2 = h.box_head.fc1, h.box_head.fc2
        D1, K1 = fc1.weight.shape
        D2 = fc2.weight.shape[0]
        NH = self.NH
        kp = lambda k: ops.kpad(k, dtype)
        ops.bias_act_bwd(w["dlogits"], M, NH, dpre=w["dS"])
        ops.gemm_nt(w["dS"], sh["WhT"], M, D2, kp(NH), out=w["dH2"].view(1, M, D2))
        ops.bias_act_bwd(w["dH2"], M, D2, saved=w["H2"], mask=masks[1] if masks else None, drop_p=drop_p, dpre=w["dP2"])
        s1 = w["dH1"].shape[0]
        ops.gemm_nt(w["dP2"], sh["W2T"], M, D1, kp(D2), out=w["dH1"], splits=s1)
        if "dP1" not in w or w["dP1"].shape != w["H1"].shape:
            w["dP1"] = torch.zeros_like(w["H1"])
        ops.bias_act_bwd(w["dH1"], M, D1, saved=w["H1"], mask=masks[0] if masks else None, drop_p=drop_p, dpre=w["dP1"])
        return self._feature_gradient(w, fg, M, D1, K1, dtype, refresh_w1t)

    # ---- backward ------------------------------------------------------------------------------------
    def backward(self, st, gouts):
        h = self.h
        w, M, dtype = st["w"], st["M"], st["dtype"]
        sh = self.sh
        fc1, fc2 = h.box_head.fc1, h.box_head.fc2
        D1, K1 = fc1.weight.shape
        D2 = fc2.weight.shape[0]
        NH = self.NH
        kp = lambda k: ops.kpad(k, dtype)
        Mp = kp(M)
        dev = self.arena_w.device
        # per-loss upstream gradients -> per-column scale of dlogits (stays on the device)
        if gouts is None or isinstance(gouts, float):
            # d(scale * sum of losses): every loss has the same upstream gradient (1: GraphedTrainStep; 1 / ITER_SIZE:
            # Trainer through backward_losses) - a cached device vector, no autograd pass
            nl, val = len(st["loss_list"]), 1.0 if gouts is None else float(gouts)
            cache = self._scale_vecs
            colscale = cache.get((nl, val, dev))
            if colscale is None:
                if len(cache) > 8:
                    cache.clear()
                colscale = cache[(nl, val, dev)] = torch.full((nl,), val, dtype=torch.float32, device=dev)
        else:
            g = [torch.zeros((), device=dev) if x is None else x.float().reshape(()) for x in gouts]
            if st.get("csc") and not (gouts[0] is not None and gouts[1] is not None and torch.equal(g[0], g[1])):
                # both CSC losses act on the same cls / det columns and their dlogits were written as one sum
                raise DrnError("loss_cls_pos and loss_cls_neg must be back-propagated with one common weight (the "
                               "reference trainer sums the loss dict)")
            colscale = torch.stack(g)  # one entry per loss; columns find theirs through the static index table
        key = tuple(st["head_cols"])
        if self._colidx_key != key:
            trained = dict(st["head_cols"])
            idx = torch.full((NH,), -1, dtype=torch.int32)
            for n, _, o, c in self.cols:
                if n in trained:
                    idx[o: o + c] = trained[n]
            self._colidx, self._colidx_key = idx.to(dev), key
        colidx = self._colidx
        acc = self._grads_valid and fc2.weight.grad is not None  # fc1.weight.grad is not materialised in bucket modes
        if self.accum_small:
            # pipelined optimizer with WSL.ITER_SIZE > 1: the small tensors always accumulate (one captured graph serves every
            # position of the window); the optimizer clears their region of the arena behind the closing update
            acc = True
        bo, _ = self._seg[self.cols[0][0] + ".bias"]
        wo, _ = self._seg[self.cols[0][0] + ".weight"]
        # bias gradients = column sums of the three pre-activation gradients, in two stages.  With the pipelined optimizer
        # the second stage (three 10-us launches) leaves the critical path: the partials stay in per-layer scratch and
        # `flush_colsums` adds them up on the optimizer stream right in front of the small-tensor SGD bucket
        defer = self.defer_colsum and self.grad_ready_hook is not None
        nparts = (M + 63) // 64
        self._pending_colsum = []

        def colsum_args(layer, N_, view):
            if not defer:
                return dict(colsum=view, accumulate_colsum=acc, colpart=w["colpart"])
            self._pending_colsum.append((w["colpart3"][layer], nparts, N_, view, acc))
            return dict(colsum=None, colpart=w["colpart3"][layer])

        # heads: dS, dS^T, bias grads
        ops.bias_act_bwd(w["dlogits"], M, NH, colscale=colscale, colidx=colidx, dpre=w["dS"], dpreT=w["dST"],
                         **colsum_args(0, NH, self.arena_g[bo: bo + NH]))
        ops.gemm_nt(w["dST"], w["H2T"], NH, D2, Mp, out=self.arena_g[wo: wo + NH * D2].view(1, NH, D2), accumulate=acc)
        # predictor dX + fc7's activation backward: one launch when the contraction is skinny (NH <= 256 columns) - the
        # fp32 dH2 [M, D2] never goes to memory (drn_gemm_nt_act_bwd, bit-identical to the two calls)
        m2 = st["masks"][1] if st["masks"] else None
        cs2 = colsum_args(1, D2, self._gview("fc2.bias"))
        if not (dtype == torch.bfloat16 and self.fused_pred_dx and
                ops.gemm_nt_act_bwd(w["dS"], sh["WhT"], M, D2, kp(NH), saved=w["H2"], mask=m2, drop_p=st["drop_p"],
                                    dpre=w["dP2"], dpreT=w["dP2T"], **cs2)):
            ops.gemm_nt(w["dS"], sh["WhT"], M, D2, kp(NH), out=w["dH2"].view(1, M, D2))
            ops.bias_act_bwd(w["dH2"], M, D2, saved=w["H2"], mask=m2, drop_p=st["drop_p"], dpre=w["dP2"], dpreT=w["dP2T"],
                             **cs2)
        # fc7 dX: [M, D1] over K = D2 is too few 256x256 tiles for one pass (64 at R = 2000) - split K like the forward
        # GEMMs and let the activation backward behind it sum the partials (63 -> ~45 us at the bench shape)
        s1 = self._splits(M, D1, kp(D2), dtype) if self.fc7_dx_split else 1
        pair = dtype == torch.bfloat16 and self.fc7_bwd_pair
        if pair:
            # in the paired launch the dX has about half the CUs to fill: as many (tile, K-split) items as that, not as the
            # whole chip - half the partial sums to write and for the activation backward to read (R50-C4: 4 -> 2 splits,
            # +1.3 % same box, profiles/r3_27)
            t256 = ((M + 255) // 256) * ((D1 + 255) // 256)
            s1 = self.fc7_pair_dx_splits or max(1, min(s1, 128 // max(t256, 1)))
        if w["dH1"].shape[0] != s1:
            base = self._ws[(dtype, True)]
            base["bufs"]["dH1"] = torch.zeros((s1, base["cap"], D1), dtype=torch.float32, device=dev)
            w["dH1"] = base["views"]["dH1"] = base["bufs"]["dH1"][:, :M]
        g_w = dict(A=w["dP2T"], B=w["H1T"], M=D2, N=D1, K=Mp, out=self._gview("fc2.weight", (1, D2, D1)), accumulate=acc)
        g_x = dict(A=w["dP2"], B=sh["W2T"], M=M, N=D1, K=kp(D2), out=w["dH1"], splits=s1)
        if pair:
            # fc7 weight gradient and fc7 dX are independent (both read dP2) and each leaves CUs idle on its own (128 tiles;
            # 64 tiles x 4 short K-splits): ONE persistent launch whose workgroups are divided between the two (round 3)
            ops.gemm_nt_pair(g_w, g_x)
        else:
            ops.gemm_nt(g_w["A"], g_w["B"], D2, D1, Mp, out=g_w["out"], accumulate=acc)
            ops.gemm_nt(g_x["A"], g_x["B"], M, D1, kp(D2), out=w["dH1"], splits=s1)
        # fc6 (the backbone is frozen: no dX)
        fg = st.get("fg")
        need_dp1 = fg is not None or self.kshard is not None  # (K-sharded fc6: the ranks all-gather dP1 row-major)
        if need_dp1 and ("dP1" not in w or w["dP1"].shape != w["H1"].shape):
            w["dP1"] = torch.zeros_like(w["H1"])
        ops.bias_act_bwd(w["dH1"], M, D1, saved=w["H1"], mask=st["masks"][0] if st["masks"] else None,
                         drop_p=st["drop_p"], dpre=w["dP1"] if need_dp1 else None, dpreT=w["dP1T"],
                         **colsum_args(2, D1, self._gview("fc1.bias")))
        self._tail = _Fc1Tail(dP1T=w["dP1T"], AT=w["AT"], D1=D1, K1=K1, Mp=Mp, acc=acc, A=w["A"], M=M,
                              at_row0=w.get("AT_row0", 0))
        self._tail_w = w
        if not self.defer_fc1_tail:
            self.run_fc1_tail()
        if fg is not None:
            self._feature_backward(w, fg, M, D1, K1, dtype, acc)

    def _feature_gradient(self, w, fg, M, D1, K1, dtype, refresh_w1t=True):
        """MODEL.BACKBONE.FREEZE_AT < 5 (and the CSC image-gradient passes): fc6 dX = dP1 . W1 (NT GEMM on a K-major copy
        of W1), RoIPool / ROIAlign backward (with the objectness scaling) -> gradient of the feature map."""
        h = self.h
        kp = lambda k: ops.kpad(k, dtype)
        fc1 = h.box_head.fc1
        if self._w1t_key != (dtype, K1, D1):
            self._w1t = torch.zeros((K1, kp(D1)), dtype=dtype, device=self.arena_w.device)
            self._dA = torch.zeros((1, M, kp(K1)), dtype=dtype, device=self.arena_w.device)
            self._w1t_key = (dtype, K1, D1)
        if self._dA.shape[1] != M:
            self._dA = torch.zeros((1, M, kp(K1)), dtype=dtype, device=self.arena_w.device)
        if refresh_w1t:  # the K-major copy of W1 (several CSC passes of one step share it)
            ops.transpose2d(fc1.weight.data, D1, K1, out=self._w1t)
        ops.gemm_nt(w["dP1"], self._w1t, M, K1, kp(D1), out=self._dA[:, :, :K1])
        ka = h.box_pooler.kernel_args()
        return ops.roi_pool_backward_nhwc(self._dA[0], fg["rois"], fg["obj"], fg["feat_shape"], argmax=fg["argmax"], **ka)

    def _feature_backward(self, w, fg, M, D1, K1, dtype, acc):
        dfeat = self._feature_gradient(w, fg, M, D1, K1, dtype)
        fg["hook"](dfeat, acc)
        if self.grad_ready_hook is not None:
            self.grad_ready_hook("backbone")

    def flush_colsums(self):
        """second stage of the deferred bias-gradient column sums (current stream; see backward)"""
        # (the list describes the LAST backward that ran in Python; a replayed hipGraph re-executes that backward's
        # kernels into the same scratch, so the list is kept, not consumed)
        for colpart, nparts, N_, view, acc in self._pending_colsum:
            ops.colsum_reduce(colpart, nparts, N_, view, acc)

    def _fc1_tail_window(self, win, hook, bucket, tn):
        """fc6 weight gradient of one micro-iteration of an accumulation window with a bf16 bucket.  Columns [0, split) come
        straight from A (drn_gemm_tn), the trailing ones from the A^T rows the pooling piece wrote (small-tile drn_gemm_nt) -
        the same per-element arithmetic whatever the split.  Not closing: fp32 C = the fc1.weight region of the gradient arena,
        overwritten by the window's first micro-iteration, accumulated by the others; no bucket, no optimizer launch.  Closing:
        the main columns as ONE launch that adds the accumulator, rounds to the bucket once and applies the update
        (drn_gemm_tn_acc_sgd) when the fused launch is on and takes the shape; otherwise accumulate + drn_cast2d into the
        bucket + a block update - which the trailing columns always take.  Every column is rounded once per window."""
        t = self._tail
        dP1T, AT, A, D1, K1, Mp, M, at_row0 = t.dP1T, t.AT, t.A, t.D1, t.K1, t.Mp, t.M, t.at_row0
        ga = self._gview("fc1.weight", (D1, K1))
        acc = not win.first
        split = (at_row0 if at_row0 > 0 else K1) if tn else 0
        if split < K1:
            ops.gemm_nt(dP1T, AT[split:], D1, K1 - split, Mp, out=ga[:, split:].unsqueeze(0), accumulate=acc)
            if win.closing:
                ops.cast2d(ga[:, split:], D1, K1 - split, bucket[:, split:])
                if hook is not None:
                    hook(("fc1b", 0, D1, split, K1))
        if split == 0:
            return
        ftn = self.fc1_fused_tn
        if win.closing and ftn is not None:
            plan = self._fc1_col_plan(dP1T.dtype, D1, K1)
            if plan is not None and plan[0] == split:
                if not acc:
                    ga.zero_() if split == K1 else ga[:, :split].zero_()  # a window of one micro-iteration: nothing accumulated
                if ftn(dP1T, A, D1, split, Mp, M, ga, bucket):
                    return  # gradient sum, its one rounding AND the update done by the one launch
                acc = True  # (outside the kernel's class: the unfused sequence on the accumulator as it stands)
        ops.gemm_tn(dP1T, A[:, :split], D1, split, Mp, M, out=ga[:, :split].unsqueeze(0), accumulate=acc)
        if win.closing:
            ops.cast2d(ga[:, :split], D1, split, bucket[:, :split])
            if hook is not None:
                hook(("fc1b", 0, D1, 0, split))

    def _tail_issued(self, dtype, fc1_in_arena):
        """the fc6 tail is queued: the gradients are valid, the batch's operand set may be pooled into again, and every
        parameter whose gradient lives in the arena gets its view (`fc1_in_arena`: fc1.weight's too - not in bucket modes)"""
        self._grads_valid = True
        sets = self._pools.get((dtype, True))
        if sets is not None:
            sets.current_done = True  # the last reader of this batch's A^T has been issued
        for name, p, o, n, used in self.segments:
            if used and p.grad is None and (fc1_in_arena or name != "fc1.weight"):
                p.grad = self.arena_g[o: o + n].view(p.shape)

    def run_fc1_tail(self):
        """Last piece of the explicit backward: announce the small gradients, then the fc6 weight gradient in row
        slabs (each announced as soon as its GEMM is queued).  Normally called by backward() itself; the multi-GPU
        graphed step sets `defer_fc1_tail` and calls it eagerly after replaying the captured part, so the RCCL calls
        issued from the hooks are ordinary stream work and never part of a hipGraph."""
        t = self._tail
        dP1T, AT, A, D1, K1, Mp, M, acc, at_row0 = t.dP1T, t.AT, t.A, t.D1, t.K1, t.Mp, t.M, t.acc, t.at_row0
        hook = self.grad_ready_hook
        if hook is not None:
            hook("small")  # everything except fc1.weight is final: the DP engine starts reducing it now
        bucket = self.fc1_grad_bucket  # [D1, K1] exchange buffer (bf16 or fp32) instead of the arena
        # window state of the pipelined optimizer (WSL.ITER_SIZE > 1; engine.Window): fc1.weight accumulates in the fp32 arena -
        # overwritten by the window's first micro-iteration - and is announced to the optimizer by the closing one alone
        win = self.accum_window if self.accum_small else None
        if win is not None:
            acc = not win.first
            if not win.closing:
                hook = None
        elif self.accum_small:
            raise DrnError("WSL.ITER_SIZE > 1: the pipelined optimizer was not told the window position (set_window)")
        if bucket is not None and acc and win is None:
            raise DrnError("a bucketed fc6 gradient cannot be combined with gradient accumulation")
        gw = bucket if bucket is not None else self._gview("fc1.weight", (D1, K1))
        if self.kshard is not None:
            if acc:
                raise DrnError("fc6 K-sharding cannot be combined with gradient accumulation")
            self._fc6_tail_kshard(self._tail_w, t, gw, hook)
            self._tail_issued(dP1T.dtype, fc1_in_arena=False)
            return
        # Tail balancing peels the same trailing columns off every equal-height slab (drn_gemm_nt: a small-tile launch
        # in front of each persistent one - 14 + 22 us and two launch gaps per step for two slabs).  When all slabs
        # agree on the split, ONE launch computes the peeled columns of all rows first and the slabs' main columns -
        # exact rounds - follow; same kernels' arithmetic per element (tile size does not change the summation order)
        n0 = K1
        slabs = self._fc1_slabs(D1)
        tn = self._fc1_use_tn(dP1T.dtype)
        if at_row0 > 0 and not tn:
            raise DrnError("this batch was pooled for the TN form of the fc6 weight gradient (A^T rows below %d were "
                           "not written) but the backward runs the NT form: fc1_tn / the fused update changed in "
                           "between" % at_row0)
        if win is not None and bucket is not None:
            self._fc1_tail_window(win, hook, bucket, tn)
            slabs = []
        plan = None if (acc or win is not None) else self._fc1_col_plan(dP1T.dtype, D1, K1)
        if plan is not None:
            # column slabs: the trailing columns that do not fill a slab first (small-tile NT launch on the A^T tail rows,
            # all fc6 rows), then slabs of exact rounds straight from A; every piece is announced as a block
            # ("fc1b", r0, r1, c0, c1) the moment its GEMM is queued
            n_main, wcols = plan
            if n_main < at_row0:
                raise DrnError("A^T rows %d.. are needed, the pooling launch wrote them from %d on" % (n_main, at_row0))
            if n_main < K1:
                ops.gemm_nt(dP1T, AT[n_main:], D1, K1 - n_main, Mp, out=gw[:, n_main:].unsqueeze(0))
                if hook is not None:
                    hook(("fc1b", 0, D1, n_main, K1))
            ftn = self.fc1_fused_tn
            for c0 in range(0, n_main, wcols):
                c1 = min(n_main, c0 + wcols)
                if ftn is not None and c0 == 0 and c1 == n_main and bucket is not None and \
                        ftn(dP1T, A, D1, n_main, Mp, M, gw):
                    continue  # gradient AND update done by the one launch (drn_gemm_tn_sgd)
                ops.gemm_tn(dP1T, A[:, c0:c1], D1, c1 - c0, Mp, M, out=gw[:, c0:c1].unsqueeze(0))
                if hook is not None:
                    hook(("fc1b", 0, D1, c0, c1))
            slabs = []
        if self.fc1_joint_peel and len(slabs) > 1 and not acc:
            cols = {ops.gemm_nt_main_cols(b - a, K1) for a, b in slabs}
            if len(cols) == 1 and 0 < min(cols) < K1:
                n0 = cols.pop()
                if n0 < at_row0:
                    raise DrnError("A^T rows %d.. are needed, the pooling launch wrote them from %d on" % (n0, at_row0))
                ops.gemm_nt(dP1T, AT[n0:], D1, K1 - n0, Mp, out=gw[:, n0:].unsqueeze(0))
        for r0, r1 in slabs:
            if tn:
                # main columns (exact rounds of the persistent kernel) straight from A; a slab whose peel was not part
                # of a joint launch peels its own trailing columns through the NT small-tile kernel first
                m0 = min(n0, ops.gemm_nt_main_cols(r1 - r0, K1))
                if m0 < n0:
                    if m0 < at_row0:
                        raise DrnError("A^T rows %d.. are needed, the pooling launch wrote them from %d on" % (m0, at_row0))
                    ops.gemm_nt(dP1T[r0:r1], AT[m0:n0], r1 - r0, n0 - m0, Mp, out=gw[r0:r1, m0:n0].unsqueeze(0),
                                accumulate=acc)
                if m0 > 0:
                    ops.gemm_tn(dP1T[r0:r1], A[:, :m0], r1 - r0, m0, Mp, M, out=gw[r0:r1, :m0].unsqueeze(0),
                                accumulate=acc)
            else:
                ops.gemm_nt(dP1T[r0:r1], AT[:n0], r1 - r0, n0, Mp, out=gw[r0:r1, :n0].unsqueeze(0), accumulate=acc)
            if hook is not None:
                hook(("fc1", r0, r1))
        self._tail_issued(dP1T.dtype, fc1_in_arena=bucket is None)
