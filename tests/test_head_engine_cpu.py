"""The head engine's declared state and its fc6 operand sets (modeling/head_engine.py), on the host:
  1. the state is closed: a misspelt switch raises, every attribute the optimizer, the graphed steps, the meta-architecture and
     bench.py install is a slot, a fresh engine reads the documented defaults and has no layout yet;
  2. the operand sets (`_OperandSets`, through `_HeadEngine.pool` with the pooling launch stubbed out): slot choice, the refusal of
     a third outstanding batch, an inference pass that leaves the training sets alone, grow-only allocation and its refusal while a
     captured step pins the sets, the re-zeroed K-role pad."""
import os
import re
import weakref

import pytest
import torch

import golden_util as G
from __graft_entry__ import load_package

load_package()
from drn_wsod_pytorch_amd import ops  # noqa: E402
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.modeling import build_model, head_engine, roi_heads  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(ROOT, "drn-wsod-pytorch_amd")

# the switches for A/B runs and what other objects install, with the defaults the code had as getattr() fall-backs
DEFAULTS = dict(fc1_tn=True, fused_fc7_fwd=True, fused_loss_tail=True, fused_pred_dx=True, fc7_dx_split=True, fc7_bwd_pair=True,
                fc7_pair_dx_splits=0, fc1_joint_peel=1, fc1_fused_all=1, fc1_grad_slabs=1, fc1_slab_ends=None,
                grad_ready_hook=None, feature_grad_hook=None, loss_guard=None, metrics=None, fc1_fused_tn=None,
                fc1_fused_cols=None, fc1_grad_bucket=None, kshard=None, accum_window=None, accum_small=False,
                defer_colsum=False, defer_fc1_tail=False, pcl_image_batches=False, pool_sets_pinned=None,
                pool_sets_pin_owner=None, captured_by=None)
# assigned from outside the engine's own module
ASSIGNED = {"engine.py": ["loss_guard", "accum_window", "accum_small", "defer_colsum", "kshard", "fc1_fused_cols", "fc1_slab_ends",
                          "grad_ready_hook", "fc1_grad_bucket", "fc1_fused_tn", "fc1_grad_slabs", "_transposes_fresh",
                          "_grads_valid"],
            "graphed.py": ["pool_sets_pinned", "pool_sets_pin_owner", "captured_by", "defer_fc1_tail", "feature_grad_hook"],
            "modeling/rcnn.py": ["_last_state", "feature_grad_hook"],
            "modeling/roi_heads.py": ["metrics", "pcl_image_batches"],
            "bench.py": ["fc1_tn", "fc7_bwd_pair", "fc7_pair_dx_splits", "defer_fc1_tail", "fc1_slab_ends", "fc1_joint_peel"]}


@pytest.fixture()
def model():
    return build_model(G.drn_cfg(G.MODEL_CASES["model_r50c4_tiny"], "cpu"))


def test_engine_lives_in_its_own_module_and_is_re_exported():
    assert roi_heads._HeadEngine is head_engine._HeadEngine and roi_heads._TrainFn is head_engine._TrainFn
    assert head_engine._HeadEngine.__module__.endswith("modeling.head_engine")
    assert roi_heads.dropout_seeds is head_engine.dropout_seeds and roi_heads.DROP_COUNTER_STEP == head_engine.DROP_COUNTER_STEP
    assert roi_heads.dropout_seeds(5) == (5, 5 + roi_heads.FC7_SEED_OFFSET)


def test_unknown_attribute_raises(model):
    eng = model.roi_heads._engine
    assert type(eng) is head_engine._HeadEngine and not hasattr(eng, "__dict__")
    for name in ("fc7_bwd_pairs", "fused_loss_tails", "defer_fc1_tial"):
        with pytest.raises(AttributeError):
            setattr(eng, name, 0)
    with pytest.raises(AttributeError):
        eng.fc1_joint_peal  # noqa: B018


def test_fresh_engine_reads_the_documented_defaults(model):
    eng = head_engine._HeadEngine(model.roi_heads)
    assert hasattr(eng, "_seg") is False
    for name, want in DEFAULTS.items():
        got = getattr(eng, name)
        assert got is want or (got == want and type(got) is type(want)), (name, got, want)
    assert eng.arena_w is None and eng.arena_g is None and eng.segments == [] and eng._last_state is None
    assert eng._grads_valid is False and eng._transposes_fresh is False and eng._ncu is None and eng.sh is None
    assert head_engine._HeadEngine._tn_ok is None or isinstance(head_engine._HeadEngine._tn_ok, bool)  # per process: on the class
    assert "_tn_ok" not in head_engine._HeadEngine.__slots__
    eng.ensure(torch.device("cpu"))
    assert eng._seg["fc1.weight"][1] == model.roi_heads.box_head.fc1.weight.numel()


def _assigned_in(path):
    """attribute names assigned on something called e / eng / engine / _engine in a source file (left side of a plain `=`)"""
    names = set()
    with open(path) as f:
        for line in f:
            m = re.match(r"^([^=#]*[^=!<>+\-*/%&|^ ]) *=(?!=)", line)
            if m:
                names |= set(re.findall(r"(?:\b_engine|\bengine|\be|\beng)\.([A-Za-z_][A-Za-z_0-9]*)\s*(?:,|$)", m.group(1).strip()))
    return names


def test_every_installed_attribute_is_a_slot(model):
    eng = model.roi_heads._engine
    slots = set(head_engine._HeadEngine.__slots__)
    assert set(DEFAULTS) <= slots
    for fname, names in ASSIGNED.items():
        path = os.path.join(ROOT if fname == "bench.py" else PKG, fname)
        found = _assigned_in(path)
        if fname != "bench.py":  # (bench.py reads two of its names through getattr and never assigns them)
            assert set(names) <= found, (fname, sorted(set(names) - found))
        # whatever else these files assign on something called e / eng / engine has to be declared too
        stray = {n for n in found if n not in slots}
        assert not stray, (fname, sorted(stray))
        for n in names:
            assert n in slots, (fname, n)
            setattr(eng, n, getattr(eng, n))  # accepted
    for n in ("fc1_tn", "fc7_bwd_pair", "fc1_joint_peel", "fc1_grad_slabs"):  # bench.py --engine-opt name=int
        setattr(eng, n, int(getattr(eng, n)))


# ----------------------------------------------------------------------------------------------------------- operand sets
@pytest.fixture()
def pooling(model, monkeypatch):
    """the engine of a CPU model, fp32 (no TN form, so no device self-check), the pooling launch replaced by a recorder"""
    launches = []

    def fake_pool(feat, rois, obj, out=None, out_t=None, want_argmax=False, t_first_channel=0, **ka):
        launches.append((out.data_ptr(), None if out_t is None else out_t.data_ptr(), out.shape[0]))
        return out, None

    monkeypatch.setattr(ops, "roi_pool_nhwc", fake_pool)
    eng = model.roi_heads._engine
    feat = torch.zeros((1, 4, 4, 8))

    def pool(M, training=True, **kw):
        return eng.pool(feat, torch.zeros((M, 5)), torch.zeros((M,)), training, **kw)

    return eng, pool, launches


def _ptrs(sets):
    return [(q["A_buf"].data_ptr(), None if q["AT_buf"] is None else q["AT_buf"].data_ptr()) for q in sets.sets]


def test_operand_sets_follow_the_trainer_order(pooling):
    eng, pool, launches = pooling
    tkey, ekey = (torch.float32, True), (torch.float32, False)
    s0 = pool(100, prefetch=True)                      # prefetch of batch 0
    train = eng._pools[tkey]
    assert isinstance(train, head_engine._OperandSets) and train.cap == 128 and s0 is train.sets[0] and s0["state"] == "pending"
    K1 = eng.h.box_head.fc1.weight.shape[1]
    assert s0["A"].shape == (100, ops.kpad(K1, torch.float32)) and s0["AT"].shape == (K1, ops.kpad(100, torch.float32))
    before = _ptrs(train)
    eng._mark_current(s0)                              # forward 0 consumes it
    assert s0["state"] == "current" and train.current_done is False
    s1 = pool(90, prefetch=True)                       # prefetch of batch 1: the free set, never the one in flight
    assert s1 is train.sets[1] and s1["state"] == "pending" and s1["M"] == 90
    with pytest.raises(DrnError, match="no free fc6-operand buffer set: at most one batch can be pooled ahead of the one in flight"):
        pool(80, prefetch=True)                        # a third outstanding batch
    assert [q["state"] for q in train.sets] == ["current", "pending"]
    eng._tail = None
    eng._tail_issued(torch.float32, fc1_in_arena=True)  # backward 0: its fc6 tail is queued
    assert train.current_done is True and eng._grads_valid is True
    # an inference pass in between - larger than anything the training sets hold - gets sets of its own
    e0 = pool(300, training=False)
    evals = eng._pools[ekey]
    assert evals is not train and e0["AT"] is None and e0["state"] == "current" and evals.cap == 320
    assert _ptrs(train) == before and train.cap == 128 and [q["state"] for q in train.sets] == ["current", "pending"]
    e1 = pool(10, training=False)                      # (inference: no backward to wait for; the other set is free)
    assert e1 is evals.sets[1] and e0["state"] == "free"
    assert pool(10, training=False) is evals.sets[0]
    eng._mark_current(s1)                              # forward 1 consumes ITS set: the training pair moves on, not the inference one
    assert [q["state"] for q in train.sets] == ["free", "current"] and train.current_done is False
    assert [q["state"] for q in evals.sets] == ["current", "free"]
    s2 = pool(100, prefetch=True)                      # prefetch of batch 2 takes the freed set, in place
    assert s2 is train.sets[0] and _ptrs(train) == before
    assert launches[0][:2] == before[0] and launches[1][:2] == before[1] and launches[-1][:2] == before[0]
    # no free set: the current one is taken only once its backward has been issued
    eng._mark_current(s2)
    assert pool(100, prefetch=True) is train.sets[1]
    assert [q["state"] for q in train.sets] == ["current", "pending"] and train.current_done is False
    with pytest.raises(DrnError, match="no free fc6-operand buffer set"):
        pool(100, prefetch=True)
    eng._tail_issued(torch.float32, fc1_in_arena=True)
    assert pool(100, prefetch=True) is train.sets[0] and _ptrs(train) == before


def test_operand_sets_grow_only_and_refuse_while_pinned(pooling):
    eng, pool, _ = pooling
    key = (torch.float32, True)
    pool(100, slot=0)
    sets = eng._pools[key]
    first = _ptrs(sets)
    pool(64, slot=0)                                   # smaller: views of the same buffers
    assert _ptrs(sets) == first and sets.cap == 128

    class Step:
        pass

    owner = Step()
    eng.pool_sets_pinned, eng.pool_sets_pin_owner = key, weakref.ref(owner)
    pool(128, slot=0)                                  # within the capacity: fine while pinned
    with pytest.raises(DrnError, match=r"are pinned by a captured step \(GraphedTrainStep\) and cannot grow from 128 to 129 proposals"):
        pool(129, slot=0)
    assert _ptrs(sets) == first
    pool(129, training=False)                          # the pin names the training sets only
    del owner                                          # the pin lapses with its owner
    pool(129, slot=0)
    assert sets.cap == 192 and _ptrs(sets) != first and [q["state"] for q in sets.sets] == ["current", "free"]
    eng.pool_sets_pinned, eng.pool_sets_pin_owner = key, None  # a pin without an owner holds
    with pytest.raises(DrnError, match="cannot grow from 192 to 200"):
        pool(200, slot=0)


def test_operand_set_rezeroes_the_k_role_pad_when_m_changes(pooling):
    eng, pool, _ = pooling
    s = pool(100, slot=0)
    assert s["AT"].shape[1] == 128
    s["AT_buf"].fill_(1.0)                             # batch 0 wrote its 100 columns (and here: everything)
    s = pool(70, slot=0)
    assert s["AT"].shape[1] == 96 and s["A"].shape[0] == 70
    assert not s["AT_buf"][:, 70:96].any() and bool(s["AT_buf"][:, :70].all()) and bool(s["AT_buf"][:, 96:].all())
    s["AT_buf"].fill_(1.0)
    pool(70, slot=0)                                   # same M: nothing to re-zero
    assert bool(s["AT_buf"].all())
