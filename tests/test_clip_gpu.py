"""SOLVER.CLIP_GRADIENTS on the device (detectron2/solver/build.py:19-90: every parameter clipped on its own, right before SGD.step):
  1. drn_grad_norms against the fp64 norm of the stored values, with a bound derived from the kernel's summation order;
  2. value clipping in the fused SGD kernel, bit-exact against torch.nn.utils.clip_grad_value_ + the oracle's SGD;
  3. norm clipping: bit-exact given the device norms, and against torch.nn.utils.clip_grad_norm_ end to end;
  4. the block form equals the flat form, and clip_mode 0 equals the unclipped entry points;
  5. through the model: a Trainer step with the key set in the config clips both arenas (FAILS where the key is ignored);
  6. the graphed, pipelined step with value clipping equals the plain clipped Trainer; norm clipping is refused there.

The summation order of drn_grad_norms (csrc/optim.hip), for the chain depth D used below: a thread adds its 16-byte vectors lane by
lane (segment of 1 500 003 fp32 elements over 512 x 256 threads: at most 3 vectors per thread -> 3 additions; as a bf16 bucket: 2),
joins the 4 (bf16: 8) lanes in a tree (2; bf16: 3), adds its scalar tail element (1), then the 6 levels of the wave butterfly, the 2
levels of the LDS tree over the 4 waves; the second launch adds 512 partials as 2 per thread + 6 + 2.  D = 3 + 2 + 1 + 6 + 2 + 2 + 6 + 2
= 24 for both dtypes (the unaligned segments, read by the scalar path, hold at most one element per thread: a shorter chain)."""
import numpy as np
import pytest
import torch

import golden_util as G
from __graft_entry__ import load_package
from oracle import wsod_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24  # unit roundoff of fp32
D_CHAIN = 24
INF = float("inf")
SEG_DT = [("off", "<i8"), ("cnt", "<i8"), ("lr", "<f4"), ("wd", "<f4")]

# test_sgd_step's four segments (the 2nd and 3rd start at offsets that are no multiple of 4), then: one element; an all-zero
# gradient; 1 500 003 elements at a 16-byte aligned offset = three sweeps of a 512 x 256 x 4 grid plus a scalar tail of 3
NAMES = ["a.weight", "a.bias", "b.weight", "b.bias", "c.bias", "z.weight", "big.weight"]
SIZES = [1000, 37, 5000, 64, 1, 130, 1500003]
ZERO = "z.weight"


@pytest.fixture(scope="module")
def drn():
    load_package()
    import drn_wsod_pytorch_amd.ops as ops

    return ops


def _table(cfg, names=NAMES, sizes=SIZES):
    segs = np.zeros(len(names), dtype=SEG_DT)
    o = 0
    for i, (n, s) in enumerate(zip(names, sizes)):
        b = n.endswith("bias")
        segs[i] = (o, s, cfg.base_lr * (cfg.bias_lr_factor if b else 1), cfg.weight_decay_bias if b else cfg.weight_decay)
        o += s
    return segs, torch.from_numpy(segs.view(np.uint8)).to(DEV)


def _grads(rs):
    g = {n: torch.from_numpy(rs.standard_normal(s).astype(np.float32)) for n, s in zip(NAMES, SIZES)}
    g[ZERO].zero_()
    return g


def _cat(d):
    return torch.cat([d[n] for n in NAMES])


def _sum_bound(p):
    """relative error bound of the norm: (D + 2) u on the sum (D dependent additions; the term itself - the product with grad_scale
    and the square - is two more roundings); p = 2: half of it plus one u for the root"""
    e = (D_CHAIN + 2) * U
    return e / 2 + U if p == 2 else e


def _ref_norm64(x, p, scale):
    v = np.abs(x.double().numpy() * scale)
    return float(v.max()) if p == INF else float(v.sum()) if p == 1 else float(np.sqrt((v * v).sum()))


# ------------------------------------------------------------------------------------------------------------ 1. norms
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("p", [1, 2, INF])
def test_grad_norms_fp32(drn, p, scale):
    """fp32 gradient arena, seven segments: every norm within the derived bound of the fp64 norm of the same values (D = 24, module
    docstring: relative error of the sum <= (D + 2) 2^-24; p = 2: half of it + 2^-24); inf: the fp32 maximum, bit for bit; the
    all-zero segment exactly 0; two launches identical bits."""
    g = _grads(np.random.RandomState(71))
    _, segs_dev = _table(O.OracleCfg())
    flat = _cat(g).to(DEV)
    out = drn.grad_norms(flat, segs_dev, len(NAMES), p, scale)
    again = drn.grad_norms(flat, segs_dev, len(NAMES), p, scale, out=torch.full_like(out, -1.0))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == (len(NAMES),)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    got = out.cpu()
    for i, n in enumerate(NAMES):
        if p == INF:
            assert float(got[i]) == float((g[n] * scale).abs().max()), n
        else:
            ref = _ref_norm64(g[n], p, scale)
            err = abs(float(got[i]) - ref)
            print(n, p, scale, "rel err %.3g (bound %.3g)" % (err / max(ref, 1e-300), _sum_bound(p)))
            assert err <= _sum_bound(p) * ref, (n, float(got[i]), ref)
    assert float(got[NAMES.index(ZERO)]) == 0.0


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("p", [1, 2, INF])
def test_grad_norms_bf16_bucket(drn, p, scale):
    """a bf16 bucket that covers ONE tensor of the arena (grad_off = the tensor's offset, as test_sgd_step_bf16_bucket passes it):
    the 1 500 003-element tensor (8 elements per 16-byte load, scalar tail of 3) and a short one whose bucket starts unaligned"""
    rs = np.random.RandomState(72)
    for n0, n1, shift in ((1000, 1500003, 0), (1000, 4096 + 3, 1)):
        seg = np.zeros(1, dtype=SEG_DT)
        seg[0] = (n0, n1, 0.01, 5e-4)
        seg_dev = torch.from_numpy(seg.view(np.uint8)).to(DEV)
        g16 = torch.from_numpy(rs.standard_normal(n1 + shift).astype(np.float32)).to(torch.bfloat16)
        bucket = g16.to(DEV)[shift:]  # shift = 1: the bucket's first element sits 2 bytes past a 16-byte boundary (scalar path)
        out = drn.grad_norms(bucket, seg_dev, 1, p, scale, grad_off=n0)
        again = drn.grad_norms(bucket, seg_dev, 1, p, scale, grad_off=n0)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), again.view(torch.int32))
        stored = g16[shift:].float()
        if p == INF:
            assert float(out[0]) == float((stored * scale).abs().max())
        else:
            ref = _ref_norm64(stored, p, scale)
            err = abs(float(out[0]) - ref)
            print(n1, p, scale, "rel err %.3g (bound %.3g)" % (err / ref, _sum_bound(p)))
            assert err <= _sum_bound(p) * ref, (n1, float(out[0]), ref)


def test_grad_norms_refuses_bad_arguments(drn):
    from drn_wsod_pytorch_amd._cabi import DrnError

    _, segs_dev = _table(O.OracleCfg())
    flat = torch.zeros(sum(SIZES), device=DEV)
    with pytest.raises(DrnError, match="NORM_TYPE"):
        drn.grad_norms(flat, segs_dev, len(NAMES), 3)
    with pytest.raises(DrnError):
        drn.grad_norms(flat, segs_dev, len(NAMES), 2, workspace=torch.empty(16, dtype=torch.uint8, device=DEV))  # too small


# ------------------------------------------------------------------------------------------- 2. value clipping, bit-exact
def _cpu_clip_value(g, scale, c):
    out = {}
    for n, t in g.items():
        q = torch.nn.Parameter(torch.zeros_like(t))
        q.grad = t * scale
        torch.nn.utils.clip_grad_value_([q], c)
        out[n] = q.grad
    return out


def test_value_clipping_bit_exact(drn):
    """three steps, momentum 0.9, the oracle's weight / bias groups, bf16 shadow, grad_scale 0.5, CLIP_VALUE 0.5: weights, momentum
    and shadow torch.equal to (g * 0.5 -> torch.nn.utils.clip_grad_value_ -> O.SGDState.step) on the CPU"""
    cfg = O.OracleCfg()
    rs = np.random.RandomState(73)
    p = {n: torch.from_numpy(rs.standard_normal(s).astype(np.float32)) for n, s in zip(NAMES, SIZES)}
    flat = _cat(p).to(DEV)
    mom = torch.zeros_like(flat)
    shadow = torch.zeros(flat.shape, dtype=torch.bfloat16, device=DEV)
    _, segs_dev = _table(cfg)
    opt = O.SGDState(cfg)
    scale, c = 0.5, 0.5
    for step in range(3):
        g = _grads(rs)
        share = float(((_cat(g) * scale).abs() > c).float().mean())
        assert 0.10 <= share <= 0.90, share  # ~32 % of standard-normal entries exceed 1.0 = c / scale
        opt.step(p, _cpu_clip_value(g, scale, c))
        drn.sgd_step(flat, mom, _cat(g).to(DEV), segs_dev, len(NAMES), cfg.momentum, step == 0, scale, shadow=shadow,
                     clip=(drn.CLIP_VALUE, c, None))
        ref = _cat(p)
        assert torch.equal(flat.cpu(), ref), step
        assert torch.equal(mom.cpu(), _cat(opt.buf)), step
        assert torch.equal(shadow.float().cpu(), ref.to(torch.bfloat16).float()), step


# ------------------------------------------------------------------------------------------------------ 3. norm clipping
def _coef32(norms, c):
    """torch.nn.utils.clip_grad_norm_'s coefficient in fp32, by its own expression: clamp(max_norm / (total_norm + 1e-6), max = 1)
    with max_norm a Python float (torch evaluates that quotient as reciprocal(total_norm + 1e-6) * max_norm; so does the kernel)"""
    return torch.clamp(c / (norms.float() + 1e-6), max=1.0)


@pytest.mark.parametrize("p", [1, 2, INF])
def test_norm_clipping_bit_exact_given_the_device_norms(drn, p):
    """(a) the norms are read back, coef is formed on the CPU in fp32 as torch forms it, (g * 0.5) * coef -> O.SGDState.step:
    torch.equal.  CLIP_VALUE = the median of the segments' reference norms of step 0, so that some segments are scaled, some pass
    with coef clamped to 1 and the all-zero one stays as it is."""
    cfg = O.OracleCfg()
    rs = np.random.RandomState(74)
    w = {n: torch.from_numpy(rs.standard_normal(s).astype(np.float32)) for n, s in zip(NAMES, SIZES)}
    flat = _cat(w).to(DEV)
    mom = torch.zeros_like(flat)
    shadow = torch.zeros(flat.shape, dtype=torch.bfloat16, device=DEV)
    _, segs_dev = _table(cfg)
    opt = O.SGDState(cfg)
    scale, c = 0.5, None
    for step in range(3):
        g = _grads(rs)
        if c is None:
            c = float(np.median([_ref_norm64(g[n], p, scale) for n in NAMES]))
        gd = _cat(g).to(DEV)
        norms = drn.grad_norms(gd, segs_dev, len(NAMES), p, scale)
        coef = _coef32(norms.cpu(), c)
        if step == 0:
            assert int((coef < 1).sum()) >= 2 and int((coef == 1).sum()) >= 2, coef
            assert float(coef[NAMES.index(ZERO)]) == 1.0
        opt.step(w, {n: (g[n] * scale) * coef[i] for i, n in enumerate(NAMES)})
        drn.sgd_step(flat, mom, gd, segs_dev, len(NAMES), cfg.momentum, step == 0, scale, shadow=shadow,
                     clip=(drn.CLIP_NORM, c, norms))
        ref = _cat(w)
        assert torch.equal(flat.cpu(), ref), step
        assert torch.equal(mom.cpu(), _cat(opt.buf)), step
        assert torch.equal(shadow.float().cpu(), ref.to(torch.bfloat16).float()), step


@pytest.mark.parametrize("p,with_inf", [(1, False), (2, False), (INF, False), (2, True)])
def test_norm_clipping_against_torch(drn, p, with_inf):
    """(b) torch.nn.utils.clip_grad_norm_ per parameter (fp32, as the reference runs it) + O.SGDState on the CPU against grad_norms +
    the clipped kernel, three steps.  Only coef may differ, by e = the relative bound of test 1, so the clipped gradient d differs by
    at most e |d|, the momentum by that summed with the momentum's weights, and the weights by lr times that; asserted with that
    bound TIMES 2.  Two terms are added to that rule, each stated here:
      * the reference's own error.  torch's fp32 CPU norm is not exact: against the fp64 norm of the same values it is off by
        2.0e-5 .. 2.3e-5 (L2) and 1.2e-6 .. 3.1e-6 (L1) on the 1 500 003-element segment (<= 1e-6 on the short ones; printed below
        for every step), where drn_grad_norms is within 5e-8 (test 1).  With e alone the momentum of that segment misses the bound
        by a factor of 11 on the first step (1.35e-7 against 1.2e-8 measured on an MI355X).  e_ref = |torch's fp32 norm - fp64 norm| /
        fp64 norm is measured here per segment and step, on the reference alone, and added to 2 e for that segment;
      * one rounding.  Two fp32 computations whose inputs differ in the last bits can round a result to different neighbours: one
        spacing (2^-23 of the result) is added once per step to the momentum (where g is near 0 the momentum is wd * w + d and e |d|
        is far below its spacing) and once per step to the weight (lr * e * |d| ~ 1e-9 is below the 6e-8 spacing of a weight
        near 1: no fp32 computation could meet the rule without it).  Nothing else is added.
    with_inf: an inf entry in one segment - norm inf, coef 0, NaN at that entry and zero gradient elsewhere in the segment, in both;
    the NaNs sit in the same places and every other segment is held to the bound."""
    cfg = O.OracleCfg()
    rs = np.random.RandomState(75)
    w = {n: torch.from_numpy(rs.standard_normal(s).astype(np.float32)) for n, s in zip(NAMES, SIZES)}
    flat = _cat(w).to(DEV)
    mom = torch.zeros_like(flat)
    segs, segs_dev = _table(cfg)
    opt = O.SGDState(cfg)
    scale, c = 0.5, None
    sp = 2.0 ** -23
    lr = torch.cat([torch.full((s,), float(segs[i]["lr"])) for i, s in enumerate(SIZES)])
    wd = torch.cat([torch.full((s,), float(segs[i]["wd"])) for i, s in enumerate(SIZES)])
    tol_m = torch.zeros(sum(SIZES))
    tol_w = torch.zeros(sum(SIZES))
    for step in range(3):
        g = _grads(rs)
        if with_inf and step == 1:
            g["b.weight"][123] = INF
        if c is None:
            c = float(np.median([_ref_norm64(g[n], p, scale) for n in NAMES]))
        clipped, e_seg = {}, []
        for n in NAMES:
            q = torch.nn.Parameter(torch.zeros_like(g[n]))
            q.grad = g[n] * scale
            n32 = float(torch.nn.utils.clip_grad_norm_([q], c, norm_type=p))
            clipped[n] = q.grad
            n64 = _ref_norm64(g[n], p, scale)
            e_ref = abs(n32 - n64) / n64 if 0 < n64 < INF else 0.0
            print(n, p, step, "torch's fp32 norm: rel err %.3g against fp64 (drn_grad_norms' bound %.3g)" % (e_ref, _sum_bound(p)))
            e_seg.append(2 * _sum_bound(p) + e_ref)
        e = torch.cat([torch.full((s,), v) for s, v in zip(SIZES, e_seg)])
        opt.step(w, clipped)
        gd = _cat(g).to(DEV)
        norms = drn.grad_norms(gd, segs_dev, len(NAMES), p, scale)
        drn.sgd_step(flat, mom, gd, segs_dev, len(NAMES), cfg.momentum, step == 0, scale, clip=(drn.CLIP_NORM, c, norms))
        ref_w, ref_m, d = _cat(w), _cat(opt.buf), _cat(clipped)
        got_w, got_m = flat.cpu(), mom.cpu()
        assert torch.equal(torch.isnan(got_w), torch.isnan(ref_w)) and torch.equal(torch.isnan(got_m), torch.isnan(ref_m))
        assert bool(torch.isnan(ref_w).any()) == (with_inf and step >= 1)
        fin = lambda t: torch.nan_to_num(t.abs(), nan=0.0, posinf=0.0)
        # m = mom m + (d + wd w); w -= lr m: what e |d| (and, through wd, the weights' difference) becomes + one spacing each
        tol_m = cfg.momentum * tol_m + e * fin(d) + wd * tol_w + sp * fin(ref_m)
        tol_w = tol_w + lr * tol_m + sp * fin(ref_w)
        ok = ~torch.isnan(ref_w)
        assert bool(((got_m - ref_m).abs()[ok] <= tol_m[ok]).all()), (step, float(((got_m - ref_m).abs()[ok] - tol_m[ok]).max()))
        assert bool(((got_w - ref_w).abs()[ok] <= tol_w[ok]).all()), (step, float(((got_w - ref_w).abs()[ok] - tol_w[ok]).max()))
        if with_inf and step == 1:
            o = int(segs[NAMES.index("b.weight")]["off"])
            bad = torch.isnan(got_w).nonzero().flatten().tolist()
            assert bad == [o + 123]  # the other elements of the segment saw a zero gradient, the other segments are untouched
            assert float(norms[NAMES.index("b.weight")]) == INF


# ------------------------------------------------------------------------------------------ 4. block and flat forms agree
@pytest.mark.parametrize("mode", ["value", "norm"])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_clipped_block_form_equals_flat(drn, gdt, mode):
    """sgd_step_block(clip=...) over the 2-D partition of test_sgd_step_block_equals_flat == ONE flat clipped step, bit for bit
    (weights, momentum, bf16 shadow), for both clip modes and both gradient dtypes; and the clipping really acted."""
    rs = np.random.RandomState(17)
    n0, rows, ld = 192, 70, 1000
    tot = n0 + rows * ld + 64
    w = torch.from_numpy(rs.standard_normal(tot).astype(np.float32)).to(DEV)
    seg = np.zeros(1, dtype=SEG_DT)
    seg[0] = (n0, rows * ld, 0.01, 5e-4)
    seg_dev = torch.from_numpy(seg.view(np.uint8)).to(DEV)
    wa, wb, wc = w.clone(), w.clone(), w.clone()
    ma, mb, mc = torch.zeros_like(w), torch.zeros_like(w), torch.zeros_like(w)
    sa, sb = torch.zeros_like(w, dtype=torch.bfloat16), torch.zeros_like(w, dtype=torch.bfloat16)
    blocks = [(0, rows, 768, 1000), (0, rows, 0, 256), (0, 32, 256, 768), (32, rows, 256, 512), (32, rows, 512, 768)]
    for step in range(3):
        g = torch.from_numpy(rs.standard_normal(rows * ld).astype(np.float32)).to(DEV).to(gdt)
        if gdt == torch.float32:
            gfull = torch.zeros_like(w)
            gfull[n0: n0 + rows * ld] = g
            ga, goff = gfull, 0
        else:
            ga, goff = g, n0
        if mode == "value":
            clip = (drn.CLIP_VALUE, 0.5, None)
        else:
            norms = drn.grad_norms(ga, seg_dev, 1, 2, 0.5, grad_off=goff)  # ~ 0.5 sqrt(70000) = 132: scaled by ~0.38
            clip = (drn.CLIP_NORM, 50.0, norms)
        drn.sgd_step(wa, ma, ga, seg_dev, 1, 0.9, step == 0, 0.5, shadow=sa, grad_off=goff, clip=clip)
        for r0, r1, c0, c1 in blocks:
            drn.sgd_step_block(wb, mb, ga, seg_dev, r0, r1 - r0, c0, c1 - c0, ld, 0.9, step == 0, 0.5, shadow=sb, grad_off=goff,
                               clip=clip)
        drn.sgd_step(wc, mc, ga, seg_dev, 1, 0.9, step == 0, 0.5, grad_off=goff)  # unclipped
        assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(sa, sb), step
        assert not torch.equal(wa, wc)
    assert torch.equal(wb[:n0], w[:n0]) and torch.equal(wb[n0 + rows * ld:], w[n0 + rows * ld:])


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_clip_mode_none_equals_the_unclipped_entry_points(drn, gdt):
    """drn_sgd_step_clip / drn_sgd_step_block_clip with clip_mode 0 == drn_sgd_step / drn_sgd_step_block, bit for bit"""
    rs = np.random.RandomState(18)
    n0, rows, ld = 192, 70, 1000
    tot = n0 + rows * ld + 64
    w = torch.from_numpy(rs.standard_normal(tot).astype(np.float32)).to(DEV)
    seg = np.zeros(1, dtype=SEG_DT)
    seg[0] = (n0, rows * ld, 0.01, 5e-4)
    seg_dev = torch.from_numpy(seg.view(np.uint8)).to(DEV)
    st = [[w.clone(), torch.zeros_like(w), torch.zeros_like(w, dtype=torch.bfloat16)] for _ in range(4)]
    none = (drn.CLIP_NONE, 0.0, None)
    for step in range(2):
        g = torch.from_numpy(rs.standard_normal(rows * ld).astype(np.float32)).to(DEV).to(gdt)
        if gdt == torch.float32:
            ga, goff = torch.zeros_like(w), 0
            ga[n0: n0 + rows * ld] = g
        else:
            ga, goff = g, n0
        for k, clip in ((0, None), (1, none)):
            drn.sgd_step(st[k][0], st[k][1], ga, seg_dev, 1, 0.9, step == 0, 0.5, shadow=st[k][2], grad_off=goff, clip=clip)
        for k, clip in ((2, None), (3, none)):
            drn.sgd_step_block(st[k][0], st[k][1], ga, seg_dev, 0, rows, 0, ld, ld, 0.9, step == 0, 0.5, shadow=st[k][2],
                               grad_off=goff, clip=clip)
        for a, b in ((0, 1), (2, 3), (0, 2)):
            assert all(torch.equal(x, y) for x, y in zip(st[a], st[b])), (step, a, b)
    assert not torch.equal(st[0][0], w)


# ------------------------------------------------------------------------------------------------- 5. through the model
def _forever(batch):
    while True:
        yield batch


def _one_trainer_step(name, freeze_at, clip=None):
    """One Trainer step of the fixture model from its seeded weights.  Returns (optimizer, weights before, gradient arenas as the
    step saw them, weights after), each {parameter name: CPU tensor} over the optimizer's used groups."""
    from drn_wsod_pytorch_amd.engine import Trainer, build_optimizer

    ocfg, d = G.MODEL_CASES[name], G.load(name)
    cfg, model = G.drn_model(ocfg, int(d["seed"]), DEV, freeze_at, "fp32")
    if clip is not None:
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
        cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = clip
    model.roi_heads.box_head.dropout_p = 0.0
    model.train()
    opt = build_optimizer(cfg, model)
    eng = model.roi_heads._engine
    groups = [g for g in opt.param_groups if g["used"]]

    def read(heads, trunk):
        return {g["name"]: (trunk if g.get("bb") else heads)[g["off"]: g["off"] + g["cnt"]].detach().cpu().clone() for g in groups}

    w0 = read(eng.arena_w, opt._bb["w"] if opt._bb else None)
    tr = Trainer(cfg, model, _forever(G.drn_inputs(G.batch_from(d))), optimizer=opt)
    tr.run_step()
    torch.cuda.synchronize()
    grads = read(eng.arena_g, opt._bb["g"] if opt._bb else None)
    w1 = read(eng.arena_w, opt._bb["w"] if opt._bb else None)
    return opt, ocfg, w0, grads, w1


@pytest.mark.parametrize("name,freeze_at", [("model_r50c4_tiny", 5), ("model_r18dc5_tiny", 2)])
@pytest.mark.parametrize("clip_type", ["value", "norm"])
def test_trainer_step_honours_the_config_key(name, freeze_at, clip_type):
    """One plain unclipped step gives the gradient arena(s); CLIP_VALUE = the median |g| of fc2.weight (value) or the median of the
    per-parameter norms (norm); from the same initial weights one Trainer step with SOLVER.CLIP_GRADIENTS set in the config must
    equal (CPU clip of that arena as in tests 2 / 3a -> O.SGDState), bit for bit - for the heads' arena (frozen trunk) and, with
    FREEZE_AT 2 on the smallest trunk of the fixtures, for the trunk's arena too (deterministic mode: the RoI backward's float
    atomics would make the two runs' trunk gradients differ in the last bits).  Where the key is ignored the parameters come out
    unclipped and this fails."""
    pkg = load_package()
    pkg.set_deterministic(True)
    try:
        _, ocfg, w0, g, w_plain = _one_trainer_step(name, freeze_at)
        if freeze_at < 5:
            assert any(n.startswith("backbone.") for n in g)
        if clip_type == "value":
            fc2 = [n for n in g if n.endswith("fc2.weight")]
            assert len(fc2) == 1
            c = float(g[fc2[0]].abs().median())
        else:
            c = float(np.median([float(t.double().norm()) for t in g.values()]))
        assert c > 0
        opt, _, w0b, gb, w1 = _one_trainer_step(name, freeze_at, (clip_type, c))
        for n in w0:
            assert torch.equal(w0[n], w0b[n]) and torch.equal(g[n], gb[n]), n  # same start, same gradients
        if clip_type == "value":
            clipped = _cpu_clip_value(g, 1.0, c)
            share = float(torch.cat([(t.abs() > c).float().reshape(-1) for t in g.values()]).mean())
            assert 0.01 < share < 0.99, share
        else:
            names, norms = opt.last_grad_norms()
            assert names == list(g)
            norms = norms.cpu()
            for i, n in enumerate(names):
                ref = float(g[n].double().norm())
                assert abs(float(norms[i]) - ref) <= _sum_bound(2) * ref, n
            coef = _coef32(norms, c)
            assert bool((coef < 1).any()) and bool((coef == 1).any())
            clipped = {n: g[n] * coef[i] for i, n in enumerate(names)}
        p = {n: t.clone() for n, t in w0.items()}
        O.SGDState(ocfg).step(p, clipped)
        for n in p:
            assert torch.equal(w1[n], p[n]), n
        assert any(not torch.equal(w1[n], w_plain[n]) for n in p)  # and clipping changed the step
    finally:
        pkg.set_deterministic(False)
        pkg.set_precision("fp32")


# ------------------------------------------------------------------------------------------------------ 6. graphed step
def test_graphed_pipelined_step_with_value_clipping_equals_the_plain_trainer():
    """GraphedTrainStep on enable_pipelined() (every bucket's update through the clipping entry points, fc6 dW unfused) against the
    plain clipped Trainer from the same weights, three steps over three batches: the comparison of
    test_graphed_step_with_captured_sgd_follows_the_lr_schedule (1e-6 of a tensor's scale).  CLIP_TYPE 'norm' is refused."""
    from drn_wsod_pytorch_amd._cabi import DrnError
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, Trainer, build_optimizer

    name = "model_r50c4_tiny"
    d = G.load(name)
    ocfg = G.MODEL_CASES[name]
    base = G.batch_from(d)
    alt = dict(base[0])
    alt["image"] = (255.0 - base[0]["image"]).contiguous()
    alt["objectness_logits"] = base[0]["objectness_logits"].flip(0).contiguous()
    alt2 = dict(base[0])
    alt2["image"] = base[0]["image"].flip(2).contiguous()
    alt2["gt_classes"] = (base[0]["gt_classes"] + 1) % ocfg.num_classes
    seq = [G.drn_inputs([b]) for b in (base[0], alt, alt2, base[0])]
    _, _, _, g, _ = _one_trainer_step(name, 5)
    c = float(g[[n for n in g if n.endswith("fc2.weight")][0]].abs().median())

    def make(clip_type):
        cfg, model = G.drn_model(ocfg, int(d["seed"]), DEV, 5, "fp32")
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
        cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = clip_type, c
        model.roi_heads.box_head.dropout_p = 0.0
        model.train()
        return cfg, model, build_optimizer(cfg, model)

    res = []
    for graphed in (False, True):
        cfg, model, opt = make("value")
        if graphed:
            opt.enable_pipelined()
            stepper = GraphedTrainStep(model, opt, seq[0])
            for i in range(3):
                stepper.step(seq[i], seq[i + 1])
        else:
            tr = Trainer(cfg, model, iter(seq + seq), optimizer=opt)
            for i in range(3):
                tr.run_step()
        torch.cuda.synchronize()
        res.append({n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters() if p.requires_grad})
        if graphed:
            stepper.release()
    for n in res[0]:
        a, b = res[0][n], res[1][n]
        assert np.abs(a - b).max() <= 1e-6 * max(np.abs(a).max(), 1e-3), n
    # the clipping acted: the unclipped trainer ends somewhere else
    cfg, model = G.drn_model(ocfg, int(d["seed"]), DEV, 5, "fp32")
    model.roi_heads.box_head.dropout_p = 0.0
    model.train()
    tr = Trainer(cfg, model, iter(seq + seq), optimizer=build_optimizer(cfg, model))
    for i in range(3):
        tr.run_step()
    torch.cuda.synchronize()
    plain = {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters() if p.requires_grad}
    assert any(np.abs(plain[n] - res[0][n]).max() > 1e-4 * max(np.abs(plain[n]).max(), 1e-3) for n in plain)
    _, _, opt = make("norm")
    with pytest.raises(DrnError, match=r"SOLVER\.CLIP_GRADIENTS.*plain step\(\)"):
        opt.enable_pipelined()
