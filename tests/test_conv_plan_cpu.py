"""CPU test of the convolution forward's kernel choice as drn_conv2d_plan reports it (the query is host-only: pointers are
inspected, never dereferenced, so dummy addresses of the wanted alignment stand in for tensors).

The expected kinds in golden/conv_plan_recorded.json were RECORDED from the library as it was before the choice moved into
conv_fwd_plan: a build of that commit whose conv launchers returned a code instead of launching, driven through
drn_conv2d_nhwc_q with the cases of blocks() below.  They are never regenerated from the code under test: a row that
changes is a layer that changed kernel.  One character per case: 'a' + kind - 1, upper case with DRN_CONV_KIND_FP8_K16,
'!' = DRN_ERR_ARG; the file holds each block run-length coded (a character, then its repeat count when above one)."""
import importlib
import json
import os
import re

import pytest

import golden_util as G
from __graft_entry__ import build

F32, BF16, FP8 = 0, 1, 2
ES = {F32: 4, BF16: 2, FP8: 1}
RECORDED = os.path.join(G.ROOT, "tests", "golden", "conv_plan_recorded.json")

# dummy, distinct, 256-byte aligned addresses of x, w, y, residual, scale, bias
BASE = {"x": 1 << 28, "w": 2 << 28, "y": 3 << 28, "res": 4 << 28, "scale": 5 << 28, "bias": 6 << 28}


def case(H, W, Cin, Cout, k=1, Nb=1, dt=BF16, out=None, res=None, stride=1, pad=None, dil=1, kh=None, kw=None, affine=True, **over):
    """one call of drn_conv2d_nhwc_q / drn_conv2d_plan as a dict; `res` = the residual's dtype or None; `over` overrides fields
    (ldw / ldy / ldres, or x / w / y / res / scale / bias = byte offset from the aligned dummy address, None = NULL)"""
    kh, kw = kh or k, kw or k
    es = ES.get(dt, 2)
    c = dict(Nb=Nb, H=H, W=W, Cin=Cin, Cout=Cout, KH=kh, KW=kw, stride=stride, pad=dil * (kh // 2) if pad is None else pad, dil=dil,
             ldw=(kh * kw * Cin * es + 127) // 128 * 128 // es, ldy=Cout, ldres=Cout, relu=1, dt=dt, out=dt if out is None else out,
             rdt=0 if res is None else res, x=0, w=0, y=0, res=None if res is None else 0, scale=0 if affine else None,
             bias=0 if affine else None)
    c.update(over)
    return c


def call_args(c):
    p = lambda n: None if c[n] is None else BASE[n] + c[n]
    return (p("x"), p("w"), p("y"), p("scale"), p("bias"), p("res"), c["Nb"], c["H"], c["W"], c["Cin"], c["Cout"], c["KH"], c["KW"],
            c["stride"], c["pad"], c["dil"], c["ldw"], c["ldy"], c["ldres"], c["relu"], c["dt"], c["out"], c["rdt"], 1.0)


# ---- real layers ---------------------------------------------------------------------------------------------------------------
def _half(h):  # 3x3 / stride 2 / pad 1 conv, and the 3x3 / stride 2 / pad 1 pool
    return (h + 2 - 2 - 1) // 2 + 1


def _pool2(h, s):  # MaxPool2d(2, s)
    return (h - 2) // s + 1


def ws_resnet(depth, dc5, H, W):
    """(H, W, Cin, Cout, k, stride, dil, has_residual) of every conv of the WS-ResNet trunk: deep stem at 1/2, res2 at 1/4, res3 at
    1/8, res4 (and res5 of the dilated-C5 form, both dilation 2) behind res3's pool of stride 2 (C4) / 1 (dilated C5)"""
    L = [(H, W, 0, 64, 3, 2, 1, False)]
    h, w = _half(H), _half(W)
    L += [(h, w, 64, 64, 3, 1, 1, False)] * 2
    h, w = _pool2(h, 2), _pool2(w, 2)
    cin, cout, bc = 64, 64 if depth == 18 else 256, 64
    for stage in (2, 3, 4, 5) if dc5 else (2, 3, 4):
        dil = 2 if dc5 and stage >= 4 else 1
        for first in (True, False):
            ci = cin if first else cout
            if depth == 18:
                L += [(h, w, ci, cout, 3, 1, dil, False), (h, w, cout, cout, 3, 1, dil, True)]
            else:
                L += [(h, w, ci, bc, 1, 1, 1, False), (h, w, bc, bc, 3, 1, dil, False), (h, w, bc, cout, 1, 1, 1, True)]
            if first and ci != cout:
                L.append((h, w, ci, cout, 1, 1, 1, False))
        if stage == 2:
            h, w = _pool2(h, 2), _pool2(w, 2)
        elif stage == 3:
            h, w = (_pool2(h, 1), _pool2(w, 1)) if dc5 else (_pool2(h, 2), _pool2(w, 2))
        cin, cout, bc = cout, cout * 2, bc * 2
    return L


def std_resnet(dc5, H, W):
    """the standard ResNet-50 / 101 trunk (stride in the 1x1): 7x7 stem, res2 .. res5, res5 dilated (stride 1) in the DC5 form"""
    L = [(H, W, 0, 64, 7, 2, 1, False)]
    h, w = _half(_half(H)), _half(_half(W))
    cin, cout, bc = 64, 256, 64
    for stage in (2, 3, 4, 5):
        s = 1 if stage == 2 or (stage == 5 and dc5) else 2
        dil = 2 if stage == 5 and dc5 else 1
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        L += [(h, w, cin, bc, 1, s, 1, False), (ho, wo, bc, bc, 3, 1, dil, False), (ho, wo, bc, cout, 1, 1, 1, True),
              (h, w, cin, cout, 1, s, 1, False)]
        h, w = ho, wo
        L += [(h, w, cout, bc, 1, 1, 1, False), (h, w, bc, bc, 3, 1, dil, False), (h, w, bc, cout, 1, 1, 1, True)]
        cin, cout, bc = cout, cout * 2, bc * 2
    return L


def vgg16(d2, H, W):
    L, h, w, cin = [], H, W, 0
    for i, (cout, n) in enumerate(((64, 2), (128, 2), (256, 3), (512, 3), (512, 3))):
        dil = 2 if d2 and i == 4 else 1
        for _ in range(n):
            L.append((h, w, cin, cout, 3, 1, dil, False))
            cin = cout
        if i < 3 or (i == 3 and not d2):
            h, w = _pool2(h, 2), _pool2(w, 2)
        elif i == 3:
            h, w = _pool2(h, 1), _pool2(w, 1)
    return L


SIZES = ((800, 1216), (608, 800), (480, 640), (224, 224))
# (dtype, out_dtype, res_dtype) of a layer: bf16, fp32, and the fp8 trunk's: fp8 throughout, fp8 -> bf16 feature map, bf16 shortcut
DTYPES = ((BF16, BF16, BF16), (F32, F32, F32), (FP8, FP8, FP8), (FP8, BF16, FP8), (FP8, FP8, BF16))


def real_layers(sizes=SIZES, nbs=(1, 2, 4)):
    seen, out = set(), []
    for H, W in sizes:
        layers = []
        for depth in (18, 50):  # (depth 101 repeats depth 50's layers)
            for dc5 in (False, True):
                layers += ws_resnet(depth, dc5, H, W)
        layers += std_resnet(False, H, W) + std_resnet(True, H, W) + vgg16(False, H, W) + vgg16(True, H, W)
        for (h, w, cin, cout, k, s, dil, has_res) in layers:
            for Nb in nbs:
                for dt, odt, rdt in DTYPES:
                    if cin == 0:  # the image: channels padded to one 16-byte chunk; the fp8 trunk's stem reads bf16 and writes fp8
                        d, ci, o = (BF16, 8, FP8) if dt == FP8 else (dt, 16 // ES[dt], odt)
                    else:
                        d, ci, o = dt, cin, odt
                    key = (h, w, ci, cout, k, s, dil, has_res, Nb, d, o, rdt if has_res else 0)
                    if key in seen:
                        continue
                    seen.add(key)
                    out.append(case(h, w, ci, cout, k, Nb, d, o, rdt if has_res else None, stride=s, dil=dil, pad=dil * (k // 2)))
    return out


# ---- both sides of every threshold of the cascade -------------------------------------------------------------------------------
def threshold_cases():
    out = []
    # one image's pixels: 64 * t for the 64x64-tile counts around CUs / 4, CUs, 4 CUs (256 and 64 CUs) and the ks / k2 limits;
    # 1023 / 1024; 256 * {99, 100, 191, 192} (t256); 128 * and 256 * {39, 40, 159, 160} (t128 * 8 against 5 CUs, narrow and wide)
    hw = [(t, 64) for t in (1, 3, 4, 8, 15, 16, 17, 39, 40, 41, 63, 64, 65, 66, 100000 // 64 // 64, 128, 255, 256, 257, 258, 1023, 1024, 1025, 1026)]
    hw += [(33, 31), (32, 32), (7, 7), (14, 14), (28, 28), (99, 256), (100, 256), (191, 256), (192, 256), (39, 128), (40, 128),
           (159, 128), (160, 128), (39, 256), (40, 256), (159, 256), (160, 256), (50, 256), (96, 256)]
    for H, W in hw:
        for Cout in (64, 65, 127, 128, 255, 256, 512, 1024):
            for Cin in (64, 192, 256, 448, 512, 576, 640, 960, 1024, 1984, 2048):  # slabs 1, 3 / 4, 7 / 8, 9 / 10, 15 / 16, 31 / 32
                out.append(case(H, W, Cin, Cout, 1, res=BF16 if Cin % 128 == 0 else None))
        for Cout in (64, 128, 256, 512):
            for Cin in (64, 128, 256, 512):  # slabs 9, 18, 36, 72
                out.append(case(H, W, Cin, Cout, 3))
    # the LDS-resident patch kernel's pixel threshold (32768, and 5000 as the tests set it); with and without a shortcut, batched
    for H, W in ((181, 181), (127, 258), (128, 256), (256, 256), (70, 71), (50, 100), (71, 71)):
        for Nb in (1, 2):
            out += [case(H, W, 64, 64, 3, Nb), case(H, W, 64, 64, 3, Nb, res=BF16), case(H, W, 64, 64, 3, Nb, out=FP8),
                    case(H, W, 64, 64, 3, Nb, dil=2), case(H, W, 64, 128, 3, Nb)]
    # the small-map kernels: batch 64 / 65, a batch that leaves the "small" tiled class, taps 32 / 33, other operand types
    for Nb in (1, 8, 64, 65, 128):
        for H, W in ((7, 7), (14, 14), (28, 28), (56, 56)):
            for Cin, Cout, k in ((256, 256, 3), (1024, 256, 1), (512, 2048, 1), (64, 64, 3), (1024, 2048, 1), (256, 64, 1)):
                for dt, o, r in DTYPES:
                    out.append(case(H, W, Cin, Cout, k, Nb, dt, o, r if k == 1 else None))
    for kh, kw in ((4, 8), (3, 11), (8, 4), (5, 7), (7, 7)):
        for H, W in ((40, 40), (100, 100)):
            out += [case(H, W, 64, 128, kh=kh, kw=kw, pad=0), case(H, W, 128, 256, kh=kh, kw=kw, pad=0)]
    # fp32 slabs are 32 channels: 31 / 32 slabs, odd / even
    for H, W in ((7, 7), (14, 14), (20, 20), (32, 32), (64, 64)):
        for Cin in (96, 128, 224, 256, 288, 992, 1024):
            out += [case(H, W, Cin, 256, 1, dt=F32), case(H, W, Cin * 4, 256, 1, dt=FP8), case(H, W, Cin * 4, 64, 1, dt=FP8, out=BF16)]
    return out


# ---- misalignment: each pointer off by 4 and by 8 bytes, leading dimensions with ld & 3 and ld & 7 non-zero ------------------------------
def misaligned_cases():
    base = [case(200, 304, 64, 64, 3, res=BF16),       # patch
            case(200, 304, 64, 256, 1, res=BF16),      # 256x256 ping-pong
            case(100, 152, 256, 256, 3, res=BF16),     # pp8
            case(50, 76, 256, 1024, 1, res=BF16),      # ring
            case(50, 76, 1024, 256, 1, res=BF16),
            case(14, 14, 256, 256, 3, res=BF16),       # small map
            case(50, 76, 1024, 256, 1, dt=FP8, res=FP8)]
    out = list(base)
    for c in base:
        for name in ("x", "w", "y", "res", "scale", "bias"):
            for off in (4, 8):
                out.append(dict(c, **{name: off}))
        for name in ("ldy", "ldres"):
            for extra in (2, 4, 8):
                out.append(dict(c, **{name: c[name] + extra}))
        out.append(dict(c, ldw=c["ldw"] + 128 // ES[c["dt"]]))
        out += [dict(c, scale=None), dict(c, bias=None), dict(c, scale=None, bias=None)]
    return out


# ---- one row per DRN_ERR_ARG condition of drn_conv2d_nhwc_q (and their nearest accepted neighbours) ----------------------------------
def argument_cases():
    ok = case(14, 14, 256, 256, 3, res=BF16)
    return [ok, dict(ok, x=None), dict(ok, w=None), dict(ok, y=None), dict(ok, dt=3), dict(ok, dt=-1), dict(ok, out=3), dict(ok, rdt=3),
            dict(ok, res=None, rdt=3), dict(ok, Cin=4), dict(ok, Cin=12, dt=F32), dict(ok, Cin=8, dt=FP8), dict(ok, ldw=ok["ldw"] + 4),
            dict(ok, ldw=ok["ldw"] + 8), case(2, 14, 64, 64, 3, pad=0), case(14, 2, 64, 64, 3, pad=0), dict(ok, Nb=0), dict(ok, Nb=-1),
            case(2048, 2048, 512, 64, 1), case(2048, 2048, 512, 64, 1, dt=FP8), case(2048, 2048, 256, 64, 1, dt=F32),
            dict(ok, ldw=ok["ldw"] - 64), dict(ok, ldw=9 * 256), case(14, 14, 72, 64, 1, ldw=72), case(14, 14, 72, 64, 1)]


# every conv knob at every non-default value the tests and tools use
KNOBS = {"ksplit0": {5: 0}, "ks_tiles40": {7: 40}, "k2_tiles0": {8: 0}, "k2_tiles_large": {8: 100000}, "patch0": {9: 0},
         "patch5000": {9: 5000}, "fp8_k64_0": {13: 0}, "ring0": {23: 0}, "ring64": {23: 64}, "ring128": {23: 128}, "pp0": {24: 0},
         "pp300": {24: 300}, "pp8_0": {25: 0}, "pp8_2": {25: 2}, "pp8_wide0": {29: 0}, "pp8_wide2": {29: 2},
         # the "everything off" setting of the pinned-kernel tests
         "all_off": {25: 0, 23: 0, 8: 0, 5: 0, 24: 0}}


def blocks():
    """[(name, {knob: value}, cus, [case, ...])], deterministic"""
    real, swept = real_layers(), real_layers(sizes=((800, 1216), (224, 224)), nbs=(1, 2))
    synth = threshold_cases() + misaligned_cases() + argument_cases()
    out = [("real/256", {}, 256, real), ("real/64", {}, 64, real), ("synth/256", {}, 256, synth), ("synth/64", {}, 64, synth),
           ("swept/256", {}, 256, swept)]
    for name, knobs in KNOBS.items():
        out += [("synth/256/" + name, knobs, 256, synth), ("swept/256/" + name, knobs, 256, swept)]
    return out


def encode(rc):
    if rc < 0:
        return "!" if rc == -1 else "?"
    ch = chr(ord("a") + (rc & 0xff) - 1)
    return ch.upper() if rc & 0x100 else ch


def run_blocks(fn, tune):
    """fn(*call_args(case), cus) -> code; tune(knob, value) -> previous value.  Each knob is restored after its rows."""
    got = {}
    for name, knobs, cus, cases in blocks():
        prev = [(k, tune(k, v)) for k, v in knobs.items()]
        try:
            got[name] = "".join(encode(fn(*call_args(c), cus)) for c in cases)
        finally:
            for k, old in reversed(prev):
                tune(k, old)
    return got


@pytest.fixture(scope="module")
def ops():
    build()
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


@pytest.fixture(scope="module")
def recorded():
    return {name: "".join(ch * int(n or 1) for ch, n in re.findall(r"(\D)(\d*)", rle)) for name, rle in json.load(open(RECORDED)).items()}


def test_ops_conv_kinds_equal_header(ops):
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    want = {name: int(val, 0) for name, val in re.findall(r"^#define DRN_(CONV_KIND_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)\b", hdr, re.M)}
    mine = {n: v for n, v in vars(ops).items() if n.startswith("CONV_KIND_") and isinstance(v, int)}
    assert len(want) == 12 and mine == want, set(mine.items()) ^ set(want.items())
    kinds = sorted(v for n, v in want.items() if n != "CONV_KIND_FP8_K16")
    assert kinds == list(range(1, 12)) and want["CONV_KIND_FP8_K16"] == 0x100
    assert set(ops.CONV_KINDS_TILED) == {ops.CONV_KIND_TILED_64, ops.CONV_KIND_TILED_128X64, ops.CONV_KIND_TILED_128}


def test_recorded_table_is_not_vacuous(recorded):
    """asserted on the RECORDED data alone: every kind and the K = 16 flag at least five times, every knob setting moves a row"""
    allrows = "".join(recorded.values())
    for ch in "abcdefghijk":
        assert allrows.count(ch) + allrows.count(ch.upper()) >= 5, ch
    assert sum(ch.isupper() for ch in allrows) >= 5
    assert allrows.count("!") >= 15
    for name in KNOBS:
        moved = sum(a != b for pre in ("synth/256", "swept/256")
                    for a, b in zip(recorded[pre], recorded[pre + "/" + name]))
        assert moved >= 1, name
    assert recorded["real/256"] != recorded["real/64"] and recorded["synth/256"] != recorded["synth/64"]


def test_plan_reproduces_recorded_kinds(ops, recorded):
    lib = ops.C.lib()
    got = run_blocks(lib.drn_conv2d_plan, lib.drn_tune)
    assert set(got) == set(recorded)
    bl = {name: cases for name, _, _, cases in blocks()}
    for name in got:
        assert len(got[name]) == len(recorded[name]) == len(bl[name]), name
        bad = [(i, recorded[name][i], got[name][i], bl[name][i]) for i in range(len(got[name])) if got[name][i] != recorded[name][i]]
        assert not bad, "%s: %d rows changed kernel, first (row, recorded, now, case): %r" % (name, len(bad), bad[0])
    # the knobs are back at their defaults: the default block reads the same again
    assert "".join(encode(lib.drn_conv2d_plan(*call_args(c), 256)) for c in bl["synth/256"]) == recorded["synth/256"]


def test_ops_conv2d_plan_takes_tensors(ops, recorded):
    """ops.conv2d_plan takes what ops.conv2d_nhwc_q takes (nothing is dereferenced: host tensors do) and gives the recorded kinds"""
    import torch
    c = case(50, 76, 1024, 256, 1, res=BF16)
    bl = {name: cases for name, _, _, cases in blocks()}
    want = lambda block: ord(recorded[block][bl[block].index(c)]) - ord("a") + 1
    x = torch.zeros((1, 50, 76, 1024), dtype=torch.bfloat16)
    w = torch.zeros((256, 1024), dtype=torch.bfloat16)
    sc, bi, res = torch.ones(256), torch.zeros(256), torch.zeros((1, 50, 76, 256), dtype=torch.bfloat16)
    plan = lambda: ops.conv2d_plan(x, w, 256, 1, 1, 1, 0, 1, sc, bi, torch.bfloat16, residual=res, relu=True, cus=256)
    assert plan() == want("synth/256") == ops.CONV_KIND_RING_64
    with ops.tuned({ops.TUNE_CONV_RING: 128}):
        assert plan() == want("synth/256/ring128") == ops.CONV_KIND_RING_128
    with ops.tuned(KNOBS["all_off"]):
        assert plan() == want("synth/256/all_off") and plan() in ops.CONV_KINDS_TILED
    assert plan() == ops.CONV_KIND_RING_64
    with pytest.raises(ops.C.DrnError):
        ops.conv2d_plan(x[..., :4].contiguous(), w, 256, 1, 1, 1, 0, 1, sc, bi, torch.bfloat16)
