"""Golden label statistics of the UNMODIFIED reference (build container only).

    cd <repo> && python tests/golden/gen_golden_metrics.py [seed]

Reruns the model_r50c4_tiny case of gen_golden.py - same yaml, options, n_img = 2, R = 48, 128 x 96, two SGD steps, dropout
patched to identity - through gen_golden's own helpers, and after each step reads every `*_r{k}` scalar the
reference's EventStorage holds for that iteration: fast_rcnn/{cls_accuracy,fg_cls_accuracy,false_negative}_r{k}
(fast_rcnn.py:1098-1126) and roi_head/num_{fg,bg,ig}_samples_r{k} (roi_heads.py:338-349, roi_heads_oicr.py:366-374).  Also stored:
the minimum over all rows, branches and steps of (top logit - second logit) / max|logit| of the refinement logits.  The package's
fp32 path agrees with the reference to about 1e-4, so with a margin of 1e-3 or more no arg-max can flip; below that the script
REFUSES to write.  model_r50c4_tiny's own seeds (weights 32, inputs 49) give a margin of 8.2e-5 and are refused; seed 132
(weights 132, inputs 149) gives 1.4e-3 and is the one the committed fixture holds, so the fixture carries its inputs as well.
Data only: names and numbers, no reference source text.
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as GG  # noqa: E402  (installs the reference harness on import)
from detectron2.utils.events import EventStorage  # noqa: E402

NAME, YAML, SEED, N_IMG, R, H, W, STEPS = "metrics_r50c4_tiny", "PascalVOC-Detection/oicr_WSR_50_DC5_1x.yaml", 132, 2, 48, 128, 96, 2
MIN_MARGIN = 1e-3
_BRANCH = re.compile(r"_r\d+$")


def _val(v):
    return float(v[0] if isinstance(v, tuple) else v)  # (newer storages keep (value, iteration))


def main(seed=SEED):
    from detectron2.solver import build_optimizer

    opts = GG.TINY_R50 + GG.C4
    cfg, model = GG.rh.build_reference_model(YAML, opts)
    GG.fill_reference(model, seed)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    batch = GG.make_inputs(N_IMG, R, K, H, W, seed + 17)
    model.train()
    opt = build_optimizer(cfg, model)
    logits = []
    hooks = []
    for n, m in model.named_modules():
        if re.search(r"box_refinery_\d+\.cls_score$", n):
            hooks.append(m.register_forward_hook(lambda mod, inp, out: logits.append(out.detach().clone())))
    assert len(hooks) == cfg.WSL.REFINE_NUM, [n for n, _ in model.named_modules()]
    per_step, margin = [], float("inf")
    with EventStorage() as storage, GG.DropoutPatch(None):
        for step in range(STEPS):
            del logits[:]
            opt.zero_grad()
            losses = model(GG.to_ref_inputs(batch))
            sum(losses.values()).backward()
            opt.step()
            hist = storage.histories()
            now = {}
            for k, h in hist.items():
                if _BRANCH.search(k) and ("fast_rcnn/" in k or "roi_head/" in k):
                    vals = [v for v, it in h.values() if int(it) == storage.iter]
                    if vals:
                        assert len(vals) == 1, (k, vals)
                        now[k] = float(vals[0])
            per_step.append(now)
            assert len(logits) == cfg.WSL.REFINE_NUM
            for x in logits:
                top = torch.topk(x, 2, dim=1).values
                margin = min(margin, float(((top[:, 0] - top[:, 1]) / x.abs().max(dim=1).values).min()))
            storage.step()
    names = sorted(set().union(*[set(s) for s in per_step]))
    print("seed", seed, "margin", margin, "scalars per step", [len(s) for s in per_step])
    if not margin >= MIN_MARGIN:
        raise SystemExit("refusing to write: the smallest relative arg-max margin %.3g is below %.0e - another seed is needed"
                         % (margin, MIN_MARGIN))
    d = {"seed": np.int64(seed), "steps": np.int64(STEPS), "min_margin": np.float64(margin), "names": np.array(names)}
    GG.flat_batch(batch, d)  # the inputs travel with the fixture (needed whenever the seed is not model_r50c4_tiny's)
    for s, now in enumerate(per_step):
        d["step%d" % s] = np.array([now.get(k, 0.0) for k in names], dtype=np.float64)
        d["present%d" % s] = np.array([k in now for k in names], dtype=np.bool_)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes")
    for s, now in enumerate(per_step):
        print(s, now)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    main(int(sys.argv[1]) if len(sys.argv) > 1 else SEED)
