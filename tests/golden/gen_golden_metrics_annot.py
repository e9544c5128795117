"""Golden annotated-box scalars of the UNMODIFIED reference (build container only).

    cd <repo> && python tests/golden/gen_golden_metrics_annot.py [seed]

The tiny case of gen_golden_metrics.py - same yaml, options, n_img = 2, R = 48, 128 x 96, two SGD steps, dropout patched to identity,
through gen_golden's own helpers - and after each step the six UN-suffixed scalars the reference's EventStorage holds for that
iteration: roi_head/num_{fg,bg,ig}_samples (label_and_sample_proposals against the annotated boxes, roi_heads.py:256-353) and
fast_rcnn/{cls_accuracy,fg_cls_accuracy,false_negative} (WSDDNOutputs._log_accuracy of the MIL scores, fast_rcnn.py:213-235), each
with a present-flag.  Also stored: the MIL scores and the annotated-box labels of every step (so the restatement of
tests/annot_metrics_util.py can be held against the reference without a GPU), and the minimum over all rows and steps of
(top score - second score) / max|score| of the MIL scores.  The package's fp32 path agrees with the reference to about 1e-4, so with
a margin of 1e-3 or more no arg-max can flip; below that the script REFUSES to write, for the reason gen_golden_metrics.py gives.
The fixture carries its inputs.  Data only: names and numbers, no reference source text.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as GG  # noqa: E402  (installs the reference harness on import)
from detectron2.utils.events import EventStorage  # noqa: E402

NAME, YAML, SEED, N_IMG, R, H, W, STEPS = ("metrics_annot_r50c4_tiny", "PascalVOC-Detection/oicr_WSR_50_DC5_1x.yaml", 132, 2, 48, 128,
                                           96, 2)
MIN_MARGIN = 1e-3
NAMES = ("roi_head/num_fg_samples", "roi_head/num_bg_samples", "roi_head/num_ig_samples", "fast_rcnn/cls_accuracy",
         "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative")


def main(seed=SEED):
    from detectron2.solver import build_optimizer

    opts = GG.TINY_R50 + GG.C4
    cfg, model = GG.rh.build_reference_model(YAML, opts)
    GG.fill_reference(model, seed)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    batch = GG.make_inputs(N_IMG, R, K, H, W, seed + 17)
    model.train()
    opt = build_optimizer(cfg, model)
    scores, labels = [], []
    heads = model.roi_heads
    hook = heads.box_predictor.register_forward_hook(lambda mod, inp, out: scores.append(out[0].detach().clone()))
    real_label = heads.label_and_sample_proposals

    def spy(proposals, targets, *a, **kw):  # the first call of a step is the one against the annotated boxes (no suffix)
        out = real_label(proposals, targets, *a, **kw)
        if not kw.get("suffix") and not (len(a) > 1 and a[1]):
            labels.append(torch.cat([p.gt_classes for p in (out[0] if isinstance(out, tuple) else out)]).clone())
        return out

    heads.label_and_sample_proposals = spy
    per_step, margin, kept = [], float("inf"), []
    with EventStorage() as storage, GG.DropoutPatch(None):
        for step in range(STEPS):
            del scores[:], labels[:]
            opt.zero_grad()
            losses = model(GG.to_ref_inputs(batch))
            sum(losses.values()).backward()
            opt.step()
            now = {}
            for k, h in storage.histories().items():
                if k in NAMES:
                    vals = [v for v, it in h.values() if int(it) == storage.iter]
                    if vals:
                        assert len(vals) == 1, (k, vals)
                        now[k] = float(vals[0])
            per_step.append(now)
            assert len(scores) == 1 and len(labels) == 1, (len(scores), len(labels))
            x = scores[0]
            assert x.shape == (N_IMG * R, K), x.shape
            top = torch.topk(x, 2, dim=1).values
            margin = min(margin, float(((top[:, 0] - top[:, 1]) / x.abs().max(dim=1).values).min()))
            kept.append((x.numpy().astype(np.float32), labels[0].numpy().astype(np.int64)))
            storage.step()
    hook.remove()
    print("seed", seed, "margin", margin, "scalars per step", [len(s) for s in per_step])
    if not margin >= MIN_MARGIN:
        raise SystemExit("refusing to write: the smallest relative arg-max margin %.3g is below %.0e - another seed is needed"
                         % (margin, MIN_MARGIN))
    d = {"seed": np.int64(seed), "steps": np.int64(STEPS), "min_margin": np.float64(margin), "names": np.array(NAMES),
         "num_classes": np.int64(K), "iou_thresholds": np.array(cfg.MODEL.ROI_HEADS.IOU_THRESHOLDS, dtype=np.float64),
         "iou_labels": np.array(cfg.MODEL.ROI_HEADS.IOU_LABELS, dtype=np.int64)}
    GG.flat_batch(batch, d)
    for s, now in enumerate(per_step):
        d["step%d" % s] = np.array([now.get(k, 0.0) for k in NAMES], dtype=np.float64)
        d["present%d" % s] = np.array([k in now for k in NAMES], dtype=np.bool_)
        d["mil_scores%d" % s], d["labels%d" % s] = kept[s]
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes")
    for s, now in enumerate(per_step):
        print(s, now)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    main(int(sys.argv[1]) if len(sys.argv) > 1 else SEED)
