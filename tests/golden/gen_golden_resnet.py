"""Golden vectors of the plain-ResNet WSDDN recipes (wsddn_R_50_DC5_1x.yaml, wsddn_R_101_DC5_1x.yaml), from the UNMODIFIED
reference (build container only).

    cd <repo> && python tests/golden/gen_golden_resnet.py [models] [state] [ckpt]

Uses the helpers of tests/golden/gen_golden.py (case_full_model, ref_harness) as they are.  Writes
  model_r50std_tiny.npz / model_r101std_tiny.npz   two images, two SGD steps, inference, the res5 map
  ref_yaml_cfgs_resnet.json                        the merged configs of the two yaml files (settings only)
  ref_state_resnet.json                            state_dict keys / shapes, trainable names, class names, output shape
                                                   of the two FULL-SIZE reference models
  ckpt_r50std_tiny.npz                             a synthetic MSRA-named (R-50.pkl blob names) checkpoint pushed through
                                                   the reference's convert_c2_detectron_names / align_and_update_state_dicts
Fixtures are arrays, names and settings; no reference source text is stored."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as GG  # noqa: E402  (installs the reference import harness)

rh = GG.rh

R50 = "PascalVOC-Detection/wsddn_R_50_DC5_1x.yaml"
R101 = "PascalVOC-Detection/wsddn_R_101_DC5_1x.yaml"
# the widths of the existing tiny fixtures (gen_golden.TINY_R50); FC_DIM shrinks FastRCNNConvFCHead, DAN_DIM the DAN neck
TINY_STD = ["MODEL.RESNETS.STEM_OUT_CHANNELS", "8", "MODEL.RESNETS.RES2_OUT_CHANNELS", "32",
            "MODEL.RESNETS.WIDTH_PER_GROUP", "8", "MODEL.ROI_HEADS.NUM_CLASSES", "5"]
TINY_R50STD = TINY_STD + ["MODEL.ROI_BOX_HEAD.FC_DIM", "64"]
TINY_R101STD = TINY_STD + ["MODEL.ROI_BOX_HEAD.DAN_DIM", "[48, 64]"]


def case_yaml_cfgs(name):
    import yaml

    from __graft_entry__ import load_package

    load_package()
    from drn_wsod_pytorch_amd.config import add_wsl_config, get_cfg

    out = {}
    for rel in (R50, R101):
        cfg = get_cfg()
        add_wsl_config(cfg)
        cfg.merge_from_file(os.path.join(rh.REF, "projects", "WSL", "configs", rel))
        out[rel] = yaml.safe_load(cfg.dump())
    path = os.path.join(HERE, name + ".json")
    with open(path, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
    print("wrote", path)


def case_state(name):
    """the two recipes at FULL size in the reference: what a released checkpoint has to fit"""
    out = {}
    for rel in (R50, R101):
        cfg, model = rh.build_reference_model(rel)
        sd = model.state_dict()
        shp = model.backbone.output_shape()
        out[rel] = {
            "keys": list(sd.keys()), "shapes": [list(t.shape) for t in sd.values()],
            "trainable": [n for n, p in model.named_parameters() if p.requires_grad],
            "classes": {"backbone": type(model.backbone).__name__, "stem": type(model.backbone.stem).__name__,
                        "block": type(model.backbone.res2[0]).__name__, "box_head": type(model.roi_heads.box_head).__name__,
                        "roi_heads": type(model.roi_heads).__name__,
                        "box_predictor": type(model.roi_heads.box_predictor).__name__},
            "output_shape": {k: {"channels": v.channels, "stride": v.stride} for k, v in shp.items()},
            "n_backbone_keys": sum(k.startswith("backbone.") for k in sd),
        }
        print(rel, len(sd), "keys,", out[rel]["n_backbone_keys"], "backbone;", out[rel]["classes"], out[rel]["output_shape"])
        del model, sd
    path = os.path.join(HERE, name + ".json")
    with open(path, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
    print("wrote", path)


def msra_style_name(model_key):
    """blob name of the ImageNet MSRA files (R-50.pkl / R-101.pkl) for a trunk key: conv1_w, res_conv1_bn_{s,b},
    res2_0_branch2a_w, res2_0_branch1_bn_s, ...; None for keys those files lack (FrozenBN statistics - the files hold
    the folded affine only - and everything outside the trunk)"""
    if not model_key.startswith("backbone."):
        return None
    parts = model_key[len("backbone."):].split(".")
    if parts[-2] == "norm":
        if parts[-1] not in ("weight", "bias"):
            return None
        leaf, body = {"weight": "bn_s", "bias": "bn_b"}[parts[-1]], parts[:-2]
    else:
        leaf, body = {"weight": "w", "bias": "b"}[parts[-1]], parts[:-1]
    if body[0] == "stem":
        return ("res_conv1_" if leaf.startswith("bn") else "conv1_") + leaf
    body = [{"conv1": "branch2a", "conv2": "branch2b", "conv3": "branch2c", "shortcut": "branch1"}.get(x, x) for x in body]
    return "_".join(body + [leaf])


def case_checkpoint_msra(name, yaml_rel, opts):
    """the recipe of gen_golden.case_checkpoint with the MSRA blob names: every blob filled with its own 1-based index; decoys:
    the classifier of the ImageNet file (fc1000_*), a *_momentum blob, a shape mismatch"""
    import importlib.util

    cfg, model = rh.build_reference_model(yaml_rel, opts)
    spec = importlib.util.spec_from_file_location("ref_c2_model_loading",
                                                  os.path.join(rh.REF, "detectron2", "checkpoint", "c2_model_loading.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sd = model.state_dict()
    ckpt, ckeys, cshapes = {}, [], []

    def add(c, shape):
        ckpt[c] = torch.full(shape, float(len(ckeys) + 1))
        ckeys.append(c)
        cshapes.append(np.array(shape))

    for k, t in sd.items():
        c = msra_style_name(k)
        if c is None:
            continue
        shape = tuple(t.shape)
        if k.endswith("res3.1.conv2.weight"):
            shape = shape[:-1] + (shape[-1] + 1,)  # shape mismatch: must be skipped with a warning
        add(c, shape)
    for extra, shape in (("fc1000_w", (10, 256)), ("fc1000_b", (10,)), ("res2_0_branch2a_w_momentum", (3,))):
        add(extra, shape)
    d = {"ckpt_keys": np.array(ckeys), "model_keys": np.array(list(sd.keys()))}
    for i, sh in enumerate(cshapes):
        d["ckpt_shape%d" % i] = sh
    blobs = {k: v for k, v in ckpt.items() if not k.endswith("_momentum")}
    msd = {k: torch.full_like(v, -1.0) for k, v in sd.items()}
    mod.align_and_update_state_dicts(msd, blobs, c2_conversion=True)
    # every loaded tensor is constant = 1-based index of its source blob; -1: the model key kept its own value
    d["map_c2"] = np.array([int(v.reshape(-1)[0].item()) for v in msd.values()], dtype=np.int64)
    new_w, new_to_orig = mod.convert_c2_detectron_names(dict(blobs))
    d["renamed"] = np.array(sorted(new_w.keys()))
    d["renamed_orig"] = np.array([new_to_orig[k] for k in sorted(new_w.keys())])
    d["cfg_opts"] = np.array([yaml_rel] + list(opts))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **d)
    print("wrote", path, "loaded:", int((d["map_c2"] > 0).sum()), "of", len(sd), "model keys from", len(blobs), "blobs")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["models", "cfgs", "state", "ckpt"]
    if "models" in which:
        # 160 x 192 (and 152 x 188, zero-padded into the same batch): the stride-32 res5 map of R-50 is 5 x 6
        GG.case_full_model("model_r50std_tiny", R50, TINY_R50STD, 71, 2, 32, 160, 192)
        GG.case_full_model("model_r101std_tiny", R101, TINY_R101STD, 72, 2, 32, 160, 192)
    if "cfgs" in which:
        case_yaml_cfgs("ref_yaml_cfgs_resnet")
    if "state" in which:
        case_state("ref_state_resnet")
    if "ckpt" in which:
        case_checkpoint_msra("ckpt_r50std_tiny", R50, TINY_R50STD)
