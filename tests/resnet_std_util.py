"""Helpers of the plain-ResNet WSDDN tests (wsddn_R_50_DC5_1x.yaml / wsddn_R_101_DC5_1x.yaml): the recipes are loaded from
their recorded merged configs (tests/golden/ref_yaml_cfgs_resnet.json, written by tests/golden/gen_golden_resnet.py from the
unmodified yaml files), the tiny fixtures add the overrides they recorded themselves (`cfg_opts`)."""
import json
import os

import yaml

import golden_util as G

R50 = "PascalVOC-Detection/wsddn_R_50_DC5_1x.yaml"
R101 = "PascalVOC-Detection/wsddn_R_101_DC5_1x.yaml"
CASES = {"model_r50std_tiny": R50, "model_r101std_tiny": R101}
CFGS = os.path.join(G.GOLDEN, "ref_yaml_cfgs_resnet.json")
STATE = os.path.join(G.GOLDEN, "ref_state_resnet.json")


def recorded_cfg(yaml_rel, tmp_dir, opts=(), device="cpu"):
    """get_cfg() + add_wsl_config() + merge_from_file(<the recorded merged config, written back as a yaml file>)"""
    from __graft_entry__ import load_package

    load_package()
    from drn_wsod_pytorch_amd.config import add_wsl_config, get_cfg

    with open(CFGS) as f:
        rec = json.load(f)[yaml_rel]
    path = os.path.join(str(tmp_dir), os.path.basename(yaml_rel))
    with open(path, "w") as f:
        f.write(yaml.safe_dump(rec))
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(path)
    cfg.merge_from_list(["MODEL.DEVICE", device, "MODEL.WEIGHTS", ""] + [str(o) for o in opts])
    return cfg


def reference_state(yaml_rel):
    with open(STATE) as f:
        return json.load(f)[yaml_rel]


def tiny_model(name, tmp_dir, device="cuda", precision="fp32"):
    """the fixture's model: recorded recipe + the fixture's overrides, filled with the name-seeded weights the reference
    model held when the fixture was written -> (cfg, model, fixture dict)"""
    from __graft_entry__ import load_package

    pkg = load_package()
    pkg.set_precision(precision)
    from drn_wsod_pytorch_amd.modeling import build_model

    d = G.load(name)
    opts = [str(o) for o in d["cfg_opts"]]
    assert opts[0] == CASES[name]
    cfg = recorded_cfg(opts[0], tmp_dir, opts[1:], device)
    model = build_model(cfg)
    sd = model.state_dict()
    seed = int(d["seed"])
    model.load_state_dict({n: (t if n in ("pixel_mean", "pixel_std") else G.O.seeded_tensor(n, tuple(t.shape), seed))
                           for n, t in sd.items()})
    return cfg, model, d
