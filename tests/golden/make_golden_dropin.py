#!/usr/bin/env python3
"""Generates tests/golden/g15_dropin_layout.json by importing THE REFERENCE'S OWN model, operator and loss
modules on this package (ngp_amd.install_as_reference_modules registers it as `vren` / `tinycudann` /
`torch_scatter`) and recording what tests/test_dropin_reference_import.py checks this package against:

  ngp_configs       for each NGP configuration, the reference NGP's state_dict layout (name -> shape), cascades,
                    grid_size and rgb_net.n_input_dims, built on this package's tinycudann surface
  used_attributes   every attribute the reference's sources read from the three drop-in modules
  operator_classes  the autograd operator classes the reference's render() uses (present in its custom_functions)
  loss_weights      the lambda_* weights of the reference's NeRFLoss

Needs a checkout of the reference:  python tests/golden/make_golden_dropin.py <path to the reference checkout>
Nothing is computed on a GPU.  The fixture holds names and numbers only and regenerates byte-identically.
"""
import importlib.util
import json
import os
import re
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))

NGP_CONFIGS = ({"scale": 0.5}, {"scale": 8.0, "embed_a": True, "embed_a_len": 8}, {"scale": 0.5, "use_skybox": True})
OPERATOR_CLASSES = ("RayAABBIntersector", "RaySphereIntersector", "RayMarcher", "VolumeRenderer", "RefLoss", "TruncExp",
                    "TruncTanh")
LOSS_WEIGHTS = ("lambda_opa", "lambda_distortion", "lambda_depth_mono", "lambda_normal_mono", "lambda_normal_ref_rp",
                "lambda_normal_ref_ro", "lambda_sky", "lambda_semantic")


def used_attributes(ref):
    """attribute names the reference's python sources read from vren / tinycudann (as tcnn) / torch_scatter"""
    alias = {"vren": "vren", "tcnn": "tinycudann", "tinycudann": "tinycudann", "torch_scatter": "torch_scatter"}
    used = {m: set() for m in ("vren", "tinycudann", "torch_scatter")}
    for dirpath, dirnames, filenames in os.walk(ref):
        dirnames[:] = sorted(d for d in dirnames if not d.startswith(".") and d != "__pycache__")
        for fn in sorted(filenames):
            if not fn.endswith(".py"):
                continue
            src = open(os.path.join(dirpath, fn)).read()
            for mod, attr in re.findall(r"\b(vren|tcnn|tinycudann|torch_scatter)\.([A-Za-z_][A-Za-z0-9_]*)", src):
                used[alias[mod]].add(attr)
            for mod, names in re.findall(r"^\s*from\s+(vren|tinycudann|torch_scatter)\s+import\s+([^\n#]+)", src, re.M):
                used[mod].update(n.split(" as ")[0].strip(" ()") for n in names.split(","))
    return {m: sorted(v) for m, v in used.items()}


def main(ref):
    sys.path.insert(0, ROOT)
    import ngp_amd
    ngp_amd.install_as_reference_modules()
    sys.path.insert(0, ref)
    import models.custom_functions as ref_cf      # imports vren, torch_scatter
    import models.rendering  # noqa: F401         # imports vren and the operator classes
    import models.networks as ref_net             # imports tinycudann, vren
    configs = []
    for kw in NGP_CONFIGS:
        m = ref_net.NGP(**kw)
        configs.append({"kwargs": kw, "state_dict": {k: list(v.shape) for k, v in m.state_dict().items()},
                        "cascades": int(m.cascades), "grid_size": int(m.grid_size),
                        "rgb_net_n_input_dims": int(m.rgb_net.n_input_dims)})
    for name in OPERATOR_CLASSES:
        assert hasattr(ref_cf, name), name
    spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(ref, "losses.py"))
    ref_losses = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_losses)
    rl = ref_losses.NeRFLoss()
    fixture = {"ngp_configs": configs, "used_attributes": used_attributes(ref),
               "operator_classes": list(OPERATOR_CLASSES), "loss_weights": {k: getattr(rl, k) for k in LOSS_WEIGHTS}}
    path = os.path.join(OUT, "g15_dropin_layout.json")
    with open(path, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "models")):
        raise SystemExit("usage: make_golden_dropin.py <path to the reference checkout>")
    main(os.path.abspath(sys.argv[1]))
