"""Drop-in check: with this package registered as `vren` / `tinycudann` / `torch_scatter`
(ngp_amd.install_as_reference_modules), everything the reference's own model, operator and loss modules read
from those three names exists here, this package's NGP has exactly the parameter / buffer names and shapes the
reference's NGP class has when built on this tinycudann surface, and the loss carries the reference's weights
— so reference checkpoints and training scripts see the layout they expect.  What the reference's modules
expect is recorded in tests/golden/g15_dropin_layout.json (tests/golden/make_golden_dropin.py imports the
reference on this package to write it).  Nothing is computed (no GPU here)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g15_dropin_layout.json")

SCRIPT = r'''
import json
import sys
sys.path.insert(0, %(root)r)
import ngp_amd
ngp_amd.install_as_reference_modules()
fx = json.load(open(%(fixture)r))
import vren, tinycudann, torch_scatter
assert vren is ngp_amd.vren and tinycudann is ngp_amd.tinycudann and torch_scatter is ngp_amd.torch_scatter
# every attribute the reference's sources read from the three modules
for mod, names in fx["used_attributes"].items():
    m = sys.modules[mod]
    assert names, mod
    for name in names:
        assert callable(getattr(m, name, None)), (mod, name)
from ngp_amd.networks import NGP
for cfg in fx["ngp_configs"]:
    ours = NGP(**cfg["kwargs"])
    a = {k: tuple(v) for k, v in cfg["state_dict"].items()}
    b = {k: tuple(v.shape) for k, v in ours.state_dict().items()}
    assert a == b, (cfg["kwargs"], sorted(set(a.items()) ^ set(b.items())))
    assert cfg["cascades"] == ours.cascades and cfg["grid_size"] == ours.grid_size
    assert cfg["rgb_net_n_input_dims"] == ours.rgb_net.n_input_dims
# the operator classes the reference's render() uses exist with the same names here
import ngp_amd.custom_functions as cf
for name in fx["operator_classes"]:
    assert hasattr(cf, name), name
for fn in ("ray_aabb_intersect", "ray_sphere_intersect", "morton3D", "morton3D_invert", "packbits", "raymarching_train",
           "raymarching_test", "composite_alpha_fw", "composite_train_fw", "composite_train_bw", "composite_test_fw",
           "composite_refloss_fw", "composite_refloss_bw", "distortion_loss_fw", "distortion_loss_bw"):
    assert callable(getattr(vren, fn)), fn
# our loss carries the same weights as the reference's
from ngp_amd.losses import NeRFLoss
ol = NeRFLoss()
assert len(fx["loss_weights"]) == 8
for k, v in fx["loss_weights"].items():
    assert getattr(ol, k) == v, (k, getattr(ol, k), v)
print("DROPIN_OK")
'''


def test_reference_modules_import_and_build_on_this_package():
    out = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "fixture": FIXTURE}], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "DROPIN_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
