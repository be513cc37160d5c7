"""tools/step_bench.py: one spec per recipe behind one parser (host only: nothing here launches)."""
import dataclasses
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "step_bench.py")

# the legs of every recipe, under the names the tools of the recipes' own commits gave them (use_exposure's tool had two)
LEGS = {
    "semantic": ("default", "module", "fused"),
    "normal_mono": ("default", "module", "fused"),
    "depth_mono": ("default", "module", "fused"),
    "multi_terms": ("default", "module", "multi"),
    "use_exposure": ("layered", "fused"),
    "use_skybox": ("default", "module", "fused"),
    "normal_ref": ("default", "module", "fused"),
    "masked": ("default", "layered", "fused"),
    "embed_a": ("none", "tensor", "fused"),
    "pose": ("none", "torch", "kernels"),
}


def _help(*argv):
    out = subprocess.run([sys.executable, TOOL, *argv, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("step_bench_under_test", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_import_initialises_nothing():
    """in a process of its own: importing the tool neither initialises the GPU nor loads libngp_hip.so"""
    code = ("import runpy, sys, torch; runpy.run_path(sys.argv[1], run_name='step_bench'); from ngp_amd import _lib; "
            "print('cuda', torch.cuda.is_initialized(), 'lib', _lib._lib is not None)")
    out = subprocess.run([sys.executable, "-c", code, TOOL], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["cuda", "False", "lib", "False"], out.stdout


def test_every_option_of_the_recipe_has_a_spec(tool):
    from ngp_amd.recipe import Recipe
    options = [f.name for f in dataclasses.fields(Recipe) if f.init and f.name not in ("fused_loss", "unit_exposure_rgb")]
    assert sorted(tool.SPECS) == sorted(options)
    assert {name: tuple(spec.legs) for name, spec in tool.SPECS.items()} == LEGS


def test_help_names_all_recipes():
    out = _help()
    for name in LEGS:
        assert re.search(rf"\b{name}\b", out), name


@pytest.mark.parametrize("recipe", sorted(LEGS))
def test_recipe_help_shows_exactly_its_legs(recipe):
    out = _help(recipe)
    shown = set(re.findall(r"\{(\w+(?:,\w+)+)\}", out))
    assert shown == {",".join(LEGS[recipe])}, shown
    for flag in ("--rays", "--steps", "--warmup", "--windows", "--solo"):
        assert flag in out, flag
