"""Which options combine, pinned as two full matrices (no GPU): every combination NGPTrainer's constructor accepts and every
combination of flags tools/train_dataset.py's parse_args accepts, against tests/golden/recipe_matrix.json.  The golden holds
the accepted combinations and the totals only; every other combination must be refused, the constructor's with a ValueError
and the tool's with exit code 2.  `python tests/test_recipe_host.py --record` rewrites the golden from the tree it runs in:
after adding an option (one row of recipe.py's table), extend the axes below and record again."""
import contextlib
import io
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "recipe_matrix.json")
ALL = ("semantic", "normal_mono", "depth_mono")

# ------------------------------------------------------------------------------------------- the constructor's axes
MODELS = list(itertools.product(("Sigmoid", "None"), (False, True), (False, True)))   # rgb_act, use_skybox, differentiable_normals
CLASSES = (7, 9, 17)
BOOLS = ("msk_model", "pose_refiner", "semantic", "normal_mono", "depth_mono", "use_exposure", "use_skybox", "normal_ref",
         "render_sky", "force_sharded")
MULTI = ((), ("depth_mono",), ALL)
LOSS = (None, "normal_ref", "semantic")

# ------------------------------------------------------------------------------------------- the tool's axes
FLAGS = ("--embed_msk", "--embed_a", "--optimize_ext", "--render_semantic", "--normal_mono", "--depth_mono", "--use_exposure",
         "--use_skybox", "--normal_ref", "--random_bg")
SOURCES = (("--root_dir", "x"), ("--make_proxy", "d"))
LAYOUTS = ("nerf", "tnt", "colmap")


class _Reached(Exception):
    """the constructor got as far as its parameter store: every check of the options lies before that"""


class _Head:
    n_output_dims = 7


class _Model:          # what the construction checks look at
    semantic_header = _Head()

    def __init__(self, rgb_act, use_skybox, differentiable_normals):
        self.rgb_act, self.use_skybox, self.differentiable_normals = rgb_act, use_skybox, differentiable_normals

    def named_parameters(self):
        raise _Reached


def constructor_matrix(NGPTrainer):
    """-> (number of combinations, sorted keys of the accepted ones); anything but acceptance or ValueError propagates"""
    accepted, total = [], 0
    for model, classes, multi, loss in itertools.product(MODELS, CLASSES, MULTI, LOSS):
        head = f"model={model[0]}{'+sky' if model[1] else ''}{'+dn' if model[2] else ''} num_classes={classes}"
        for bits in itertools.product((False, True), repeat=len(BOOLS)):
            on = dict(zip(BOOLS, bits))
            kw = dict(num_classes=classes, multi_terms=multi, force_sharded=on["force_sharded"],
                      msk_model=object() if on["msk_model"] else None, pose_refiner=object() if on["pose_refiner"] else None,
                      render_kwargs={"use_skybox": True} if on["render_sky"] else None, loss_kwargs={loss: True} if loss else None,
                      **{k: on[k] for k in ("semantic", "normal_mono", "depth_mono", "use_exposure", "use_skybox", "normal_ref")})
            total += 1
            try:
                NGPTrainer(_Model(*model), **kw)
            except _Reached:
                accepted.append(" ".join([head] + [b for b in BOOLS if on[b]] + ([f"multi_terms={'+'.join(multi)}"] if multi else [])
                                         + ([f"loss_kwargs={loss}"] if loss else [])))
            except ValueError:
                pass
    return total, sorted(accepted)


def cli_matrix(td):
    """-> (number of calls, sorted argument lines of the accepted ones); anything but acceptance or exit code 2 propagates"""
    accepted, total = [], 0
    for source, layout, multi in itertools.product(SOURCES, LAYOUTS, MULTI):
        base = list(source) + ["--dataset_name", layout] + (["--multi_terms"] + list(multi) if multi else [])
        for bits in itertools.product((False, True), repeat=len(FLAGS)):
            argv = base + [f for f, b in zip(FLAGS, bits) if b]
            total += 1
            try:
                with contextlib.redirect_stderr(io.StringIO()):
                    td.parse_args(argv)
            except SystemExit as e:
                assert e.code == 2, argv
            else:
                accepted.append(" ".join(argv))
    return total, sorted(accepted)


def _modules():
    for p in (ROOT, os.path.join(ROOT, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import train_dataset as td
    from ngp_amd.trainer import NGPTrainer
    return NGPTrainer, td


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_constructor_matrix_is_the_recorded_one(monkeypatch):
    monkeypatch.delenv("NGP_FORCE_SHARDED", raising=False)
    total, accepted = constructor_matrix(_modules()[0])
    g = _golden()["constructor"]
    assert total == g["total"] == 221184 and len(g["accepted"]) == 657
    assert accepted == g["accepted"], (sorted(set(accepted) - set(g["accepted"])), sorted(set(g["accepted"]) - set(accepted)))


def test_cli_matrix_is_the_recorded_one():
    total, accepted = cli_matrix(_modules()[1])
    g = _golden()["cli"]
    assert total == g["total"] == 18432 and len(g["accepted"]) == 260
    assert accepted == g["accepted"], (sorted(set(accepted) - set(g["accepted"])), sorted(set(g["accepted"]) - set(accepted)))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(pytest.main([__file__, "-q"]))
    os.environ.pop("NGP_FORCE_SHARDED", None)
    NGPTrainer, td = _modules()
    out = {}
    for name, (total, accepted) in (("constructor", constructor_matrix(NGPTrainer)), ("cli", cli_matrix(td))):
        out[name] = {"total": total, "n_accepted": len(accepted), "accepted": accepted}
        print(name, total, len(accepted))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
