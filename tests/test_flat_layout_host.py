"""trainer.flat_layout: where every parameter lies in the flat store, as a pure function of [(name, numel)] and the number
of ranks (no GPU, launches nothing).  The alignment rules every kernel that sweeps the store relies on (every slice starts
on 16 bytes; every bucket, and so every rank's shard of it, is a whole number of 16-byte groups per rank), over worlds 1, 2,
3 and 8 and name lists with and without the two tables, with sizes that are no multiple of 4; and for the models the GPU
tests train, the layout the trainer's _flatten produced at 0798391 (tests/golden/flat_layouts.json, recorded there on
the meta device, one rank)."""
import json
import os

import pytest
import torch

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_layouts.json")
RGB, XYZ = "rgb_encoder.params", "xyz_encoder.params"
MLPS = [("xyz_net.0.weight", 130), ("xyz_net.0.bias", 1), ("rgb_net.params", 7), ("semantic_header.params", 3)]
BEHIND = [("msk_model.mask_encoder.params", 1026), ("msk_model.mask_net.0.bias", 3), ("embedding_a.weight", 7 * 5)]
NAME_LISTS = {
    "model_order": [(XYZ, 4099)] + MLPS[:2] + [(RGB, 1001)] + MLPS[2:],      # the tables are moved to the front, colour first
    "without_colour_table": [(XYZ, 4099)] + MLPS,
    "without_tables": MLPS,
    "tables_only": [(XYZ, 130), (RGB, 7)],
    "mask_and_codes_behind": [(XYZ, 4099)] + MLPS[:2] + [(RGB, 1001)] + MLPS[2:] + BEHIND,
    "multiples_of_four": [(RGB, 4096), (XYZ, 2048), ("xyz_net.0.weight", 128)],
}


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("case", list(NAME_LISTS))
def test_alignment_order_and_buckets(ngp, case, world):
    from ngp_amd.trainer import flat_layout
    named = NAME_LISTS[case]
    lay = flat_layout(named, world)
    given = [n for n, _ in named]
    lead = [n for n in (RGB, XYZ) if n in given]
    assert list(lay.names) == lead + [n for n in given if n not in lead] and lay.world == world
    assert {n: k for n, (_, k) in lay.slices.items()} == dict(named) and len(lay.sizes) == len(named)
    has_colour = RGB in given
    assert lay.bounds == ((0, lay.b0, lay.total) if has_colour else (0, lay.total)) and lay.total == lay.bounds[-1]
    assert (lay.b0 > 0) == has_colour
    for lo, hi in zip(lay.bounds, lay.bounds[1:]):
        assert hi > lo and (hi - lo) % (4 * world) == 0
    end = 0
    for name, size in zip(lay.names, lay.sizes):
        off, numel = lay.slices[name]
        assert off % 4 == 0 and off == end and numel <= size < numel + 4 + 4 * world     # in order, no overlap, little padding
        end = off + size
        bucket = 0 if (has_colour and name == RGB) else len(lay.bounds) - 2
        assert lay.bounds[bucket] <= off and off + numel <= lay.bounds[bucket + 1]
    assert end == lay.total
    if has_colour:      # alone in bucket 0
        assert lay.slices[RGB][0] == 0 and all(off >= lay.b0 for n, (off, _) in lay.slices.items() if n != RGB)
    if given and lay.names[:2] == (RGB, XYZ) and len(given) > 2:
        assert lay.mlp_lo == lay.slices[lay.names[2]][0] > lay.b0
    else:
        assert lay.mlp_lo == 0
    with pytest.raises((AttributeError, TypeError)):
        lay.total = 0


def _models(ngp):
    from ngp_amd.implicit_mask import implicit_mask
    NGP = ngp.networks.NGP
    with torch.device("meta"):
        return {
            "default": (NGP(scale=0.5), None, None),
            "tone_mapped": (NGP(scale=0.5, rgb_act="None"), None, None),
            "skybox": (NGP(scale=0.5, use_skybox=True), None, None),
            "masked": (NGP(scale=0.5), implicit_mask(), None),
            "embed_a": (NGP(scale=0.5, embed_a=True, embed_a_len=8), None, torch.nn.Embedding(8, 8)),
            "scale8_masked_embed_a": (NGP(scale=8.0, embed_a=True, embed_a_len=4), implicit_mask(), torch.nn.Embedding(3, 4)),
        }


def test_layouts_of_the_trained_models_are_the_recorded_ones(ngp):
    from ngp_amd.trainer import flat_layout
    with open(GOLDEN_FILE) as f:
        recorded = json.load(f)["layouts"]
    models = _models(ngp)
    assert sorted(models) == sorted(recorded)
    for name, (model, msk, emb) in models.items():
        named = [(n, p.numel()) for n, p in model.named_parameters() if p.numel() > 0]
        named += [("msk_model." + n, p.numel()) for n, p in msk.named_parameters()] if msk is not None else []
        named += [("embedding_a.weight", emb.weight.numel())] if emb is not None else []
        lay, want = flat_layout(named, 1), recorded[name]
        assert list(lay.names) == want["names"], name
        assert {n: list(s) for n, s in lay.slices.items()} == want["slices"], name
        assert list(lay.bounds) == want["bounds"] and lay.mlp_lo == want["mlp_lo"] and lay.total == want["bounds"][-1], name
