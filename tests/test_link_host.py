"""link.FieldLink without a GPU: the rules a trainer and the field share (which waits clear the parameter events and
which leave them, the norm-bound counters, the "no trainer" defaults), with stub events that count their waits."""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Ev:
    def __init__(self):
        self.waits = 0

    def wait(self):
        self.waits += 1


class Stage:
    """what bound_note reads of a networks._Mlp2Bwd"""

    def __init__(self, fused):
        self.fused, self.norm_noted = fused, True   # (norm_noted: the elementwise stage has added the sum, nothing to launch)


@pytest.fixture()
def link(ngp):
    from ngp_amd.link import FieldLink
    return FieldLink()


def _pending(link):
    link.params_ready, link.rgb_params_ready = Ev(), Ev()
    return link.params_ready, link.rgb_params_ready


def test_fresh_link_means_no_trainer(link):
    assert link.grad_sinks == {} and link.side_stream is None and link.heads_stream is None
    assert link.params_ready is None and link.rgb_params_ready is None and link.acc_zeroed is None
    assert link.norm_acc is None and link.hits == 0 and link.ok is True
    assert link.take_param_events() == (None, None) and link.take_acc_zeroed() is None
    link.wait_params()
    link.join_params()                     # nothing pending: nothing happens
    with pytest.raises(AttributeError):    # a misspelt name is an error, not "no trainer"
        link.param_ready = Ev()


def test_take_param_events_returns_and_clears_both(link):
    p, c = _pending(link)
    assert link.take_param_events() == (p, c)
    assert link.params_ready is None and link.rgb_params_ready is None
    assert p.waits == 0 and c.waits == 0   # the caller waits, where each of its streams first reads the piece


def test_wait_params_waits_and_clears(link):
    p, c = _pending(link)
    link.wait_params()
    assert (p.waits, c.waits) == (1, 1) and link.params_ready is None and link.rgb_params_ready is None


def test_wait_params_without_the_colour_table_leaves_its_event_pending(link):
    p, c = _pending(link)
    link.wait_params(rgb_table=False)
    assert (p.waits, c.waits) == (1, 0) and link.params_ready is None and link.rgb_params_ready is c


def test_join_params_waits_on_both_and_clears_neither(link):
    p, c = _pending(link)
    link.join_params()
    assert (p.waits, c.waits) == (1, 1) and link.params_ready is p and link.rgb_params_ready is c
    link.join_params(rgb_table=False)      # the masked step: the first piece only
    assert (p.waits, c.waits) == (2, 1) and link.params_ready is p and link.rgb_params_ready is c


def test_take_acc_zeroed_clears(link):
    ev = link.acc_zeroed = Ev()
    assert link.take_acc_zeroed() is ev and link.acc_zeroed is None and ev.waits == 0


def test_bound_note_and_its_counters(link):
    link.bound_note(Stage(fused=True), 0, 3, 10)         # no accumulator (not a bound step): nothing
    assert link.hits == 0 and link.ok is True
    link.hits, link.ok = 5, False
    link.begin_bound_step(object())
    assert link.hits == 0 and link.ok is True and link.norm_acc is not None
    link.bound_note(Stage(fused=False), 0, 3, 10)        # a non-fused stage spoils the bound and is not counted
    assert link.hits == 0 and link.ok is False
    link.begin_bound_step(object())
    link.bound_note(Stage(fused=True), 0, 3, 10)
    link.bound_note(Stage(fused=True), 1, 1, 10)
    assert link.hits == 2 and link.ok is True
    link.bound_spoiled()
    assert link.hits == 2 and link.ok is False
    link.begin_bound_step(None)                          # a step off the bound route takes the accumulator away
    assert link.norm_acc is None and link.hits == 0 and link.ok is True


def test_the_link_is_no_part_of_the_state_dict(ngp):
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.networks import NGP
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "g15_dropin_layout.json")))
    (cfg,) = [c for c in fx["ngp_configs"] if c["kwargs"] == {"scale": 0.5}]
    model = NGP(scale=0.5)
    assert sorted(model.state_dict()) == sorted(cfg["state_dict"])
    assert type(model.link).__name__ == "FieldLink" and not isinstance(model.link, torch.nn.Module)
    assert model.grid_rng is None and model.xyz_encoder.grad_buffer is None and model.rgb_encoder.on_grad_ready is None
    msk = implicit_mask()
    assert sorted(msk.state_dict()) == ["mask_encoder.params", "mask_net.0.bias", "mask_net.0.weight", "mask_net.2.bias",
                                        "mask_net.2.weight"]
    assert msk.link.grad_sinks == {} and msk.link is not model.link
