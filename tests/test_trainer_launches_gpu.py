"""Everything one NGPTrainer.step enqueues, written out in order, whichever module enqueues it: every ngp_* entry call
(`call` of _lib.py, patched in every module of the package that bound it) and the stream-ordering operations issued from
Python (Stream.wait_stream, Stream.wait_event, Event.record, Event.wait; one that runs inside another, as the record and
wait inside wait_stream, is not listed again).  An entry is [name, stream role, arguments]:

  role       caller, colour-forward, optimizer or march-ahead (the roles of test_gpu_parity._record_step_launches); any
             other stream fails the case.
  arguments  scalars verbatim; a tensor as ["t", buffer, offset, strides] with the trainer buffer whose storage it lives
             in (flat_param, flat_grad, exp_avg, exp_avg_sq, scalars, norm_acc, need_exact, pose_param, pose_grad,
             pose_exp_avg, pose_exp_avg_sq, else other) and its offset from that buffer's start (from its storage's for
             `other`); a grid layout as "desc".  wait_stream names the role of the stream waited for; wait_event and
             Event.wait name the trace index at which the event was recorded, or "earlier" for one from before the step.

The lists in tests/golden/trainer_step_traces.json pin launch identity, not values.  They were recorded on an MI355X from
the trainer as it stood at 0798391 (one 150-line step(), one 110-line optimizer_step()), every case twice in processes of
their own; an argument on which the two recordings differed would be the wildcard "*" and be listed per case under
"wildcards" in the JSON file.  None did: every case seeds torch's generator, and the marcher then draws the same samples
(the sample counts in the lists are exact).  Where a trace cannot see a difference the case asserts values behind the step:
the trainer's own zero_() calls on scalars and norm_acc, and flat_grad clear.

Every case builds a fresh trainer and steps on 1024 rays; the cases without an option use _lego_batch() on
_grid_model(ngp, seed=3), the others the model and scene of their option's own GPU test module.  Run with `-m gpu`."""
import json
import os
import sys

import pytest
import torch

from test_gpu_parity import DEV, _grid_model, _lego_batch

pytestmark = pytest.mark.gpu

_TORCH_STREAM_POOL = 32   # (c10: kStreamsPerPool) streams per device and priority, handed out round-robin
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_step_traces.json")
_BUFFERS = ("flat_param", "flat_grad", "exp_avg", "exp_avg_sq", "scalars", "norm_acc", "need_exact", "pose_param", "pose_grad",
            "pose_exp_avg", "pose_exp_avg_sq")


def _buffer_table(tr):
    """[(name, storage address, first element, one past the last)] of the trainer's own buffers"""
    table = []
    for name in _BUFFERS:
        b = getattr(tr, name, None)
        if isinstance(b, torch.Tensor):
            table.append((name, b.untyped_storage().data_ptr(), b.storage_offset(), b.storage_offset() + b.numel()))
    return table


def record_step(ngp, tr, step):
    """runs step() -> the trace described in the module docstring"""
    from ngp_amd import _lib, networks
    caller = torch.cuda.current_stream().cuda_stream
    roles = {caller: "caller", networks._stream("colour", DEV).cuda_stream: "colour-forward",
             tr._opt_stream.cuda_stream: "optimizer", tr._march_ahead.stream.cuda_stream: "march-ahead"}
    assert len(roles) == 4
    table = _buffer_table(tr)
    trace, recorded, keep, depth = [], {}, [], [0]

    def role(stream=None):
        st = (torch.cuda.current_stream() if stream is None else stream).cuda_stream
        assert st in roles, f"entry {len(trace)}: a stream that is none of the trainer's four"
        return roles[st]

    def describe(a):
        if isinstance(a, torch.Tensor):
            base, off = a.untyped_storage().data_ptr(), a.storage_offset()
            for name, ptr, lo, hi in table:
                if ptr == base and lo <= off < hi:
                    return ["t", name, off - lo, list(a.stride())]
            return ["t", "other", off, list(a.stride())]
        if a is None or isinstance(a, (bool, int, float)):
            return a
        return "desc"

    real_call = _lib.call

    def recording_call(name, *args):
        trace.append([name, role(), [describe(a) for a in args]])
        return real_call(name, *args)

    def stream_op(cls, method, entry):
        real = getattr(cls, method)

        def patched(self, *args):
            if depth[0] == 0:
                trace.append(entry(self, *args))
            depth[0] += 1
            try:
                return real(self, *args)
            finally:
                depth[0] -= 1
        return cls, method, patched

    def event_recorded(ev, stream=None):
        keep.append(ev)
        recorded[id(ev)] = len(trace)
        return ["Event.record", role(stream), []]

    def which(ev):
        return recorded.get(id(ev), "earlier")

    ops = [stream_op(torch.cuda.Stream, "wait_stream", lambda self, other: ["Stream.wait_stream", role(self), [role(other)]]),
           stream_op(torch.cuda.Stream, "wait_event", lambda self, ev: ["Stream.wait_event", role(self), [which(ev)]]),
           stream_op(torch.cuda.Event, "record", event_recorded),
           stream_op(torch.cuda.Event, "wait", lambda self, stream=None: ["Event.wait", role(stream), [which(self)]])]
    package = _lib.__name__.rsplit(".", 1)[0]      # (the package's own name; ngp_amd.* are the same module objects)
    users = [m for name, m in list(sys.modules.items())
             if m is not None and name.startswith(package + ".") and getattr(m, "call", None) is real_call]
    assert _lib in users and networks in users
    with pytest.MonkeyPatch.context() as mp:
        for m in users:
            mp.setattr(m, "call", recording_call)
        for cls, method, patched in ops:
            mp.setattr(cls, method, patched)
        step()
    return json.loads(json.dumps(trace))


def _trainer(ngp, model=None, **kw):
    from ngp_amd.trainer import NGPTrainer
    # the field's own colour-forward stream is drawn on first use: in a process that starts here it must not be drawn
    # behind the 32 below, where the pool has come round to this trainer's optimizer stream
    ngp.networks._stream("colour", DEV)
    tr = NGPTrainer(_grid_model(ngp, seed=3) if model is None else model, lr=1e-2, **kw)
    # (test_field_launches_gpu._trainer_step_launches says why: this trainer drew 2 of torch's pool of 32 streams, draw the
    # other 30 so that every later module finds the pool where it would be without this test)
    assert tr._opt_stream is not None and tr._march_ahead.stream is not None
    for _ in range(_TORCH_STREAM_POOL - 2):
        torch.cuda.Stream(device=DEV)
    return tr


def _scene_batch(scene, seed, n_rays=1024, **gt_kw):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    img, pix = scene.sample_batch(n_rays, generator=gen)
    o, d = scene.rays(img, pix)
    gt, _ = scene.ground_truth(o, d, n_quad=64, **gt_kw)
    return o, d, gt, img, pix, gen


def _second_step(ngp, tr, *args, **kw):
    tr.step(*args, **kw)                                         # (the step with the all-cells occupancy update)
    return record_step(ngp, tr, lambda: tr.step(*args, **kw))


def _bound(ngp):
    tr = _trainer(ngp)
    return tr, _second_step(ngp, tr, *_lego_batch())


def _ahead(ngp, steps_before, global_step=None):
    """records the step behind `steps_before` steps with next_rays; global_step: one plain step (for the occupancy grid),
    then the recorded step is taken at that count"""
    tr = _trainer(ngp)
    batches = [_lego_batch(seed=5 + i) for i in range(steps_before + 2)]
    for i in range(steps_before):
        tr.step(*batches[i], next_rays=batches[i + 1][:2])
    if global_step is not None:
        tr.step(*_lego_batch(seed=4))
        tr.global_step = global_step
    b, nxt = batches[steps_before], batches[steps_before + 1]
    return tr, record_step(ngp, tr, lambda: tr.step(*b, next_rays=nxt[:2]))


def _early_share(ngp):
    tr = _trainer(ngp)
    tr.norm_bound = False
    return tr, _second_step(ngp, tr, *_lego_batch())


def _unannounced(ngp):
    tr = _trainer(ngp)
    tr.norm_bound = False
    assert tr.model.rgb_encoder.on_grad_ready == tr._early_norm_share

    def unannounced():   # (test_optim_gpu.ROUTES["full_sum"]) a backward that step() did not announce
        tr._norm_share_armed = False
        tr._early_norm_share()
    tr.model.rgb_encoder.on_grad_ready = unannounced
    return tr, _second_step(ngp, tr, *_lego_batch())


def _module_route(ngp):
    tr = _trainer(ngp)
    tr.recipe.fused_loss = False
    return tr, _second_step(ngp, tr, *_lego_batch())


def _exposure(ngp):
    import test_tonemap_gpu as M
    from ngp_amd.synthetic import LegoProxy
    tr = _trainer(ngp, M._field_model(ngp, 71), use_exposure=True, unit_exposure_rgb=0.73)
    o, d, gt, _, _, gen = _scene_batch(LegoProxy(n_images=4, img_wh=(32, 32), device=DEV), 72)
    e = torch.tensor(M.TIMES, device=DEV)[torch.randint(5, (1024,), device=DEV, generator=gen)]
    return tr, _second_step(ngp, tr, o, d, gt, exposure=e)


def _masked(ngp):
    import test_mask_gpu as M
    from ngp_amd.implicit_mask import implicit_mask
    model, msk, scene = M._train_setup(ngp, 51, 0.5, 8, 64)
    tr = _trainer(ngp, model, msk_model=msk)
    o, d, gt, img, pix, _ = _scene_batch(scene, 52)
    uvi = implicit_mask.uvi(torch.stack([pix // 64, pix % 64], -1), img, (64, 64), 8)
    return tr, _second_step(ngp, tr, o, d, gt, uvi=uvi)


def _embed_a(ngp):
    import test_embed_a_gpu as M
    from ngp_amd.synthetic import LegoProxy
    torch.manual_seed(61)
    model = ngp.networks.NGP(scale=0.5, embed_a=True, embed_a_len=8).to(DEV)
    M._add_grid(model)
    tr = _trainer(ngp, model, embedding_a=torch.nn.Embedding(8, 8).to(DEV))
    o, d, gt, img, _, _ = _scene_batch(LegoProxy(n_images=8, img_wh=(64, 64), device=DEV), 62)
    return tr, _second_step(ngp, tr, o, d, gt, img_idxs=img)


def _pose(ngp):
    import test_pose_gpu as M
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    torch.manual_seed(71)
    model = ngp.networks.NGP(scale=0.5).to(DEV)
    M._add_grid(model)
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.5)
    scene = LegoProxy(n_images=3, img_wh=(24, 24), device=DEV)
    tr = _trainer(ngp, model, pose_refiner=PoseRefiner(scene.poses, scene.directions).to(DEV), pose_lr=1e-4)
    _, _, gt, img, pix, _ = _scene_batch(scene, 72)
    return tr, _second_step(ngp, tr, None, None, gt, img_idxs=img, pix_idxs=pix)


def _multi_terms(ngp):
    import tail_harness as H
    from ngp_amd.synthetic import LegoProxy
    terms = ("semantic", "normal_mono", "depth_mono")
    torch.manual_seed(52)
    tr = _trainer(ngp, H._grid_buffers(ngp.networks.NGP(scale=0.5).to(DEV)), multi_terms=terms)
    scene = LegoProxy(n_images=10, img_wh=(100, 100), device=DEV)
    o, d, gt, _, _, gen = _scene_batch(scene, 51)
    targets = {H.TERMS[k][1]: v for k, v in H._scene_targets(scene, o, d, 7, gen, terms).items()}
    return tr, _second_step(ngp, tr, o, d, gt, **targets)


def _sky(ngp):
    import test_sky_gpu as M
    from ngp_amd.synthetic import LegoProxy
    model = M._sky_field_model(ngp, 62)
    tr = _trainer(ngp, model, use_skybox=True)
    o, d, gt, _, _, _ = _scene_batch(LegoProxy(n_images=10, img_wh=(100, 100), device=DEV), 61, sky=True)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    tr.global_step = tr.warmup_steps
    assert tr.sky_active()
    return tr, record_step(ngp, tr, lambda: tr.step(o, d, gt))


def _normal_ref(ngp):
    import test_normal_ref_gpu as M
    tr = _trainer(ngp, M._model(ngp, 92), normal_ref=True)
    o, d, gt, _, _ = M._batch(1024, 91)
    return tr, _second_step(ngp, tr, o, d, gt)


CASES = {
    "bound": _bound,                                              # the second step of a default trainer
    "ahead_update_late": lambda ngp: _ahead(ngp, 0),              # step 0: the update, this batch marched now, the next one's behind render()
    "ahead_hit": lambda ngp: _ahead(ngp, 2),                      # the pending march taken, the next launched before the forward
    "ahead_before_update": lambda ngp: _ahead(ngp, 0, 15),        # global_step = 15: nothing is marched ahead
    "early_share": _early_share,                                  # the colour table's share summed from the encoder hook
    "unannounced": _unannounced,                                  # one full sum
    "module_route": _module_route,                                # NeRFLoss and loss.backward()
    "exposure": _exposure,                                        # seeded default terms + the unit-exposure term, one backward
    "masked": _masked,                                            # join_params(rgb_table=False) ahead of the mask field
    "embed_a": _embed_a,
    "pose": _pose,                                                # _pose_step's three launches ahead of the sweep
    "multi_terms": _multi_terms,
    "sky": _sky,                                                  # global_step = warmup_steps
    "normal_ref": _normal_ref,                                    # two seeded outputs in one backward
}


def run_case(ngp, case):
    """-> (trainer, trace) with the device idle behind the step"""
    torch.manual_seed(7)
    tr, trace = CASES[case](ngp)
    tr.wait()
    torch.cuda.synchronize()
    return tr, trace


def _matches(got, want):
    return want == "*" or got == want


@pytest.fixture(scope="module")
def expected():
    with open(GOLDEN_FILE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", list(CASES))
def test_trainer_step_trace(ngp, expected, case):
    tr, got = run_case(ngp, case)
    want = expected[case]
    assert [(name, role) for name, role, _ in got] == [(name, role) for name, role, _ in want]
    for i, ((name, _, ga), (_, _, wa)) in enumerate(zip(got, want)):
        assert len(ga) == len(wa) and all(_matches(g, w) for g, w in zip(ga, wa)), f"entry {i} ({name}): {ga} != {wa}"
    # what a trace cannot see: the trainer's own zero_() calls and the Adam launches' clearing of the gradient
    assert float(tr.scalars[0]) == 0 and not bool(tr.norm_acc.any())
    assert not bool(tr.flat_grad.any())
    if tr.pose_refiner is not None:
        assert not bool(tr.pose_grad.any())
