"""render(model, rays_o, rays_d, **kwargs) — the L2 render API of the reference
(models/rendering.py:13-251) on the MI355X operator surface.

Train keys: deltas, ts, rays_a, total_samples, sigma, xyzs, vr_samples, opacity, depth, rgb,
            normal_pred, semantic, ws, Ro, Rp                     (rendering.py:205-251)
Test keys:  opacity, depth, rgb, normal_pred, normal_raw, semantic, total_samples, points, mask
                                                                   (rendering.py:176-185)
kwargs read: test_time, to_cpu, to_numpy, exp_step_factor, embedding_a, num_classes, max_samples,
             T_threshold, use_skybox, random_bg (+ passed through to the model).
embedding_a: a (n_rays, E) tensor (expanded per sample here) or, at training time, appearance.RayCodes(table, img_idxs).
"""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import vren
from ._lib import call
from .appearance import RayCodes
from .custom_functions import RayAABBIntersector, RayMarcher, RefLoss, VolumeRenderer, mark_full_cover

MAX_SAMPLES = 1024
NEAR_DISTANCE = 0.01


def render(model, rays_o, rays_d, **kwargs):
    if kwargs.get('test_time', False) and isinstance(kwargs.get('embedding_a'), RayCodes):
        raise ValueError("RayCodes is the training route's embedding_a; test-time rendering takes a (1, E) tensor "
                         "(e.g. embedding.weight[0:1], or FrameEmbedding(pose, mode='mean'))")
    rays_o = rays_o.contiguous()
    rays_d = rays_d.contiguous()
    marched = kwargs.get('marched', None)
    if marched is not None and not kwargs.get('test_time', False):
        hits_t = marched.hits_t   # AABB + marcher already ran for exactly these rays (MarchAhead)
    else:
        hits_t = intersect_scene(model, rays_o, rays_d)

    fn = _render_rays_test if kwargs.get('test_time', False) else _render_rays_train
    results = fn(model, rays_o, rays_d, hits_t, **kwargs)
    if kwargs.get('to_cpu', False):
        for k, v in results.items():
            v = v.cpu()
            if kwargs.get('to_numpy', False):
                v = v.numpy()
            results[k] = v
    return results


def intersect_scene(model, rays_o, rays_d):
    """ray / scene-AABB intersection with the near clamp of rendering.py:25-30 -> hits_t (N_rays,1,2)"""
    _, hits_t, _ = RayAABBIntersector.apply(rays_o, rays_d, model.center, model.half_size, 1)
    # 0 <= t1 < NEAR_DISTANCE -> NEAR_DISTANCE, one fused launch
    call("clamp_near", hits_t, hits_t.shape[0], 1, NEAR_DISTANCE)
    return hits_t


class MarchAhead:
    """The ray-only front of a training step — AABB test, near clamp, occupancy marcher — for the
    NEXT ray batch, on its own HIP stream.

    None of it reads a network parameter, so it can run under the current step's backward /
    optimizer.  The sample count comes back through a pinned host word and an event on that
    stream: the host waits for the marcher alone, never for the main stream, and is therefore a
    step ahead of the device when it enqueues the field kernels (the reference synchronises the
    whole device at this point every step, custom_functions.py:93).  The result is handed to
    render(..., marched=...) and is only valid for the same rays and the occupancy bitfield it
    was marched with (the trainer does not march across a density-grid update)."""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device=device)
        self.count_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.pending = None

    def launch(self, model, rays_o, rays_d, exp_step_factor=0.):
        main = torch.cuda.current_stream()
        self.stream.wait_stream(main)   # the rays and the bitfield were produced on the main stream
        with torch.cuda.stream(self.stream), torch.no_grad():
            hits_t = intersect_scene(model, rays_o, rays_d)
            noise = torch.rand_like(rays_o[:, 0])
            out = vren.raymarching_train_untrimmed(rays_o, rays_d, hits_t[:, 0], model.density_bitfield,
                                                   model.cascades, model.scale, exp_step_factor, noise,
                                                   model.grid_size, MAX_SAMPLES)
            self.count_host.copy_(out[5][:1], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        self.pending = (rays_o, rays_d, exp_step_factor, hits_t, out, done)

    def take(self, rays_o, rays_d, exp_step_factor=0.):
        """-> the marched batch if it was launched for exactly these tensors, else None"""
        p, self.pending = self.pending, None
        if p is None or p[0] is not rays_o or p[1] is not rays_d or p[2] != exp_step_factor:
            return None
        _, _, _, hits_t, (rays_a, xyzs, dirs, deltas, ts, counter), done = p
        done.synchronize()
        n = int(self.count_host[0])
        main = torch.cuda.current_stream()
        main.wait_event(done)
        for t in (hits_t, rays_a, xyzs, dirs, deltas, ts, counter):
            t.record_stream(main)   # allocated on the side stream's pool, consumed on the main stream
        m = _Marched()
        m.hits_t, m.rays_a, m.total_samples = hits_t, rays_a, counter[0]
        m.xyzs, m.dirs, m.deltas, m.ts = xyzs[:n], dirs[:n], deltas[:n], ts[:n]
        return m


class _Marched:
    __slots__ = ("hits_t", "rays_a", "xyzs", "dirs", "deltas", "ts", "total_samples")


def render_chunks(model, rays_o, rays_d, chunk_size, **kwargs):
    """render() in chunks of `chunk_size` rays (render.py:33-48): per-ray results concatenated,
    `total_samples` kept as a list"""
    results = {}
    for i in range(0, rays_o.shape[0], chunk_size):
        ret = render(model, rays_o[i:i + chunk_size], rays_d[i:i + chunk_size], **dict(kwargs))
        for k, v in ret.items():
            results.setdefault(k, []).append(v)
    for k in results:
        if k != 'total_samples':
            results[k] = torch.cat(results[k], 0)
    return results


@torch.no_grad()
def render_dense(model, rays_o, rays_d, z_vals, **kwargs):
    """The dense-sample path of rendering_noCUDA.py:103-214 on the HIP kernels: the field at the
    caller's depths `z_vals` (N_rays, S), composited as raw2outputs does (custom_functions.py:280-321:
    dists = diff(z)·|d| with a last interval of 1e10, no early termination).  Used to compare this
    library with the reference's noCUDA path on identical rays AND identical samples.
    -> opacity, depth, rgb, normal_raw, normal_pred, semantic (logit sums), ws (N_rays, S)"""
    classes = kwargs.get('num_classes', 7)
    rays_o, rays_d, z_vals = rays_o.contiguous(), rays_d.contiguous(), z_vals.contiguous()
    n_rays, S = z_vals.shape
    dev = rays_o.device
    xyzs = (rays_o[:, None, :] + rays_d[:, None, :] * z_vals[:, :, None]).reshape(-1, 3).contiguous()
    dirs = rays_d[:, None, :].expand(-1, S, -1).reshape(-1, 3).contiguous()
    sigmas, rgbs, normals_raw, normals_pred, sems = model(xyzs, dirs, **kwargs)
    dists = torch.cat([z_vals[:, 1:] - z_vals[:, :-1], torch.full_like(z_vals[:, :1], 1e10)], -1)
    dists = (dists * torch.norm(rays_d, dim=-1, keepdim=True)).reshape(-1).contiguous()
    idx = torch.arange(n_rays, device=dev, dtype=torch.int64)
    rays_a = torch.stack([idx, idx * S, torch.full_like(idx, S)], -1).contiguous()
    out = {}
    ts = z_vals.reshape(-1).contiguous()
    _, out['opacity'], out['depth'], out['rgb'], out['normal_pred'], out['semantic'], ws = vren.composite_train_fw(
        sigmas.contiguous(), rgbs.contiguous(), normals_pred.contiguous(), sems.contiguous(), dists, ts, rays_a,
        0.0, classes)
    out['normal_raw'] = vren.composite_train_fw(
        sigmas.contiguous(), rgbs.contiguous(), normals_raw.contiguous(), sems.contiguous(), dists, ts, rays_a,
        0.0, classes)[4]
    out['ws'] = ws.view(n_rays, S)
    return out


def volume_render(model, rays_o, rays_d, hits_t, opacity, depth, rgb, normal_pred, normal_raw, sem, **kwargs):
    """Progressive test-time marching (rendering.py:46-133): the per-ray accumulators are updated
    in place; returns the total number of samples evaluated.

    Same rounds, same samples per round and same compositing as the reference, with less work per
    round: the reference compacts the valid samples with a boolean mask, evaluates the field on
    them and scatters five result tensors back into zero-filled padded ones (~110 launches and
    three host syncs per round); here the field runs on the padded block directly — the marcher's
    padding rows are zeros, 6 % of the slots on the proxy scene, the compositor reads the first
    N_eff samples of a ray only, and a field row does not depend on the other rows of the batch, so
    every per-ray result is bit-identical — which leaves ~25 launches and one sync per round.
    `volume_render_reference` keeps the literal loop (reference_test_loop=True selects it)."""
    if kwargs.get('reference_test_loop', False):
        return volume_render_reference(model, rays_o, rays_d, hits_t, opacity, depth, rgb, normal_pred, normal_raw,
                                       sem, **kwargs)
    N_rays = len(rays_o)
    device = rays_o.device
    exp_step_factor = kwargs.get('exp_step_factor', 0.)
    classes = kwargs.get('num_classes', 7)
    T_threshold = kwargs.get('T_threshold', 1e-4)
    samples = 0
    total_samples = torch.zeros((), dtype=torch.int64, device=device)
    alive_indices = torch.arange(N_rays, device=device)
    min_samples = 1 if exp_step_factor == 0 else 4
    f32 = torch.float32
    while samples < kwargs.get('max_samples', MAX_SAMPLES):
        N_alive = len(alive_indices)
        if N_alive == 0:
            break
        N_samples = max(min(N_rays // N_alive, 64), min_samples)
        samples += N_samples
        n_pts = N_alive * N_samples
        xyzs = torch.zeros(n_pts, 3, dtype=f32, device=device)      # padding rows must hold finite inputs
        dirs = torch.zeros(n_pts, 3, dtype=f32, device=device)
        deltas = torch.empty(N_alive, N_samples, dtype=f32, device=device)   # read up to N_eff only
        ts = torch.empty(N_alive, N_samples, dtype=f32, device=device)
        N_eff_samples = torch.empty(N_alive, dtype=torch.int32, device=device)
        call("raymarching_test", rays_o, rays_d, hits_t, alive_indices, model.density_bitfield, int(model.cascades),
             float(model.scale), float(exp_step_factor), int(model.grid_size), MAX_SAMPLES, int(N_samples), N_alive,
             xyzs, dirs, deltas, ts, N_eff_samples)
        total_samples += N_eff_samples.sum()
        sigmas, rgbs, normals_pred, normals_raw, sems = model.forward_test(xyzs, dirs, **kwargs)
        call("composite_test_fw", sigmas.contiguous(), rgbs.contiguous(), normals_pred.contiguous(),
             normals_raw.contiguous(), sems.contiguous(), deltas, ts, hits_t, alive_indices, float(T_threshold),
             int(classes), N_eff_samples, N_alive, int(N_samples), opacity, depth, rgb, normal_pred, normal_raw, sem)
        alive_indices = alive_indices[alive_indices >= 0]   # the one host sync of the round

    if kwargs.get('use_skybox', False):
        rgb_bg = model.forward_skybox(rays_d)
        rgb += rgb_bg * (1 - opacity)[:, None]
    return total_samples


def volume_render_reference(model, rays_o, rays_d, hits_t, opacity, depth, rgb, normal_pred, normal_raw, sem, **kwargs):
    """the literal loop of rendering.py:46-133 (mask, compact, evaluate, scatter back)"""
    N_rays = len(rays_o)
    device = rays_o.device
    exp_step_factor = kwargs.get('exp_step_factor', 0.)
    classes = kwargs.get('num_classes', 7)
    T_threshold = kwargs.get('T_threshold', 1e-4)
    samples = 0
    total_samples = 0
    alive_indices = torch.arange(N_rays, device=device)
    # synthetic scenes are mostly background: 1 sample per round retires those rays quickly
    min_samples = 1 if exp_step_factor == 0 else 4

    while samples < kwargs.get('max_samples', MAX_SAMPLES):
        N_alive = len(alive_indices)
        if N_alive == 0:
            break
        N_samples = max(min(N_rays // N_alive, 64), min_samples)
        samples += N_samples

        xyzs, dirs, deltas, ts, N_eff_samples = vren.raymarching_test(
            rays_o, rays_d, hits_t, alive_indices, model.density_bitfield, model.cascades, model.scale,
            exp_step_factor, model.grid_size, MAX_SAMPLES, N_samples)
        total_samples += N_eff_samples.sum()
        xyzs = xyzs.reshape(-1, 3)
        dirs = dirs.reshape(-1, 3)
        valid_mask = ~torch.all(dirs == 0, dim=1)
        if valid_mask.sum() == 0:
            break

        n_pts = len(xyzs)
        sigmas = torch.zeros(n_pts, device=device)
        rgbs = torch.zeros(n_pts, 3, device=device)
        normals_pred = torch.zeros(n_pts, 3, device=device)
        normals_raw = torch.zeros(n_pts, 3, device=device)
        sems = torch.zeros(n_pts, classes, device=device)

        _sigmas, _rgbs, _normals_pred, _normals_raw, _sems = \
            model.forward_test(xyzs[valid_mask], dirs[valid_mask], **kwargs)
        sigmas[valid_mask] = _sigmas.detach().float()
        rgbs[valid_mask] = _rgbs.detach().float()
        normals_pred[valid_mask] = _normals_pred.float()
        normals_raw[valid_mask] = _normals_raw.float()
        sems[valid_mask] = _sems.float()

        vren.composite_test_fw(
            sigmas.view(N_alive, N_samples), rgbs.view(N_alive, N_samples, 3),
            normals_pred.view(N_alive, N_samples, 3), normals_raw.view(N_alive, N_samples, 3),
            sems.view(N_alive, N_samples, classes), deltas, ts, hits_t, alive_indices, T_threshold, classes,
            N_eff_samples, opacity, depth, rgb, normal_pred, normal_raw, sem)
        alive_indices = alive_indices[alive_indices >= 0]

    if kwargs.get('use_skybox', False):
        rgb_bg = model.forward_skybox(rays_d)
    else:
        rgb_bg = torch.zeros(3, device=device)
    rgb += rgb_bg * (1 - opacity)[:, None]
    return total_samples


@torch.no_grad()
def _render_rays_test(model, rays_o, rays_d, hits_t, **kwargs):
    hits_t = hits_t[:, 0, :].contiguous()
    classes = kwargs.get('num_classes', 7)
    N_rays = len(rays_o)
    device = rays_o.device
    opacity = torch.zeros(N_rays, device=device)
    depth = torch.zeros(N_rays, device=device)
    rgb = torch.zeros(N_rays, 3, device=device)
    normal_pred = torch.zeros(N_rays, 3, device=device)
    normal_raw = torch.zeros(N_rays, 3, device=device)
    sem = torch.zeros(N_rays, classes, device=device)
    mask = torch.zeros(N_rays, device=device)

    total_samples = volume_render(model, rays_o, rays_d, hits_t, opacity, depth, rgb, normal_pred, normal_raw, sem,
                                  **kwargs)
    results = {
        'opacity': opacity, 'depth': depth, 'rgb': rgb,
        'normal_pred': F.normalize(normal_pred, dim=-1),
        'normal_raw': F.normalize(normal_raw, dim=-1),
        'semantic': torch.argmax(sem, dim=-1, keepdim=True),
        'total_samples': total_samples,
        'points': rays_o + rays_d * depth.unsqueeze(-1),
        'mask': mask,
    }
    return results


def _render_rays_train(model, rays_o, rays_d, hits_t, **kwargs):
    exp_step_factor = kwargs.get('exp_step_factor', 0.)
    T_threshold = kwargs.get('T_threshold', 1e-4)
    classes = kwargs.get('num_classes', 7)
    results = {}
    marched = kwargs.pop('marched', None)
    if marched is not None:
        rays_a, xyzs, dirs, total_samples = marched.rays_a, marched.xyzs, marched.dirs, marched.total_samples
        results['deltas'], results['ts'] = marched.deltas, marched.ts
    else:
        with torch.no_grad():
            rays_a, xyzs, dirs, results['deltas'], results['ts'], total_samples = RayMarcher.apply(
                rays_o, rays_d, hits_t[:, 0], model.density_bitfield, model.cascades, model.scale, exp_step_factor,
                model.grid_size, MAX_SAMPLES)
    mark_full_cover(rays_a)   # the marcher's segments tile [0, N): the compositor may skip its zero-fills
    results['rays_a'] = rays_a
    results['total_samples'] = total_samples
    pose = kwargs.pop('_pose', None)
    if pose is not None:
        # pose refinement (pose.PoseRefiner, image and pixel of every ray): the samples were marched from the rays' values;
        # from here on they carry a gradient that ngp_pose_rays_bwd takes to dR and dT
        xyzs, dirs = pose[0].attach_samples(xyzs, dirs, results['ts'], rays_a, pose[1], pose[2])

    # per-ray tensor kwargs (embedding_a, exposure, ...) are repeated per sample; like the
    # reference this rewrites kwargs in place (rendering.py:217-219).  RayCodes (the embedding table and the rays' image
    # indices) is not expanded here: it is handed the batch's segments and the field broadcasts it with one launch
    for k, v in kwargs.items():
        if isinstance(v, torch.Tensor):
            kwargs[k] = torch.repeat_interleave(v[rays_a[:, 0]], rays_a[:, 2], 0, output_size=xyzs.shape[0])
        elif isinstance(v, RayCodes):
            kwargs[k] = v.for_batch(rays_a)
    fused = kwargs.pop('_fused_loss', None)
    if fused is not None and _fused_tail_ok(model, kwargs, exp_step_factor, classes, fused):
        return _render_loss_fused(model, results, xyzs, dirs, rays_a, T_threshold, classes, fused, kwargs, rays_d)
    sigmas, rgbs, normals_raw, normals_pred, sems = model(xyzs, dirs, **kwargs)
    results['sigma'] = sigmas
    results['xyzs'] = xyzs

    (results['vr_samples'], results['opacity'], results['depth'], results['rgb'], results['normal_pred'],
     results['semantic'], results['ws']) = VolumeRenderer.apply(
        sigmas.contiguous(), rgbs.contiguous(), normals_pred.contiguous(), sems.contiguous(),
        results['deltas'], results['ts'], rays_a, T_threshold, classes)

    rgb_bg = None  # black background (synthetic scenes): rgb + 0*(1-opacity) is rgb, skip the ops
    if kwargs.get('use_skybox', False):
        rgb_bg = model.forward_skybox(rays_d)
    elif exp_step_factor != 0 and kwargs.get('random_bg', False):
        rgb_bg = torch.rand(3, device=rays_o.device)
    if rgb_bg is not None:
        results['rgb'] = results['rgb'] + rgb_bg * (1 - results['opacity'])[:, None]

    # Ref-NeRF normal regularisers (rendering.py:243-249)
    normals_diff, normals_ori = _RefLossInputs.apply(normals_raw, normals_pred, dirs)
    results['Ro'], results['Rp'] = RefLoss.apply(
        sigmas.detach().contiguous(), normals_diff, normals_ori,
        results['deltas'], results['ts'], rays_a, T_threshold)
    # NeRFLoss(normal_ref=True) needs Ro to reach the density field through normals_raw (reference:
    # create_graph=True, networks.py:186-196); the default field returns detached analytic normals
    results['Ro']._ngp_normals_have_grad = bool(normals_raw.requires_grad)
    return results


def _fused_tail_ok(model, kwargs, exp_step_factor, classes, fused=None):
    """the one-launch render + loss tail covers the default recipe: sigmoid colours (no tone mapper), black or random
    constant background (a skybox network only when `fused`, a FusedTail, says `sky`: ngp_render_loss_fused_sky), detached
    analytic normals, at most 8 classes (1 to 16 when `fused` names the semantic term)"""
    sem = fused is not None and 'semantic' in fused.terms
    sky = bool(kwargs.get('use_skybox', False))
    if sky and not (fused is not None and fused.sky and getattr(model, 'use_skybox', False)):
        return False
    return (getattr(model, 'rgb_act', 'Sigmoid') == 'Sigmoid'
            and not getattr(model, 'differentiable_normals', False) and (1 <= classes <= 16 if sem else classes <= 8)
            and hasattr(model, '_field'))


MULTI_TERMS = ('semantic', 'normal_mono', 'depth_mono')   # bit i of ngp_render_loss_fused_multi's term_mask
MULTI_WS_INTS = 30                                        # NGP_MULTI_WS_INTS


class TailLayout(NamedTuple):
    """one float32 accumulator per launch, [terms (n_terms) | - | vr_samples (int64) at float vr_at | workspace (ws_ints
    int32) at float ws_at], laid out so that the entry clears it with one memset.  ws_at None: no workspace inside the
    accumulator (the semantic entry's is an allocation of its own, which its label count clears)."""
    n_terms: int
    acc: int
    vr_at: int
    ws_at: Optional[int]
    ws_ints: int


# entry ngp_render_loss_fused[_<key>] -> its layout (ws_ints: NGP_SEM_WS_INTS, NGP_NRM_WS_INTS, NGP_DEP_WS_INTS, NGP_MULTI_WS_INTS)
TAIL_LAYOUT = {
    'default': TailLayout(4, 6, 4, None, 0),
    'masked': TailLayout(5, 8, 6, None, 0),
    'sem': TailLayout(6, 8, 6, None, 8),
    'nrm': TailLayout(5, 12, 6, 8, 4),
    'dep': TailLayout(5, 26, 6, 8, 18),
    'multi': TailLayout(8, 10 + MULTI_WS_INTS, 8, 10, MULTI_WS_INTS),
}
_PACKED_ENTRY = dict(zip(MULTI_TERMS, ('sem', 'nrm', 'dep')))


class FusedTail:
    """what render(..., _fused_loss=) takes: the colour target and NeRFLoss's default weights, and at most one of
    mask (n_rays[, 1]) with size_delta: the embed_msk recipe (ngp_render_loss_fused_masked);
    terms: {'semantic': (labels (n_rays) int64, lambda_sem, lambda_sky), 'normal_mono': (normals_gt (n_rays, 3) float32,
        lambda_nm), 'depth_mono': (depth_gt (n_rays) float32, lambda_dm, scene_scale)}, a non-empty subset.  packed=True
        takes exactly one term and selects that term's own entry with its packed terms (ngp_render_loss_fused_sem / _nrm /
        _dep); packed=False selects ngp_render_loss_fused_multi and its 8 terms.
    sky=True (with neither): the background is a colour per ray, the skybox's (ngp_render_loss_fused_sky).  That entry has
        the default entry's accumulator, so `entry` stays 'default'; `symbol` names what is called.
    normal_ref=(lambda_rp, lambda_ro): NeRFLoss's normal_ref terms behind the entry, whichever it is without a mask or a
        skybox (_NormalRefFn: ngp_normal_ref_tail on the entry's ws, Ro and Rp); the model then hands out d(sigma)/dx with a
        graph (NGP.second_order_normals).  The entry and its terms stay what they are; the two terms come beside them.
    `entry` is the key of TAIL_LAYOUT the combination selects."""
    __slots__ = ('rgb_gt', 'lambda_opa', 'lambda_dist', 'mask', 'size_delta', 'terms', 'packed', 'entry', 'sky', 'normal_ref')

    def __init__(self, rgb_gt, lambda_opa, lambda_dist, mask=None, size_delta=0.0, terms=None, packed=False, sky=False,
                 normal_ref=None):
        if sky and (mask is not None or terms is not None):
            raise ValueError("the fused tail composites over a skybox with the default terms only: no mask, no optional terms")
        if normal_ref is not None and (sky or mask is not None):
            raise ValueError("normal_ref goes behind the default, the packed and the multi entries: no mask, no skybox")
        self.normal_ref = None if normal_ref is None else (float(normal_ref[0]), float(normal_ref[1]))
        self.sky = bool(sky)
        if terms is not None and (not terms or any(k not in MULTI_TERMS for k in terms)):
            raise ValueError(f"the multi tail takes a non-empty subset of {MULTI_TERMS}: got {tuple(terms)}")
        if mask is not None and terms is not None:
            raise ValueError("the fused tail takes a mask or optional terms, not both")
        if packed and (terms is None or len(terms) != 1):
            raise ValueError(f"packed=True selects one term's own entry: got {tuple(terms or ())}")
        self.rgb_gt, self.lambda_opa, self.lambda_dist = rgb_gt, lambda_opa, lambda_dist
        self.mask, self.size_delta, self.terms, self.packed = mask, size_delta, dict(terms or {}), bool(packed)
        if terms is None:
            self.entry = 'default' if mask is None else 'masked'
        else:
            self.entry = _PACKED_ENTRY[next(iter(terms))] if packed else 'multi'

    @property
    def symbol(self):
        """the C entry behind ngp_: the TAIL_LAYOUT key's, or the per-ray-background twin of the default entry"""
        if self.sky:
            return "render_loss_fused_sky"
        return "render_loss_fused" + ("" if self.entry == 'default' else "_" + self.entry)


class _RenderLossFn(torch.autograd.Function):
    """The tail of a training step as ONE launch (ngp_render_loss_fused and its five siblings, chosen by `tail`, a
    FusedTail): normals, softmax, compositing, Ref-NeRF regularisers, distortion loss, NeRFLoss's default terms, the terms
    `tail` adds, AND their gradients w.r.t. the field's outputs.
    mask: (n_rays) or (n_rays, 1), the transient mask of the embed_msk recipe (None without one): terms (5) = [loss, rgb,
        opacity, distortion, r_ms], and the mask gets the gradient the same launch computes.
    'semantic': a label outside [0, classes) is ignored (256, the reference's ignore_index, and an 8-bit 255 among them); a
        batch without a valid label has CELoss = 0 and a zero logit gradient, where torch's cross-entropy gives NaN.
    'normal_mono': a row of three exact zeros marks a ray without a normal, which takes no part in the term (the divisor
        stays 3 n_rays).
    'depth_mono': the raw monocular depth (z = depth_gt / 25; zero, negative and NaN mark a ray without depth, which takes
        no part in the fit, the term or any gradient).  A fit kernel ahead of the tail leaves the batch's least-squares
        scale and shift of the composited depths in the workspace (a singular system: (0, 0)); the term reaches the field
        through d_sigmas alone.
    terms: (4) = [loss, rgb, opacity, distortion]; packed, one of [CELoss, sky_depth], [normal_mono], [depth_mono] behind
        them; the multi entry's (8) = [loss, rgb, opacity, distortion, CELoss, sky_depth, normal_mono, depth_mono], a term
        that is not named exactly 0.  The class logits and the normal head's raw output get a gradient only when their
        term is named.
    forward returns (terms, total, vr, opacity, depth, rgb, normal, sem, ws, Ro, Rp, workspace): the workspace as int32
    (the labels' n_valid at int 0; the fit's scale, shift and n_valid at int 12, 13, 14 of the depth entry's and at int
    24, 25, 26 of the multi entry's), None where the entry has none.  Only terms is differentiable, and only through
    terms[0] with a unit seed (NGPTrainer's use): backward hands the gradients computed in forward to the field.
    rgb_bg: None, one colour (3), or with tail.sky one colour per ray (n_rays_total, 3), indexed by rays_a's ray index: the
        skybox's.  Only then does it get a gradient, g_rgb (1 - opacity) of its ray, from the same launch."""

    @staticmethod
    def forward(ctx, sig, rgb_o, sem_logits, np_raw, mask, dsig_dx, dirs, deltas, ts, rays_a, tail, scale3, T_thr, classes,
                rgb_bg=None):
        n, nr = sig.shape[0], rays_a.shape[0]
        dev = sig.device
        f32 = torch.float32
        named = tail.terms
        labels = normals_gt = depth_gt = mask_c = None
        lambda_sem = lambda_sky = lambda_nm = lambda_dm = 0.0
        scene_scale = 1.0
        if mask is not None:
            if mask.numel() != nr:
                raise ValueError(f"mask has {mask.numel()} entries for {nr} rays")
            mask_c = mask.contiguous()
        if 'semantic' in named:
            labels, lambda_sem, lambda_sky = named['semantic']
            if labels.numel() != nr or labels.dtype != torch.int64:
                raise ValueError(f"labels must be {nr} int64 entries, one per ray: got {tuple(labels.shape)} {labels.dtype}")
            if not 1 <= classes <= 16 or sem_logits.shape[1] < classes:
                raise ValueError(f"the semantic tail takes 1 to 16 classes: got {classes} for logits {tuple(sem_logits.shape)}")
            labels = labels.contiguous().view(-1)
        if 'normal_mono' in named:
            normals_gt, lambda_nm = named['normal_mono']
            if tuple(normals_gt.shape) != (nr, 3) or normals_gt.dtype != f32:
                raise ValueError(f"normals must be ({nr}, 3) float32, one row per ray: got {tuple(normals_gt.shape)} "
                                 f"{normals_gt.dtype}")
            normals_gt = normals_gt.contiguous()
        if 'depth_mono' in named:
            depth_gt, lambda_dm, scene_scale = named['depth_mono']
            if tuple(depth_gt.shape) != (nr,) or depth_gt.dtype != f32:
                raise ValueError(f"depths must be ({nr},) float32, one per ray: got {tuple(depth_gt.shape)} {depth_gt.dtype}")
            depth_gt = depth_gt.contiguous()
        total = torch.empty(nr, dtype=torch.int64, device=dev)
        E = lambda *shape: torch.empty(*shape, dtype=f32, device=dev)   # (the caching allocator launches nothing)
        opacity, depth, rgb, normal, Ro, Rp, sem = E(nr), E(nr), E(nr, 3), E(nr, 3), E(nr), E(nr, 3), E(nr, classes)
        ws, d_sig, d_rgb = E(n), E(n), E(n, 3)
        d_sem = E(n, classes) if labels is not None else None
        d_np = E(n, 3) if normals_gt is not None else None
        d_mask = E(nr) if mask is not None else None
        d_bg = None
        if tail.sky:
            if rgb_bg is None or rgb_bg.dim() != 2 or rgb_bg.shape[1] != 3 or rgb_bg.shape[0] < nr or rgb_bg.dtype != f32:
                raise ValueError(f"the sky tail takes a float32 background of at least ({nr}, 3), one row per ray: got "
                                 f"{None if rgb_bg is None else tuple(rgb_bg.shape)}")
            rgb_bg = rgb_bg.contiguous()
            # the launch writes the row of every ray rays_a names; only a batch that leaves rays out needs the fill
            d_bg = E(nr, 3) if rgb_bg.shape[0] == nr else torch.zeros_like(rgb_bg)
        lay = TAIL_LAYOUT[tail.entry]
        acc = E(lay.acc)
        terms, vr = acc[:lay.n_terms], acc[lay.vr_at:lay.vr_at + 2].view(torch.int64)
        if lay.ws_at is not None:
            wsp = acc[lay.ws_at:].view(torch.int32)
        else:
            wsp = torch.empty(lay.ws_ints, dtype=torch.int32, device=dev) if lay.ws_ints else None
        # what each entry takes behind rgb_bg, and behind dL_drgbs
        sem_a, nrm_a = (labels, float(lambda_sem), float(lambda_sky)), (normals_gt, float(lambda_nm))
        dep_a = (depth_gt, float(lambda_dm), float(scene_scale))
        bits = sum(1 << i for i, k in enumerate(MULTI_TERMS) if k in named)
        own_in, own_out = {
            'default': ((), ()),
            'masked': ((mask_c, float(tail.size_delta)), (d_mask,)),
            'sem': (sem_a, (wsp, d_sem)),
            'nrm': (nrm_a, (wsp, d_np)),
            'dep': (dep_a, (wsp,)),
            'multi': ((bits,) + sem_a + nrm_a + dep_a, (wsp, d_sem, d_np)),
        }[tail.entry]
        if tail.sky:
            own_out = (d_bg,)
        call(tail.symbol, sig, rgb_o, dsig_dx, scale3, np_raw,
             np_raw.stride(0), sem_logits, sem_logits.stride(0), dirs, deltas, ts, rays_a, tail.rgb_gt.contiguous(), rgb_bg,
             *own_in, float(T_thr), int(classes), nr, float(tail.lambda_opa), float(tail.lambda_dist), total, vr, opacity,
             depth, rgb, normal, sem, ws, Ro, Rp, terms, d_sig, d_rgb, *own_out)
        ctx.save_for_backward(d_sig, d_rgb, d_sem, d_np, d_mask, d_bg)
        ctx.pad_sem, ctx.pad_np = sem_logits.shape[1] - classes, np_raw.shape[1] - 3
        ctx.mask_shape = mask.shape if mask is not None else None
        ctx.set_materialize_grads(False)             # no zero-filled gradient tensors for the other outputs
        ctx.mark_non_differentiable(*[t for t in (total, vr, opacity, depth, rgb, normal, sem, ws, Ro, Rp, wsp) if t is not None])
        return terms, total, vr, opacity, depth, rgb, normal, sem, ws, Ro, Rp, wsp

    @staticmethod
    def backward(ctx, g_terms, *_unused):
        d_sig, d_rgb, d_sem, d_np, d_mask, d_bg = ctx.saved_tensors
        if d_sem is not None and ctx.pad_sem:
            d_sem = F.pad(d_sem, (0, ctx.pad_sem))
        if d_np is not None and ctx.pad_np:
            d_np = F.pad(d_np, (0, ctx.pad_np))
        if d_mask is not None:
            d_mask = d_mask.view(ctx.mask_shape)
        return (d_sig, d_rgb, d_sem, d_np, d_mask) + (None,) * 9 + (d_bg,)


class _NormalRefFn(torch.autograd.Function):
    """NeRFLoss(normal_ref=True)'s two terms behind a fused tail, one entry call (ngp_normal_ref_tail) on what the tail left:
    ws (constants here: RefLoss composites with detached sigmas), Ro and Rp.
    -> ref_terms (2) = [lambda_rp mean(Rp), lambda_ro mean(Ro)], the means NeRFLoss takes (over 3 n_rays and n_rays).
    The gradients w.r.t. dsig_dx (d(sigma)/dx in normalised coordinates, scale3 applied inside) and the normal head's raw
    output are computed in forward and handed over in backward, as _RenderLossFn does: ref_terms is differentiable only
    with a unit seed on BOTH entries (NGPTrainer's use)."""

    @staticmethod
    def forward(ctx, dsig_dx, np_raw, dirs, ws, rays_a, Ro, Rp, scale3, lambda_rp, lambda_ro):
        n, nr = dsig_dx.shape[0], rays_a.shape[0]
        dev = dsig_dx.device
        if np_raw.stride(1) != 1:
            np_raw = np_raw.contiguous()
        d_grads = torch.empty(n, 3, dtype=torch.float32, device=dev)
        d_np = torch.empty(n, 3, dtype=torch.float32, device=dev)
        if not getattr(rays_a, "_ngp_full_cover", False):   # samples outside every segment: no gradient
            d_grads.zero_()
            d_np.zero_()
        ref_terms = torch.empty(2, dtype=torch.float32, device=dev)
        call("normal_ref_tail", dsig_dx.contiguous(), scale3, np_raw, np_raw.stride(0), dirs.contiguous(), ws, rays_a, nr, Ro, Rp,
             float(lambda_rp), float(lambda_ro), 0, d_grads, d_np, ref_terms)
        ctx.save_for_backward(d_grads, d_np)
        ctx.pad_np = np_raw.shape[1] - 3
        ctx.set_materialize_grads(False)
        return ref_terms

    @staticmethod
    def backward(ctx, g_terms):
        if g_terms is None:
            return (None,) * 10
        d_grads, d_np = ctx.saved_tensors
        if ctx.pad_np:
            d_np = F.pad(d_np, (0, ctx.pad_np))
        return (d_grads, d_np) + (None,) * 8


def _render_loss_fused(model, results, xyzs, dirs, rays_a, T_threshold, classes, fused, kwargs, rays_d=None):
    """fused: the FusedTail of render(..., _fused_loss=)"""
    sig, rgb_o, dsig_dx, np_raw, sem_logits = model._field(xyzs, dirs, kwargs)
    if fused.normal_ref is not None and not dsig_dx.requires_grad:
        raise RuntimeError("FusedTail(normal_ref=...) needs d(sigma)/dx with a graph: set model.second_order_normals = True "
                           "(the Ro term must reach the density field)")
    rgb_bg = None
    if fused.sky:   # as in the reference, the skybox takes precedence over random_bg
        if not kwargs.get('use_skybox', False):
            raise ValueError("FusedTail(sky=True) goes with render(..., use_skybox=True)")
        rgb_bg = model.skybox_rgb(rays_d)
    elif kwargs.get('exp_step_factor', 0.) != 0 and kwargs.get('random_bg', False):
        rgb_bg = torch.rand(3, device=xyzs.device)      # rendering.py:239 (drawn at the same place in the RNG stream)
    (terms, total, vr, opacity, depth, rgb, normal, sem, ws, Ro, Rp, _) = _RenderLossFn.apply(
        sig, rgb_o, sem_logits, np_raw, fused.mask, dsig_dx, dirs.contiguous(), results['deltas'], results['ts'], rays_a, fused,
        model._inv_span(), T_threshold, classes, rgb_bg)
    results['sigma'] = sig
    results['xyzs'] = xyzs
    results['vr_samples'] = vr[0]
    results['opacity'], results['depth'], results['rgb'] = opacity, depth, rgb
    results['normal_pred'], results['semantic'], results['ws'] = normal, sem, ws
    results['Ro'], results['Rp'] = Ro, Rp
    results['Ro']._ngp_normals_have_grad = False
    results['_loss_terms'] = terms        # terms[0] carries the graph: NGPTrainer seeds its backward with 1
    if fused.normal_ref is not None:
        # behind the tail, on its stream: [lambda_rp mean(Rp), lambda_ro mean(Ro)], seeded with (1, 1) beside terms
        results['_ref_terms'] = _NormalRefFn.apply(dsig_dx, np_raw, dirs, ws, rays_a, Ro, Rp, model._inv_span(),
                                                   *fused.normal_ref)
    return results


class _RefLossInputs(torch.autograd.Function):
    """normals_diff = (n_raw - n_pred)^2 (N,3), normals_ori = clamp(<n_raw, normalize(dir)>, 0)^2 (N)
    in one launch (the reference spends ~12 elementwise launches here, rendering.py:243-245)."""

    @staticmethod
    def forward(ctx, normals_raw, normals_pred, dirs):
        normals_raw, normals_pred, dirs = normals_raw.contiguous(), normals_pred.contiguous(), dirs.contiguous()
        n = normals_raw.shape[0]
        ndiff = torch.empty(n, 3, dtype=torch.float32, device=dirs.device)
        nori = torch.empty(n, dtype=torch.float32, device=dirs.device)
        call("refloss_inputs", normals_raw, normals_pred, dirs, n, ndiff, nori)
        ctx.save_for_backward(normals_raw, normals_pred, dirs)
        return ndiff, nori

    @staticmethod
    def backward(ctx, g_diff, g_ori):
        normals_raw, normals_pred, dirs = ctx.saved_tensors
        e = normals_raw - normals_pred
        d_raw = d_pred = None
        if g_diff is not None:
            d_raw = 2 * e * g_diff
            d_pred = -d_raw
        if g_ori is not None:
            dn = F.normalize(dirs, p=2, dim=-1, eps=1e-6)
            dot = torch.clamp(torch.sum(normals_raw * dn, dim=-1, keepdim=True), min=0.)
            t = 2 * dot * dn * g_ori[:, None]
            d_raw = t if d_raw is None else d_raw + t
        return d_raw, d_pred, None


# name-mangled aliases the reference module exposes internally
__render_rays_train = _render_rays_train
__render_rays_test = _render_rays_test
