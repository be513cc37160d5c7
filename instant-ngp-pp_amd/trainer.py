"""Training schedule of the reference's NeRFSystem (train.py:82-345) without Lightning:

  every 16 steps update_density_grid(0.01*1024/sqrt(3), warmup = step < 256)   train.py:272-275
  render() -> NeRFLoss -> sum of term means -> backward                        train.py:279-307
  gradient clipping by global norm 50, Adam(lr, eps=1e-8)                      train.py:244,435
  CosineAnnealingLR over the epochs down to lr/30, stepped once per epoch      train.py:249-251
  ray-batch data parallel: every rank draws its own rays, gradients are averaged  train.py:430-432

MI355X-specific structure:
  * all parameters live in ONE flat fp32 buffer (rgb table | xyz table | MLPs) with matching flat
    gradient / Adam-state buffers, laid out by flat_layout(); the Adam launches also apply the clip
    coefficient and zero the gradient;
  * the hash-grid scatter kernels accumulate straight into the flat gradient buffer (no
    zeros_like + add pass over 800 MB);
  * on one GPU clip + Adam run on the optimizer stream as a sweep of two pieces, [xyz table | MLPs]
    first and the rgb table second, each with an event the field waits for where it first reads
    those parameters (NGPTrainer._sweep);
  * with world_size > 1 the optimizer is sharded (ZeRO-1 style): gradients are reduce-scattered
    over RCCL (the rgb-table bucket, 77 % of the bytes, as soon as its scatter-add is enqueued, so
    it overlaps the density-path backward), every rank runs clip + Adam on its 1/N slice only
    (Adam's 6.4 GB/step of HBM traffic becomes 6.4/N GB), and the updated parameter slices are
    all-gathered.  Same bytes on xGMI as an all-reduce, 1/N of the optimizer time and state
    (NGPTrainer._sharded_step).

NGPTrainer.step and NGPTrainer._sweep are schedules: their bodies are the ordered calls of the stages,
which are methods because the state they share lives on the trainer (DESIGN.md section 5 draws both).
"""
import math
import os
from types import MappingProxyType
from typing import Dict, NamedTuple, Tuple

import torch
import torch.distributed as dist

from ._lib import call
from .appearance import RayCodes
from .losses import NeRFLoss, nerf_loss_and_grads
from .recipe import _TAIL_TERMS, resolve
from .rendering import MAX_SAMPLES, TAIL_LAYOUT, FusedTail, MarchAhead, _fused_tail_ok, render

_f32 = torch.float32
ADAM = (0.9, 0.999, 1e-8, 0.0)   # beta1, beta2, eps, weight decay of every Adam launch (train.py:244)
_COLOUR_TABLE, _DENSITY_TABLE = "rgb_encoder.params", "xyz_encoder.params"


class FlatLayout(NamedTuple):
    """where every parameter lies in the flat store (elements of fp32); flat_layout() makes it, nothing changes it"""
    names: Tuple[str, ...]                    # the store's order
    slices: Dict[str, Tuple[int, int]]        # name -> (offset, numel)
    sizes: Tuple[int, ...]                    # the padded length of every slice, in the store's order
    total: int
    b0: int                                   # end of the colour table's bucket, 0 without one
    bounds: Tuple[int, ...]                   # of the buckets: (0, b0, total), or (0, total) without a colour bucket
    mlp_lo: int                               # first element behind the two tables, 0 where they do not lead the store
    world: int


def flat_layout(named_sizes, world=1):
    """[(name, numel)] in the model's order (the mask model's and the appearance codes behind it) and the number of
    ranks -> the FlatLayout: the colour table, then the density table, then the rest as given; every slice starts on 16
    bytes; bucket 0 is the colour table alone, bucket 1 everything else, each divisible by 4 * world so that every rank's
    shard of it starts on 16 bytes too.  Launches nothing."""
    lead = {_COLOUR_TABLE: 0, _DENSITY_TABLE: 1}
    named = sorted(named_sizes, key=lambda ns: lead.get(ns[0], 2))
    names = tuple(n for n, _ in named)
    colour = names[0] == _COLOUR_TABLE
    quantum = 4 * world
    sizes = [(numel + 3) // 4 * 4 for _, numel in named]
    if colour:
        sizes[0] = (sizes[0] + quantum - 1) // quantum * quantum
    rest = sum(sizes[1:] if colour else sizes)
    sizes[-1] += (quantum - rest % quantum) % quantum
    total, b0 = sum(sizes), sizes[0] if colour else 0
    slices, off = {}, 0
    for (n, numel), sz in zip(named, sizes):
        slices[n] = (off, numel)
        off += sz
    bounds = (0, b0, total) if b0 else (0, total)
    # first element behind the two tables (the MLP parameters): their share of the norm is always summed exactly
    mlp_lo = slices[names[2]][0] if colour and names[1:2] == (_DENSITY_TABLE,) and len(names) > 2 else 0
    assert all(o % 4 == 0 for o, _ in slices.values()) and all((hi - lo) % quantum == 0 for lo, hi in zip(bounds, bounds[1:]))
    return FlatLayout(names, MappingProxyType(slices), tuple(sizes), total, b0, bounds, mlp_lo, world)


class GradBuckets:
    """Collectives over contiguous buckets of the flat gradient / parameter buffers (device
    agnostic: the gloo CPU tests drive this class directly).

    all-reduce mode   : reduce_bucket(i) sums bucket i over the ranks (async), wait() joins.
    sharded mode      : reduce_scatter_bucket(i, out) gives rank r the summed slice r of bucket i
                        (RCCL reduce-scatter into the rank's own shard buffer),
                        all_gather_bucket(i, flat_param, shard) publishes each rank's updated
                        parameter slice to everyone.
    Buckets must be a multiple of world*4 elements long in sharded mode (the trainer pads).
    """

    def __init__(self, flat_grad, boundaries, group=None, solo=True):
        self.flat = flat_grad
        self.bounds = list(boundaries)  # [0, b1, ..., n]
        self.group = group
        self.works = []
        # solo=False: a ONE-rank process group still sends every collective of the N>1 path through
        # the backend (a rehearsal of the RCCL calls on a single-GPU box, see NGPTrainer.force_sharded)
        self.solo = solo
        # set to a list to record every collective issued from now on: (op, bucket, payload bytes, HIP stream the
        # call was enqueued behind) — bench.py --gpus N prints it per rank
        self.trace = None

    def _issue(self, op, i, nbytes, fn):
        """runs fn() (which issues one collective and returns its work object or None).  With `trace` set the
        collective is also TIMED: HIP events on the issuing stream before the call and behind the work's completion
        (the work is waited for at once, so the traced steps serialise their collectives: durations are those of
        each collective by itself beside whatever the other streams run, not the overlapped schedule)."""
        if self.trace is None:
            return fn()
        rec = {"op": op, "bucket": int(i), "bytes": int(nbytes),
               "stream": int(torch.cuda.current_stream().cuda_stream) if self.flat.is_cuda else 0}
        if self.flat.is_cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            w = fn()
            if w is not None:
                w.wait()
            e1.record()
            rec["events"] = (e0, e1)
        else:
            w = fn()
        self.trace.append(rec)
        return w

    @property
    def world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    @property
    def rank(self):
        return dist.get_rank(self.group) if dist.is_available() and dist.is_initialized() else 0

    def _native_rs(self):
        return dist.get_backend(self.group) == "nccl"

    def shard_range(self, i):
        lo, hi = self.bounds[i], self.bounds[i + 1]
        s = (hi - lo) // self.world
        return lo + self.rank * s, lo + (self.rank + 1) * s

    def reduce_bucket(self, i):
        if self.world == 1 and self.solo:
            return
        lo, hi = self.bounds[i], self.bounds[i + 1]
        self.works.append(self._issue("all_reduce", i, 4 * (hi - lo), lambda: dist.all_reduce(
            self.flat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True)))

    def reduce_scatter_bucket(self, i, out):
        """out (own buffer, 1/world of the bucket) <- this rank's slice of the bucket summed over ranks"""
        if self.world == 1 and self.solo:
            return
        lo, hi = self.bounds[i], self.bounds[i + 1]
        if self._native_rs():
            self.works.append(self._issue("reduce_scatter", i, 4 * (hi - lo), lambda: dist.reduce_scatter_tensor(
                out, self.flat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True)))
        else:  # gloo has no reduce-scatter: all-reduce, then the owner copies its slice out
            a, b = self.shard_range(i)

            def via_all_reduce():
                dist.all_reduce(self.flat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True).wait()
                out.copy_(self.flat[a:b])
            self._issue("reduce_scatter", i, 4 * (hi - lo), via_all_reduce)
            self.works.append(None)       # one entry per bucket, in issue order (NGPTrainer sums each shard behind its own)

    def all_gather_bucket(self, i, flat_param, shard, detach=False):
        """flat_param[bucket i] <- concatenation over ranks of `shard` (own buffer)"""
        if self.world == 1 and self.solo:
            return None
        lo, hi = self.bounds[i], self.bounds[i + 1]
        if self._native_rs():
            w = self._issue("all_gather", i, 4 * (hi - lo), lambda: dist.all_gather_into_tensor(
                flat_param[lo:hi], shard, group=self.group, async_op=True))
        else:
            s = (hi - lo) // self.world
            views = [flat_param[lo + r * s: lo + (r + 1) * s] for r in range(self.world)]
            w = self._issue("all_gather", i, 4 * (hi - lo), lambda: dist.all_gather(views, shard, group=self.group, async_op=True))
        if detach:
            return w   # the caller waits for it where the gathered parameters are first read
        self.works.append(w)
        return None

    def wait(self):
        for w in self.works:
            if w is not None:
                w.wait()
        self.works = []

    def take_works(self):
        """hands the pending work objects (issue order) to the caller, who waits for them one by one"""
        ws, self.works = self.works, []
        return ws


def shard_seed(base_seed, rank):
    """per-rank decorrelated ray sampling (the reference leaves this to
    DataLoader worker seeding)"""
    return int(base_seed) + int(rank)


def _adam(entry, param, grad, exp_avg, exp_avg_sq, lr, step, coef, *last):
    """Adam with this clip coefficient (a device scalar) over one contiguous piece.  entry: adam_step or adam_step_width;
    last: that entry's closing arguments (whether the launch clears the gradient[, the launch width])"""
    call(entry, param, grad, exp_avg, exp_avg_sq, grad.numel(), float(lr), *ADAM, step, coef, *last)


class NGPTrainer:
    def __init__(self, model, lr=1e-2, num_epochs=20, steps_per_epoch=1000, clip_norm=50.0,
                 exp_step_factor=0.0, num_classes=7, density_threshold=0.01, render_kwargs=None, group=None,
                 force_sharded=None, loss_kwargs=None, msk_model=None, embedding_a=None, pose_refiner=None, pose_lr=1e-6,
                 semantic=False, normal_mono=False, depth_mono=False, multi_terms=(), use_exposure=False,
                 unit_exposure_rgb=0.5, use_skybox=False, normal_ref=False):
        """The options semantic, normal_mono, depth_mono, multi_terms, use_exposure (with unit_exposure_rgb), use_skybox,
        normal_ref and pose_refiner are described in recipe.py, each next to its row of the table that says what it combines
        with, what it needs from step() and which clip route its step takes; recipe.resolve() checks them here.
        embedding_a: the nn.Embedding(n_imgs, embed_a_len) of the embed_a recipe (or a FrameEmbedding, whose table is
        taken), for a model built with embed_a=True.  Its weight joins the flat store behind the model's parameters as
        'embedding_a.weight' (the reference keeps it in net_opt, train.py:238-244: one Adam, one schedule, one clip), step()
        then needs img_idxs=, and the field reads and differentiates the table through ngp_embed_a_fwd / ngp_embed_a_bwd.
        msk_model: an implicit_mask (the reference's embed_msk recipe, train.py:112-113, 280-299).  Its parameters join
        the flat store behind the model's as 'msk_model.<key>' (one Adam, one schedule, one clip: the reference keeps it in
        net_opt), step() then needs uvi=, and the step stays on the fused render + loss tail and on the norm-bound clip.
        loss_kwargs: the flags train.py:289-300 hands to NeRFLoss (recipe.OPTIONAL_LOSS_TERMS, scale, ...): the
        launch-per-operation route of the options above, which recipe.py describes beside each option's row.  Any
        optional term takes the step to the NeRFLoss module; normal_ref there also switches the model to differentiable
        normals (the Ro term must reach the density table through normals_raw, reference networks.py:186-196).
        force_sharded: take the sharded-optimizer path (reduce-scatter / Adam on the slice / all-gather)
        even with ONE rank in the process group, so that a single-GPU box can rehearse every RCCL call of
        the N>1 path; None reads the environment variable NGP_FORCE_SHARDED."""
        self.model = model
        self.msk_model = msk_model
        self.embedding_a = getattr(embedding_a, "embedding_a", embedding_a)
        if self.embedding_a is not None:
            E = model.rgb_net.n_input_dims - 144 if getattr(model, "embed_a", False) else 0
            if tuple(self.embedding_a.weight.shape[1:]) != (E,):
                raise ValueError(f"embedding_a has codes of length {tuple(self.embedding_a.weight.shape[1:])}, the model "
                                 f"was built with embed_a={bool(E)}, embed_a_len={E}")
        self.force_sharded = bool(os.environ.get("NGP_FORCE_SHARDED")) if force_sharded is None else bool(force_sharded)
        self.pose_refiner, self.pose_lr = pose_refiner, float(pose_lr)
        self.base_lr = lr
        self.num_epochs = num_epochs
        self.steps_per_epoch = steps_per_epoch
        self.clip_norm = clip_norm
        self.exp_step_factor = exp_step_factor
        self.num_classes = num_classes
        self.density_threshold = density_threshold
        self.render_kwargs = dict(render_kwargs or {})
        self.loss_fn = NeRFLoss()
        self.loss_kwargs = dict(loss_kwargs or {})
        joined = dist.is_available() and dist.is_initialized()
        world = dist.get_world_size(group) if joined else 1
        self.recipe = resolve(
            model, msk_model=msk_model, embedding_a=self.embedding_a, pose_refiner=pose_refiner, render_kwargs=self.render_kwargs,
            loss_kwargs=self.loss_kwargs, num_classes=num_classes, force_sharded=self.force_sharded, ranks=world,
            semantic=semantic, normal_mono=normal_mono, depth_mono=depth_mono, multi_terms=multi_terms,
            use_exposure=use_exposure, unit_exposure_rgb=unit_exposure_rgb, use_skybox=use_skybox, normal_ref=normal_ref)
        if self.recipe.normal_ref:
            model.second_order_normals = True
        if self.loss_kwargs.get("normal_ref"):
            model.differentiable_normals = True
        self.warmup_steps = 256
        self.update_interval = 16
        self.global_step = 0
        self.group = group
        # Launch width of the Adam sweep (ngp_adam_step_width): how the sweep shares the CUs with the next step's density path
        # decides a few per cent of the step, and which width wins depends on the loop around the trainer (resident batches
        # or a loader at the head of every step) and on the box.  None = measure: after the all-cells
        # warm-up, windows of `update_interval` steps alternate between the candidates (4 windows each, timed with HIP
        # events on the optimizer stream, no host synchronisation), then the faster one stays.  The result of a step does
        # not depend on the width.  NGP_ADAM_WIDTH=<n> / adam_width=<n> fixes it.
        w = os.environ.get("NGP_ADAM_WIDTH", "")
        self.adam_width = int(w) if w.isdigit() else None
        self.adam_candidates = (512, 256)
        self.adam_tune = (320, 4)            # first step of the measurement, windows per candidate
        self._tune_events, self._tune_widths = [], []
        self._grad_zeroed = None
        self._flatten(world, forced=bool(self.force_sharded and joined))
        dev = self.flat_param.device
        self._opt_stream = torch.cuda.Stream(device=dev) if dev.type == "cuda" else None
        self._march_ahead = MarchAhead(dev) if dev.type == "cuda" else None
        # the seed of the fused tail's terms ([1, 0, ...]: the loss is term 0; as many as the recipe's entry has), of the two
        # normal_ref terms, and the tone-mappers' inputs at zero log-radiance and unit exposure
        n_terms = TAIL_LAYOUT[FusedTail(None, 0.0, 0.0, mask=self.msk_model, terms=dict.fromkeys(self.recipe.tail_terms) or None,
                                        packed=self.recipe.packed).entry].n_terms
        self._terms_seed = torch.tensor([1.0] + [0.0] * (n_terms - 1), device=dev)
        self._ref_seed = torch.ones(2, device=dev)
        self._unit_inputs = (torch.zeros(1, 3, device=dev), torch.ones(1, 1, device=dev))
        self._link_field()
        if pose_refiner is not None:
            self._own_poses()

    # ------------------------------------------------------------------ flat parameter store
    def _flatten(self, world, forced):
        """allocates the flat store as flat_layout() lays it out for `world` ranks and re-points the parameters and their
        gradients into it; forced: the sharded path with ONE rank in the group (force_sharded)"""
        named = [(n, p) for n, p in self.model.named_parameters() if p.numel() > 0]
        if self.msk_model is not None:   # behind the model's: in the tail whose squares are always summed exactly (_mlp_lo)
            named += [("msk_model." + n, p) for n, p in self.msk_model.named_parameters()]
        if self.embedding_a is not None:   # likewise in that tail
            named += [("embedding_a.weight", self.embedding_a.weight)]
        params = dict(named)
        lay = self.layout = flat_layout([(n, p.numel()) for n, p in named], world)
        self.names, self.slices, self._mlp_lo, total = list(lay.names), dict(lay.slices), lay.mlp_lo, lay.total
        dev = params[lay.names[0]].device
        self.sharded = world > 1 or forced
        self.flat_param = torch.zeros(total, dtype=_f32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=_f32, device=dev)
        self.scalars = torch.zeros(2, dtype=_f32, device=dev)  # [sum of squares, clip coefficient]
        # clipping from a norm bound (ngp_clip_decide): sum_s ||dz2[s]|| of the two MLPs that feed the encoders, and the
        # device flag "the bound did not settle it: compute the exact norm"
        self.norm_acc = torch.zeros(2, dtype=_f32, device=dev)
        self.need_exact = torch.zeros(1, dtype=torch.int32, device=dev)
        for n, (off, numel) in lay.slices.items():
            p = params[n]
            view = self.flat_param[off:off + numel].view_as(p)
            view.copy_(p.data)
            p.data = view
            p.grad = self.flat_grad[off:off + numel].view_as(p)
        # bucket 0 = rgb table, bucket 1 = everything else
        self.buckets = GradBuckets(self.flat_grad, lay.bounds, group=self.group, solo=not forced)
        # Adam state: whole buffer on one GPU; with N ranks each rank keeps (and updates) only its
        # 1/N slice of every bucket — reduce-scatter gradients, Adam on the slice, all-gather params
        if self.sharded:
            self.shards = [self.buckets.shard_range(i) for i in range(len(lay.bounds) - 1)]
            self.exp_avg = [torch.zeros(b - a, dtype=_f32, device=dev) for a, b in self.shards]
            self.exp_avg_sq = [torch.zeros(b - a, dtype=_f32, device=dev) for a, b in self.shards]
            # master copy of this rank's parameter slices and the landing buffers of the reduce-scatter
            self.param_shard = [self.flat_param[a:b].clone() for a, b in self.shards]
            self.grad_shard = [torch.zeros(b - a, dtype=_f32, device=dev) for a, b in self.shards]
        else:
            self.exp_avg = torch.zeros(total, dtype=_f32, device=dev)
            self.exp_avg_sq = torch.zeros(total, dtype=_f32, device=dev)
        self.norm_bound = bool(self._mlp_lo and dev.type == "cuda" and not self.sharded and hasattr(self.model, "xyz_net"))
        self._bound_step = False
        self._norm_share_armed = False   # step() arms it: exactly one backward per optimizer step
        self._norm_share_fired = 0

    def _link_field(self):
        """everything the field does on this trainer's behalf: the model's and the mask model's FieldLink (link.py) and the
        two encoders' per-table slots (tinycudann.Encoding)"""
        m, link = self.model, self.model.link
        # the backwards of the field, the appearance codes and the mask field add straight into these views of the flat gradient
        lin1, lin2 = m.xyz_net[0], m.xyz_net[2]
        sinks = {"W1": lin1.weight, "b1": lin1.bias, "W2": lin2.weight, "b2": lin2.bias, "rgb_p": m.rgb_net.params,
                 "nrm_p": m.norm_pred_header.params, "sem_p": m.semantic_header.params}
        if self.embedding_a is not None:
            sinks["embedding_a"] = self.embedding_a.weight
        tone = m._stock_tonemappers()
        if tone:   # ngp_tonemap_bwd's sinks (networks._ToneMapFn); other tone-mappers keep autograd's route
            sinks.update({f"tone_{i}": t.params for i, t in enumerate(tone)})
        if getattr(m, "_stock_skybox", None) and m._stock_skybox():   # ngp_skybox_bwd's sink (networks._SkyFn)
            sinks["sky"] = m.skybox_rgb_net.params
        link.grad_sinks = {name: p.grad for name, p in sinks.items()}
        if self.msk_model is not None:
            k, (l1, l2) = self.msk_model, (self.msk_model.mask_net[0], self.msk_model.mask_net[2])
            k.link.grad_sinks = {"table": k.mask_encoder.params.grad, "W1": l1.weight.grad, "b1": l1.bias.grad,
                                 "W2": l2.weight.grad, "b2": l2.bias.grad}
        if self.flat_param.is_cuda and not self.sharded:
            # Four streams, one per hardware queue of the HIP runtime's default pool (DESIGN.md section 5,
            # profiles/r03_occupancy_shaping.txt (12)): the backward's table scatters of THIS trainer's model go on the optimizer
            # stream (clip + Adam follow them there anyway) and its two heads on the march-ahead stream (idle in the middle of
            # the forward) instead of streams of their own, which would share queues by the accident of creation order.
            link.side_stream, link.heads_stream = self._opt_stream, self._march_ahead.stream
        # the scatter kernels accumulate directly into the flat gradient (networks._FieldFn, tinycudann._GridFwd)
        for enc in (m.rgb_encoder, m.xyz_encoder):
            enc.grad_buffer = enc.params.grad
        # bucket 0's reduce-scatter is fired from the colour encoder's backward (overlaps the rest)
        self.hooked0 = bool(self.sharded and self.layout.b0)
        if self.hooked0:
            m.rgb_encoder.on_grad_ready = lambda: self.buckets.reduce_scatter_bucket(0, self.grad_shard[0])
            m.rgb_encoder.grad_ready_is_collective = True   # the field's backward then scatters colour first
        elif self.layout.b0 and self.flat_param.is_cuda:
            # one GPU: the colour table's share of the gradient norm (77 % of the entries) is summed right behind its
            # scatter, beside the density head's backward, instead of on the path between the last scatter and Adam
            m.rgb_encoder.on_grad_ready = self._early_norm_share

    def _own_poses(self):
        """dR and dT move into one buffer [parameters | gradients | exp_avg | exp_avg_sq], each part [dR | dT] with both
        pieces 16-byte aligned; ngp_pose_rays_bwd adds straight into the gradient part"""
        ref, dev = self.pose_refiner, self.flat_param.device
        if ref.dR.device != dev:
            raise ValueError(f"pose_refiner is on {ref.dR.device}, the model on {dev}")
        n = ref.dR.numel()
        seg = (n + 3) // 4 * 4
        buf = torch.zeros(4, 2 * seg, dtype=_f32, device=dev)
        self.pose_param, self.pose_grad, self.pose_exp_avg, self.pose_exp_avg_sq = buf[0], buf[1], buf[2], buf[3]
        for k, p in enumerate((ref.dR, ref.dT)):
            view = self.pose_param[k * seg:k * seg + n].view_as(p)
            view.copy_(p.data)
            p.data = view
            p.grad = self.pose_grad[k * seg:k * seg + n].view_as(p)
        ref.grad_sink = (ref.dR.grad, ref.dT.grad)
        self.pose_scalars = torch.zeros(2, dtype=_f32, device=dev)   # [sum of squares, clip coefficient]
        self.pose_steps = 0

    def _pose_step(self):
        """clip_grad_norm_(clip_norm) and Adam(pose_lr, eps=1e-8) over [dR | dT]; the gradient is cleared by the Adam launch"""
        self.pose_steps += 1
        n = self.pose_grad.numel()
        self.pose_scalars.zero_()
        call("sumsq", self.pose_grad, n, self.pose_scalars[0:1])
        call("clip_coef", self.pose_scalars[0:1], float(self.clip_norm), 1.0, self.pose_scalars[1:2])
        _adam("adam_step", self.pose_param, self.pose_grad, self.pose_exp_avg, self.pose_exp_avg_sq, self.pose_lr,
              self.pose_steps, self.pose_scalars[1:2], 1)

    def _unit_exposure_rgb(self):
        """the tone-mappers at zero log-radiance and unit exposure, (1, 3) with a graph to their parameters"""
        return self.model.log_radiance_to_rgb(self._unit_inputs[0], exposure=self._unit_inputs[1])

    def _unit_exposure_term(self):
        """-> (unit (1,3), the gradient of the term w.r.t. it, the term): mean over the channels of
        0.5 (unit - unit_exposure_rgb)^2 (train.py:301-306), seeded directly as the default terms are"""
        unit = self._unit_exposure_rgb()
        with torch.no_grad():
            diff = unit - self.recipe.unit_exposure_rgb
            return unit, diff / 3.0, 0.5 * (diff * diff).mean()

    def _early_norm_share(self):
        """the colour encoder's on_grad_ready on one GPU: the colour table's sum of squares behind its scatter, once per
        announced backward and not on a bound step"""
        if self._norm_share_armed and not self._bound_step:
            self._norm_share_fired += 1
            if self._norm_share_fired == 1:
                b0 = self.layout.b0
                call("sumsq", self.flat_grad[0:b0], b0, self.scalars[0:1])

    # ------------------------------------------------------------------ schedule
    def lr_at(self, epoch):
        eta_min = self.base_lr / 30
        return eta_min + (self.base_lr - eta_min) * (1 + math.cos(math.pi * epoch / self.num_epochs)) / 2

    def sky_active(self):
        """whether the step about to be taken composites over the skybox: a trainer built with use_skybox=True, from
        global_step >= warmup_steps on (train.py:160)"""
        return bool(self.recipe.use_skybox and self.global_step >= self.warmup_steps)

    def step(self, rays_o, rays_d, rgb_gt, next_rays=None, target=None, uvi=None, img_idxs=None, pix_idxs=None, labels=None,
             normals=None, depths=None, exposure=None, **loss_kwargs):
        """one training step on this rank's ray batch; returns (loss tensor, results dict).

        labels, normals, depths, exposure: the per-ray targets of the options the trainer was built with (recipe.py describes
        each next to its option's row): exactly those it needs, any other is refused.  A trainer built with a term on the
        fused tail, with use_skybox=True (the skybox joins the step from global_step >= warmup_steps on) or with
        normal_ref=True takes no target= and no per-step loss term.

        uvi: (n_rays, 3) input of the trainer's msk_model (implicit_mask.uvi), required when there is one.
        img_idxs: (n_rays) image index of every ray, required when the trainer has an embedding_a or a pose_refiner.
        pix_idxs: (n_rays) pixel index of every ray (into the refiner's `directions`), required with a pose_refiner; rays_o
        and rays_d are then None (the rays come from the refiner's current dR, dT) and there is no next_rays: a march-ahead
        would use poses that are one update old.

        target: further per-ray supervision for NeRFLoss's optional terms ('normal', 'label', 'depth': the
        batch dictionary of train.py:299); loss_kwargs: per-step additions to the trainer's loss_kwargs
        (e.g. mask=..., step=...).

        next_rays = (rays_o, rays_d) of the FOLLOWING step, if the caller already has them (a
        data loader that is one batch ahead): their AABB test and occupancy march are then run on a
        side stream under this step's backward and the next call picks the result up, provided it
        is called with the very same tensors and no density-grid update lies in between."""
        recipe = self.recipe
        recipe.check_step(rays_o, rays_d, rgb_gt, next_rays=next_rays, target=target, uvi=uvi, img_idxs=img_idxs,
                          pix_idxs=pix_idxs, labels=labels, normals=normals, depths=depths, exposure=exposure,
                          loss_kwargs=loss_kwargs)
        sky_on = self.sky_active()
        default_recipe = bool(recipe.fused_loss and not loss_kwargs and not target)
        rays_o, rays_d = self._rays(rays_o, rays_d, img_idxs, pix_idxs)
        self._join_grad_zeroing()
        self._update_occupancy()
        marched, march_next = self._take_march(rays_o, rays_d, next_rays)
        extra, mask = self._render_extras(rays_o, rgb_gt, default_recipe, sky_on, uvi, img_idxs, pix_idxs, exposure,
                                          {"labels": labels, "normals": normals, "depths": depths})
        results = render(self.model, rays_o, rays_d, exp_step_factor=self.exp_step_factor,
                         num_classes=self.num_classes, marched=marched, **self.render_kwargs, **extra)
        if march_next is not None:
            march_next()
        self._announce_backward(default_recipe)
        recipe.check_took_fused_tail(results, extra.get('_fused_loss'), sky_on)
        if '_loss_terms' in results:
            loss = self._backward_fused_tail(results)
        elif default_recipe and not recipe.masked:
            loss = self._backward_seeded_terms(results, rgb_gt, exposure)
        else:
            loss = self._backward_loss_module(results, rgb_gt, target, loss_kwargs, mask, exposure)
        self.optimizer_step()
        return loss.detach(), results

    # ------------------------------------------------------------------ the stages of step(), in its order
    def _rays(self, rays_o, rays_d, img_idxs, pix_idxs):
        """with a pose_refiner: the batch's rays from the current dR, dT (ngp_pose_rays on the caller's stream)"""
        if self.pose_refiner is None:
            return rays_o, rays_d
        with torch.no_grad():   # the values only: the graph starts at the samples (rendering._render_rays_train)
            return self.pose_refiner.rays(img_idxs, pix_idxs)

    def _join_grad_zeroing(self):
        """sharded: the caller's stream waits for the fill that cleared flat_grad behind the previous optimizer step"""
        ev, self._grad_zeroed = self._grad_zeroed, None
        if ev is not None:
            ev.wait()

    def _update_occupancy(self):
        """every update_interval steps: the model's occupancy-grid update, on the caller's stream"""
        if self.global_step % self.update_interval == 0:
            self.model.update_density_grid(self.density_threshold * MAX_SAMPLES / 3 ** 0.5,
                                           warmup=self.global_step < self.warmup_steps)

    def _take_march(self, rays_o, rays_d, next_rays):
        """-> (this batch's march as MarchAhead left it, or None for render() to march inline; the next batch's launch as
        a callable to run behind render(), or None).  Launches the AABB test and the march on the march-ahead stream: this
        batch's when none is in flight for it, the next batch's unless an occupancy update lies before its step."""
        ahead, model, esf = self._march_ahead, self.model, self.exp_step_factor
        if ahead is None:
            return None, None
        marched = ahead.take(rays_o, rays_d, esf)
        if next_rays is None:
            return marched, None
        late = marched is None
        if late:   # nothing in flight for this batch: march it now, same route
            ahead.launch(model, rays_o, rays_d, esf)
            marched = ahead.take(rays_o, rays_d, esf)
        if (self.global_step + 1) % self.update_interval == 0:
            return marched, None
        if late:   # the host has just waited for this batch's march (a step that starts with an occupancy update): the
            # device is idle until the forward is enqueued - the next batch's march goes behind it
            return marched, lambda: ahead.launch(model, next_rays[0], next_rays[1], esf)
        ahead.launch(model, next_rays[0], next_rays[1], esf)
        return marched, None

    def _render_extras(self, rays_o, rgb_gt, default_recipe, sky_on, uvi, img_idxs, pix_idxs, exposure, given):
        """-> (render()'s keywords beyond the trainer's render_kwargs, the mask or None).  With a msk_model: its forward on
        the caller's stream, behind the sweep's first piece.  On the default recipe: the FusedTail that makes render() end
        in one render + loss launch; given: step()'s targets of the tail's terms by argument name."""
        model, recipe, extra, mask = self.model, self.recipe, {}, None
        if recipe.masked:
            model.link.join_params(rgb_table=False)   # the mask parameters sit in the Adam sweep's first piece
            mask = self.msk_model(uvi)
        if default_recipe and rays_o.is_cuda:
            # render + loss + the loss's gradients as one launch behind the field (rendering._RenderLossFn)
            fn, terms = self.loss_fn, recipe.tail_terms
            tail = extra['_fused_loss'] = FusedTail(
                rgb_gt, fn.lambda_opa, fn.lambda_distortion, mask=mask,
                # size_delta of the step being taken (losses.py:60-69, 85)
                size_delta=fn.Annealing.getWeight(self.global_step) if recipe.masked else 0.0,
                terms={n: _TAIL_TERMS[n].entry(self, given[_TAIL_TERMS[n].arg], rays_o.device) for n in terms} or None,
                packed=recipe.packed, sky=sky_on,
                normal_ref=(fn.lambda_normal_ref_rp, fn.lambda_normal_ref_ro) if recipe.normal_ref else None)
            if terms and not _fused_tail_ok(model, self.render_kwargs, self.exp_step_factor, self.num_classes, tail):
                # (rgb_act or differentiable_normals changed after construction, ...): never a step without the targets
                raise RuntimeError(f"{recipe.asked}: the model no longer fits the fused tail (rendering._fused_tail_ok); the "
                                   "targets would be left out of the loss")
        if self.embedding_a is not None:
            extra['embedding_a'] = RayCodes(self.embedding_a.weight, img_idxs)
        if self.pose_refiner is not None:
            extra['_pose'] = (self.pose_refiner, img_idxs, pix_idxs)
        if exposure is not None:
            extra['exposure'] = exposure.detach().to(_f32).reshape(-1, 1)
        if sky_on:
            extra['use_skybox'] = True
        return extra, mask

    def _announce_backward(self, default_recipe):
        """everything the clip route needs before the backward runs (launches nothing): one backward follows, then the
        optimizer step, whose _clip_route() reads and disarms what is set here"""
        model = self.model
        self._norm_share_armed, self._norm_share_fired = True, 0
        # clip_grad_norm_(50) from an upper bound of the norm (ngp_clip_decide) instead of the 0.8 GB sum-of-squares
        # pass: only on the default recipe, where the fused field backward is the one writer of the table gradients, and
        # with the options for which the bound holds (recipe.py says why, row by row)
        self._bound_step = bool(self.norm_bound and default_recipe and not model.differentiable_normals
                                and not self.recipe.exact_norm())
        model.link.begin_bound_step(self.norm_acc if self._bound_step else None)
        if self.norm_bound:
            model.rgb_encoder._bound_valid = model.xyz_encoder._bound_valid = True

    def _backward_fused_tail(self, results):
        """the fused tail's route: the backward of the whole step from the entry's terms (and, with normal_ref, the two
        terms behind it), seeded in one call (one backward per step: _norm_share_armed) -> the loss"""
        terms = results.pop('_loss_terms')
        loss = terms[0]
        if self.recipe.tail_terms:
            results['loss_terms'] = terms.detach()   # the entry's terms (rendering._RenderLossFn): for a caller's log
        if not self.recipe.normal_ref:
            torch.autograd.backward([terms], [self._terms_seed])
            return loss
        # [the entry's terms | normal_ref_rp, normal_ref_ro], loss with both
        ref_terms = results.pop('_ref_terms')
        with torch.no_grad():
            all_terms = torch.cat([terms, ref_terms])
            all_terms[0] += ref_terms.sum()
        results['loss_terms'] = all_terms
        torch.autograd.backward([terms, ref_terms], [self._terms_seed, self._ref_seed])
        return all_terms[0]

    def _backward_seeded_terms(self, results, rgb_gt, exposure):
        """the default terms without the fused tail (a tone-mapped model, CPU tensors): same value and gradients as
        sum(term.mean()) over NeRFLoss's default terms, the gradients seeded directly (no loss node, no multiplications by
        1); with exposure the unit-exposure term in the same backward call -> the loss"""
        terms, (d_rgb, d_op, d_ws) = nerf_loss_and_grads(
            results["rgb"], results["opacity"], results["ws"], results["deltas"], results["ts"],
            results["rays_a"], rgb_gt, self.loss_fn.lambda_opa, self.loss_fn.lambda_distortion)
        outs, seeds = [results["rgb"], results["opacity"]], [d_rgb, d_op]
        if d_ws is not None:
            outs.append(results["ws"])
            seeds.append(d_ws)
        if exposure is not None:
            # train.py:301-306; seeded in the same backward call (one backward per step: _norm_share_armed)
            unit, d_unit, term = self._unit_exposure_term()
            terms = torch.cat([terms, term.reshape(1)])
            terms[0] += term
            results['loss_terms'] = terms
            outs.append(unit)
            seeds.append(d_unit)
        torch.autograd.backward(outs, seeds)
        return terms[0]

    def _backward_loss_module(self, results, rgb_gt, target, loss_kwargs, mask, exposure):
        """the launch-per-operation route: NeRFLoss with the trainer's and the step's loss_kwargs, the sum of the term
        means, loss.backward() -> the loss"""
        batch = {"rgb": rgb_gt}
        batch.update(target or {})
        kw = dict(self.loss_kwargs)
        kw.update(loss_kwargs)
        if self.recipe.masked:
            kw.update(embed_msk=True, mask=mask, step=self.global_step)
        loss_d = self.loss_fn(results, batch, **kw)
        if exposure is not None:
            unit = self._unit_exposure_rgb()
            loss_d['unit_exposure'] = 0.5 * (unit - self.recipe.unit_exposure_rgb) ** 2
        loss = sum(lo.mean() for lo in loss_d.values())
        if exposure is not None:
            # [loss, rgb, opacity, distortion, (the optional terms of loss_kwargs, in NeRFLoss's order,) unit_exposure]
            results['loss_terms'] = torch.stack([loss.detach()] + [lo.detach().mean() for lo in loss_d.values()])
        loss.backward()
        return loss

    def _adam_width_now(self, stream):
        """the sweep's launch width for this step; runs the measurement described in __init__ while it lasts"""
        if self.adam_width is not None:
            return self.adam_width
        start, rounds = self.adam_tune
        W, cands = self.update_interval, self.adam_candidates
        k = self.global_step - 1 - start          # (global_step was advanced already: 1-based here)
        n_win = rounds * len(cands)
        if k < 0:
            return cands[0]
        if not self._tune_events and k > 0:        # the start was missed (a resumed run): begin at the next window boundary
            self.adam_tune = (-(-(self.global_step - 1) // W) * W, rounds)
            return cands[0]
        if k % W == 0 and k // W <= n_win and len(self._tune_events) == k // W:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(stream)                      # window boundary: the same point of every step, on the optimizer stream
            self._tune_events.append(ev)
        if k < n_win * W:
            return cands[(k // W) % len(cands)]
        if len(self._tune_events) == n_win + 1 and self._tune_events[-1].query():
            ms = [a.elapsed_time(b) for a, b in zip(self._tune_events, self._tune_events[1:])]
            med = []
            for c in range(len(cands)):
                v = sorted(ms[c::len(cands)])
                med.append(0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2]))
            best = min(range(len(cands)), key=lambda c: med[c])
            # the default keeps its place unless another width is faster by more than the windows' own spread
            self.adam_width = cands[best] if med[best] < 0.99 * med[0] else cands[0]
            self.adam_tune_ms = dict(zip(cands, med))
            self._tune_events = []
            return self.adam_width
        return cands[0]

    def optimizer_step(self):
        """clip_grad_norm_(clip_norm) + Adam at the lr of the epoch this step belongs to (the scheduler ticks at epoch
        boundaries), behind the pose step where there is one"""
        self.global_step += 1
        lr = self.lr_at(min((self.global_step - 1) // self.steps_per_epoch, self.num_epochs))
        if self.pose_refiner is not None:
            self._pose_step()   # three small launches on the main stream, where the next step's rays read dR and dT
        if self.sharded:
            self._sharded_step(lr)
        else:
            self._sweep(lr)

    # ------------------------------------------------------------------ one GPU: clip + Adam as a sweep on the optimizer stream
    def _sweep(self, lr):
        """clip + Adam stream 6.4 GB and touch no ray data: they run on the optimizer stream behind everything the caller's
        stream holds, and the field waits on its link's `params_ready` / `rgb_params_ready` where it first reads the
        respective parameters (the ray-only front of the next step is on MarchAhead's stream anyway)."""
        side = self._opt_stream
        side.wait_stream(torch.cuda.current_stream())
        route = self._clip_route()
        with torch.cuda.stream(side):
            if route == "bound":
                self._clip_from_bound()
            else:
                self._clip_from_sum(early=route == "early")
            density_and_mlps, colour = self._adam_pieces(lr, side)
            if route == "bound":
                self._clear_accumulators_behind(side)
        self.model.link.params_ready, self.model.link.rgb_params_ready = density_and_mlps, colour

    def _clip_route(self):
        """which clip this optimizer step takes, from what _announce_backward armed and the backward left behind, all of
        which it disarms: 'bound' (the norm bound held on both tables: ngp_clip_decide_rest), 'early' (scalars[0] holds the
        colour table's share, summed from the encoder's hook) or 'full' (one sum over the whole gradient).  Launches nothing."""
        m, link = self.model, self.model.link
        early = self._norm_share_armed and self._norm_share_fired == 1
        self._norm_share_armed, self._norm_share_fired = False, 0
        bounded = bool(self._bound_step and link.hits == 2 and link.ok
                       and m.rgb_encoder._bound_valid and m.xyz_encoder._bound_valid)
        self._bound_step = False
        link.norm_acc = None
        return "bound" if bounded else "early" if early else "full"

    def _clip_from_bound(self):
        """the clip coefficient from the backward's norm bound and the MLP gradients' exact squares (three launches on
        the optimizer stream; the exact norm after all where the bound does not settle it, decided on the device)"""
        m, n, lo = self.model, self.layout.total, self._mlp_lo
        Kp = m.rgb_net.padded_in
        rgb_p, lin1, lin2 = m.rgb_net.params, m.xyz_net[0], m.xyz_net[2]
        # (the MLP gradients' exact sum of squares is formed by the same launch, into scalars[0])
        call("clip_decide_rest", self.norm_acc, rgb_p, 128 * Kp, rgb_p[128 * Kp:], rgb_p.numel() - 128 * Kp,
             lin1.weight, lin1.weight.numel(), lin2.weight, lin2.weight.numel(), self.flat_grad[lo:n], n - lo,
             self.scalars[0:1], float(self.clip_norm), 1.0, self.scalars[1:2], self.need_exact)
        # bound >= clip_norm (not seen in training): the exact norm after all, decided on the device
        call("sumsq_if", self.flat_grad[0:lo], lo, self.scalars[0:1], self.need_exact)
        call("clip_coef_if", self.scalars[0:1], float(self.clip_norm), 1.0, self.scalars[1:2], self.need_exact)

    def _clip_from_sum(self, early):
        """the clip coefficient from the exact sum of squares on the optimizer stream: what the early share left out
        (early) or the whole gradient; both accumulators are clear behind it"""
        n, b0 = self.layout.total, self.layout.b0
        if early:
            call("sumsq", self.flat_grad[b0:n], n - b0, self.scalars[0:1])
        else:
            self.scalars[0:1].zero_()
            call("sumsq", self.flat_grad, n, self.scalars[0:1])
        call("clip_coef", self.scalars[0:1], float(self.clip_norm), 1.0, self.scalars[1:2])
        self.scalars[0:1].zero_()   # ready for the next step's early share
        self.norm_acc.zero_()

    def _adam_pieces(self, lr, side):
        """Adam on the optimizer stream in two pieces, [density table | MLPs] first — the next forward starts on them —
        then the colour table, which the field does not read before its colour branch -> the event behind either piece"""
        n, b0 = self.layout.total, self.layout.b0
        events = {}
        width = self._adam_width_now(side)
        for lo, hi in ((b0, n), (0, b0)):
            if hi > lo:
                _adam("adam_step_width", self.flat_param[lo:hi], self.flat_grad[lo:hi], self.exp_avg[lo:hi],
                      self.exp_avg_sq[lo:hi], lr, self.global_step, self.scalars[1:2], 1, width)
            ev = torch.cuda.Event()
            ev.record(side)
            events[lo] = ev
        return events[b0], events[0]

    def _clear_accumulators_behind(self, side):
        """a bound step: scalars[0] and norm_acc are cleared behind the Adam launches, not before them, with an event
        on the link: the next backward adds into both and waits for it (networks._FieldFn.backward)"""
        self.scalars[0:1].zero_()
        self.norm_acc.zero_()
        ev = torch.cuda.Event()
        ev.record(side)
        self.model.link.acc_zeroed = ev

    # ------------------------------------------------------------------ N ranks: reduce-scatter, Adam on the slice, all-gather
    def _sharded_step(self, lr):
        """the sharded optimizer step: reduce-scatter, the shards' sums, clip and Adam on this rank's slices (caller's
        stream), all-gather; the fill that clears flat_grad runs beside them on the optimizer stream"""
        world = self.layout.world
        self.scalars.zero_()
        # sharded: bucket 0's reduce-scatter was issued from the colour encoder's backward
        nb = len(self.layout.bounds) - 1
        first = 1 if self.hooked0 else 0
        for i in range(first, nb):
            self.buckets.reduce_scatter_bucket(i, self.grad_shard[i])
        # global gradient norm = sqrt(sum over ranks of the shard sums).  Every shard is summed as soon as ITS
        # reduce-scatter has landed: the colour table's share (77 % of the entries) is read while the second bucket
        # is still on the wire (the one-GPU path's early norm share, kept in the sharded path).
        works = self.buckets.take_works()
        order = ([0] if self.hooked0 else []) + list(range(first, nb))
        assert len(works) == len(order)
        for w, i in zip(works, order):
            if w is not None:
                w.wait()
            g = self.grad_shard[i]
            call("sumsq", g, g.numel(), self.scalars[0:1])
        # all contributions are in the shard buffers now.  The scatter kernels add into flat_grad, so it has to be zero
        # again before the next backward: Adam clears only the rank's own 1/N (the shard buffers), the other (N-1)/N of
        # the accumulation buffer has no kernel that reads it on this rank — one 0.8 GB fill (0.15 ms of HBM writes) on
        # the optimizer stream, beside the norm / Adam of the slices and the all-gathers; the next backward joins it
        if self._opt_stream is not None:
            self._opt_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._opt_stream):
                self.flat_grad.zero_()
                self._grad_zeroed = torch.cuda.Event()
                self._grad_zeroed.record(self._opt_stream)
        else:
            self.flat_grad.zero_()
        dist.all_reduce(self.scalars[0:1], op=dist.ReduceOp.SUM, group=self.group)
        call("clip_coef", self.scalars[0:1], float(self.clip_norm), 1.0 / world, self.scalars[1:2])
        # per bucket: Adam on the slice, then publish it.  [density table | MLPs] first, the colour table
        # (77 % of the bytes) second; the field waits for each gather where it first reads those
        # parameters, so the small gather is in flight while the colour slice is still being updated and
        # the large one runs under the next step's marcher and density path
        works = {}
        for i in range(nb - 1, -1, -1):
            _adam("adam_step", self.param_shard[i], self.grad_shard[i], self.exp_avg[i], self.exp_avg_sq[i], lr,
                  self.global_step, self.scalars[1:2], 0)
            works[i] = self.buckets.all_gather_bucket(i, self.flat_param, self.param_shard[i], detach=True)
        self.model.link.params_ready, self.model.link.rgb_params_ready = works[nb - 1], (works[0] if nb == 2 else None)

    def wait(self):
        """make the current stream wait for a pending side-stream optimizer step (call before reading
        parameters / gradients outside the model's own forward)"""
        self._join_grad_zeroing()
        self.model.link.join_params()

    # ------------------------------------------------------------------ parameter store <-> shards
    def sync_shards(self):
        """Sharded optimizer only: the rank's master parameter slices (what Adam updates and the all-gather
        publishes) are re-read from the flat parameter buffer.  Call after ANY write into the model's
        parameters from outside the optimizer (checkpoint load, manual initialisation): otherwise the next
        all-gather overwrites those writes with the stale slices."""
        self.wait()
        if self.sharded:
            with torch.no_grad():
                for ps, (a, b) in zip(self.param_shard, self.shards):
                    ps.copy_(self.flat_param[a:b])

    def load_ckpt(self, ckpt_path, model_name='model', prefixes_to_ignore=()):
        """utils.load_ckpt into the trainer's flat parameter store (values are copied into the existing
        views, shapes are checked), followed by sync_shards()."""
        from .ckpt import load_ckpt
        self.wait()
        load_ckpt(self.model, ckpt_path, model_name, prefixes_to_ignore)
        self.sync_shards()

    # ------------------------------------------------------------------ multi-GPU helpers
    def broadcast_state(self, src=0):
        """start every rank from rank `src`'s parameters and occupancy grid (DDP does this at
        construction and re-broadcasts buffers every forward; train.py:431)"""
        if self.buckets.world == 1 and self.buckets.solo:
            return
        dist.broadcast(self.flat_param, src, group=self.group)
        self.sync_shards()
        for name in ("density_grid", "density_bitfield"):
            if hasattr(self.model, name):
                dist.broadcast(getattr(self.model, name), src, group=self.group)
