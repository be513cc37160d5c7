"""Which of NGPTrainer's options combine, what each needs from step() and which clip route its step takes: one table, read
by the constructor (resolve), by step() (Recipe.check_step, check_took_fused_tail, exact_norm) and by
tools/train_dataset.py's flag checks (conflicts).  Host only: nothing here launches.  A new option is one row of _OPTIONS
(and, for a term on the tail, one of _TAIL_TERMS) and a re-recorded tests/golden/recipe_matrix.json."""
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional, Tuple

import torch

from .rendering import MULTI_TERMS, TAIL_LAYOUT

_f32 = torch.float32


class _TailTerm(NamedTuple):
    """one of NeRFLoss's optional terms on the fused render + loss tail, as NGPTrainer sees it"""
    arg: str                 # step()'s argument that carries the term's target
    what: str
    bad: Callable            # (target, n_rays) -> what the target must do instead, None for a good one
    entry: Callable          # (trainer, target, device) -> the term's entry of FusedTail.terms
    classes: Tuple[int, int]   # num_classes the tail takes with this term (of several terms: the larger of either end)
    exact_norm: bool         # the term's head adds to the colour table's gradient, outside the norm bound


_TAIL_TERMS = {
    "semantic": _TailTerm(
        "labels", "the class of every ray",
        lambda x, n: None if x.numel() == n else f"hold {n} entries, one per ray: got {tuple(x.shape)}",
        lambda tr, x, dev: (x.view(-1).to(torch.int64), tr.loss_fn.lambda_semantic, tr.loss_fn.lambda_sky),
        (1, 16), True),
    "normal_mono": _TailTerm(
        "normals", "the target normal of every ray",
        lambda x, n: None if x.dim() == 2 and tuple(x.shape) == (n, 3) and x.is_floating_point()
        else f"be ({n}, 3) float: got {tuple(x.shape)} {x.dtype}",
        lambda tr, x, dev: (x.to(dev, _f32).contiguous(), tr.loss_fn.lambda_normal_mono),
        (0, 8), True),
    "depth_mono": _TailTerm(
        "depths", "the monocular depth of every ray",
        lambda x, n: None if tuple(x.shape) == (n,) and x.is_floating_point()
        else f"be ({n},) float: got {tuple(x.shape)} {x.dtype}",
        lambda tr, x, dev: (x.to(dev, _f32).contiguous(), tr.loss_fn.lambda_depth_mono, float(tr.model.scale)),
        (0, 8), False),
}
assert tuple(_TAIL_TERMS) == MULTI_TERMS

OPTIONAL_LOSS_TERMS = ("normal_ref", "normal_mono", "semantic", "depth_mono", "embed_msk")   # of loss_kwargs: the NeRFLoss module's


# name -> (label in a refusal, or a function that writes it; predicate).  g: resolve()'s arguments, `optional` (a term of
# OPTIONAL_LOSS_TERMS in loss_kwargs), `sharded`, and of the tail option in charge the terms it names (`named`), the classes
# the tail takes with them (`lo`..`hi`) and the width of the model's semantic head (`head`)
_CONDITIONS = {
    "msk_model": ("a msk_model", lambda g: g.msk_model is not None),
    "pose_refiner": ("a pose_refiner", lambda g: g.pose_refiner is not None),
    "skybox": ("a skybox", lambda g: g.render_kwargs.get("use_skybox") or getattr(g.model, "use_skybox", False)),
    "render_skybox": ("render_kwargs['use_skybox']", lambda g: g.render_kwargs.get("use_skybox")),
    "render_skybox_named": ("render_kwargs['use_skybox'] (the launch-per-operation route: name one of the two)",
                            lambda g: "use_skybox" in g.render_kwargs),
    "tone_mapped": ("rgb_act != 'Sigmoid'", lambda g: getattr(g.model, "rgb_act", "Sigmoid") != "Sigmoid"),
    "optional": ("an optional term in loss_kwargs", lambda g: g.optional),
    "diff_normals": ("differentiable normals", lambda g: getattr(g.model, "differentiable_normals", False)),
    "ranks": ("more than one rank", lambda g: g.sharded),
    "classes_range": (lambda g: f"num_classes = {g.num_classes} " + (f"outside {g.lo}..{g.hi}" if g.lo else f"above {g.hi}"),
                      lambda g: not g.lo <= int(g.num_classes) <= g.hi),
    "classes_head": (lambda g: f"a model with {g.head} classes for num_classes = {g.num_classes}",
                     lambda g: "semantic" in g.named and g.head != int(g.num_classes)),
}


class _Option(NamedTuple):
    name: str                # the Recipe's field (the constructor's argument; 'pose': a pose_refiner)
    head: str                # of its refusal; {asked} is the option as it was given
    refuses: Tuple[str, ...]   # other options and _CONDITIONS, in the order a refusal lists them
    notes: dict = {}         # refused name -> what the refusal adds in brackets
    message: Optional[str] = None   # the whole refusal, where it is a sentence of its own
    needs: Optional[Callable] = None   # (model) -> what is wrong with it, None for a model the option can train
    implies: Tuple[str, ...] = ()   # the conditions that hold for a model that passes `needs`
    tail: bool = False       # puts optional terms on the fused tail: one such option at a time, the last one given speaks
    # the step stays on the fused tail (no target=, no per-step loss term, CUDA only): (render()'s results, launch, what is lost)
    pins: Optional[Tuple[Tuple[str, ...], str, str]] = None
    exact_norm: bool = False   # the step takes the exact gradient norm (tail options: their terms say, _TAIL_TERMS)


_ON_TAIL = "{asked} runs on the fused render + loss tail, which does not take "
_TAIL = dict(head=_ON_TAIL, tail=True, pins=(("_loss_terms",), "", "the targets would be left out of the loss"),
             refuses=MULTI_TERMS + ("multi_terms", "msk_model", "pose_refiner", "skybox", "tone_mapped", "optional", "diff_normals",
                                    "classes_range", "classes_head"))

# In the order the constructor checks them.  Every option combines with embedding_a and random_bg; what else it combines
# with is what its row does not refuse.  Each term on the tail is also a flag of loss_kwargs, which with
# step(target={...}) remains the launch-per-operation route through the NeRFLoss module.
_OPTIONS = (
    # pose_refiner: a pose.PoseRefiner (the reference's --optimize_ext, train.py:143-149, 225-230).  step() takes img_idxs=
    # and pix_idxs= instead of ray tensors and forms the rays from the current dR, dT; the samples enter the field requiring
    # a gradient, which ngp_pose_rays_bwd reduces per image.  dR and dT live in a buffer of their own OUTSIDE the flat
    # store, as the reference keeps them out of net_opt: their own Adam at the constant `pose_lr` and their own clip at
    # clip_norm (Lightning clips per optimizer).  The norm bound is not shown to hold on the field's dL/dx route.
    _Option("pose", "", ("ranks",), exact_norm=True,
            message="pose refinement runs on one rank: a sharded trainer takes no pose_refiner"),
    # only the field's dL/dx and dL/dd feed the pose gradient; the Ro term (rendering._RefLossInputs returns no gradient for
    # dirs), a skybox (a function of rays_d) and second-order normals would leave it silently incomplete
    _Option("pose", "", ("optional", "render_skybox", "diff_normals"),
            message="pose refinement runs on the fused render + loss tail: a trainer with a pose_refiner takes no optional "
                    "loss term, no skybox and no differentiable normals"),
    # use_exposure: the reference's HDR-NeRF recipe (--use_exposure, train.py:99, 169-170, 301-306).  step() needs exposure=
    # (the exposure time of every ray), which reaches the three tone-mappers (ngp_tonemap_fwd / ngp_tonemap_bwd) through
    # render(), and the loss gains unit_exposure = 0.5 (tone(0, exposure=1) - unit_exposure_rgb)^2, its mean over the
    # channels; results['loss_terms'] holds [loss, rgb, opacity, distortion, unit_exposure] (on the NeRFLoss module's route
    # the optional terms' means sit between distortion and unit_exposure).  The term touches only the tone-mapper
    # parameters, whose squares are always summed exactly: the clip route is that of any tone-mapped model.
    _Option("use_exposure", "{asked} does not combine with ", ("msk_model", "pose_refiner", "skybox"),
            needs=lambda m: None if getattr(m, "rgb_act", "Sigmoid") == "None" else
            "use_exposure=True needs a model built with rgb_act='None' (log-radiance and the three tone-mappers): this one has "
            f"rgb_act={getattr(m, 'rgb_act', 'Sigmoid')!r}",
            implies=("tone_mapped",)),
    # semantic: the reference's render_semantic recipe (train.py:197, 293; losses.py:120-123) on ngp_render_loss_fused_sem.
    # step() needs labels= (n_rays) int64; a label outside [0, num_classes) is ignored (256, the reference's ignore_index,
    # and an 8-bit image's 255), and a batch without a valid label has a zero CE term where torch's cross-entropy gives NaN.
    _Option("semantic", **_TAIL),
    # normal_mono: losses.py:111-118 (the predicted-normal head against per-pixel normal maps) on ngp_render_loss_fused_nrm.
    # step() needs normals= (n_rays, 3) float; three exact zeros mark a ray without a normal (the divisor stays 3 n_rays).
    _Option("normal_mono", **_TAIL),
    # depth_mono: losses.py:7-30, 125-131 (composited depth against monocular depth up to the batch's least-squares scale and
    # shift) on ngp_render_loss_fused_dep (a fit kernel, then the tail).  step() needs depths= (n_rays) float, the raw depth
    # (z = depth / 25); zero, negative and NaN mark a ray without depth, which takes no part in the fit, the term or any
    # gradient (the mean stays over n_rays); the falloff's scene scale is the model's `scale`.  The term reaches the
    # parameters through d_sigmas alone, which the density head's backward notes: the norm bound holds.
    _Option("depth_mono", **_TAIL),
    # multi_terms: a non-empty subset of MULTI_TERMS TOGETHER on ngp_render_loss_fused_multi, as the reference's street-scene
    # recipes use them.  step() needs exactly the named terms' targets; results['loss_terms'] holds the 8 terms [loss, rgb,
    # opacity, distortion, CELoss, sky_depth, normal_mono, depth_mono].
    _Option("multi_terms", **_TAIL),
    # use_skybox: the reference's skybox recipe (--use_skybox, train.py:160): from global_step >= warmup_steps on the step
    # passes use_skybox to render(), the colours come from ngp_skybox_fwd (networks._SkyFn), the tail composites over them
    # per ray (ngp_render_loss_fused_sky) and hands the background's gradient to ngp_skybox_bwd, which adds straight into
    # the flat gradient.  Before that the step is the default recipe and the sky parameters get a zero gradient.  The
    # skybox takes precedence over random_bg.  It adds nothing to a table gradient and its own parameters lie where squares
    # are always summed exactly: the norm bound holds.  render_kwargs={'use_skybox': True} (without this flag) remains the
    # launch-per-operation route, from step 0.
    _Option("use_skybox", _ON_TAIL,
            MULTI_TERMS + ("multi_terms", "msk_model", "pose_refiner", "use_exposure", "tone_mapped", "optional", "diff_normals",
                           "render_skybox_named"),
            needs=lambda m: None if getattr(m, "use_skybox", False) else
            "use_skybox=True needs a model built with use_skybox=True (skybox_dir_encoder and skybox_rgb_net)",
            implies=("skybox",), pins=(("_loss_terms",), "", "the step would run without its skybox kernels")),
    # normal_ref: losses.py:107-109 (lambda_normal_ref_rp mean(Rp) + lambda_normal_ref_ro mean(Ro)).  The trainer sets
    # model.second_order_normals: the field hands out d(sigma)/dx with a graph, whose backward is the grid's double backward,
    # ngp_density_head_bwd2 and four existing products (networks._FieldFn); behind the tail ngp_normal_ref_tail forms both
    # terms and their gradients (rendering._NormalRefFn), seeded with `terms` in the step's one backward call.
    # results['loss_terms'] holds [loss, rgb, opacity, distortion, normal_ref_rp, normal_ref_ro], with multi_terms the two
    # behind the eight.  The norm bound is not shown to hold for the second-order contributions.
    # loss_kwargs={'normal_ref': True} remains the launch-per-operation route (differentiable normals).
    _Option("normal_ref", "{asked} runs on the fused field node and the fused render + loss tail, which do not take ",
            MULTI_TERMS + ("msk_model", "pose_refiner", "skybox", "use_exposure", "tone_mapped", "diff_normals", "optional", "ranks"),
            notes=dict({t: "name the term in multi_terms" for t in MULTI_TERMS},
                       diff_normals="the launch-per-operation route: name one of the two"),
            pins=(("_loss_terms", "_ref_terms"), " with its normal_ref launch", "the two terms would be left out of the loss"),
            exact_norm=True),
)


def _asked(name, value):
    return f"multi_terms={value}" if name == "multi_terms" else f"{name}=True"


@dataclass
class Recipe:
    """what resolve() decided; step() reads it.  The default is the default recipe of a trainer without options"""
    semantic: bool = False
    normal_mono: bool = False
    depth_mono: bool = False
    multi_terms: Tuple[str, ...] = ()
    use_exposure: bool = False
    unit_exposure_rgb: float = 0.5
    use_skybox: bool = False
    normal_ref: bool = False
    fused_loss: bool = True      # default recipe (rgb + opacity + distortion); False -> the NeRFLoss module
    masked: bool = False         # the trainer has a msk_model
    embed_a: bool = False        # ... an embedding_a
    pose: bool = False           # ... a pose_refiner
    tail_terms: Tuple[str, ...] = field(init=False, default=())   # the terms trained on the fused tail, in MULTI_TERMS' order
    packed: bool = field(init=False, default=False)   # they take one term's own entry
    asked: Optional[str] = field(init=False, default=None)   # the option that asked for them, as it was given

    def __post_init__(self):
        for name in ("multi_terms",) + MULTI_TERMS:
            if getattr(self, name):
                self.tail_terms = self.multi_terms if name == "multi_terms" else (name,)
                self.packed, self.asked = name != "multi_terms", _asked(name, self.multi_terms)
                break

    def _pinned(self):
        """(the option as it was given, its row) of every option that pins the step to the fused tail, in the table's order"""
        return [(self.asked if o.tail else _asked(o.name, True), o) for o in _OPTIONS if o.pins and getattr(self, o.name)]

    def exact_norm(self):
        """whether the step takes the exact gradient norm whatever the norm bound says"""
        return bool(any(o.exact_norm and getattr(self, o.name) for o in _OPTIONS)
                    or any(_TAIL_TERMS[t].exact_norm for t in self.tail_terms))

    def check_step(self, rays_o, rays_d, rgb_gt, next_rays=None, target=None, uvi=None, img_idxs=None, pix_idxs=None,
                   labels=None, normals=None, depths=None, exposure=None, loss_kwargs=None):
        """every check of step()'s arguments, before its first launch"""
        n = rgb_gt.shape[0]
        if self.masked and uvi is None:
            raise ValueError("this trainer has a msk_model: step() needs uvi= (implicit_mask.uvi of the ray batch)")
        if self.embed_a and img_idxs is None:
            raise ValueError("this trainer has an embedding_a: step() needs img_idxs= (the image index of every ray)")
        if self.use_exposure:
            if exposure is None:
                raise ValueError("this trainer was built with use_exposure=True: step() needs exposure= (the exposure time "
                                 "of every ray)")
            if not (torch.is_tensor(exposure) and exposure.is_floating_point() and exposure.numel() == n
                    and exposure.dim() in (1, 2)):
                raise ValueError(f"exposure= must be ({n},) or ({n}, 1) float: got "
                                 f"{tuple(exposure.shape) if torch.is_tensor(exposure) else type(exposure).__name__}")
            if not exposure.is_cuda:
                raise RuntimeError("exposure must be a CUDA tensor")
        elif exposure is not None:
            raise ValueError("exposure= is for a trainer built with use_exposure=True")
        given = {"labels": labels, "normals": normals, "depths": depths}
        for name, t in _TAIL_TERMS.items():
            if name in self.tail_terms:
                if given[t.arg] is None:
                    raise ValueError(f"this trainer was built with {self.asked}: step() needs {t.arg}= ({t.what})")
                why = t.bad(given[t.arg], n)
                if why:
                    raise ValueError(f"{t.arg}= must {why}")
            elif given[t.arg] is not None:
                raise ValueError(f"{t.arg}= is for a trainer built with {name}=True or with multi_terms naming '{name}'"
                                 + (f": this one has {self.asked}" if self.asked else ""))
        for asked, _ in self._pinned():
            if target or loss_kwargs:
                raise ValueError(f"this trainer was built with {asked}: the step stays on the fused render + loss tail and "
                                 "takes no target= and no per-step loss term")
            if not rays_o.is_cuda:
                raise RuntimeError(f"{asked} needs CUDA tensors: the fused tail has no other route")
        if self.pose:
            if rays_o is not None or rays_d is not None or next_rays is not None:
                raise ValueError("this trainer has a pose_refiner: step() forms the rays itself from img_idxs= and pix_idxs= "
                                 "(pass rays_o = rays_d = None and no next_rays: a march-ahead would use poses one update old)")
            if img_idxs is None or pix_idxs is None:
                raise ValueError("this trainer has a pose_refiner: step() needs img_idxs= and pix_idxs=")
            if target or loss_kwargs:
                raise ValueError("this trainer has a pose_refiner: the step stays on the fused render + loss tail and takes "
                                 "no target= and no per-step loss term")
        elif pix_idxs is not None:
            raise ValueError("pix_idxs= is for a trainer with a pose_refiner")

    def check_took_fused_tail(self, results, fused, sky_on):
        """behind render(): never a step without the kernels its options stand for (rgb_act or differentiable_normals
        changed after construction, a model without _field, ...).  fused: the FusedTail the step handed to render(), if any"""
        for asked, o in self._pinned():
            if o.name == "use_skybox" and not sky_on:
                continue
            keys, launch, lost = o.pins
            if (fused is None or any(k not in results for k in keys)
                    or (o.tail and results['_loss_terms'].numel() != TAIL_LAYOUT[fused.entry].n_terms)):
                raise RuntimeError(f"{asked}: render() did not take the fused tail{launch} (rendering._fused_tail_ok); {lost}")


def resolve(model, *, msk_model=None, embedding_a=None, pose_refiner=None, render_kwargs=None, loss_kwargs=None, num_classes=7,
            ranks=1, force_sharded=False, semantic=False, normal_mono=False, depth_mono=False, multi_terms=(),
            use_exposure=False, unit_exposure_rgb=0.5, use_skybox=False, normal_ref=False):
    """NGPTrainer's option arguments -> the Recipe, or the ValueError that says what does not combine.  Writes nothing"""
    optional = any((loss_kwargs or {}).get(k) for k in OPTIONAL_LOSS_TERMS)
    multi_terms = (multi_terms,) if isinstance(multi_terms, str) else tuple(multi_terms or ())
    bad_multi = [t for t in multi_terms if t not in MULTI_TERMS] or len(set(multi_terms)) != len(multi_terms)
    on = dict(pose=pose_refiner is not None, use_exposure=bool(use_exposure), semantic=bool(semantic),
              normal_mono=bool(normal_mono), depth_mono=bool(depth_mono),
              multi_terms=() if bad_multi else tuple(t for t in MULTI_TERMS if t in multi_terms),
              use_skybox=bool(use_skybox), normal_ref=bool(normal_ref))
    tail = [o.name for o in _OPTIONS if o.tail and on[o.name]]
    named = tuple(t for t in MULTI_TERMS if on[t] or t in on["multi_terms"])
    lo, hi = (max((_TAIL_TERMS[t].classes[k] for t in named), default=0) for k in (0, 1))
    g = SimpleNamespace(model=model, msk_model=msk_model, pose_refiner=pose_refiner, render_kwargs=render_kwargs or {},
                        optional=optional, num_classes=num_classes, sharded=ranks > 1 or force_sharded, named=named, lo=lo, hi=hi,
                        head=getattr(getattr(model, "semantic_header", None), "n_output_dims", None))
    for o in _OPTIONS:
        if o.tail and bad_multi:
            raise ValueError(f"multi_terms is a subset of {MULTI_TERMS} without repeats: got {multi_terms}")
        if not on[o.name] or (o.tail and o.name != tail[-1]):   # of the tail options the last one speaks, the others are refused
            continue
        wrong = o.needs and o.needs(model)
        if wrong:
            raise ValueError(wrong)
        why = []
        for r in o.refuses:
            if r in _CONDITIONS:
                label, bad = _CONDITIONS[r][0], _CONDITIONS[r][1](g)
                label = label(g) if callable(label) else label
            else:
                label, bad = _asked(r, on[r]), on[r] and r != o.name
            if bad:
                why.append(f"{label} ({o.notes[r]})" if r in o.notes else label)
        if why:
            raise ValueError(o.message or o.head.format(asked=_asked(o.name, on[o.name])) + ", ".join(why))
    return Recipe(fused_loss=not optional, masked=msk_model is not None, embed_a=embedding_a is not None,
                  unit_exposure_rgb=float(unit_exposure_rgb), **on)


def conflicts(option_names):
    """the pairs (option, what it refuses) among `option_names` (which may name the conditions 'msk_model' and 'pose_refiner'),
    whatever the model: a condition also counts where it holds for the model another option needs (`implies`)"""
    names = set(option_names)
    holds = {c: o.name for o in _OPTIONS if o.name in names for c in o.implies}
    return [(o.name, r if r in names else holds[r]) for o in _OPTIONS if o.name in names
            for r in o.refuses if r != o.name and (r in names or r in holds) and holds.get(r) != o.name]
