"""The one harness behind tests/test_{fused,semantic,normal,depth,multi}_tail_gpu.py: the six C entries of the fused
render + loss tail (render_loss_fused_kernel behind ngp_render_loss_fused and its _masked, _sem, _nrm, _dep and _multi
siblings) differ in a few arguments, a workspace and some bars, and ENTRIES states exactly that.  Everything else is here
once: the seeded batches and targets, the cached restatements, the direct call (run_entry), the comparer
(against_reference, with its bars in bars()) and the three route comparisons (fused route against the launch-per-operation
route, rendering._RenderLossFn against the direct call, the trainer's route against the module's).

The bars are stated by the test module that owns them (module docstrings); bars() restates them per entry, and does not
flatten the differences between the entries.  The structural checks (ownership, the sample counts, the workgroup counts,
exact zeros behind a stop, the background of empty rays, n_valid, the fit, +0 for a term that is not named) are applied to
every entry whose restatement states the property.  tests/test_tail_harness_host.py guards the comparer itself."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

import depth_tail_reference as DR
import fused_tail_reference as R
import multi_tail_reference as M
import normal_tail_reference as NR
import semantic_tail_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"          # (a CPU script that records the calls points this at "cpu")
FW_RTOL, FW_ATOL, BW_RTOL, BW_ATOL, NOISE_FACTOR = 2e-5, 2e-6, 2e-4, 2e-5, 8.0
REORDER = 2.0 ** -24          # relative change of a sum of n non-negative float32 terms under reordering: at most n * this
ULP = 2.0 ** -23              # two roundings of one double sum to float32
SEM, NRM, DEP = 1, 2, 4
PER_RAY = ("opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp")
PER_SAMPLE = ("ws", "d_sig", "d_rgb", "d_sem", "d_np")
INPUTS = ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3", "mask")
WRAPPER_OUTS = ("terms", "total", "vr", "opacity", "depth", "rgb", "normal", "sem", "ws", "Ro", "Rp")
DEFAULTS = dict(T_thr=1e-4, classes=7, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D, size_delta=0.0, lam_sem=SR.LAMBDA_SEM,
                lam_sky=SR.LAMBDA_SKY, lam_nm=NR.LAMBDA_NM, lam_dm=DR.LAMBDA_DM, scene_scale=1.0, use_bg=True, use_scale=False)

# The learning rate of the six-step trajectory comparisons of the normal, depth and multi tails is TRAJ_LR = 3e-4, not the
# 1e-2 of a training run.  Reason: six Adam steps are not a well-conditioned function of the gradients at 1e-2.  Adam's step
# is lr g / (|g| + eps) with eps = 1e-8; the colour table's gradient is summed with float atomics, whose order leaves about
# 3e-10 of absolute noise (1e-7 of the largest entry, 1.6e-3: measured as the module route against itself, and the same for
# the fused route against itself, also with every kernel serialised, so no race is involved), and for the table entries
# whose gradient is of the order of eps that noise moves the step by up to lr x 3e-10 / 1e-8 = 0.03 lr.  At lr = 1e-2 the
# SAME route run twice from the same seeds is 3e-4 apart in the table after two steps and 3e-5 to 1.7e-4 apart in
# rgb_net.params after three to six (module route against itself: 4.5e-5 after three steps) - at and beyond the atol of
# 5e-5, whatever the route under test does.  The effect is linear in lr: at 3e-4 it is a thirtieth, an order below the
# atol, while six steps still move the parameters by up to 1.8e-3, 36 times the atol, so a gradient that is wrong or missing
# still misses the bars.  Figures: profiles/normal_tail.txt.
TRAJ_LR = 3e-4


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------- the entries
def _f32(w):
    return w.view(np.float32).astype(np.float64)


def _nrm_counts(got, blocks, mask):
    if got["done"][0] != blocks:
        return f"workspace: {got['done'][0]} workgroups counted, {blocks} launched"


def _dep_counts(got, blocks, mask):
    if got["done"].tolist() != [blocks, blocks]:
        return f"workspace: {got['done'].tolist()} workgroups counted by the fit and the tail, {blocks} launched each"


def _multi_counts(got, blocks, mask):
    want = [blocks if (mask & SEM) else 0, blocks if (mask == NRM or mask == (NRM | DEP)) else 0, blocks if mask & DEP else 0,
            blocks if mask == DEP else 0]
    if got["counts"].tolist() != want:
        form = "one count for all terms" if bin(mask).count("1") > 1 else "single form"
        return f"workspace: counts {got['counts'].tolist()}, expected {want} ({form})"


# One row per C entry: what differs between the entries, and nothing else.
#   c          the entry's name behind ngp_
#   n_terms, vr_at, ws_at, ws_ints
#              the accumulator the runner lays out: terms at float 0, vr_samples (int64) at float vr_at, the workspace (int32)
#              at float ws_at (None: in an allocation of its own) - literal numbers, which rendering.TAIL_LAYOUT is held to
#   inputs     what the entry takes behind rgb_bg, outputs: behind dL_drgbs, both in call order (cfg names, targets, 'mask'
#              the per-ray transient mask of the batch, 'term_mask' the multi entry's bits; a target or an output of a term
#              that the multi entry's mask does not name is passed as None)
#   dense_logits  the logits are passed as (n, classes) contiguous, not as the leading columns of the batch's matrix
#   decode     workspace (int32 array) -> the entries of `got` read from it
#   counts     (got, workgroups launched, term mask) -> a message if the finished-workgroup counts are not those expected
#   n_valid    (name in the message, key of got, key of ref, bit)
#   finish, noise_of   the restatement: tests/{fused,semantic,normal,depth,multi}_tail_reference.py
#   classes    the class counts the entry takes
#   weights    cfg names of the weights of terms[4:], grads: (key, rule) in the order they are compared, see bars()
ENTRIES = {
    "default": dict(c="render_loss_fused", n_terms=4, vr_at=4, ws_at=None, ws_ints=0, inputs=(), outputs=(),
                    finish=lambda st, x, tg, classes, **kw: R.finish(st, x, **kw), noise_of=R.noise_of, classes=range(0, 9),
                    weights=(), term_floor="fw", grads=(("d_sig", "shared"), ("d_rgb", "shared"))),
    "masked": dict(c="render_loss_fused_masked", n_terms=5, vr_at=6, ws_at=None, ws_ints=0, inputs=("mask", "size_delta"),
                   outputs=("d_mask",),
                   finish=lambda st, x, tg, classes, **kw: R.finish(st, x, masked=True, **kw), noise_of=R.noise_of,
                   classes=range(0, 9), weights=("size_delta",), term_floor="fw",
                   grads=(("d_sig", "shared"), ("d_rgb", "shared"), ("d_mask", "one"))),
    "sem": dict(c="render_loss_fused_sem", n_terms=6, vr_at=6, ws_at=None, ws_ints=8, inputs=("labels", "lam_sem", "lam_sky"),
                outputs=("workspace", "d_sem"), dense_logits=True, decode=lambda w: dict(n_valid=w),
                n_valid=(("n_valid workspace", "n_valid", "n_valid", SEM),),
                finish=lambda st, x, tg, classes, **kw: SR.finish(st, x, tg["labels"], classes, **kw), noise_of=SR.noise_of,
                classes=range(1, 17), weights=("lam_sem", "lam_sky"), term_floor="bw",
                # d_sigmas carries the sky term: 8 x noise, floor 2e-5 / n_rays
                grads=(("d_rgb", "shared"), ("d_sig", "one"), ("d_sem", "lam_sem"))),
    "nrm": dict(c="render_loss_fused_nrm", n_terms=5, vr_at=6, ws_at=8, ws_ints=4, inputs=("normals", "lam_nm"),
                outputs=("workspace", "d_np"), decode=lambda w: dict(done=w[2:3].astype(np.int64)), counts=_nrm_counts,
                finish=lambda st, x, tg, classes, **kw: NR.finish(st, x, tg["normals"], **kw), noise_of=NR.noise_of,
                classes=range(0, 9), weights=("lam_nm",), term_floor="bw",
                grads=(("d_sig", "shared"), ("d_rgb", "shared"), ("d_np", "lam_nm"))),
    "dep": dict(c="render_loss_fused_dep", n_terms=5, vr_at=6, ws_at=8, ws_ints=18, inputs=("depths", "lam_dm", "scene_scale"),
                outputs=("workspace",),
                decode=lambda w: dict(fit=_f32(w[12:14]), n_valid=int(w[14]), done=w[15:17].astype(np.int64),
                                      sums=w[:12].view(np.float64)),
                counts=_dep_counts, n_valid=(("n_valid", "n_valid", "n_valid", DEP),), fit_prints_n_valid=True,
                finish=lambda st, x, tg, classes, **kw: DR.finish(st, x, tg["depths"], **kw), noise_of=DR.noise_of,
                classes=range(0, 9), weights=("lam_dm",), term_floor=None,
                # d_sigmas carries the depth term: 8 x noise, no floor
                grads=(("d_rgb", "shared"), ("d_sig", None))),
    "multi": dict(c="render_loss_fused_multi", n_terms=8, vr_at=8, ws_at=10, ws_ints=30,
                  inputs=("term_mask", "labels", "lam_sem", "lam_sky", "normals", "lam_nm", "depths", "lam_dm", "scene_scale"),
                  outputs=("workspace", "d_sem", "d_np"),
                  # counts: finished workgroups of sem / multi, nrm / multi, the fit, dep's tail
                  decode=lambda w: dict(n_valid_labels=int(w[0]), fit=_f32(w[24:26]), n_valid_depths=int(w[26]),
                                        counts=w[[6, 10, 27, 28]].astype(np.int64)),
                  counts=_multi_counts, n_valid=(("n_valid of the labels", "n_valid_labels", "n_valid_labels", SEM),
                                                 ("n_valid of the fit", "n_valid_depths", "n_valid_depths", DEP)),
                  finish=lambda st, x, tg, classes, mask, **kw: M.finish(st, x, M.MASKS[mask], tg, classes, **kw),
                  noise_of=M.noise_of, classes=range(0, 17), weights=("lam_sem", "lam_sky", "lam_nm", "lam_dm"), term_floor=None,
                  grads=(("d_rgb", "shared"), ("d_sig", None), ("d_sem", None), ("d_np", None))),
}
BIT = dict(labels=SEM, d_sem=SEM, normals=NRM, d_np=NRM, depths=DEP)          # the term_mask bit an input / output belongs to
TERM_BITS = ((4, SEM), (5, SEM), (6, NRM), (7, DEP))          # slot of the multi entry's terms -> the bit that names it


def named(entry, key, cfg):
    """whether the entry's call has this input / output (the multi entry: whether its mask names the term)"""
    return entry != "multi" or key not in BIT or bool(cfg.get("mask", 0) & BIT[key])


# ------------------------------------------------------------------------------------------------- fixtures
_BATCH, _TARGETS, _STATE, _REF = {}, {}, {}, {}


def _frozen(cache, key, make):
    if key not in cache:
        cache[key] = make()
        for v in cache[key].values() if isinstance(cache[key], dict) else [cache[key]]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return cache[key]


def batch(name, wide=False):
    """'crafted' or the random batch of int(name) rays, computed once, read-only; wide: with 16 logit columns, the first 8
    the batch's own (the semantic and multi entries)"""
    if wide:
        return _frozen(_BATCH, (name, True), lambda: SR.widen(batch(name)))
    return _frozen(_BATCH, (name, False), lambda: R.make_crafted(0) if name == "crafted" else R.make_random(int(name)))


def labels_for(name, classes, valid=True):
    """semantic_tail_reference.labels_for on the wide batch"""
    return _frozen(_TARGETS, ("labels", name, classes, valid), lambda: SR.labels_for(batch(name, True), classes, valid=valid))


def make_normals(name, kind="mixed"):
    """the batch's seeded normals: 'mixed' (a fifth of the rows zero) or 'none' (all zero)"""
    x = batch(name)
    return _frozen(_TARGETS, ("normals", name, kind),
                   lambda: NR.make_normals(x) if kind == "mixed" else np.zeros((x["n_rays"], 3), np.float32))


def make_depths(name, kind="mixed"):
    """the batch's seeded depths: 'mixed' (a fifth of the rows 0, negative or NaN), 'none', 'one'"""
    return _frozen(_TARGETS, ("depths", name, kind), lambda: DR.make_depths(batch(name), kind=kind))


def multi_targets(name, classes, T_thr=1e-4, labels="mixed", normals="mixed", depths="mixed"):
    """the multi entry's seeded labels, normals (drawn against the normals composited at T_thr) and depths"""
    x = batch(name, True)
    c = max(classes, 1)
    return dict(labels=_frozen(_TARGETS, ("m-labels", name, c, labels), lambda: M.make_labels(x, c, valid=labels == "mixed")),
                normals=_frozen(_TARGETS, ("m-normals", name, T_thr, normals), lambda: M.make_normals(x, kind=normals, T_thr=T_thr)),
                depths=_frozen(_TARGETS, ("m-depths", name, depths), lambda: M.make_depths(x, kind=depths)))


def reference(entry, name, targets=None, **cfg):
    """(float64 restatement, its float32 noise) of an entry on a batch, targets ({'labels', 'normals', 'depths'}: those the
    entry reads) and arguments: computed once, shared, read-only.  The per-ray part (render, in float64 and in float32 at
    the float64 stops) is shared between all entries and all losses that differ only in finish()'s arguments."""
    e, tg = ENTRIES[entry], targets or {}
    key = (entry, name) + tuple((k, v.tobytes()) for k, v in sorted(tg.items())) + tuple(sorted(cfg.items()))
    if key not in _REF:
        x = batch(name, True)
        rkw = {k: v for k, v in cfg.items() if k in R.RENDER_KEYS}
        fkw = {k: v for k, v in cfg.items() if k not in R.RENDER_KEYS}
        rkey = (name,) + tuple(sorted(rkw.items()))
        if rkey not in _STATE:
            hi = R.render(x, **rkw)
            _STATE[rkey] = (hi, R.render(x, dtype=torch.float32, stops=hi["stops"], **rkw))
        hi, lo = _STATE[rkey]
        classes = cfg.get("classes", 7)
        ref = e["finish"](hi, x, tg, classes, **fkw)
        _REF[key] = (ref, e["noise_of"](e["finish"](lo, x, tg, classes, **fkw), ref))
    return _REF[key]


# ------------------------------------------------------------------------------------------------- the direct call
def run_entry(ngp, entry, x, targets=None, n_rays=None, ld=None, adjacent=True, garbage=-5, twice=False, **cfg):
    """one direct call of the C entry on the first n_rays rows (default: all).  Every output is pre-filled with NaN,
    total_samples with -7, vr_samples with -(2^40) - 3 (NaN bits where it lies in the accumulator), the workspace with
    `garbage`; per-ray buffers have one entry per ray of the batch.  adjacent: terms, vr_samples and the workspace in one
    buffer as rendering._RenderLossFn lays them out (one fill), else in separate allocations.  ld: the two heads as the
    leading columns of ld-wide matrices whose other columns hold NaN.  twice: a second call on the same buffers must leave
    every per-ray and per-sample output as the first did, bit for bit."""
    e, tg = ENTRIES[entry], targets or {}
    c = dict(DEFAULTS, **cfg)
    classes = int(c["classes"])
    rows = len(x["rays_a"]) if n_rays is None else n_rays
    NR_, n = x["n_rays"], x["n"]
    t = {k: T(x[k]) for k in INPUTS}
    nrm, sem = t["nrm"], t["sem"][:, :classes].contiguous() if e.get("dense_logits") else t["sem"]
    if ld is not None:
        wide = torch.full((2, n, ld), float("nan"), device=DEV)
        wide[0, :, :3], wide[1, :, :sem.shape[1]] = nrm, sem
        nrm, sem = wide[0], wide[1]
    E = lambda *s: torch.full(s, float("nan"), device=DEV)
    total = torch.full((NR_,), -7, dtype=torch.int64, device=DEV)
    n_terms, vr_at, ws_at, ws_ints = e["n_terms"], e["vr_at"], e["ws_at"], e["ws_ints"]
    ws_ = None
    if adjacent:
        acc = E(8 if ws_at is None else ws_at + ws_ints)
        terms, vr = acc[:n_terms], acc[vr_at:vr_at + 2].view(torch.int64)
        if ws_at is not None:
            ws_ = acc[ws_at:].view(torch.int32)
    else:
        terms, vr = E(n_terms), torch.full((1,), -(2 ** 40) - 3, dtype=torch.int64, device=DEV)
        assert vr.data_ptr() != terms.data_ptr() + 4 * vr_at
    if ws_ints and ws_ is None:
        ws_ = torch.zeros(ws_ints, dtype=torch.int32, device=DEV)
        assert ws_at is None or ws_.data_ptr() != terms.data_ptr() + 4 * ws_at
    if ws_ is not None:
        ws_.fill_(garbage)
    o = dict(opacity=E(NR_), depth=E(NR_), rgb=E(NR_, 3), normal=E(NR_, 3), sem=E(NR_, classes), ws=E(n), Ro=E(NR_),
             Rp=E(NR_, 3), terms=terms, d_sig=E(n), d_rgb=E(n, 3))
    shape = dict(d_mask=(NR_,), d_sem=(n, classes), d_np=(n, 3))
    o.update({k: E(*shape[k]) for k in e["outputs"] if k != "workspace" and named(entry, k, c)})

    def arg(k):
        if k == "term_mask":
            return int(c["mask"])
        if k == "mask":
            return t["mask"]
        if k in ("labels", "normals", "depths"):
            return T(tg[k]) if named(entry, k, c) else None
        return float(c[k])
    args = (t["sig"], t["rgbs"], t["dsig"], t["scale3"] if c["use_scale"] else None, nrm, nrm.stride(0), sem, sem.stride(0),
            t["dirs"], t["deltas"], t["ts"], t["rays_a"], t["gt"], t["bg"] if c["use_bg"] else None, *map(arg, e["inputs"]),
            float(c["T_thr"]), classes, rows, float(c["lam_o"]), float(c["lam_d"]), total, vr, o["opacity"], o["depth"], o["rgb"],
            o["normal"], o["sem"], o["ws"], o["Ro"], o["Rp"], o["terms"], o["d_sig"], o["d_rgb"],
            *(ws_ if k == "workspace" else o.get(k) for k in e["outputs"]))

    def call():
        ngp._lib.call(e["c"], *args)
        if DEV == "cuda":
            torch.cuda.synchronize()
    call()
    o["total"], o["vr"] = total, vr
    out = {k: N(v).copy() for k, v in o.items()}
    if twice:
        call()
        for k, v in o.items():
            if k != "terms":
                assert np.array_equal(N(v), out[k], equal_nan=v.dtype.is_floating_point), f"second call: {k}"
        np.testing.assert_allclose(N(o["terms"]), out["terms"], rtol=(rows // 8 + 1) * REORDER, atol=0)
    if "decode" in e:
        out.update(e["decode"](N(ws_).copy()))
    return out


# ------------------------------------------------------------------------------------------------- the comparer
def where(x, key, item, n_rays=None):
    """'ray 5 (row 2, case (65, 63))[, sample 64 of the segment]' of an entry of a per-ray or per-sample output"""
    rows = x["rays_a"][:n_rays]
    if key in PER_SAMPLE:
        row, k = R.owned(x, n_rays)
        if row[item] < 0:
            return f"sample {item}, owned by no ray"
        return f"ray {rows[row[item], 0]} (row {row[item]}, case {x['cases'][row[item]]}), sample {k[item]} of the segment"
    hit = np.nonzero(rows[:, 0] == item)[0]
    return f"ray {item} (row {hit[0]}, case {x['cases'][hit[0]]})" if len(hit) else f"ray {item}, in no row"


def bars(entry, ref, noise, n_rows, cfg):
    """{key: bar, of the shape of ref[key]} in the order the comparer reports them: the per-ray and per-sample outputs, the
    fit where the entry has one, the terms.  The rules (the owning modules' docstrings):
      opacity, depth, rgb, normal, sem, ws    FW_ATOL + FW_RTOL |ref|
      Ro, Rp                                  max(8 x noise, FW_ATOL)
      a gradient, by its rule in ENTRIES      'shared': BW_ATOL / n_rays + BW_RTOL |ref|; None: 8 x noise; 'one' or the cfg
                                              name of a weight: max(8 x noise, BW_ATOL / n_rays x that weight)
      fit                                     8 x noise
      terms[0:4]                              max(8 x noise, FW_ATOL x the term's weight (1, 1, lambda_o, lambda_d))
      terms[4:], by term_floor in ENTRIES     'fw': the same with the weight of ENTRIES' `weights`; 'bw': max(8 x noise,
                                              BW_ATOL / n_rays x that weight); None: 8 x noise"""
    e = ENTRIES[entry]
    c = dict(DEFAULTS, one=1.0, **cfg)
    out = {key: FW_ATOL + FW_RTOL * np.abs(ref[key]) for key in ("opacity", "depth", "rgb", "normal", "sem", "ws")}
    for key in ("Ro", "Rp"):
        out[key] = max(NOISE_FACTOR * noise[key], FW_ATOL)
    for key, rule in e["grads"]:
        if key not in ref or not named(entry, key, c):
            continue
        if rule == "shared":
            out[key] = BW_ATOL / n_rows + BW_RTOL * np.abs(ref[key])
        else:
            out[key] = NOISE_FACTOR * noise[key] if rule is None else max(NOISE_FACTOR * noise[key], BW_ATOL / n_rows * c[rule])
    if "fit" in ref:
        out["fit"] = NOISE_FACTOR * noise["fit"]
    weights = np.array([1.0, 1.0, c["lam_o"], c["lam_d"]] + [c[k] for k in e["weights"]])
    t = NOISE_FACTOR * noise["terms"]
    t[:4] = np.maximum(t[:4], FW_ATOL * weights[:4])
    if e["term_floor"] is not None:
        t[4:] = np.maximum(t[4:], (FW_ATOL if e["term_floor"] == "fw" else BW_ATOL / n_rows) * weights[4:])
    out["terms"] = t
    return {k: np.broadcast_to(v, np.shape(ref[k])) if k != "terms" else v for k, v in out.items()}


def against_reference(entry, tag, got, ref, noise, x, cfg, ray_ok=None, smp_ok=None):
    """every output of one call against the restatement.  ray_ok / smp_ok: the rays / samples that are compared (default:
    all that a processed row owns).  Prints each figure, then fails with the list of outputs that miss."""
    e = ENTRIES[entry]
    n_rays, mask = cfg.get("n_rays"), cfg.get("mask", 0)
    rows = x["rays_a"][:n_rays]
    n_rows = len(rows)
    ray_own = np.zeros(x["n_rays"], bool)
    ray_own[rows[:, 0]] = True
    row_of, k_of = R.owned(x, n_rays)
    smp_own = row_of >= 0
    ray_ok = ray_own if ray_ok is None else ray_ok & ray_own
    smp_ok = smp_own if smp_ok is None else smp_ok & smp_own
    everything = ray_ok.sum() == n_rows
    per_ray = [k for k in PER_RAY + ("d_mask",) if k in got]
    per_sample = [k for k in PER_SAMPLE if k in got]
    bar = bars(entry, ref, noise, n_rows, cfg)
    misses = []

    def held(key, sel):
        g, w, b = got[key].astype(np.float64), ref[key], bar[key]
        if g.size == 0:
            return
        scale = n_rows if key.startswith("d_") else 1.0
        width = g.size // len(g)
        sel = np.broadcast_to(sel.reshape(sel.shape + (1,) * (g.ndim - 1)), g.shape)
        err = np.where(sel, np.nan_to_num(np.abs(g - w), nan=np.inf), 0.0)          # (a NaN misses)
        ratio = np.where(sel, err / np.maximum(np.nan_to_num(b), 1e-300), 0.0)
        worst = int(np.argmax(ratio))
        print(f"FIG {tag} {key}: max|err| {scale * err.max():.3g}" + (f" (times n_rays = {scale})" if scale != 1 else "") +
              f", worst err/bar {ratio.ravel()[worst]:.3g}")
        bad = sel & ~(err <= b)
        if bad.any():
            misses.append(f"{key}: {bad.sum()} of {sel.sum()} miss; worst at {where(x, key, worst // width, n_rays)}: got "
                          f"{g.ravel()[worst]!r}, reference {w.ravel()[worst]!r}, bar {b.ravel()[worst]:.3g}")

    # exact: the counts of the workspace and of the samples
    note = e["counts"](got, (n_rows + 7) // 8, mask) if "counts" in e else None
    if note:
        misses.append(note)
    for what, gk, rk, bit in e.get("n_valid", ()):
        if named(entry, {SEM: "labels", DEP: "depths"}[bit], cfg) and np.ravel(got[gk])[0] != ref[rk]:
            misses.append(f"{what}: got {np.ravel(got[gk])[0]}, reference {ref[rk]}")
    if not np.array_equal(got["total"][ray_ok], ref["total"][ray_ok]):
        i = int(np.nonzero(ray_ok & (got["total"] != ref["total"]))[0][0])
        misses.append(f"total_samples: {where(x, 'total', i, n_rays)}: got {got['total'][i]}, reference {ref['total'][i]}")
    if got["vr"][0] != got["total"][ray_own].sum() or (everything and got["vr"][0] != ref["vr"][0]):
        misses.append(f"vr_samples: got {got['vr'][0]}, sum of total_samples {got['total'][ray_own].sum()}, reference {ref['vr'][0]}")
    # what no processed row owns (the gap, the other rows' rays) is left alone
    for key in per_ray + per_sample:
        if not np.isnan(got[key][~(smp_own if key in PER_SAMPLE else ray_own)]).all():
            misses.append(f"{key}: entries that no processed row owns were written")
    if not (got["total"][~ray_own] == -7).all():
        misses.append("total_samples: entries that no processed row owns were written")
    # everything behind a stop is exactly 0
    stop = ref["stops"][np.maximum(row_of, 0)]
    behind = smp_ok & (stop >= 0) & (k_of > stop)
    for key in per_sample:
        if got[key][behind].any() or np.isnan(got[key][behind]).any():
            i = int(np.nonzero(behind)[0][0])
            misses.append(f"{key}: not exactly 0 behind a stop, e.g. {where(x, 'ws', i, n_rays)}")
    if "d_np" in got and "has" in ref:          # nor has a sample without weight, or on a ray without a target, a gradient
        dead = smp_ok & ((np.nan_to_num(ref["ws"]) == 0) | ~ref["has"][np.maximum(row_of, 0)])
        if got["d_np"][dead].any() or np.isnan(got["d_np"][dead]).any():
            misses.append(f"d_np: {int((got['d_np'][dead] != 0).any(1).sum())} samples without weight or target are not exactly 0")
    # rays without samples give the background (black without one)
    empty = ray_own.copy()
    empty[rows[:, 0]] = rows[:, 2] == 0
    want_bg = x["bg"].astype(np.float32) if cfg.get("use_bg", True) else np.zeros(3, np.float32)
    if empty.any() and not (
            np.array_equal(got["rgb"][empty], np.broadcast_to(want_bg, got["rgb"][empty].shape))
            and not got["opacity"][empty].any() and not got["depth"][empty].any()):
        misses.append("rays without samples: not the background with zero opacity and depth")
    # the bars
    for key in bar:
        if key in per_ray or key in per_sample:
            held(key, smp_ok if key in PER_SAMPLE else ray_ok)
    if "fit" in bar and everything:              # (a, b) depend on every row: compared when no row is borderline
        print(f"FIG {tag} fit: got {got['fit']}, |err| {np.abs(got['fit'] - ref['fit'])}, bars {bar['fit']}" +
              (f", n_valid {got['n_valid']}" if e.get("fit_prints_n_valid") else ""))
        for i, nm in enumerate("ab"):
            if not abs(got["fit"][i] - ref["fit"][i]) <= bar["fit"][i]:
                misses.append(f"fit {nm}: got {got['fit'][i]!r}, reference {ref['fit'][i]!r}, bar {bar['fit'][i]:.3g}")
    n_terms = e["n_terms"]
    assert got["terms"].shape == (n_terms,) == ref["terms"].shape
    print(f"FIG {tag} terms: got {got['terms']}, |err| {np.abs(got['terms'] - ref['terms'])}, bars {bar['terms']}")
    for i in range(n_terms):
        if not abs(float(got["terms"][i]) - ref["terms"][i]) <= bar["terms"][i]:
            misses.append(f"terms[{i}]: got {got['terms'][i]!r}, reference {ref['terms'][i]!r}, bar {bar['terms'][i]:.3g}")
    for i, bit in TERM_BITS if entry == "multi" else ():
        if not mask & bit and not (got["terms"][i] == 0 and not np.signbit(got["terms"][i])):
            misses.append(f"terms[{i}]: {got['terms'][i]!r} for a term that is not named")
    print(f"FIG {tag} float32 noise of the restatement: " + ", ".join(f"{k} {np.max(v):.3g}" for k, v in noise.items()))
    assert not misses, f"{tag}:\n  " + "\n  ".join(misses)


def _same_launch(a, b, n_blocks, keys=None):
    """two launches that must agree bit for bit (NaN where nothing was written included), except for the loss terms when
    more than one workgroup adds to them: float atomics in arrival order, at most n_blocks * 2^-24 relative apart"""
    for k in keys or [k for k in a if k != "terms"]:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    if n_blocks == 1:
        assert np.array_equal(a["terms"], b["terms"])
    else:
        np.testing.assert_allclose(a["terms"], b["terms"], rtol=n_blocks * REORDER, atol=0)


SHARED = ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "ws", "d_sig", "d_rgb")


def same_as_default(ngp, entry, x, targets, zero, n_rays=None):
    """the entry with its weights `zero` (a dict of zeros) against ngp_render_loss_fused on the same rows: every shared output
    bit for bit; the four shared terms bit for bit when one workgroup forms them, else within the reordering of one float
    atomic per workgroup.  -> the entry's outputs"""
    blocks = len(x["rays_a"]) // 8 + 1 if n_rays is None else (n_rays + 7) // 8
    a = run_entry(ngp, entry, x, targets, n_rays=n_rays, **zero)
    b = run_entry(ngp, "default", x, n_rays=n_rays)
    for key in SHARED:
        assert np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (key, n_rays)
    if blocks == 1:
        assert np.array_equal(a["terms"][:4], b["terms"])
    else:
        np.testing.assert_allclose(a["terms"][:4], b["terms"], rtol=blocks * REORDER, atol=0)
    return a


# ------------------------------------------------------------------------------------------------- the routes
def _close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _grid_buffers(model):
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    return model


def _scene_labels(scene, o, d, classes, gen):
    """the scene's labels (0-4, 256), with a fifth of the rays spread over all `classes`: valid labels or 256 only"""
    lab = scene.ground_truth_labels(o, d, n_quad=64)
    rnd = torch.randint(classes, lab.shape, device=DEV, generator=gen)
    lab = torch.where(torch.rand(lab.shape, device=DEV, generator=gen) < 0.2, rnd, lab)
    assert bool(((lab >= 0) & (lab < classes) | (lab == 256)).all())
    return lab


def _nonzero_normals(scene, o, d, gen):
    """the scene's normals where it has one, a random direction elsewhere, lengths 0.3 to 5: every target non-zero, which
    is where the entry and NeRFLoss._normal_mono state the same loss"""
    nrm = scene.ground_truth_normals(o, d, n_quad=64)
    rnd = torch.nn.functional.normalize(torch.randn(nrm.shape, device=DEV, generator=gen), dim=-1)
    nrm = torch.where((nrm != 0).any(-1, keepdim=True), nrm, rnd)
    nrm = nrm * (0.3 + 4.7 * torch.rand(len(nrm), 1, device=DEV, generator=gen))
    assert bool((nrm != 0).any(-1).all())
    return nrm.contiguous()


def _mono_depths(scene, o, d):
    """the scene's depths as a monocular map: 25 (0.37 D + 0.11) where the ray has one, 0 (invalid) elsewhere; no NaN, which
    the module route would carry into its loss"""
    D = scene.ground_truth_depths(o, d, n_quad=64)
    dep = torch.where(D > 0, 25.0 * (0.37 * D + 0.11), torch.zeros_like(D))
    assert 0.02 < float((dep > 0).float().mean()) < 0.98
    return dep.contiguous()


# per optional term: the key of NeRFLoss's target and of NGPTrainer.step's keyword, and the names of its losses
TERMS = {"semantic": ("label", "labels", ("CELoss", "sky_depth")), "normal_mono": ("normal", "normals", ("normal_mono",)),
         "depth_mono": ("depth", "depths", ("depth_mono",))}


def _scene_targets(scene, o, d, classes, gen, terms=tuple(TERMS)):
    """{term: its target on these rays}, drawn from `gen` in the order of TERMS"""
    make = {"semantic": lambda: _scene_labels(scene, o, d, classes, gen), "normal_mono": lambda: _nonzero_normals(scene, o, d, gen),
            "depth_mono": lambda: _mono_depths(scene, o, d)}
    return {k: make[k]() for k in TERMS if k in terms}


def fused_against_layered(ngp, terms, classes=None, packed=True):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background draw
    on both routes.  A: render + NeRFLoss with the named terms + sum of means + autograd; B: render with
    _fused_loss=FusedTail(gt, lambda_o, lambda_d, terms={...}, packed=packed) through rendering._RenderLossFn.  The outputs
    rtol 2e-5 / atol 2e-6, the terms rtol 1e-4, the parameter gradients within 3e-4 of the largest entry
    (tests/test_mask_gpu.py's tolerances for its masked-tail-against-layered comparison).  -> (terms of B, parameter
    gradients of B, the targets)"""
    from ngp_amd.losses import NeRFLoss
    from ngp_amd.rendering import FusedTail, render
    from ngp_amd.synthetic import LegoProxy
    torch.manual_seed(33)
    model = _grid_buffers(ngp.networks.NGP(scale=8.0, **({} if classes is None else {"classes": classes})).to(DEV))
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.5)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    scene = LegoProxy(n_images=6, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(34)
    img, pix = scene.sample_batch(1500, generator=gen)
    o, d = scene.rays(img, pix)
    gt = torch.rand(1500, 3, device=DEV, generator=gen)
    tg = _scene_targets(scene, o, d, classes, gen, terms)
    f = NeRFLoss()
    lam = {"semantic": (f.lambda_semantic, f.lambda_sky), "normal_mono": (f.lambda_normal_mono,),
           "depth_mono": (f.lambda_depth_mono, 8.0)}
    names = ["rgb", "opacity", "distortion"] + [n for k in TERMS if k in terms for n in TERMS[k][2]]
    n_terms = len(names) + 1 if packed else 8
    named_p = [(n, p) for n, p in model.named_parameters() if p.numel() > 0]
    out = {}
    for fused in (False, True):
        for _, p in named_p:
            p.grad = None
        torch.manual_seed(35)
        kw = dict(exp_step_factor=1 / 256, random_bg=True, **({} if classes is None else {"num_classes": classes}))
        if fused:
            tail = FusedTail(gt, f.lambda_opa, f.lambda_distortion, terms={k: (tg[k],) + lam[k] for k in tg}, packed=packed)
            res = render(model, o, d, _fused_loss=tail, **kw)
            assert "_loss_terms" in res
            t = res.pop("_loss_terms")
            assert t.shape == (n_terms,) and t.requires_grad
            torch.autograd.backward([t], [torch.tensor([1.0] + [0] * (n_terms - 1), device=DEV)])
            t = N(t)
        else:
            res = render(model, o, d, **kw)
            ld = f(res, dict({TERMS[k][0]: v for k, v in tg.items()}, rgb=gt), **{k: True for k in tg},
                   **({"scale": 8.0} if "depth_mono" in tg else {}))
            loss = sum(v.mean() for v in ld.values())
            loss.backward()
            # (the module's normal_mono entry is (R, 3): its mean is the entry's term)
            t = np.array([float(loss.detach())] + [float(ld[n].detach().mean()) for n in names], np.float32)
        out[fused] = (res, t, {n: None if p.grad is None else N(p.grad).copy() for n, p in named_p})
    ra, ta, ga = out[False]
    rb, tb, gb = out[True]
    assert int(ra["total_samples"]) == int(rb["total_samples"]) > 0
    for key in ("opacity", "depth", "rgb", "normal_pred", "semantic", "ws", "Ro", "Rp"):
        _close(N(rb[key]), N(ra[key]), 2e-5, 2e-6)
    print("FIG autograd terms A", ta, "terms B", tb)
    _close(tb, ta, 1e-4, 1e-9)
    for name in ga:
        a, b = ga[name], gb[name]
        if a is None:
            assert b is None or not b.any(), name
            continue
        scale = np.abs(a).max()
        print(f"FIG autograd grad {name}: max|a - b| / max|a| = {np.abs(a - b).max() / max(scale, 1e-300):.3g}")
        assert np.abs(a - b).max() <= 3e-4 * scale + 1e-12, (name, np.abs(a - b).max(), scale)
    for name in ("rgb_encoder.params", "xyz_encoder.params"):
        assert np.abs(gb[name]).sum() > 0, name
    return tb, gb, tg


def wrapper_against_direct(ngp, entry, x, targets, make_tail, opt_rtol=4 * REORDER, **cfg):
    """rendering._RenderLossFn on a batch with sigmas, rgbs, the logits and the normal head as leaves, and the tail that
    make_tail(t, mask leaf) builds from the device inputs t: the outputs are those of the direct call bit for bit, the terms
    within the reordering of four workgroups' atomics (terms[4:]: opt_rtol), and back-propagating terms[0] with a unit seed
    hands back the launch's gradients bit for bit - d_sigmas within 1e-6 where the fit's (a, b), sums of doubles in arrival
    order, came out an ulp apart; a head whose term is not named gets no gradient.  -> (direct, outs, t, args), args the
    wrapper's first ten arguments"""
    from ngp_amd.rendering import _RenderLossFn
    e, classes = ENTRIES[entry], cfg.get("classes", 7)
    direct = run_entry(ngp, entry, x, targets, **cfg)
    t = {k: T(x[k]) for k in INPUTS}
    t.update({k: T(v) for k, v in (targets or {}).items()})
    if e.get("dense_logits"):
        t["sem"] = t["sem"][:, :classes].contiguous()
    sig, rgbs, sem, nrm = leaves = [t[k].requires_grad_(True) for k in ("sig", "rgbs", "sem", "nrm")]
    mask = t["mask"][:, None].requires_grad_(True)
    tail = make_tail(t, mask)
    assert tail.entry == entry
    args = (*leaves, tail.mask, t["dsig"], t["dirs"], t["deltas"], t["ts"], t["rays_a"])
    outs = _RenderLossFn.apply(*args, tail, t["scale3"], 1e-4, classes, t["bg"])
    terms = outs[0]
    assert terms.shape == (e["n_terms"],) and terms.requires_grad and not any(o.requires_grad for o in outs[1:] if o is not None)
    assert e["ws_ints"] or outs[11] is None
    seed = torch.zeros_like(terms)
    seed[0] = 1.0
    torch.autograd.backward([terms], [seed])
    own = R.owned(x)[0] >= 0
    got = dict(zip(WRAPPER_OUTS, (N(o) for o in outs)))
    assert got["vr"].shape == (1,) and got["vr"].dtype == np.int64
    for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp"):
        assert np.array_equal(got[k], direct[k]), k
    assert np.array_equal(got["ws"][own], direct["ws"][own])
    np.testing.assert_allclose(got["terms"][:4], direct["terms"][:4], rtol=4 * REORDER, atol=0)
    np.testing.assert_allclose(got["terms"][4:], direct["terms"][4:], rtol=opt_rtol, atol=0)
    fit = e["decode"](N(outs[11]))["fit"] if "fit" in direct else None
    if fit is None or np.array_equal(fit, direct["fit"]):          # the same (a, b): the same gradients bit for bit
        assert np.array_equal(N(sig.grad)[own], direct["d_sig"][own])
    else:
        np.testing.assert_allclose(fit, direct["fit"], rtol=ULP, atol=0)
        np.testing.assert_allclose(N(sig.grad)[own], direct["d_sig"][own], rtol=1e-6, atol=1e-12)
    assert np.array_equal(N(rgbs.grad)[own], direct["d_rgb"][own])
    for leaf, key, width in ((sem, "d_sem", classes), (nrm, "d_np", 3)):          # padded with zeros to the input's width
        if key in direct:
            g = N(leaf.grad)
            assert g.shape == tuple(leaf.shape) and np.array_equal(g[own, :width], direct[key][own]) and not g[:, width:].any()
        else:
            assert leaf.grad is None, key
    if "d_mask" in direct:
        assert mask.grad.shape == (x["n_rays"], 1) and np.array_equal(N(mask.grad)[:, 0], direct["d_mask"])
    return direct, outs, t, args


def trainer_against_module(ngp, terms, fused_kw, lr, tracked, after_step=None):
    """NGPTrainer(**fused_kw) with step(labels= / normals= / depths=) against NGPTrainer(loss_kwargs={the named terms[,
    'scale': 0.5]}) with step(target={...}) for six steps of 1024 rays of the proxy scene (labels in range or 256, every
    normal non-zero, depths without NaN) from the same seeds: losses rtol 1e-3, xyz_net[0].weight, rgb_net.params and the
    `tracked` parameters rtol 5e-3 / atol 5e-5 (the construction and bars of
    test_trainer_fused_loss_path_matches_module_path).  after_step(model) runs behind every step of the fused route.
    -> {fused: dict(tr=, steps=, start=, end=)}, start / end the tracked parameters before and after"""
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=10, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(51)
    batches = []
    for i in range(6):
        img, pix = scene.sample_batch(1024, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        batches.append((o, d, gt, _scene_targets(scene, o, d, 7, gen, terms)))
    module_kw = dict({k: True for k in terms}, **({"scale": 0.5} if "depth_mono" in terms else {}))
    params = lambda model: [N(model.xyz_net[0].weight).copy(), N(model.rgb_net.params).copy()] + \
        [N(model.get_parameter(name)).copy() for name in tracked]
    runs = {}
    for fused in (True, False):
        torch.manual_seed(52)
        model = _grid_buffers(ngp.networks.NGP(scale=0.5).to(DEV))
        start = params(model)[2:]
        tr = NGPTrainer(model, lr=lr, **(fused_kw if fused else dict(loss_kwargs=module_kw)))
        assert tr.recipe.fused_loss == fused
        torch.manual_seed(53)
        steps = []
        for o, d, gt, tg in batches:
            if fused:
                steps.append(tr.step(o, d, gt, **{TERMS[k][1]: v for k, v in tg.items()}))
                if after_step is not None:
                    after_step(model)
            else:
                steps.append(tr.step(o, d, gt, target={TERMS[k][0]: v for k, v in tg.items()}))
        losses = [float(s[0]) for s in steps]
        tr.wait()
        end = params(model)
        runs[fused] = dict(tr=tr, steps=steps, losses=losses, params=end, start=dict(zip(tracked, start)),
                           end=dict(zip(tracked, end[2:])))
    a, b = runs[True], runs[False]
    print("FIG trainer losses fused", a["losses"], "module", b["losses"])
    _close(np.array(a["losses"]), np.array(b["losses"]), 1e-3, 1e-7)
    for k, (pa, pb) in enumerate(zip(a["params"], b["params"]), 1):
        print(f"FIG trainer params[{k}]: max|diff| {np.abs(pa - pb).max():.3g}")
        _close(pa, pb, 5e-3, 5e-5)
    return runs


def _tool(args, timeout):
    """tools/train_dataset.py in a child process with its own time limit -> its last JSON line"""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_dataset.py")] + args, capture_output=True,
                         text=True, timeout=timeout)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])
