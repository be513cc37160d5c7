"""The fused render + loss tail with several optional terms at once on the GPU (ngp_render_loss_fused_multi: the label
count, the depth fit and render_loss_fused_kernel<CMAX, 32, false, SEM, NRM, DEP>) against the parent's single entries bit
for bit, against ngp_render_loss_fused bit for bit, against the float64 restatement of tests/multi_tail_reference.py, and
the routes built on it: rendering._RenderLossFn, NGPTrainer(multi_terms=...), tools/train_dataset.py --multi_terms.

Bars.  The outputs shared with ngp_render_loss_fused are that entry's bit for bit; against the restatement they keep
tests/test_fused_tail_gpu.py's bars (opacity, depth, rgb, normal_pred, semantic, ws rtol 2e-5, atol 2e-6; d_rgbs rtol 2e-4,
atol 2e-5 / n_rays; Ro, Rp and terms[0:4] 8 times the float32 restatement's own error, not below 2e-6 times the term's
weight).  d_sigmas, d_sem, d_np, terms[4:8] and the fit's (a, b) are held to 8 times the float32 restatement's error
against float64 on that batch, with no floor: the rule and the constants (TF.NOISE_FACTOR) of the three sibling suites.
The inputs' promises (borderline rays, the sign margin of the normals, the spread of the depths, a sky ray with a valid
depth) are checked in tests/test_multi_tail_host.py.  Every figure is printed (FIG lines) before it is asserted; the
measured maxima are in profiles/multi_tail.txt, the end-to-end figures in profiles/multi_terms.txt."""
import json
import os

import numpy as np
import pytest
import torch

import multi_tail_reference as M
import test_depth_tail_gpu as DG
import test_fused_tail_gpu as TF
import test_normal_tail_gpu as NG
import test_semantic_tail_gpu as SG
from multi_tail_reference import DR, NR, R, SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N = TF.T, TF.N
PER_RAY = TF.PER_RAY
WS_INTS = 30
TRAJ_LR = NG.TRAJ_LR
ALL = M.TERMS
SEM, NRM, DEP = 1, 2, 4
_BATCH, _TARGETS, _STATE, _REF = {}, {}, {}, {}


def batch(name):
    """the batches of tests/test_fused_tail_gpu.py (crafted, random 300 / 1500) with 16 logit columns"""
    if name not in _BATCH:
        _BATCH[name] = M.make_batch(name)
        for v in _BATCH[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _BATCH[name]


def targets(name, classes, T_thr=1e-4, labels="mixed", normals="mixed", depths="mixed"):
    """the batch's seeded labels, normals (drawn against the normals composited at T_thr) and depths, computed once"""
    x = batch(name)
    keys = {"labels": ("labels", max(classes, 1), labels), "normals": ("normals", T_thr, normals), "depths": ("depths", depths)}
    make = {"labels": lambda: M.make_labels(x, max(classes, 1), valid=labels == "mixed"),
            "normals": lambda: M.make_normals(x, kind=normals, T_thr=T_thr), "depths": lambda: M.make_depths(x, kind=depths)}
    out = {}
    for k in keys:
        key = (name,) + keys[k]
        if key not in _TARGETS:
            _TARGETS[key] = make[k]()
            _TARGETS[key].setflags(write=False)
        out[k] = _TARGETS[key]
    return out


def reference(name, mask, tg, **cfg):
    """(float64 restatement, its float32 noise): the per-ray part (render, in float64 and in float32 at the float64 stops)
    is shared between the cases that differ only in the loss's arguments"""
    key = (name, mask) + tuple(v.tobytes() for v in tg.values()) + tuple(sorted(cfg.items()))
    if key not in _REF:
        x = batch(name)
        rkw = {k: v for k, v in cfg.items() if k in R.RENDER_KEYS}
        fkw = {k: v for k, v in cfg.items() if k not in R.RENDER_KEYS}
        rkey = (name,) + tuple(sorted(rkw.items()))
        if rkey not in _STATE:
            hi = R.render(x, **rkw)
            _STATE[rkey] = (hi, R.render(x, dtype=torch.float32, stops=hi["stops"], **rkw))
        hi, lo = _STATE[rkey]
        classes = cfg.get("classes", 7)
        ref = M.finish(hi, x, M.MASKS[mask], tg, classes, **fkw)
        _REF[key] = (ref, M.noise_of(M.finish(lo, x, M.MASKS[mask], tg, classes, **fkw), ref))
    return _REF[key]


def run_multi(ngp, x, mask, tg, T_thr=1e-4, classes=7, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D, lam_sem=SR.LAMBDA_SEM,
              lam_sky=SR.LAMBDA_SKY, lam_nm=NR.LAMBDA_NM, lam_dm=DR.LAMBDA_DM, scene_scale=1.0, use_bg=True, use_scale=False,
              n_rays=None, adjacent=True, garbage=-5, twice=False):
    """one direct call of ngp_render_loss_fused_multi on the first n_rays rows (default: all), every output pre-filled with
    NaN (the counts with negative numbers), the workspace with `garbage`: the entry clears it.  twice: a second call on the
    same buffers must leave every per-ray and per-sample output as the first did, bit for bit."""
    rows = len(x["rays_a"]) if n_rays is None else n_rays
    NR_, n = x["n_rays"], x["n"]
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3")}
    E = lambda *s: torch.full(s, float("nan"), device=DEV)
    total = torch.full((NR_,), -7, dtype=torch.int64, device=DEV)
    if adjacent:                # rendering.TAIL_LAYOUT['multi']: one buffer, one memset
        acc = E(10 + WS_INTS)
        terms, vr, ws_ = acc[:8], acc[8:10].view(torch.int64), acc[10:].view(torch.int32)
    else:
        terms, vr = E(8), torch.full((1,), -(2 ** 40) - 3, dtype=torch.int64, device=DEV)
        ws_ = torch.zeros(WS_INTS, dtype=torch.int32, device=DEV)
        assert vr.data_ptr() != terms.data_ptr() + 32 and ws_.data_ptr() != terms.data_ptr() + 40
    ws_.fill_(garbage)
    o = dict(opacity=E(NR_), depth=E(NR_), rgb=E(NR_, 3), normal=E(NR_, 3), sem=E(NR_, classes), ws=E(n), Ro=E(NR_),
             Rp=E(NR_, 3), terms=terms, d_sig=E(n), d_rgb=E(n, 3))
    if mask & SEM:
        o["d_sem"] = E(n, classes)
    if mask & NRM:
        o["d_np"] = E(n, 3)

    def call():
        ngp._lib.call("render_loss_fused_multi", t["sig"], t["rgbs"], t["dsig"], t["scale3"] if use_scale else None, t["nrm"],
                      t["nrm"].stride(0), t["sem"], t["sem"].stride(0), t["dirs"], t["deltas"], t["ts"], t["rays_a"], t["gt"],
                      t["bg"] if use_bg else None, int(mask), T(tg["labels"]) if mask & SEM else None, float(lam_sem),
                      float(lam_sky), T(tg["normals"]) if mask & NRM else None, float(lam_nm),
                      T(tg["depths"]) if mask & DEP else None, float(lam_dm), float(scene_scale), float(T_thr), int(classes),
                      rows, float(lam_o), float(lam_d), total, vr, o["opacity"], o["depth"], o["rgb"], o["normal"], o["sem"],
                      o["ws"], o["Ro"], o["Rp"], o["terms"], o["d_sig"], o["d_rgb"], ws_, o.get("d_sem"), o.get("d_np"))
        torch.cuda.synchronize()
    call()
    o["total"], o["vr"] = total, vr
    out = {k: N(v).copy() for k, v in o.items()}
    if twice:
        call()
        for k, v in o.items():
            if k != "terms":
                assert np.array_equal(N(v), out[k], equal_nan=v.dtype.is_floating_point), f"second call: {k}"
        np.testing.assert_allclose(N(o["terms"]), out["terms"], rtol=(rows // 8 + 1) * TF.REORDER, atol=0)
    w = N(ws_)
    out["n_valid_labels"] = int(w[0])
    out["fit"] = w[24:26].view(np.float32).astype(np.float64)
    out["n_valid_depths"] = int(w[26])
    out["counts"] = w[[6, 10, 27, 28]].astype(np.int64)   # finished workgroups: sem / multi, nrm / multi, the fit, dep's tail
    return out


def against_reference(tag, got, ref, noise, x, mask, cfg, ray_ok=None, smp_ok=None):
    """every output of one call against the restatement (module docstring's bars).  ray_ok / smp_ok: what is compared
    (default: all that a processed row owns).  Prints each figure, then fails with the list of outputs that miss."""
    n_rays = cfg.get("n_rays")
    rows = x["rays_a"][:n_rays]
    n_rows = len(rows)
    ray_own = np.zeros(x["n_rays"], bool)
    ray_own[rows[:, 0]] = True
    row_of, k_of = M.owned(x, n_rays)
    smp_own = row_of >= 0
    ray_ok = ray_own if ray_ok is None else ray_ok & ray_own
    smp_ok = smp_own if smp_ok is None else smp_ok & smp_own
    everything = ray_ok.sum() == n_rows
    per_sample = ["ws", "d_sig", "d_rgb"] + (["d_sem"] if mask & SEM else []) + (["d_np"] if mask & NRM else [])
    weights = [1.0, 1.0, cfg.get("lam_o", R.LAMBDA_O), cfg.get("lam_d", R.LAMBDA_D)]
    misses = []

    def held(key, g, w, bar, sel, scale=1.0):
        g = g.astype(np.float64)
        if g.size == 0:
            return
        width = g.size // len(g)
        sel = np.broadcast_to(sel.reshape(sel.shape + (1,) * (g.ndim - 1)), g.shape)
        w, bar = np.broadcast_to(w, g.shape), np.broadcast_to(bar, g.shape)
        err = np.where(sel, np.nan_to_num(np.abs(g - w), nan=np.inf), 0.0)          # (a NaN misses)
        ratio = np.where(sel, err / np.maximum(np.nan_to_num(bar), 1e-300), 0.0)
        worst = int(np.argmax(ratio))
        print(f"FIG {tag} {key}: max|err| {scale * err.max():.3g}" + (f" (times n_rays = {scale})" if scale != 1 else "") +
              f", worst err/bar {ratio.ravel()[worst]:.3g}")
        bad = sel & ~(err <= bar)
        if bad.any():
            misses.append(f"{key}: {bad.sum()} of {sel.sum()} miss; worst at "
                          f"{TF.where(x, 'ws' if key in per_sample else key, worst // width, n_rays)}: got "
                          f"{g.ravel()[worst]!r}, reference {w.ravel()[worst]!r}, bar {bar.ravel()[worst]:.3g}")

    blocks = (n_rows + 7) // 8
    multi = bin(mask).count("1") > 1
    want = [blocks if (mask & SEM) else 0, blocks if (mask == NRM or mask == (NRM | DEP)) else 0, blocks if mask & DEP else 0,
            blocks if mask == DEP else 0]
    if got["counts"].tolist() != want:
        misses.append(f"workspace: counts {got['counts'].tolist()}, expected {want} ({'one count for all terms' if multi else 'single form'})")
    if not np.array_equal(got["total"][ray_ok], ref["total"][ray_ok]):
        i = int(np.nonzero(ray_ok & (got["total"] != ref["total"]))[0][0])
        misses.append(f"total_samples: {TF.where(x, 'total', i, n_rays)}: got {got['total'][i]}, reference {ref['total'][i]}")
    if got["vr"][0] != got["total"][ray_own].sum() or (everything and got["vr"][0] != ref["vr"][0]):
        misses.append(f"vr_samples: got {got['vr'][0]}, sum of total_samples {got['total'][ray_own].sum()}, reference {ref['vr'][0]}")
    for key in list(PER_RAY) + per_sample:        # what no processed row owns (the gap, the other rows' rays) keeps its NaN
        own = smp_own if key in per_sample else ray_own
        if not np.isnan(got[key][~own]).all():
            misses.append(f"{key}: entries that no processed row owns were written")
    if not (got["total"][~ray_own] == -7).all():
        misses.append("total_samples: entries that no processed row owns were written")
    stop = ref["stops"][np.maximum(row_of, 0)]          # everything behind a stop is exactly 0
    behind = smp_ok & (stop >= 0) & (k_of > stop)
    for key in per_sample:
        if got[key][behind].any() or np.isnan(got[key][behind]).any():
            i = int(np.nonzero(behind)[0][0])
            misses.append(f"{key}: not exactly 0 behind a stop, e.g. {TF.where(x, 'ws', i, n_rays)}")
    empty = ray_own.copy()          # rays without samples give the background (black without one)
    empty[rows[:, 0]] = rows[:, 2] == 0
    want_bg = x["bg"].astype(np.float32) if cfg.get("use_bg", True) else np.zeros(3, np.float32)
    if empty.any() and not (np.array_equal(got["rgb"][empty], np.broadcast_to(want_bg, got["rgb"][empty].shape))
                            and not got["opacity"][empty].any() and not got["depth"][empty].any()):
        misses.append("rays without samples: not the background with zero opacity and depth")
    for key in ("opacity", "depth", "rgb", "normal", "sem"):
        held(key, got[key], ref[key], TF.FW_ATOL + TF.FW_RTOL * np.abs(ref[key]), ray_ok)
    held("ws", got["ws"], ref["ws"], TF.FW_ATOL + TF.FW_RTOL * np.abs(ref["ws"]), smp_ok)
    for key in ("Ro", "Rp"):
        held(key, got[key], ref[key], max(TF.NOISE_FACTOR * noise[key], TF.FW_ATOL), ray_ok)
    held("d_rgb", got["d_rgb"], ref["d_rgb"], TF.BW_ATOL / n_rows + TF.BW_RTOL * np.abs(ref["d_rgb"]), smp_ok, scale=n_rows)
    for key in per_sample[1:]:              # new: 8 x the float32 restatement's error on this batch
        if key != "d_rgb":
            held(key, got[key], ref[key], TF.NOISE_FACTOR * noise[key], smp_ok, scale=n_rows)
    if mask & SEM and got["n_valid_labels"] != ref["n_valid_labels"]:
        misses.append(f"n_valid of the labels: got {got['n_valid_labels']}, reference {ref['n_valid_labels']}")
    if mask & DEP:
        if got["n_valid_depths"] != ref["n_valid_depths"]:
            misses.append(f"n_valid of the fit: got {got['n_valid_depths']}, reference {ref['n_valid_depths']}")
        if everything:              # (a, b) depend on every row: compared when no row is borderline
            fit_bar = TF.NOISE_FACTOR * noise["fit"]
            print(f"FIG {tag} fit: got {got['fit']}, |err| {np.abs(got['fit'] - ref['fit'])}, bars {fit_bar}")
            for i, nm in enumerate("ab"):
                if not abs(got["fit"][i] - ref["fit"][i]) <= fit_bar[i]:
                    misses.append(f"fit {nm}: got {got['fit'][i]!r}, reference {ref['fit'][i]!r}, bar {fit_bar[i]:.3g}")
    assert got["terms"].shape == (8,)
    bars = TF.NOISE_FACTOR * noise["terms"]
    bars[:4] = np.maximum(bars[:4], TF.FW_ATOL * np.array(weights))
    print(f"FIG {tag} terms: got {got['terms']}, |err| {np.abs(got['terms'] - ref['terms'])}, bars {bars}")
    for i in range(8):
        if not abs(float(got["terms"][i]) - ref["terms"][i]) <= bars[i]:
            misses.append(f"terms[{i}]: got {got['terms'][i]!r}, reference {ref['terms'][i]!r}, bar {bars[i]:.3g}")
    for i, bit in ((4, SEM), (5, SEM), (6, NRM), (7, DEP)):
        if not mask & bit and not (got["terms"][i] == 0 and not np.signbit(got["terms"][i])):
            misses.append(f"terms[{i}]: {got['terms'][i]!r} for a term that is not named")
    print(f"FIG {tag} float32 noise of the restatement: " + ", ".join(f"{k} {np.max(v):.3g}" for k, v in noise.items()))
    assert not misses, f"{tag}:\n  " + "\n  ".join(misses)


# ------------------------------------------------------------------------------------------- a. the parent's entries
@pytest.mark.parametrize("n_rays", [None, 8])
@pytest.mark.parametrize("name,classes", [("crafted", 7), ("crafted", 10), ("1500", 8)])
def test_single_bit_masks_are_the_single_entries(ngp, name, classes, n_rays):
    """a mask with one bit launches that term's own kernel: every per-ray and per-sample output, d_sem and d_np, the labels'
    n_valid and the fit's n_valid equal ngp_render_loss_fused_sem / _nrm / _dep's on the same inputs bit for bit.  The terms
    and (a, b) bit for bit where one workgroup forms them (8 rays); elsewhere within the reordering of one float atomic per
    workgroup (terms[0:4]) and one ulp of the once-rounded double sums (the optional terms, a, b), the siblings' bars for two
    launches on the same inputs."""
    x = batch(name)
    tg = targets(name, classes)
    blocks = ((len(x["rays_a"]) if n_rays is None else n_rays) + 7) // 8
    cfg = dict(classes=classes, n_rays=n_rays, use_scale=True, T_thr=1e-4)
    singles = [(SEM, SG.run_sem(ngp, x, tg["labels"], **cfg), [4, 5])]
    if classes <= 8:
        singles += [(NRM, NG.run_nrm(ngp, x, tg["normals"], **cfg), [6]), (DEP, DG.run_dep(ngp, x, tg["depths"], scene_scale=0.5, **cfg), [7])]
    for mask, b, slots in singles:
        a = run_multi(ngp, x, mask, tg, scene_scale=0.5, **cfg)
        keys = ["total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "ws", "d_sig", "d_rgb"]
        keys += {SEM: ["d_sem"], NRM: ["d_np"], DEP: []}[mask]
        exact_fit = mask != DEP or blocks <= 2          # (two double addends commute; more arrive in any order)
        for key in keys:
            if key == "d_sig" and not exact_fit and not np.array_equal(a["fit"], b["fit"]):
                np.testing.assert_allclose(a[key], b[key], rtol=1e-6, atol=1e-12)
                continue
            assert np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (mask, key)
        if mask == SEM:
            assert a["n_valid_labels"] == int(b["n_valid"][0]) > 0
        if mask == DEP:
            assert a["n_valid_depths"] == b["n_valid"] > 1
            if exact_fit:
                assert np.array_equal(a["fit"], b["fit"]), (a["fit"], b["fit"])
            else:
                np.testing.assert_allclose(a["fit"], b["fit"], rtol=2.0 ** -23, atol=0)
        opt = np.zeros(4)
        opt[np.array(slots) - 4] = b["terms"][4:]
        print(f"FIG single mask={mask} {name} classes={classes} rows={n_rays}: terms multi {a['terms']}, single {b['terms']}")
        if blocks == 1:
            assert np.array_equal(a["terms"][1:4], b["terms"][1:4]) and np.array_equal(a["terms"][4:], opt)
            assert a["terms"][0] == b["terms"][0]
        else:
            np.testing.assert_allclose(a["terms"][:4], b["terms"][:4], rtol=blocks * TF.REORDER, atol=0)
            np.testing.assert_allclose(a["terms"][4:], opt, rtol=2.0 ** -23, atol=0)
        assert all(a["terms"][s] != 0 for s in slots)


# ------------------------------------------------------------------------------------------- b. the default entry
@pytest.mark.parametrize("name,classes,mask", [(n, c, m) for n, c in (("crafted", 7), ("crafted", 16), ("1500", 8))
                                               for m in sorted(M.MASKS) if c <= 8 or m & SEM])
def test_shared_outputs_are_the_default_entrys(ngp, name, classes, mask):
    """depth, opacity, rgb, normal_pred, sem, ws, Ro, Rp, d_rgbs and the sample counts are ngp_render_loss_fused's bit for bit
    at any weight (the 16-class forms too, but for `sem`, which the default entry does not have at that width); with every
    optional weight 0 so is d_sigmas.  (a, b) of a mask with the depth term beside others is ngp_render_loss_fused_dep's bit
    for bit on up to 16 rays (one or two workgroups: the double sums do not depend on the arrival order), which together with
    the bit-equal `depth` pins the rounded product and add of the composited depth in the new kernels."""
    x = batch(name)
    tg = targets(name, classes)
    plain = TF.run_tail(ngp, x, classes=min(classes, 8), use_scale=True)
    shared = ("total", "vr", "opacity", "depth", "rgb", "normal", "Ro", "Rp", "ws", "d_rgb")
    for zero in (False, True):
        lam = dict(lam_sem=0.0, lam_sky=0.0, lam_nm=0.0, lam_dm=0.0) if zero else {}
        got = run_multi(ngp, x, mask, tg, classes=classes, use_scale=True, scene_scale=0.5, **lam)
        for key in shared + (("d_sig",) if zero else ()):
            assert np.array_equal(got[key], plain[key], equal_nan=got[key].dtype.kind == "f"), (key, zero)
        if classes <= 8:
            assert np.array_equal(got["sem"], plain["sem"], equal_nan=True), zero
        if zero:
            assert not got["terms"][4:].any()
            blocks = len(x["rays_a"]) // 8 + 1
            np.testing.assert_allclose(got["terms"][:4], plain["terms"], rtol=blocks * TF.REORDER, atol=0)
    if mask & DEP and mask != DEP and classes <= 8:
        for rows in (7, 8, 9, 16):
            a = run_multi(ngp, x, mask, tg, classes=classes, n_rays=rows, scene_scale=0.5)
            b = DG.run_dep(ngp, x, tg["depths"], classes=classes, n_rays=rows, scene_scale=0.5)
            print(f"FIG fit mask={mask} {name} rows={rows}: multi {a['fit']}, dep {b['fit']}")
            assert np.array_equal(a["fit"], b["fit"]) and a["n_valid_depths"] == b["n_valid"] > 1
            assert np.array_equal(a["depth"], b["depth"], equal_nan=True)


# ------------------------------------------------------------------------------------------- c. the restatement
def _cases():
    out = []
    for mask in M.MULTI_MASKS:
        for classes in ((1, 5, 7, 8, 9, 10, 16) if mask & SEM else (0, 7, 8)):
            out.append((mask, classes))
    return out


@pytest.mark.parametrize("args", ["bg", "nobg-scale"])
@pytest.mark.parametrize("T_thr", [1e-4, 1e-2])
@pytest.mark.parametrize("mask,classes", _cases())
def test_crafted_edges(ngp, mask, classes, T_thr, args):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges (length 0 included), with the gap and the permuted rows; nothing is left out of the comparison.
    Among the labels a sky ray with a valid depth, so the summed depth seed is exercised."""
    x = batch("crafted")
    tg = targets("crafted", classes, T_thr)
    scale = 0.5 if args == "bg" else 8.0
    cfg = dict(T_thr=T_thr, classes=classes, scene_scale=scale, **{k: v for k, v in TF.ARGS[args].items() if k in ("use_bg", "use_scale")})
    ref, noise = reference("crafted", mask, tg, **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    if mask & SEM and mask & DEP:
        sky = M.sky_rows_with_depth(x, tg["labels"], tg["depths"])
        assert len(sky) and np.abs(ref["g_D"][sky]).max() > 0
    if mask & NRM:
        assert NR.sign_margin(x, tg["normals"], T_thr=T_thr) >= NR.SIGN_MARGIN
    got = run_multi(ngp, x, mask, tg, **cfg)
    against_reference(f"crafted mask={mask} classes={classes} T_thr={T_thr} {args}", got, ref, noise, x, mask, cfg)


@pytest.mark.parametrize("name,mask,classes,scene_scale", [("300", 3, 9, 1.0), ("300", 5, 7, 0.5), ("300", 6, 7, 8.0),
                                                           ("300", 7, 16, 0.5), ("1500", 6, 8, 0.5), ("1500", 7, 10, 8.0)])
def test_random_batch(ngp, name, mask, classes, scene_scale):
    """the random batches of tests/test_fused_tail_gpu.py, under its rule for borderline rays (within 1e-3 of T_threshold in
    float64: left out of the per-ray and per-sample comparisons, at most MAX_BORDERLINE of the batch; the loss terms are
    compared all the same, (a, b) when no ray is borderline)"""
    x = batch(name)
    tg = targets(name, classes)
    cfg = dict(classes=classes, scene_scale=scene_scale)
    ok, ray_ok, smp_ok = M.comparable(x, 1e-4, 1e-3)
    left_out = 1.0 - ok.mean()
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}")
    assert left_out <= M.MAX_BORDERLINE
    if mask & SEM and mask & DEP:
        assert len(M.sky_rows_with_depth(x, tg["labels"], tg["depths"]))
    ref, noise = reference(name, mask, tg, **cfg)
    got = run_multi(ngp, x, mask, tg, **cfg)
    against_reference(f"random-{name} mask={mask} classes={classes}", got, ref, noise, x, mask, cfg, ray_ok, smp_ok)


# ------------------------------------------------------------------------------------------- d. launch shapes
@pytest.mark.parametrize("mask", [6, 7])
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows, mask):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8), a
    second workgroup with one ray (9); the seeds scale with 1 / rows.  One row is the singular system: (a, b) = (0, 0)
    exactly.  Everything that belongs to the other rows is left alone."""
    x = batch("crafted")
    tg = targets("crafted", 7)
    cfg = dict(n_rays=rows, classes=7)
    ref, noise = reference("crafted", mask, tg, **cfg)
    got = run_multi(ngp, x, mask, tg, **cfg)
    if rows == 1:
        assert got["fit"].tolist() == [0.0, 0.0] and ref["terms"][7] > 0
    against_reference(f"crafted mask={mask} rows={rows}", got, ref, noise, x, mask, cfg)


def test_memset_branches_garbage_and_a_second_call(ngp):
    """terms, vr_samples and the workspace adjacent as rendering._RenderLossFn lays them out (one fill) and in separate
    allocations (three fills), the workspace starting as -5, as all bits set and as a large positive pattern: the entry
    clears it, so the launches agree with one another and with the restatement, and a second call on the same buffers
    leaves the same per-ray and per-sample outputs bit for bit"""
    x = batch("crafted")
    tg = targets("crafted", 7)
    cfg = dict(classes=7, scene_scale=0.5)
    runs = [("adjacent", run_multi(ngp, x, 7, tg, adjacent=True, twice=True, **cfg)),
            ("separate", run_multi(ngp, x, 7, tg, adjacent=False, twice=True, **cfg)),
            ("adjacent all-ones", run_multi(ngp, x, 7, tg, adjacent=True, garbage=-1, **cfg)),
            ("separate 0x7f7f7f7f", run_multi(ngp, x, 7, tg, adjacent=False, garbage=0x7F7F7F7F, **cfg))]
    ref, noise = reference("crafted", 7, tg, **cfg)
    a = runs[0][1]
    for tag, got in runs:
        for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "ws", "d_rgb", "d_sem", "d_np", "counts"):
            assert np.array_equal(a[k], got[k], equal_nan=a[k].dtype.kind == "f"), (tag, k)
        assert got["n_valid_labels"] == a["n_valid_labels"] and got["n_valid_depths"] == a["n_valid_depths"]
        # (the fit's five sums are doubles added in arrival order: (a, b) within an ulp, the optional terms rounded once)
        np.testing.assert_allclose(got["fit"], a["fit"], rtol=2.0 ** -23, atol=0)
        np.testing.assert_allclose(got["terms"][4:], a["terms"][4:], rtol=2.0 ** -23, atol=0)
        np.testing.assert_allclose(got["terms"][:4], a["terms"][:4], rtol=4 * TF.REORDER, atol=0)
        against_reference(f"crafted memset {tag}", got, ref, noise, x, 7, cfg)


# ------------------------------------------------------------------------------------------- e. degenerate batches
@pytest.mark.parametrize("what", ["labels", "normals", "depths-none", "depths-one"])
def test_degenerate_targets(ngp, what):
    """no valid label / every normal zero / no valid depth / one valid depth: that term is exactly 0 with exactly zero
    gradients ((a, b) = (0, 0) for the fit) while the other terms and every output keep to the restatement"""
    x = batch("crafted")
    kinds = {"labels": dict(labels="none"), "normals": dict(normals="none"), "depths-none": dict(depths="none"),
             "depths-one": dict(depths="one")}[what]
    tg = targets("crafted", 7, **kinds)
    cfg = dict(classes=7, scene_scale=0.5)
    got = run_multi(ngp, x, 7, tg, **cfg)
    own = M.owned(x)[0] >= 0
    if what == "labels":
        assert got["n_valid_labels"] == 0 and got["terms"][4] == 0.0 and not got["d_sem"][own].any()
        assert got["terms"][6] != 0 and got["terms"][7] != 0 and got["d_np"][own].any()
    elif what == "normals":
        assert got["terms"][6] == 0.0 and not got["d_np"][own].any()
        assert got["terms"][4] != 0 and got["terms"][7] != 0 and got["d_sem"][own].any()
    else:
        assert got["fit"].tolist() == [0.0, 0.0] and got["n_valid_depths"] == (0 if what == "depths-none" else 1)
        if what == "depths-none":
            assert got["terms"][7] == 0.0
        # without a fit the depth term has no gradient: d_sigmas is that of the semantic + normal form, to the restatement
        assert got["terms"][4] != 0 and got["terms"][6] != 0
    assert np.isfinite(got["terms"]).all() and np.isfinite(got["d_sig"][own]).all()
    ref, noise = reference("crafted", 7, tg, **cfg)
    against_reference(f"crafted degenerate {what}", got, ref, noise, x, 7, cfg)


# ------------------------------------------------------------------------------------------- f. autograd
_close, _grid_buffers = DG._close, DG._grid_buffers


def test_wrapper_hands_back_the_direct_call(ngp):
    """rendering._RenderLossFn with several terms on the crafted batch: the outputs are those of the direct call, and back-propagating
    terms[0] with a unit seed hands back the launch's d_sigmas, d_rgbs, d_sem and d_np bit for bit (padded with zeros to the
    inputs' widths); a term that is not named gives its input no gradient"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x = batch("crafted")
    tg = targets("crafted", 10)
    for mask in (7, 6, 5):
        classes = 10 if mask & SEM else 7
        direct = run_multi(ngp, x, mask, tg, classes=classes, use_scale=True, scene_scale=0.5)
        t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3")}
        leaves = [t[k].requires_grad_(True) for k in ("sig", "rgbs", "sem", "nrm")]
        named = {}
        if mask & SEM:
            named["semantic"] = (T(tg["labels"]), SR.LAMBDA_SEM, SR.LAMBDA_SKY)
        if mask & NRM:
            named["normal_mono"] = (T(tg["normals"]), NR.LAMBDA_NM)
        if mask & DEP:
            named["depth_mono"] = (T(tg["depths"]), DR.LAMBDA_DM, 0.5)
        rest = (None, t["dsig"], t["dirs"], t["deltas"], t["ts"], t["rays_a"])
        outs = _RenderLossFn.apply(*leaves, *rest, FusedTail(t["gt"], R.LAMBDA_O, R.LAMBDA_D, terms=named), t["scale3"], 1e-4,
                                   classes, t["bg"])
        terms = outs[0]
        assert terms.shape == (8,) and terms.requires_grad and not any(o.requires_grad for o in outs[1:] if o is not None)
        seed = torch.zeros_like(terms)
        seed[0] = 1.0
        torch.autograd.backward([terms], [seed])
        own = M.owned(x)[0] >= 0
        got = dict(zip(("terms", "total", "vr", "opacity", "depth", "rgb", "normal", "sem", "ws", "Ro", "Rp"), (N(o) for o in outs)))
        for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp"):
            assert np.array_equal(got[k], direct[k]), k
        np.testing.assert_allclose(got["terms"][:4], direct["terms"][:4], rtol=4 * TF.REORDER, atol=0)
        np.testing.assert_allclose(got["terms"][4:], direct["terms"][4:], rtol=2.0 ** -23, atol=0)
        w = N(outs[11])
        assert w.shape == (WS_INTS,) and w.dtype == np.int32
        fit = w[24:26].view(np.float32).astype(np.float64)
        sig, rgbs, sem, nrm = leaves
        if not mask & DEP or np.array_equal(fit, direct["fit"]):          # the same (a, b): the same gradients bit for bit
            assert np.array_equal(N(sig.grad)[own], direct["d_sig"][own])
        else:
            np.testing.assert_allclose(fit, direct["fit"], rtol=2.0 ** -23, atol=0)
            np.testing.assert_allclose(N(sig.grad)[own], direct["d_sig"][own], rtol=1e-6, atol=1e-12)
        assert np.array_equal(N(rgbs.grad)[own], direct["d_rgb"][own])
        if mask & SEM:
            g = N(sem.grad)
            assert g.shape == (x["n"], 16) and np.array_equal(g[own, :classes], direct["d_sem"][own]) and not g[:, classes:].any()
        else:
            assert sem.grad is None
        if mask & NRM:
            assert np.array_equal(N(nrm.grad)[own], direct["d_np"][own])
        else:
            assert nrm.grad is None
    for bad in (dict(), dict(sky=(1,)), dict(semantic=(T(tg["labels"])[:5], 1.0, 1.0)), dict(normal_mono=(T(tg["normals"]).double(), 1.0)),
                dict(depth_mono=(T(tg["depths"]).reshape(-1, 1), 1.0, 1.0)), dict(depth_mono=(T(tg["depths"]), 1.0, 0.0))):
        with pytest.raises((ValueError, RuntimeError)):
            _RenderLossFn.apply(*leaves, *rest, FusedTail(t["gt"], 0.0, 0.0, terms=bad), t["scale3"], 1e-4, 7, None)


def _scene_targets(scene, o, d, classes, gen):
    return SG._scene_labels(scene, o, d, classes, gen), NG._nonzero_normals(scene, o, d, gen), DG._mono_depths(scene, o, d)


@pytest.mark.parametrize("classes", [7, 10])
def test_fused_multi_tail_matches_the_launch_per_operation_route(ngp, classes):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background
    draw on both routes, labels valid or 256, every normal non-zero, depths without NaN (where the module states the same
    loss).  A: render + NeRFLoss(semantic, normal_mono, depth_mono, scale=8) + sum of means + autograd; B: render with
    _fused_loss=FusedTail(gt, lambda_o, lambda_d, terms={...}) through rendering._RenderLossFn.  The bars of the three sibling
    comparisons: terms rtol 1e-4, parameter gradients within 3e-4 of the largest entry."""
    from ngp_amd.losses import NeRFLoss
    from ngp_amd.rendering import FusedTail, render
    from ngp_amd.synthetic import LegoProxy
    torch.manual_seed(33)
    model = _grid_buffers(ngp.networks.NGP(scale=8.0, classes=classes).to(DEV))
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.5)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    scene = LegoProxy(n_images=6, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(34)
    img, pix = scene.sample_batch(1500, generator=gen)
    o, d = scene.rays(img, pix)
    gt = torch.rand(1500, 3, device=DEV, generator=gen)
    labels, normals, depths = _scene_targets(scene, o, d, classes, gen)
    assert int(((labels == 4) & (depths > 0)).sum()) > 0 or int((labels == 4).sum()) > 100
    f = NeRFLoss()
    multi = {"semantic": (labels, f.lambda_semantic, f.lambda_sky), "normal_mono": (normals, f.lambda_normal_mono),
             "depth_mono": (depths, f.lambda_depth_mono, 8.0)}
    named = [(n, p) for n, p in model.named_parameters() if p.numel() > 0]
    out = {}
    for fused in (False, True):
        for _, p in named:
            p.grad = None
        torch.manual_seed(35)
        kw = dict(exp_step_factor=1 / 256, num_classes=classes, random_bg=True)
        if fused:
            res = render(model, o, d, _fused_loss=FusedTail(gt, f.lambda_opa, f.lambda_distortion, terms=multi), **kw)
            assert "_loss_terms" in res
            terms = res.pop("_loss_terms")
            assert terms.shape == (8,) and terms.requires_grad
            torch.autograd.backward([terms], [torch.tensor([1.0, 0, 0, 0, 0, 0, 0, 0], device=DEV)])
            terms = N(terms)
        else:
            res = render(model, o, d, **kw)
            ld = f(res, {"rgb": gt, "label": labels, "normal": normals, "depth": depths}, semantic=True, normal_mono=True,
                   depth_mono=True, scale=8.0)
            loss = sum(t.mean() for t in ld.values())
            loss.backward()
            # (the module's normal_mono entry is (R, 3): its mean is the entry's term)
            terms = np.array([float(loss.detach())] + [float(ld[n].detach().mean()) for n in
                                                        ("rgb", "opacity", "distortion", "CELoss", "sky_depth", "normal_mono",
                                                         "depth_mono")], np.float32)
        out[fused] = (res, terms, {n: None if p.grad is None else N(p.grad).copy() for n, p in named})
    ra, ta, ga = out[False]
    rb, tb, gb = out[True]
    assert int(ra["total_samples"]) == int(rb["total_samples"]) > 0
    for key in ("opacity", "depth", "rgb", "normal_pred", "semantic", "ws", "Ro", "Rp"):
        _close(N(rb[key]), N(ra[key]), 2e-5, 2e-6)
    print("FIG autograd terms A", ta, "terms B", tb)
    _close(tb, ta, 1e-4, 1e-9)
    assert (tb[4:] > 0).all()
    for name in ga:
        a, b = ga[name], gb[name]
        if a is None:
            assert b is None or not b.any(), name
            continue
        scale = np.abs(a).max()
        print(f"FIG autograd grad {name}: max|a - b| / max|a| = {np.abs(a - b).max() / max(scale, 1e-300):.3g}")
        assert np.abs(a - b).max() <= 3e-4 * scale + 1e-12, (name, np.abs(a - b).max(), scale)
    for name in ("semantic_header.params", "norm_pred_header.params", "rgb_encoder.params", "xyz_encoder.params"):
        if name in gb:
            assert np.abs(gb[name]).sum() > 0, name


# ------------------------------------------------------------------------------------------- g. the trainer
def _was_bound_step(model):
    """whether the step just taken ran on the norm-bound clip: only then do the two MLP backwards note their sums with the
    field's link (link.FieldLink.bound_note), and nothing may have spoiled the bound"""
    return model.link.hits == 2 and model.link.ok


def test_trainer_multi_route_matches_module_route(ngp):
    """NGPTrainer(multi_terms=all three) with step(labels=, normals=, depths=) follows the trajectory of
    NGPTrainer(loss_kwargs={'semantic', 'normal_mono', 'depth_mono', 'scale': 0.5}) with step(target={...}) for six steps of
    1024 rays at lr = TRAJ_LR (test_normal_tail_gpu.py says why not 1e-2), within the siblings' bars: losses rtol 1e-3,
    parameters rtol 5e-3 / atol 5e-5.  The fused route takes the exact gradient norm (the heads add to the colour table)."""
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=10, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(51)
    batches = []
    for i in range(6):
        img, pix = scene.sample_batch(1024, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        batches.append((o, d, gt) + _scene_targets(scene, o, d, 7, gen))
    out = []
    for fused in (True, False):
        torch.manual_seed(52)
        model = _grid_buffers(ngp.networks.NGP(scale=0.5).to(DEV))
        kw = dict(multi_terms=ALL) if fused else dict(loss_kwargs={"semantic": True, "normal_mono": True, "depth_mono": True,
                                                                    "scale": 0.5})
        tr = NGPTrainer(model, lr=TRAJ_LR, **kw)
        assert tr.fused_loss == fused and tr.multi_terms == (ALL if fused else ())
        assert not (tr.semantic or tr.normal_mono or tr.depth_mono)
        torch.manual_seed(53)
        if fused:
            steps = []
            for o, d, gt, lab, nrm, dep in batches:
                steps.append(tr.step(o, d, gt, labels=lab, normals=nrm, depths=dep))
                assert not _was_bound_step(model)
            assert all(s[1]["loss_terms"].shape == (8,) for s in steps)
            opt = np.stack([N(s[1]["loss_terms"])[4:] for s in steps])
            print("FIG trainer optional terms per step", opt.tolist())
            assert (opt > 0).all()
        else:
            steps = [tr.step(o, d, gt, target={"label": lab, "normal": nrm, "depth": dep}) for o, d, gt, lab, nrm, dep in batches]
        losses = [float(s[0]) for s in steps]
        tr.wait()
        out.append((losses, N(model.xyz_net[0].weight).copy(), N(model.rgb_net.params).copy(),
                    N(model.xyz_encoder.params).copy(), N(model.semantic_header.params).copy()))
    print("FIG trainer losses fused", out[0][0], "module", out[1][0])
    _close(np.array(out[0][0]), np.array(out[1][0]), 1e-3, 1e-7)
    for k in (1, 2, 3, 4):
        print(f"FIG trainer params[{k}]: max|diff| {np.abs(out[0][k] - out[1][k]).max():.3g}")
        _close(out[0][k], out[1][k], 5e-3, 5e-5)


def test_trainer_multi_argument_checks(ngp):
    """every combination the multi tail does not cover raises ValueError; the route combines with appearance codes and a
    random background; any non-empty subset trains; degenerate targets train on; ('depth_mono',) alone keeps the norm-bound
    clip; a model that leaves the fused tail makes step() raise"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=4, img_wh=(20, 20), device=DEV)
    make = lambda **kw: _grid_buffers(ngp.networks.NGP(scale=0.5, **kw).to(DEV))
    model = make()
    refused = [dict(msk_model=implicit_mask().to(DEV)), dict(pose_refiner=PoseRefiner(scene.poses, scene.directions).to(DEV)),
               dict(semantic=True), dict(normal_mono=True), dict(depth_mono=True), dict(render_kwargs={"use_skybox": True}),
               dict(loss_kwargs={"normal_mono": True}), dict(loss_kwargs={"semantic": True}),
               dict(loss_kwargs={"depth_mono": True}), dict(loss_kwargs={"normal_ref": True}), dict(num_classes=5)]
    for kw in refused:
        with pytest.raises(ValueError):
            NGPTrainer(model, multi_terms=ALL, **kw)
    assert model.differentiable_normals is False
    for model_kw in (dict(rgb_act="None"), dict(use_skybox=True)):
        with pytest.raises(ValueError):
            NGPTrainer(make(**model_kw), multi_terms=ALL)
    img, pix = scene.sample_batch(64)
    o, d = scene.rays(img, pix)
    gt = torch.rand(64, 3, device=DEV)
    lab = torch.randint(0, 7, (64,), device=DEV)
    lab[::9] = 256
    nrm = torch.randn(64, 3, device=DEV)
    nrm[::4] = 0
    dep = 25 * (0.2 + torch.rand(64, device=DEV))
    dep[::5] = float("nan")
    full = dict(labels=lab, normals=nrm, depths=dep)
    model = make(embed_a=True, embed_a_len=4)
    emb = torch.nn.Embedding(4, 4).to(DEV)
    tr = NGPTrainer(model, multi_terms=ALL, embedding_a=emb, exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, labels=lab, normals=nrm)
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, target={"depth": None}, **full)
    loss, res = tr.step(o, d, gt, img_idxs=img, **full)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all() and res["loss_terms"].shape == (8,)
    loss, res = tr.step(o, d, gt, img_idxs=img, labels=torch.full_like(lab, 256), normals=torch.zeros_like(nrm),
                        depths=torch.zeros_like(dep))
    tr.wait()
    t = N(res["loss_terms"])
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all() and not t[[4, 6, 7]].any()
    # a model that leaves the fused tail after construction is an error, not a step on the default loss without targets
    model.differentiable_normals = True
    with pytest.raises(RuntimeError):
        tr.step(o, d, gt, img_idxs=img, **full)
    model.differentiable_normals = False
    for terms in (("depth_mono",), ("normal_mono", "depth_mono"), ("semantic",)):
        tr = NGPTrainer(make(), multi_terms=terms)
        kw = {k: v for k, v in full.items() if {"labels": "semantic", "normals": "normal_mono", "depths": "depth_mono"}[k] in terms}
        loss, res = tr.step(o, d, gt, **kw)
        tr.wait()
        t = N(res["loss_terms"])
        assert t.shape == (8,) and np.isfinite(t).all()
        assert _was_bound_step(tr.model) == (terms == ("depth_mono",) and bool(tr.norm_bound))
        with pytest.raises(ValueError):
            tr.step(o, d, gt, **full) if len(kw) < 3 else tr.step(o, d, gt)


# ------------------------------------------------------------------------------------------- h. end to end
def test_train_dataset_with_all_three_terms_end_to_end(ngp, tmp_path):
    """the tool in a fresh child process under a time limit: the proxy scene with labels, normal and depth maps in the tnt
    layout (34 views of 80 x 80, every 8th held out), 600 steps of 2048 rays with --multi_terms semantic normal_mono
    depth_mono.  Barred: the JSON line has the four metrics and loss_terms == 8, every term is finite, held-out PSNR > 20 dB
    (the project's bar for 600 steps on a tnt export).  The metric values and the terms' first / last means are recorded
    (FIG lines, profiles/multi_terms.txt), not barred."""
    root = str(tmp_path / "scene")
    out = DG._tool(["--make_proxy", root, "--downsample", "0.1", "--proxy_views", "34", "--dataset_name", "tnt", "--num_epochs",
                    "3", "--steps_per_epoch", "200", "--batch_size", "2048", "--num_classes", "5", "--multi_terms", "semantic",
                    "normal_mono", "depth_mono"], 300)
    for sub in ("semantic", "normal", "depth"):
        assert len(os.listdir(os.path.join(root, sub))) == 34, sub
    keys = ["test_psnr_mean", "test_ssim_mean", "test_sem_acc_mean", "test_sem_miou_mean", "test_normal_deg_mean",
            "test_depth_absrel_mean"]
    keys += [f"{t}_term_{w}" for t in ("CELoss", "sky_depth", "normal_mono", "depth_mono") for w in ("first", "last")]
    for key in keys:
        assert key in out and np.isfinite(out[key]), (key, out.get(key))
    assert out["steps"] == 600 and out["img_wh"] == [80, 80] and out["loss_terms"] == 8 and out["num_classes"] == 5
    assert out["multi_terms"] == list(ALL)
    print("FIG end-to-end multi_terms: " + json.dumps({k: out[k] for k in keys}))
    assert out["test_psnr_mean"] > 20.0
