"""The depth_mono form of the fused render + loss tail on the GPU (depth_fit_kernel, then
render_loss_fused_kernel<8, 32, false, false, false, true>, behind ngp_render_loss_fused_dep) against the float64
restatement of tests/depth_tail_reference.py, and the routes built on it: rendering._RenderLossFn,
NGPTrainer(depth_mono=True), tools/train_dataset.py --depth_mono.

Bars.  The outputs this entry shares with ngp_render_loss_fused keep tests/test_fused_tail_gpu.py's bars: opacity, depth,
rgb, normal_pred, semantic, ws rtol 2e-5, atol 2e-6; d_rgbs rtol 2e-4, atol 2e-5 / n_rays; Ro, Rp and terms[0:4] 8 times
the float32 restatement's own error on the same inputs, not below 2e-6 (times the term's weight).  d_sigmas, terms[4] and
the workspace's (a, b) are held to 8 times the float32 restatement's error against float64 on that batch, with no floor
(the rule of the semantic and normal tails; d_sigmas: the largest error over the batch's samples).  The seeded depths keep
var(D) / mean(D^2) >= 0.1 over the valid rays of every batch and prefix compared here (tests/test_depth_tail_host.py).
Every figure is printed (FIG lines) before it is asserted; the measured maxima are in profiles/depth_tail.txt.

End to end (test_train_dataset_with_depths_end_to_end) held-out PSNR and depth_absrel with lambda_depth_mono = 1 and = 0
are recorded, not barred: profiles/depth_mono.txt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_tail_reference as DR
import test_fused_tail_gpu as TF

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N = TF.T, TF.N
PER_RAY, PER_SAMPLE = TF.PER_RAY, TF.PER_SAMPLE
WS_INTS = 18
TRAJ_LR = 3e-4          # learning rate of the six-step trajectory comparison: see test_normal_tail_gpu.py's write-up
_DEPTHS, _STATE, _REF = {}, {}, {}
batch = TF.batch


def depths_of(name, kind="mixed"):
    """the batch's seeded depths, computed once: 'mixed' (a fifth of the rows 0, negative or NaN), 'none', 'one'"""
    key = (name, kind)
    if key not in _DEPTHS:
        _DEPTHS[key] = DR.make_depths(batch(name), kind=kind)
        _DEPTHS[key].setflags(write=False)
    return _DEPTHS[key]


def reference(name, kind="mixed", **cfg):
    """(float64 restatement, its float32 noise): computed once per (batch, depths, arguments), shared, read-only"""
    key = (name, kind) + tuple(sorted(cfg.items()))
    if key not in _REF:
        x, depths = batch(name), depths_of(name, kind)
        rkw = {k: v for k, v in cfg.items() if k in DR.R.RENDER_KEYS}
        fkw = {k: v for k, v in cfg.items() if k not in DR.R.RENDER_KEYS}
        rkey = (name,) + tuple(sorted(rkw.items()))
        if rkey not in _STATE:
            hi = DR.R.render(x, **rkw)
            _STATE[rkey] = (hi, DR.R.render(x, dtype=torch.float32, stops=hi["stops"], **rkw))
        hi, lo = _STATE[rkey]
        ref = DR.finish(hi, x, depths, **fkw)
        _REF[key] = (ref, DR.noise_of(DR.finish(lo, x, depths, **fkw), ref))
    return _REF[key]


def run_dep(ngp, x, depths, T_thr=1e-4, classes=7, lam_o=DR.R.LAMBDA_O, lam_d=DR.R.LAMBDA_D, lam_dm=DR.LAMBDA_DM,
            scene_scale=1.0, use_bg=True, use_scale=False, n_rays=None, adjacent=True, garbage=None):
    """one direct call of ngp_render_loss_fused_dep on the first n_rays rows (default: all), every output pre-filled with
    NaN (the counts with negative numbers, the workspace with `garbage`, default -5: the entry clears it)"""
    rows = len(x["rays_a"]) if n_rays is None else n_rays
    NR_, n = x["n_rays"], x["n"]
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3")}
    E = lambda *s: torch.full(s, float("nan"), device=DEV)
    total = torch.full((NR_,), -7, dtype=torch.int64, device=DEV)
    if adjacent:                # rendering.TAIL_LAYOUT['dep']: one buffer, one memset
        acc = E(8 + WS_INTS)
        terms, vr, ws_ = acc[:5], acc[6:8].view(torch.int64), acc[8:].view(torch.int32)
    else:
        terms, vr = E(5), torch.full((1,), -(2 ** 40) - 3, dtype=torch.int64, device=DEV)
        ws_ = torch.zeros(WS_INTS, dtype=torch.int32, device=DEV)
        assert vr.data_ptr() != terms.data_ptr() + 24 and ws_.data_ptr() != terms.data_ptr() + 32
    ws_.fill_(-5 if garbage is None else garbage)
    o = dict(opacity=E(NR_), depth=E(NR_), rgb=E(NR_, 3), normal=E(NR_, 3), sem=E(NR_, classes), ws=E(n), Ro=E(NR_),
             Rp=E(NR_, 3), terms=terms, d_sig=E(n), d_rgb=E(n, 3))
    ngp._lib.call("render_loss_fused_dep", t["sig"], t["rgbs"], t["dsig"], t["scale3"] if use_scale else None, t["nrm"],
                  t["nrm"].stride(0), t["sem"], t["sem"].stride(0), t["dirs"], t["deltas"], t["ts"], t["rays_a"], t["gt"],
                  t["bg"] if use_bg else None, T(depths), float(lam_dm), float(scene_scale), float(T_thr), int(classes), rows,
                  float(lam_o), float(lam_d), total, vr, o["opacity"], o["depth"], o["rgb"], o["normal"], o["sem"], o["ws"],
                  o["Ro"], o["Rp"], o["terms"], o["d_sig"], o["d_rgb"], ws_)
    torch.cuda.synchronize()
    o["total"], o["vr"] = total, vr
    out = {k: N(v) for k, v in o.items()}
    w = N(ws_)
    out["fit"] = w[12:14].view(np.float32).astype(np.float64)
    out["n_valid"] = int(w[14])
    out["done"] = w[15:17].astype(np.int64)          # workgroups of the fit and of the tail that added their sums
    out["sums"] = w[:12].view(np.float64)
    return out


def against_reference(tag, got, ref, noise, x, cfg, ray_ok=None, smp_ok=None):
    """every output of one launch pair against the restatement (module docstring's bars).  ray_ok / smp_ok: what is
    compared (default: all that a processed row owns).  Prints each figure, then fails with the list of outputs that miss."""
    n_rays = cfg.get("n_rays")
    rows = x["rays_a"][:n_rays]
    n_rows = len(rows)
    ray_own = np.zeros(x["n_rays"], bool)
    ray_own[rows[:, 0]] = True
    row_of, k_of = DR.owned(x, n_rays)
    smp_own = row_of >= 0
    ray_ok = ray_own if ray_ok is None else ray_ok & ray_own
    smp_ok = smp_own if smp_ok is None else smp_ok & smp_own
    everything = ray_ok.sum() == n_rows
    lam_dm = cfg.get("lam_dm", DR.LAMBDA_DM)
    weights = [1.0, 1.0, cfg.get("lam_o", DR.R.LAMBDA_O), cfg.get("lam_d", DR.R.LAMBDA_D), lam_dm]
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
            misses.append(f"{key}: {bad.sum()} of {sel.sum()} miss; worst at {TF.where(x, key, worst // width, n_rays)}: got "
                          f"{g.ravel()[worst]!r}, reference {w.ravel()[worst]!r}, bar {bar.ravel()[worst]:.3g}")

    blocks = (n_rows + 7) // 8
    if got["done"].tolist() != [blocks, blocks]:
        misses.append(f"workspace: {got['done'].tolist()} workgroups counted by the fit and the tail, {blocks} launched each")
    if not np.array_equal(got["total"][ray_ok], ref["total"][ray_ok]):
        i = int(np.nonzero(ray_ok & (got["total"] != ref["total"]))[0][0])
        misses.append(f"total_samples: {TF.where(x, 'total', i, n_rays)}: got {got['total'][i]}, reference {ref['total'][i]}")
    if got["vr"][0] != got["total"][ray_own].sum() or (everything and got["vr"][0] != ref["vr"][0]):
        misses.append(f"vr_samples: got {got['vr'][0]}, sum of total_samples {got['total'][ray_own].sum()}, reference {ref['vr'][0]}")
    for key in PER_RAY + PER_SAMPLE:        # what no processed row owns (the gap, the other rows' rays) keeps its NaN
        own = smp_own if key in PER_SAMPLE else ray_own
        if not np.isnan(got[key][~own]).all():
            misses.append(f"{key}: entries that no processed row owns were written")
    if not (got["total"][~ray_own] == -7).all():
        misses.append("total_samples: entries that no processed row owns were written")
    # everything behind a stop is exactly 0
    stop = ref["stops"][np.maximum(row_of, 0)]
    behind = smp_ok & (stop >= 0) & (k_of > stop)
    for key in ("ws", "d_sig", "d_rgb"):
        if got[key][behind].any() or np.isnan(got[key][behind]).any():
            i = int(np.nonzero(behind)[0][0])
            misses.append(f"{key}: not exactly 0 behind a stop, e.g. {TF.where(x, 'ws', i, n_rays)}")
    # shared with ngp_render_loss_fused: its bars
    for key in ("opacity", "depth", "rgb", "normal", "sem"):
        held(key, got[key], ref[key], TF.FW_ATOL + TF.FW_RTOL * np.abs(ref[key]), ray_ok)
    held("ws", got["ws"], ref["ws"], TF.FW_ATOL + TF.FW_RTOL * np.abs(ref["ws"]), smp_ok)
    for key in ("Ro", "Rp"):
        held(key, got[key], ref[key], max(TF.NOISE_FACTOR * noise[key], TF.FW_ATOL), ray_ok)
    held("d_rgb", got["d_rgb"], ref["d_rgb"], TF.BW_ATOL / n_rows + TF.BW_RTOL * np.abs(ref["d_rgb"]), smp_ok, scale=n_rows)
    # new: 8 x the float32 restatement's error on this batch
    held("d_sig", got["d_sig"], ref["d_sig"], TF.NOISE_FACTOR * noise["d_sig"], smp_ok, scale=n_rows)
    if everything:              # (a, b) depend on every row: compared when no row is borderline
        fit_bar = TF.NOISE_FACTOR * noise["fit"]
        print(f"FIG {tag} fit: got {got['fit']}, |err| {np.abs(got['fit'] - ref['fit'])}, bars {fit_bar}, n_valid {got['n_valid']}")
        for i, nm in enumerate("ab"):
            if not abs(got["fit"][i] - ref["fit"][i]) <= fit_bar[i]:
                misses.append(f"fit {nm}: got {got['fit'][i]!r}, reference {ref['fit'][i]!r}, bar {fit_bar[i]:.3g}")
    if got["n_valid"] != ref["n_valid"]:
        misses.append(f"n_valid: got {got['n_valid']}, reference {ref['n_valid']}")
    assert got["terms"].shape == (5,)
    bars = np.maximum(TF.NOISE_FACTOR * noise["terms"], TF.FW_ATOL * np.array(weights))
    bars[4] = TF.NOISE_FACTOR * noise["terms"][4]
    print(f"FIG {tag} terms: got {got['terms']}, |err| {np.abs(got['terms'] - ref['terms'])}, bars {bars}")
    for i in range(5):
        if not abs(float(got["terms"][i]) - ref["terms"][i]) <= bars[i]:
            misses.append(f"terms[{i}]: got {got['terms'][i]!r}, reference {ref['terms'][i]!r}, bar {bars[i]:.3g}")
    print(f"FIG {tag} float32 noise of the restatement: " + ", ".join(f"{k} {np.max(v):.3g}" for k, v in noise.items()))
    assert not misses, f"{tag}:\n  " + "\n  ".join(misses)


def _kinds_present(x, depths, n_rays=None):
    z = depths[x["rays_a"][:n_rays, 0]]
    assert (z > 0).sum() >= 2 and (z == 0).any() and (z < 0).any() and np.isnan(z).any()


# ------------------------------------------------------------------------------------------- a. crafted edges
@pytest.mark.parametrize("scene_scale", [0.5, 8.0])
@pytest.mark.parametrize("args", ["bg", "nobg-scale"])
@pytest.mark.parametrize("T_thr", [1e-4, 1e-2])
def test_crafted_edges(ngp, T_thr, args, scene_scale):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges (length 0 included), with the gap and the permuted rows; nothing is left out of the comparison"""
    x, depths = batch("crafted"), depths_of("crafted")
    _kinds_present(x, depths)
    cfg = dict(T_thr=T_thr, scene_scale=scene_scale, **{k: v for k, v in TF.ARGS[args].items() if k in ("use_bg", "use_scale")})
    ref, noise = reference("crafted", **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    assert DR.R.comparable(x, T_thr, 1e-2)[0].all()
    assert ref["terms"][4] > 0 and np.abs(ref["g_D"]).max() > 0
    got = run_dep(ngp, x, depths, **cfg)
    against_reference(f"crafted T_thr={T_thr} {args} scale={scene_scale}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- b. random batches
@pytest.mark.parametrize("name,scene_scale", [("300", 0.5), ("1500", 8.0)])
def test_random_batch(ngp, name, scene_scale):
    """the random batches of tests/test_fused_tail_gpu.py, under its rule for borderline rays (within 1e-3 of T_threshold in
    float64: left out of the per-ray and per-sample comparisons, at most MAX_BORDERLINE of the batch; the loss terms are
    compared all the same, (a, b) when no ray is borderline)"""
    x, depths = batch(name), depths_of(name)
    _kinds_present(x, depths)
    cfg = dict(scene_scale=scene_scale)
    ok, ray_ok, smp_ok = DR.comparable(x, 1e-4, 1e-3)
    left_out = 1.0 - ok.mean()
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}")
    assert left_out <= DR.MAX_BORDERLINE
    ref, noise = reference(name, **cfg)
    got = run_dep(ngp, x, depths, **cfg)
    print(f"FIG random-{name} fit: got {got['fit']}, reference {ref['fit']}, float32 restatement's error {noise['fit']}")
    against_reference(f"random-{name} scale={scene_scale}", got, ref, noise, x, cfg, ray_ok, smp_ok)


# ------------------------------------------------------------------------------------------- c. block edges
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8), a
    second workgroup with one ray (9); the seeds scale with 1 / rows.  One row is the singular system: (a, b) = (0, 0)
    exactly.  Everything that belongs to the other rows is left alone."""
    x, depths = batch("crafted"), depths_of("crafted")
    if rows > 6:
        _kinds_present(x, depths, rows)
    cfg = dict(n_rays=rows)
    ref, noise = reference("crafted", **cfg)
    got = run_dep(ngp, x, depths, **cfg)
    if rows == 1:
        assert ref["n_valid"] == 1 and got["fit"].tolist() == [0.0, 0.0] and ref["terms"][4] > 0
    against_reference(f"crafted rows={rows}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- d. layouts, the workspace
def test_memset_branches_and_garbage_in_the_workspace(ngp):
    """terms, vr_samples and the workspace adjacent as rendering._RenderLossFn lays them out (one fill) and in separate
    allocations (three fills), the workspace starting as -5, as all bits set and as a large positive pattern: the entry
    clears it, so the four launches agree bit for bit and with the restatement"""
    x, depths = batch("crafted"), depths_of("crafted")
    runs = [("adjacent", run_dep(ngp, x, depths, adjacent=True)),
            ("separate", run_dep(ngp, x, depths, adjacent=False)),
            ("adjacent all-ones", run_dep(ngp, x, depths, adjacent=True, garbage=-1)),
            ("separate 0x7f7f7f7f", run_dep(ngp, x, depths, adjacent=False, garbage=0x7F7F7F7F))]
    ref, noise = reference("crafted")
    a = runs[0][1]
    for tag, got in runs:
        TF._same_launch(a, got, 4, keys=[k for k in a if k not in ("terms", "sums", "fit", "n_valid")])
        assert got["n_valid"] == a["n_valid"]
        # (the five sums are doubles added in arrival order: (a, b) within an ulp, the term rounded once)
        np.testing.assert_allclose(got["fit"], a["fit"], rtol=2.0 ** -23, atol=0)
        np.testing.assert_allclose(got["terms"][4], a["terms"][4], rtol=2.0 ** -23, atol=0)
        assert got["vr"][0] == ref["vr"][0]
        against_reference(f"crafted memset {tag}", got, ref, noise, x, {})


# ------------------------------------------------------------------------------------------- e. no depth at all
@pytest.mark.parametrize("kind", ["none", "one"])
def test_batch_without_a_fit(ngp, kind):
    """no ray with a valid depth (0, negative, NaN in turn), and one alone: (a, b) = (0, 0) exactly, d_sigmas is the default
    entry's bit for bit, the term exactly 0 without a valid ray, and everything finite"""
    x, depths = batch("crafted"), depths_of("crafted", kind)
    got = run_dep(ngp, x, depths)
    plain = TF.run_tail(ngp, x)
    own = DR.owned(x)[0] >= 0
    assert got["fit"].tolist() == [0.0, 0.0] and got["n_valid"] == (0 if kind == "none" else 1)
    assert np.isfinite(got["terms"]).all() and np.isfinite(got["d_sig"][own]).all()
    assert np.array_equal(got["d_sig"], plain["d_sig"], equal_nan=True)
    if kind == "none":
        assert got["terms"][4] == 0.0
    ref, noise = reference("crafted", kind)
    against_reference(f"crafted depths: {kind}", got, ref, noise, x, {})


# ------------------------------------------------------------------------------------------- f. the existing tail
@pytest.mark.parametrize("name", ["crafted", "1500"])
def test_depth_and_zero_weight_give_the_existing_tail(ngp, name):
    """`depth` is ngp_render_loss_fused's bit for bit at any weight.  lambda_dm = 0: every output this entry shares with
    ngp_render_loss_fused equals that entry's on the same inputs bit for bit; the loss terms bit for bit when one workgroup
    forms them (the first 8 rows), else within the reordering of one float atomic per workgroup"""
    x, depths = batch(name), depths_of(name)
    full = run_dep(ngp, x, depths, scene_scale=0.5)
    assert np.array_equal(full["depth"], TF.run_tail(ngp, x)["depth"], equal_nan=True)
    for n_rays, blocks in ((None, len(x["rays_a"]) // 8 + 1), (8, 1)):
        a = run_dep(ngp, x, depths, lam_dm=0.0, n_rays=n_rays)
        b = TF.run_tail(ngp, x, n_rays=n_rays)
        for key in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "ws", "d_sig", "d_rgb"):
            assert np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (key, n_rays)
        if blocks == 1:
            assert np.array_equal(a["terms"][:4], b["terms"])
        else:
            np.testing.assert_allclose(a["terms"][:4], b["terms"], rtol=blocks * TF.REORDER, atol=0)
        assert a["terms"][4] == 0.0
        assert a["n_valid"] > 0 and a["fit"][0] != 0          # the fit ran all the same


def test_argument_checks(ngp):
    """the wrapper raises on what the entry refuses: more than 8 classes, a scene scale of 0, a misaligned workspace, a
    missing target"""
    x, depths = batch("crafted"), depths_of("crafted")
    with pytest.raises(RuntimeError):
        run_dep(ngp, x, depths, classes=9)
    with pytest.raises(RuntimeError):
        run_dep(ngp, x, depths, scene_scale=0.0)
    with pytest.raises(RuntimeError):
        run_dep(ngp, x, depths, scene_scale=-1.0)
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt")}
    n, R_ = x["n"], x["n_rays"]
    E = lambda *s: torch.empty(*s, device=DEV)
    acc = E(9 + WS_INTS)
    total = torch.empty(R_, dtype=torch.int64, device=DEV)

    def call(depth_t, ws_):
        ngp._lib.call("render_loss_fused_dep", t["sig"], t["rgbs"], t["dsig"], None, t["nrm"], 3, t["sem"], 8, t["dirs"],
                      t["deltas"], t["ts"], t["rays_a"], t["gt"], None, depth_t, 1.0, 1.0, 1e-4, 7, R_, 2e-4, 3e-4, total,
                      acc[6:8].view(torch.int64), E(R_), E(R_), E(R_, 3), E(R_, 3), E(R_, 7), E(n), E(R_), E(R_, 3), acc[:5],
                      E(n), E(n, 3), ws_)
    good = acc[8:8 + WS_INTS].view(torch.int32)
    call(T(depths), good)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        call(None, good)
    with pytest.raises(RuntimeError):
        call(T(depths), None)
    with pytest.raises(RuntimeError):
        call(T(depths), acc[9:9 + WS_INTS].view(torch.int32))          # 4 bytes off an 8-byte boundary


# ------------------------------------------------------------------------------------------- g. autograd
def _close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _grid_buffers(model):
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    return model


def _mono_depths(scene, o, d):
    """the scene's depths as a monocular map: 25 (0.37 D + 0.11) where the ray has one, 0 (invalid) elsewhere; no NaN, which
    the module route would carry into its loss"""
    D = scene.ground_truth_depths(o, d, n_quad=64)
    dep = torch.where(D > 0, 25.0 * (0.37 * D + 0.11), torch.zeros_like(D))
    assert 0.02 < float((dep > 0).float().mean()) < 0.98
    return dep.contiguous()


def test_wrapper_hands_back_the_direct_call(ngp):
    """rendering._RenderLossFn with the packed depth_mono term on the crafted batch: the outputs are those of the direct call, and back-propagating
    terms[0] with a unit seed hands back the launch's d_sigmas and d_rgbs bit for bit"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x, depths = batch("crafted"), depths_of("crafted")
    direct = run_dep(ngp, x, depths, use_scale=True, scene_scale=0.5)
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3")}
    sig, rgbs = t["sig"].requires_grad_(True), t["rgbs"].requires_grad_(True)
    args = (sig, rgbs, t["sem"], t["nrm"], None, t["dsig"], t["dirs"], t["deltas"], t["ts"], t["rays_a"])
    tail = FusedTail(t["gt"], DR.R.LAMBDA_O, DR.R.LAMBDA_D, terms={"depth_mono": (T(depths), DR.LAMBDA_DM, 0.5)}, packed=True)
    outs = _RenderLossFn.apply(*args, tail, t["scale3"], 1e-4, 7, t["bg"])
    terms = outs[0]
    assert terms.shape == (5,) and terms.requires_grad and not any(o.requires_grad for o in outs[1:] if o is not None)
    seed = torch.zeros_like(terms)
    seed[0] = 1.0
    torch.autograd.backward([terms], [seed])
    own = DR.owned(x)[0] >= 0
    got = dict(zip(("terms", "total", "vr", "opacity", "depth", "rgb", "normal", "sem", "ws", "Ro", "Rp"), (N(o) for o in outs)))
    for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp"):
        assert np.array_equal(got[k], direct[k]), k
    np.testing.assert_allclose(got["terms"], direct["terms"], rtol=4 * TF.REORDER, atol=0)
    fit = N(outs[11])[12:14].view(np.float32)
    np.testing.assert_allclose(fit, direct["fit"], rtol=2.0 ** -23, atol=0)
    if np.array_equal(fit.astype(np.float64), direct["fit"]):          # the same (a, b): the same gradients bit for bit
        assert np.array_equal(N(sig.grad)[own], direct["d_sig"][own])
    else:
        np.testing.assert_allclose(N(sig.grad)[own], direct["d_sig"][own], rtol=1e-6, atol=1e-12)
    assert np.array_equal(N(rgbs.grad)[own], direct["d_rgb"][own])
    for bad in (T(depths)[:5], T(depths).double(), T(depths).reshape(-1, 1)):
        with pytest.raises(ValueError):
            _RenderLossFn.apply(*args, FusedTail(t["gt"], 0.0, 0.0, terms={"depth_mono": (bad, 0.0, 1.0)}, packed=True),
                                t["scale3"], 1e-4, 7, None)


def test_fused_depth_tail_matches_the_launch_per_operation_route(ngp):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background
    draw on both routes.  A: render + NeRFLoss(depth_mono=True, scale=8) + sum of means + autograd; B: render with
    _fused_loss=FusedTail(..., terms={'depth_mono': ...}, packed=True) through rendering._RenderLossFn.  The bars of the
    semantic and normal counterparts: terms rtol 1e-4, parameter gradients within 3e-4 of the largest entry."""
    from ngp_amd.losses import NeRFLoss
    from ngp_amd.rendering import FusedTail, render
    from ngp_amd.synthetic import LegoProxy
    torch.manual_seed(33)
    model = _grid_buffers(ngp.networks.NGP(scale=8.0).to(DEV))
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.5)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    scene = LegoProxy(n_images=6, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(34)
    img, pix = scene.sample_batch(1500, generator=gen)
    o, d = scene.rays(img, pix)
    gt = torch.rand(1500, 3, device=DEV, generator=gen)
    depths = _mono_depths(scene, o, d)
    loss_fn = NeRFLoss()
    lam = (loss_fn.lambda_opa, loss_fn.lambda_distortion, loss_fn.lambda_depth_mono)
    named = [(n, p) for n, p in model.named_parameters() if p.numel() > 0]
    out = {}
    for fused in (False, True):
        for _, p in named:
            p.grad = None
        torch.manual_seed(35)
        kw = dict(exp_step_factor=1 / 256, random_bg=True)
        if fused:
            tail = FusedTail(gt, lam[0], lam[1], terms={"depth_mono": (depths, lam[2], 8.0)}, packed=True)
            res = render(model, o, d, _fused_loss=tail, **kw)
            assert "_loss_terms" in res
            terms = res.pop("_loss_terms")
            assert terms.shape == (5,) and terms.requires_grad
            torch.autograd.backward([terms], [torch.tensor([1.0, 0, 0, 0, 0], device=DEV)])
            terms = N(terms)
        else:
            res = render(model, o, d, **kw)
            ld = loss_fn(res, {"rgb": gt, "depth": depths}, depth_mono=True, scale=8.0)
            loss = sum(t.mean() for t in ld.values())
            loss.backward()
            terms = np.array([float(loss.detach())] + [float(ld[n].detach().mean()) for n in
                                                        ("rgb", "opacity", "distortion", "depth_mono")], np.float32)
        out[fused] = (res, terms, {n: None if p.grad is None else N(p.grad).copy() for n, p in named})
    ra, ta, ga = out[False]
    rb, tb, gb = out[True]
    assert int(ra["total_samples"]) == int(rb["total_samples"]) > 0
    for key in ("opacity", "depth", "rgb", "normal_pred", "semantic", "ws", "Ro", "Rp"):
        _close(N(rb[key]), N(ra[key]), 2e-5, 2e-6)
    print("FIG autograd terms A", ta, "terms B", tb)
    _close(tb, ta, 1e-4, 1e-9)
    assert tb[4] > 0
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


# ------------------------------------------------------------------------------------------- h. the trainer
def test_trainer_depth_route_matches_module_route(ngp):
    """NGPTrainer(depth_mono=True) with step(depths=) follows the trajectory of NGPTrainer(loss_kwargs={'depth_mono': True,
    'scale': 0.5}) with step(target={'depth': ...}) for six steps of 1024 rays at lr = TRAJ_LR (test_normal_tail_gpu.py says
    why not 1e-2), within the bars of the semantic and normal counterparts: losses rtol 1e-3, parameters rtol 5e-3 / atol
    5e-5.  The fused route keeps the norm-bound clip (the term reaches the parameters through d_sigmas alone)."""
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=10, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(51)
    batches = []
    for i in range(6):
        img, pix = scene.sample_batch(1024, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        batches.append((o, d, gt, _mono_depths(scene, o, d)))
    out = []
    for fused in (True, False):
        torch.manual_seed(52)
        model = _grid_buffers(ngp.networks.NGP(scale=0.5).to(DEV))
        kw = dict(depth_mono=True) if fused else dict(loss_kwargs={"depth_mono": True, "scale": 0.5})
        tr = NGPTrainer(model, lr=TRAJ_LR, **kw)
        assert tr.fused_loss == fused and tr.depth_mono == fused
        torch.manual_seed(53)
        if fused:
            steps = [tr.step(o, d, gt, depths=dep) for o, d, gt, dep in batches]
            assert all(s[1]["loss_terms"].shape == (5,) for s in steps)
            dm = [float(s[1]["loss_terms"][4]) for s in steps]
            print("FIG trainer depth_mono term per step", dm)
            assert all(v > 0 for v in dm)
        else:
            steps = [tr.step(o, d, gt, target={"depth": dep}) for o, d, gt, dep in batches]
        losses = [float(s[0]) for s in steps]
        tr.wait()
        out.append((losses, N(model.xyz_net[0].weight).copy(), N(model.rgb_net.params).copy(),
                    N(model.xyz_encoder.params).copy()))
    print("FIG trainer losses fused", out[0][0], "module", out[1][0])
    _close(np.array(out[0][0]), np.array(out[1][0]), 1e-3, 1e-7)
    for k in (1, 2, 3):
        print(f"FIG trainer params[{k}]: max|diff| {np.abs(out[0][k] - out[1][k]).max():.3g}")
        _close(out[0][k], out[1][k], 5e-3, 5e-5)


def test_trainer_depth_argument_checks(ngp):
    """every combination the depth tail does not cover raises ValueError; the route combines with appearance codes and a
    random background; a batch without a valid depth trains on; a model that leaves the fused tail makes step() raise"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=4, img_wh=(20, 20), device=DEV)
    make = lambda **kw: _grid_buffers(ngp.networks.NGP(scale=0.5, **kw).to(DEV))
    model = make()              # (a refused construction leaves the model as it was: one model serves them all)
    refused = [dict(msk_model=implicit_mask().to(DEV)),
               dict(pose_refiner=PoseRefiner(scene.poses, scene.directions).to(DEV)),
               dict(semantic=True), dict(normal_mono=True), dict(render_kwargs={"use_skybox": True}),
               dict(loss_kwargs={"normal_mono": True}), dict(loss_kwargs={"semantic": True}),
               dict(loss_kwargs={"depth_mono": True}), dict(loss_kwargs={"normal_ref": True})]
    for kw in refused:
        with pytest.raises(ValueError):
            NGPTrainer(model, depth_mono=True, **kw)
    assert model.differentiable_normals is False
    for model_kw in (dict(rgb_act="None"), dict(use_skybox=True)):
        with pytest.raises(ValueError):
            NGPTrainer(make(**model_kw), depth_mono=True)
    img, pix = scene.sample_batch(64)
    o, d = scene.rays(img, pix)
    gt = torch.rand(64, 3, device=DEV)
    some = 25 * (0.2 + torch.rand(64, device=DEV))
    some[::5] = float("nan")
    plain = NGPTrainer(model)
    with pytest.raises(ValueError):
        plain.step(o, d, gt, depths=some)
    model = make(embed_a=True, embed_a_len=4)
    emb = torch.nn.Embedding(4, 4).to(DEV)
    tr = NGPTrainer(model, depth_mono=True, embedding_a=emb, exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img)
    for bad in (some[:5], some.reshape(-1, 1), some.to(torch.int64)):
        with pytest.raises(ValueError):
            tr.step(o, d, gt, img_idxs=img, depths=bad)
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, depths=some, target={"depth": None})
    loss, res = tr.step(o, d, gt, depths=torch.zeros(64, device=DEV), img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all() and float(res["loss_terms"][4]) == 0.0
    loss, res = tr.step(o, d, gt, depths=some, img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all() and res["loss_terms"].shape == (5,)
    # a model that leaves the fused tail after construction is an error, not a step on the default loss without depths
    model.differentiable_normals = True
    with pytest.raises(RuntimeError):
        tr.step(o, d, gt, depths=some, img_idxs=img)
    model.differentiable_normals = False


# ------------------------------------------------------------------------------------------- i. end to end
def _tool(args, timeout):
    """tools/train_dataset.py in a child process with its own time limit -> its last JSON line"""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_dataset.py")] + args, capture_output=True,
                         text=True, timeout=timeout)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def test_train_dataset_with_depths_end_to_end(ngp, tmp_path):
    """the tool in a child process: the proxy scene with monocular depth maps in the tnt layout (34 views of 80 x 80, every
    8th held out, the files 25 (0.37 D + 0.11)), 600 steps of 2048 rays with --depth_mono.  The JSON keys exist and are
    finite, the loss had five terms and the depth_mono term (mean of the last ten steps) ends below where it began (mean of
    the first ten).  Held-out PSNR and depth_absrel of that run and of a second one with --lambda_depth_mono 0 on the same
    files are recorded (FIG lines, profiles/depth_mono.txt), not barred."""
    root = str(tmp_path / "scene")
    common = ["--dataset_name", "tnt", "--num_epochs", "3", "--steps_per_epoch", "200", "--batch_size", "2048", "--depth_mono"]
    out = _tool(["--make_proxy", root, "--downsample", "0.1", "--proxy_views", "34"] + common, 300)
    assert len(os.listdir(os.path.join(root, "depth"))) == 34
    for key in ("test_psnr_mean", "test_ssim_mean", "test_depth_absrel_mean", "depth_mono_term_first", "depth_mono_term_last"):
        assert key in out and np.isfinite(out[key]), (key, out.get(key))
    assert out["steps"] == 600 and out["img_wh"] == [80, 80] and out["loss_terms"] == 5 and out["lambda_depth_mono"] == 1
    assert len(out["test_depth_absrel"]) == len(out["test_psnr"]) == 5 and np.isfinite(out["test_depth_absrel"]).all()
    print(f"FIG end-to-end lambda 1: psnr {out['test_psnr_mean']:.2f} dB (per image {out['test_psnr']}), depth_absrel mean "
          f"{out['test_depth_absrel_mean']:.4f} (per image {out['test_depth_absrel']}), depth_mono term "
          f"{out['depth_mono_term_first']:.3g} -> {out['depth_mono_term_last']:.3g}")
    assert 0 < out["depth_mono_term_last"] < out["depth_mono_term_first"]
    zero = _tool(["--root_dir", root, "--lambda_depth_mono", "0"] + common, 300)
    print(f"FIG end-to-end lambda 0: psnr {zero['test_psnr_mean']:.2f} dB (per image {zero['test_psnr']}), depth_absrel mean "
          f"{zero['test_depth_absrel_mean']:.4f} (per image {zero['test_depth_absrel']})")
    assert zero["loss_terms"] == 5 and zero["lambda_depth_mono"] == 0 and zero["depth_mono_term_last"] == 0.0
