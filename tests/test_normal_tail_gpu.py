"""The normal_mono form of the fused render + loss tail on the GPU (render_loss_fused_kernel<8, 32, false, false, true>
behind ngp_render_loss_fused_nrm) against the float64 restatement of tests/normal_tail_reference.py, and the routes
built on it: rendering._RenderLossFn, NGPTrainer(normal_mono=True), tools/train_dataset.py --normal_mono.

Bars.  The outputs this entry shares with ngp_render_loss_fused keep tests/test_fused_tail_gpu.py's bars: opacity, depth,
rgb, normal_pred, semantic, ws rtol 2e-5, atol 2e-6; d_sigmas, d_rgbs rtol 2e-4, atol 2e-5 / n_rays; Ro, Rp and
terms[0:4] 8 times the float32 restatement's own error on the same inputs, not below 2e-6 (times the term's weight).
d_normal_head and terms[4] are held to 8 times the float32 restatement's error as well, with the floor 2e-5 / n_rays
times lambda_nm.  Each case runs at NeRFLoss's weight (1e-3) and at lambda_nm = 1.  No ray is left out of a comparison
for the jump of sign(N^ - g^): the targets keep every component 1e-3 away from it by construction
(normal_tail_reference.make_normals).  Every figure is printed (FIG lines) before it is asserted; the measured maxima
are in profiles/normal_tail.txt.

Measured on one MI355X, end to end (test_train_dataset_with_normals_end_to_end, profiles/normal_mono.txt): held-out PSNR
27.35 dB and 13.0 degrees with lambda_normal_mono = 1e-3, 23.61 dB and 101.6 degrees with 0 (max - min 53.2 degrees)."""
import os
import sys

import numpy as np
import pytest
import torch

import normal_tail_reference as NR
import test_fused_tail_gpu as TF

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N = TF.T, TF.N
WEIGHTS = {"nerfloss": NR.LAMBDA_NM, "unit": 1.0}
PER_RAY = TF.PER_RAY
PER_SAMPLE = TF.PER_SAMPLE + ("d_np",)

TRAJ_LR = 3e-4          # learning rate of the six-step trajectory comparison: see that test
_NORMALS, _STATE, _REF = {}, {}, {}
batch = TF.batch


def normals_of(name, kind="mixed"):
    """the batch's seeded targets, computed once: 'mixed' (a fifth of the rows zero) or 'none' (all zero)"""
    key = (name, kind)
    if key not in _NORMALS:
        x = batch(name)
        _NORMALS[key] = NR.make_normals(x) if kind == "mixed" else np.zeros((x["n_rays"], 3), np.float32)
        _NORMALS[key].setflags(write=False)
    return _NORMALS[key]


def reference(name, kind="mixed", **cfg):
    """(float64 restatement, its float32 noise): computed once per (batch, targets, arguments), shared, read-only; the
    per-ray part (render) is shared between the cases that differ only in the loss's arguments"""
    key = (name, kind) + tuple(sorted(cfg.items()))
    if key not in _REF:
        x, normals = batch(name), normals_of(name, kind)
        rkw = {k: v for k, v in cfg.items() if k in NR.R.RENDER_KEYS}
        fkw = {k: v for k, v in cfg.items() if k not in NR.R.RENDER_KEYS}
        rkey = (name,) + tuple(sorted(rkw.items()))
        if rkey not in _STATE:
            hi = NR.R.render(x, **rkw)
            _STATE[rkey] = (hi, NR.R.render(x, dtype=torch.float32, stops=hi["stops"], **rkw))
        hi, lo = _STATE[rkey]
        ref = NR.finish(hi, x, normals, **fkw)
        _REF[key] = (ref, NR.noise_of(NR.finish(lo, x, normals, **fkw), ref))
    return _REF[key]


def run_nrm(ngp, x, normals, T_thr=1e-4, classes=7, lam_o=NR.R.LAMBDA_O, lam_d=NR.R.LAMBDA_D, lam_nm=NR.LAMBDA_NM,
            use_bg=True, use_scale=False, n_rays=None, ld=None, adjacent=True):
    """one direct call of ngp_render_loss_fused_nrm on the first n_rays rows (default: all), every output pre-filled with
    NaN (the counts with negative numbers, the workspace with -5); per-ray buffers have one entry per ray of the batch"""
    rows = len(x["rays_a"]) if n_rays is None else n_rays
    NR_, n = x["n_rays"], x["n"]
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3")}
    nrm, sem = t["nrm"], t["sem"]
    if ld is not None:          # the two heads as the leading columns of wider matrices whose other columns hold NaN
        wide = torch.full((2, n, ld), float("nan"), device=DEV)
        wide[0, :, :3], wide[1, :, :sem.shape[1]] = nrm, sem
        nrm, sem = wide[0], wide[1]
    E = lambda *s: torch.full(s, float("nan"), device=DEV)
    total = torch.full((NR_,), -7, dtype=torch.int64, device=DEV)
    if adjacent:                # rendering.TAIL_LAYOUT['nrm']: one buffer, one memset
        acc = E(12)
        terms, vr, ws_ = acc[:5], acc[6:8].view(torch.int64), acc[8:12].view(torch.int32)
    else:
        terms, vr = E(5), torch.full((1,), -(2 ** 40) - 3, dtype=torch.int64, device=DEV)
        ws_ = torch.full((4,), -5, dtype=torch.int32, device=DEV)
        assert vr.data_ptr() != terms.data_ptr() + 24 and ws_.data_ptr() != terms.data_ptr() + 32
    o = dict(opacity=E(NR_), depth=E(NR_), rgb=E(NR_, 3), normal=E(NR_, 3), sem=E(NR_, classes), ws=E(n), Ro=E(NR_),
             Rp=E(NR_, 3), terms=terms, d_sig=E(n), d_rgb=E(n, 3), d_np=E(n, 3))
    ngp._lib.call("render_loss_fused_nrm", t["sig"], t["rgbs"], t["dsig"], t["scale3"] if use_scale else None, nrm,
                  nrm.stride(0), sem, sem.stride(0), t["dirs"], t["deltas"], t["ts"], t["rays_a"], t["gt"],
                  t["bg"] if use_bg else None, T(normals), float(lam_nm), float(T_thr), int(classes), rows, float(lam_o),
                  float(lam_d), total, vr, o["opacity"], o["depth"], o["rgb"], o["normal"], o["sem"], o["ws"], o["Ro"], o["Rp"],
                  o["terms"], o["d_sig"], o["d_rgb"], ws_, o["d_np"])
    torch.cuda.synchronize()
    o["total"], o["vr"] = total, vr
    out = {k: N(v) for k, v in o.items()}
    out["done"] = N(ws_)[2:3].astype(np.int64)          # workgroups that added their sum
    return out


def against_reference(tag, got, ref, noise, x, cfg, ray_ok=None, smp_ok=None):
    """every output of one launch against the restatement (module docstring's bars).  ray_ok / smp_ok: what is compared
    (default: all that a processed row owns).  Prints each figure, then fails with the list of outputs that miss."""
    n_rays = cfg.get("n_rays")
    rows = x["rays_a"][:n_rays]
    n_rows = len(rows)
    ray_own = np.zeros(x["n_rays"], bool)
    ray_own[rows[:, 0]] = True
    smp_own = NR.owned(x, n_rays)[0] >= 0
    ray_ok = ray_own if ray_ok is None else ray_ok & ray_own
    smp_ok = smp_own if smp_ok is None else smp_ok & smp_own
    everything = ray_ok.sum() == n_rows
    lam_nm = cfg.get("lam_nm", NR.LAMBDA_NM)
    weights = [1.0, 1.0, cfg.get("lam_o", NR.R.LAMBDA_O), cfg.get("lam_d", NR.R.LAMBDA_D), lam_nm]
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
            what = "d_sig" if key == "d_np" else key
            misses.append(f"{key}: {bad.sum()} of {sel.sum()} miss; worst at {TF.where(x, what, worst // width, n_rays)}: got "
                          f"{g.ravel()[worst]!r}, reference {w.ravel()[worst]!r}, bar {bar.ravel()[worst]:.3g}")

    if got["done"][0] != (n_rows + 7) // 8:
        misses.append(f"workspace: {got['done'][0]} workgroups counted, {(n_rows + 7) // 8} launched")
    if not np.array_equal(got["total"][ray_ok], ref["total"][ray_ok]):
        i = int(np.nonzero(ray_ok & (got["total"] != ref["total"]))[0][0])
        misses.append(f"total_samples: {TF.where(x, 'total', i, n_rays)}: got {got['total'][i]}, reference {ref['total'][i]}")
    if got["vr"][0] != got["total"][ray_own].sum() or (everything and got["vr"][0] != ref["vr"][0]):
        misses.append(f"vr_samples: got {got['vr'][0]}, sum of total_samples {got['total'][ray_own].sum()}, reference {ref['vr'][0]}")
    for key in PER_RAY + PER_SAMPLE:        # what no processed row owns is left alone
        own = smp_own if key in PER_SAMPLE else ray_own
        if not np.isnan(got[key][~own]).all():
            misses.append(f"{key}: entries that no processed row owns were written")
    if not (got["total"][~ray_own] == -7).all():
        misses.append("total_samples: entries that no processed row owns were written")
    # shared with ngp_render_loss_fused: its bars
    for key in ("opacity", "depth", "rgb", "normal", "sem"):
        held(key, got[key], ref[key], TF.FW_ATOL + TF.FW_RTOL * np.abs(ref[key]), ray_ok)
    held("ws", got["ws"], ref["ws"], TF.FW_ATOL + TF.FW_RTOL * np.abs(ref["ws"]), smp_ok)
    for key in ("Ro", "Rp"):
        held(key, got[key], ref[key], max(TF.NOISE_FACTOR * noise[key], TF.FW_ATOL), ray_ok)
    for key in ("d_sig", "d_rgb"):
        held(key, got[key], ref[key], TF.BW_ATOL / n_rows + TF.BW_RTOL * np.abs(ref[key]), smp_ok, scale=n_rows)
    # new: 8 x the float32 restatement's error, floor 2e-5 / n_rays x lambda_nm
    held("d_np", got["d_np"], ref["d_np"], max(TF.NOISE_FACTOR * noise["d_np"], TF.BW_ATOL / n_rows * lam_nm), smp_ok,
         scale=n_rows)
    # exactly zero: behind the stop, without weight, on a ray without a target
    dead = smp_ok & ((np.nan_to_num(ref["ws"]) == 0) | ~ref["has"][np.maximum(NR.owned(x, n_rays)[0], 0)])
    if got["d_np"][dead].any() or np.isnan(got["d_np"][dead]).any():
        misses.append(f"d_np: {int((got['d_np'][dead] != 0).any(1).sum())} samples without weight or target are not exactly 0")
    assert got["terms"].shape == (5,)
    bars = np.maximum(TF.NOISE_FACTOR * noise["terms"], TF.FW_ATOL * np.array(weights))
    bars[4] = max(TF.NOISE_FACTOR * noise["terms"][4], TF.BW_ATOL / n_rows * lam_nm)
    print(f"FIG {tag} terms: got {got['terms']}, |err| {np.abs(got['terms'] - ref['terms'])}, bars {bars}")
    for i in range(5):
        if not abs(float(got["terms"][i]) - ref["terms"][i]) <= bars[i]:
            misses.append(f"terms[{i}]: got {got['terms'][i]!r}, reference {ref['terms'][i]!r}, bar {bars[i]:.3g}")
    print(f"FIG {tag} float32 noise of the restatement: " + ", ".join(f"{k} {np.max(v):.3g}" for k, v in noise.items()))
    assert not misses, f"{tag}:\n  " + "\n  ".join(misses)


def _zeros_present(x, normals, n_rays=None):
    g = normals[x["rays_a"][:n_rays, 0]]
    zero = ~(g != 0).any(1)
    assert zero.any() and (~zero).any()


# ------------------------------------------------------------------------------------------- a. crafted edges
@pytest.mark.parametrize("use_scale", [False, True])
@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_crafted_edges(ngp, weights, use_scale):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges (length 0 included), with the gap and the permuted rows; nothing is left out of the comparison"""
    x, normals = batch("crafted"), normals_of("crafted")
    _zeros_present(x, normals)
    cfg = dict(lam_nm=WEIGHTS[weights], use_scale=use_scale)
    ref, noise = reference("crafted", **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    assert NR.sign_margin(x, normals) >= NR.SIGN_MARGIN
    assert ref["terms"][4] > 0 and np.nanmax(np.abs(ref["d_np"])) > 0
    got = run_nrm(ngp, x, normals, **cfg)
    against_reference(f"crafted {weights} scale3={use_scale}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- b. random batches
@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("name", ["300", "1500"])
def test_random_batch(ngp, name, weights):
    """the random batches of tests/test_fused_tail_gpu.py, under its rule for borderline rays (within 1e-3 of
    T_threshold in float64: left out of the per-ray and per-sample comparisons, at most MAX_BORDERLINE of the batch; the
    loss terms are compared all the same).  No ray is left out for the sign's jump."""
    x, normals = batch(name), normals_of(name)
    _zeros_present(x, normals)
    cfg = dict(lam_nm=WEIGHTS[weights])
    ok, ray_ok, smp_ok = NR.comparable(x, 1e-4, 1e-3)
    left_out = 1.0 - ok.mean()
    margin = NR.sign_margin(x, normals)
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}, rays left out for the "
          f"sign's jump 0 (smallest |N^ - g^| component {margin:.3g})")
    assert left_out <= NR.MAX_BORDERLINE and margin >= NR.SIGN_MARGIN
    ref, noise = reference(name, **cfg)
    got = run_nrm(ngp, x, normals, **cfg)
    against_reference(f"random-{name} {weights}", got, ref, noise, x, cfg, ray_ok, smp_ok)


# ------------------------------------------------------------------------------------------- c. block edges
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8),
    a second workgroup with one ray (9); the seeds scale with 1 / rows.  Everything that belongs to the other rows is
    left alone."""
    x, normals = batch("crafted"), normals_of("crafted")
    if rows > 2:
        _zeros_present(x, normals, rows)
    cfg = dict(n_rays=rows, lam_nm=1.0)
    ref, noise = reference("crafted", **cfg)
    got = run_nrm(ngp, x, normals, **cfg)
    against_reference(f"crafted rows={rows}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- d. layouts
def test_wide_normal_rows(ngp):
    """normal_head (and sem_logits) as the leading columns of 20-wide matrices whose other columns hold NaN: d_normal_head
    stays dense (n, 3) and every output is that of the dense call, bit for bit"""
    x, normals = batch("crafted"), normals_of("crafted")
    cfg = dict(use_scale=True, lam_nm=1.0)
    a = run_nrm(ngp, x, normals, **cfg)
    b = run_nrm(ngp, x, normals, ld=20, **cfg)
    assert np.isfinite(a["terms"]).all() and b["d_np"].shape == (x["n"], 3)
    TF._same_launch(a, b, 4)


def test_memset_branches(ngp):
    """terms, vr_samples and the workspace adjacent as rendering._RenderLossFn lays them out (one fill) and in separate
    allocations (three fills), all pre-filled with NaN / negative numbers"""
    x, normals = batch("crafted"), normals_of("crafted")
    a = run_nrm(ngp, x, normals, adjacent=True)
    b = run_nrm(ngp, x, normals, adjacent=False)
    TF._same_launch(a, b, 4)
    assert a["terms"][4] == b["terms"][4]          # rounded once: no dependence on the order of the workgroups
    ref, noise = reference("crafted")
    for tag, got in (("adjacent", a), ("separate", b)):
        assert got["vr"][0] == ref["vr"][0]
        against_reference(f"crafted memset {tag}", got, ref, noise, x, {})


# ------------------------------------------------------------------------------------------- e. no target at all
def test_batch_without_a_normal(ngp):
    """every target (0, 0, 0): the term is exactly 0, d_normal_head exactly 0 where a row owns the sample, everything
    finite, and the rest as the restatement"""
    x, normals = batch("crafted"), normals_of("crafted", "none")
    cfg = dict(lam_nm=1.0)
    got = run_nrm(ngp, x, normals, **cfg)
    own = NR.owned(x)[0] >= 0
    assert got["terms"][4] == 0.0 and np.isfinite(got["terms"]).all()
    assert not got["d_np"][own].any() and not np.isnan(got["d_np"][own]).any()
    assert np.isfinite(got["d_sig"][own]).all() and np.isfinite(got["d_rgb"][own]).all()
    ref, noise = reference("crafted", "none", **cfg)
    against_reference("crafted no target", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- f. the existing tail
@pytest.mark.parametrize("name", ["crafted", "1500"])
def test_zero_weight_gives_the_existing_tail(ngp, name):
    """lambda_nm = 0: every output this entry shares with ngp_render_loss_fused equals that entry's on the same inputs bit
    for bit; the loss terms bit for bit when one workgroup forms them (the first 8 rows), else within the reordering of
    one float atomic per workgroup"""
    x, normals = batch(name), normals_of(name)
    own = NR.owned(x)[0] >= 0
    for n_rays, blocks in ((None, len(x["rays_a"]) // 8 + 1), (8, 1)):
        a = run_nrm(ngp, x, normals, lam_nm=0.0, n_rays=n_rays)
        b = TF.run_tail(ngp, x, n_rays=n_rays)
        for key in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "ws", "d_sig", "d_rgb"):
            assert np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (key, n_rays)
        if blocks == 1:
            assert np.array_equal(a["terms"][:4], b["terms"])
        else:
            np.testing.assert_allclose(a["terms"][:4], b["terms"], rtol=blocks * TF.REORDER, atol=0)
        assert a["terms"][4] == 0.0
        sel = NR.owned(x, n_rays)[0] >= 0
        assert not a["d_np"][sel].any() and not np.isnan(a["d_np"][sel]).any()
    assert own.any()


def test_argument_checks(ngp):
    """the wrapper raises on what the entry refuses: more than 8 classes, a narrow normal head, a misaligned workspace,
    a missing target"""
    x, normals = batch("crafted"), normals_of("crafted")
    with pytest.raises(RuntimeError):
        run_nrm(ngp, x, normals, classes=9)
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt")}
    n, R_ = x["n"], x["n_rays"]
    E = lambda *s: torch.empty(*s, device=DEV)
    acc = E(13)
    total = torch.empty(R_, dtype=torch.int64, device=DEV)

    def call(normals_t, ws_, ld_normal=3):
        ngp._lib.call("render_loss_fused_nrm", t["sig"], t["rgbs"], t["dsig"], None, t["nrm"], ld_normal, t["sem"], 8, t["dirs"],
                      t["deltas"], t["ts"], t["rays_a"], t["gt"], None, normals_t, 1e-3, 1e-4, 7, R_, 2e-4, 3e-4, total,
                      acc[6:8].view(torch.int64), E(R_), E(R_), E(R_, 3), E(R_, 3), E(R_, 7), E(n), E(R_), E(R_, 3), acc[:5],
                      E(n), E(n, 3), ws_, E(n, 3))
    good = acc[8:12].view(torch.int32)
    call(T(normals), good)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        call(None, good)
    with pytest.raises(RuntimeError):
        call(T(normals), acc[9:13].view(torch.int32))          # 4 bytes off an 8-byte boundary
    with pytest.raises(RuntimeError):
        call(T(normals), good, ld_normal=2)


# ------------------------------------------------------------------------------------------- g. autograd
def _close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _grid_buffers(model):
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    return model


def _nonzero_normals(scene, o, d, gen):
    """the scene's normals where it has one, a random direction elsewhere, lengths 0.3 to 5: every target non-zero, which
    is where the entry and NeRFLoss._normal_mono state the same loss"""
    nrm = scene.ground_truth_normals(o, d, n_quad=64)
    rnd = torch.nn.functional.normalize(torch.randn(nrm.shape, device=DEV, generator=gen), dim=-1)
    nrm = torch.where((nrm != 0).any(-1, keepdim=True), nrm, rnd)
    nrm = nrm * (0.3 + 4.7 * torch.rand(len(nrm), 1, device=DEV, generator=gen))
    assert bool((nrm != 0).any(-1).all())
    return nrm.contiguous()


def test_fused_normal_tail_matches_the_launch_per_operation_route(ngp):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background
    draw on both routes, every target non-zero.  A: render + NeRFLoss(normal_mono=True) + sum of means + autograd; B:
    render with _fused_loss=FusedTail(..., terms={'normal_mono': ...}, packed=True) through rendering._RenderLossFn.  The
    bars of the semantic counterpart: terms rtol 1e-4, parameter gradients within 3e-4 of the largest entry."""
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
    normals = _nonzero_normals(scene, o, d, gen)
    loss_fn = NeRFLoss()
    lam = (loss_fn.lambda_opa, loss_fn.lambda_distortion, loss_fn.lambda_normal_mono)
    named = [(n, p) for n, p in model.named_parameters() if p.numel() > 0]
    out = {}
    for fused in (False, True):
        for _, p in named:
            p.grad = None
        torch.manual_seed(35)
        kw = dict(exp_step_factor=1 / 256, random_bg=True)
        if fused:
            tail = FusedTail(gt, lam[0], lam[1], terms={"normal_mono": (normals, lam[2])}, packed=True)
            res = render(model, o, d, _fused_loss=tail, **kw)
            assert "_loss_terms" in res
            terms = res.pop("_loss_terms")
            assert terms.shape == (5,) and terms.requires_grad
            torch.autograd.backward([terms], [torch.tensor([1.0, 0, 0, 0, 0], device=DEV)])
            terms = N(terms)
        else:
            res = render(model, o, d, **kw)
            ld = loss_fn(res, {"rgb": gt, "normal": normals}, normal_mono=True)
            loss = sum(t.mean() for t in ld.values())
            loss.backward()
            terms = np.array([float(loss.detach())] + [float(ld[n].detach().mean()) for n in
                                                        ("rgb", "opacity", "distortion", "normal_mono")], np.float32)
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
    for name in ("norm_pred_header.params", "rgb_encoder.params", "xyz_encoder.params"):
        assert np.abs(gb[name]).sum() > 0, name


def test_wrapper_hands_back_the_direct_call(ngp):
    """rendering._RenderLossFn with the packed normal_mono term on the crafted batch: the outputs are those of the direct call, and back-propagating
    terms[0] with a unit seed hands back the launch's d_sigmas, d_rgbs and d_normal_head bit for bit"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x, normals = batch("crafted"), normals_of("crafted")
    direct = run_nrm(ngp, x, normals, use_scale=True)
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3")}
    sig, rgbs, head = t["sig"].requires_grad_(True), t["rgbs"].requires_grad_(True), t["nrm"].requires_grad_(True)
    args = (sig, rgbs, t["sem"], head, None, t["dsig"], t["dirs"], t["deltas"], t["ts"], t["rays_a"])
    tail = FusedTail(t["gt"], NR.R.LAMBDA_O, NR.R.LAMBDA_D, terms={"normal_mono": (T(normals), NR.LAMBDA_NM)}, packed=True)
    outs = _RenderLossFn.apply(*args, tail, t["scale3"], 1e-4, 7, t["bg"])
    terms = outs[0]
    assert terms.shape == (5,) and terms.requires_grad and not any(o.requires_grad for o in outs[1:] if o is not None)
    seed = torch.zeros_like(terms)
    seed[0] = 1.0
    torch.autograd.backward([terms], [seed])
    own = NR.owned(x)[0] >= 0
    got = dict(zip(("terms", "total", "vr", "opacity", "depth", "rgb", "normal", "sem", "ws", "Ro", "Rp"), (N(o) for o in outs)))
    for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp"):
        assert np.array_equal(got[k], direct[k]), k
    np.testing.assert_allclose(got["terms"], direct["terms"], rtol=4 * TF.REORDER, atol=0)
    assert got["terms"][4] == direct["terms"][4]
    assert np.array_equal(N(sig.grad)[own], direct["d_sig"][own])
    assert np.array_equal(N(rgbs.grad)[own], direct["d_rgb"][own])
    assert head.grad.shape == (x["n"], 3) and np.array_equal(N(head.grad)[own], direct["d_np"][own])
    for bad in (T(normals)[:5], T(normals).double(), T(normals)[:, :2]):
        with pytest.raises(ValueError):
            _RenderLossFn.apply(*args, FusedTail(t["gt"], 0.0, 0.0, terms={"normal_mono": (bad, 0.0)}, packed=True),
                                t["scale3"], 1e-4, 7, None)


# ------------------------------------------------------------------------------------------- h. the trainer
def test_trainer_normal_route_matches_module_route(ngp):
    """NGPTrainer(normal_mono=True) with step(normals=) follows the trajectory of NGPTrainer(loss_kwargs={'normal_mono':
    True}) with step(target={'normal': ...}) for six steps of 1024 rays (every target non-zero), within the bars of the
    semantic counterpart: losses rtol 1e-3, parameters rtol 5e-3 / atol 5e-5, norm_pred_header.params included, which moved.

    The learning rate is TRAJ_LR = 3e-4, not the 1e-2 of a training run.  Reason: six Adam steps are not a well-conditioned
    function of the gradients at 1e-2.  Adam's step is lr g / (|g| + eps) with eps = 1e-8; the colour table's gradient is
    summed with float atomics, whose order leaves about 3e-10 of absolute noise (1e-7 of the largest entry, 1.6e-3:
    measured as the module route against itself, and the same for the fused route against itself, also with every kernel
    serialised, so no race is involved), and for the table entries whose gradient is of the order of eps that noise moves
    the step by up to lr x 3e-10 / 1e-8 = 0.03 lr.  At lr = 1e-2 the SAME route run twice from the same seeds is 3e-4
    apart in the table after two steps and 3e-5 to 1.7e-4 apart in rgb_net.params after three to six (module route
    against itself: 4.5e-5 after three steps) - at and beyond the atol of 5e-5, whatever the route under test does.  The
    effect is linear in lr: at 3e-4 it is a thirtieth, an order below the atol, while six steps still move the parameters
    by up to 1.8e-3, 36 times the atol, so a gradient that is wrong or missing still misses the bars.
    Figures: profiles/normal_tail.txt."""
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=10, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(51)
    batches = []
    for i in range(6):
        img, pix = scene.sample_batch(1024, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        batches.append((o, d, gt, _nonzero_normals(scene, o, d, gen)))
    out = []
    for fused in (True, False):
        torch.manual_seed(52)
        model = _grid_buffers(ngp.networks.NGP(scale=0.5).to(DEV))
        start = N(model.norm_pred_header.params).copy()
        kw = dict(normal_mono=True) if fused else dict(loss_kwargs={"normal_mono": True})
        tr = NGPTrainer(model, lr=TRAJ_LR, **kw)
        assert tr.fused_loss == fused and tr.normal_mono == fused
        torch.manual_seed(53)
        if fused:
            steps = [tr.step(o, d, gt, normals=nrm) for o, d, gt, nrm in batches]
        else:
            steps = [tr.step(o, d, gt, target={"normal": nrm}) for o, d, gt, nrm in batches]
        losses = [float(s[0]) for s in steps]
        tr.wait()
        out.append((losses, N(model.xyz_net[0].weight).copy(), N(model.rgb_net.params).copy(),
                    N(model.norm_pred_header.params).copy()))
        moved = np.abs(out[-1][3] - start).max()
        print(f"FIG trainer {'fused' if fused else 'module'}: norm_pred_header moved by at most {moved:.3g}")
        assert moved > 3 * TRAJ_LR          # the head was trained: Adam moves a parameter by about lr per step
    print("FIG trainer losses fused", out[0][0], "module", out[1][0])
    _close(np.array(out[0][0]), np.array(out[1][0]), 1e-3, 1e-7)
    for k in (1, 2, 3):
        print(f"FIG trainer params[{k}]: max|diff| {np.abs(out[0][k] - out[1][k]).max():.3g}")
        _close(out[0][k], out[1][k], 5e-3, 5e-5)


def test_trainer_normal_argument_checks(ngp):
    """a missing or misshapen normals= and every combination the normal tail does not cover raise ValueError; the route
    combines with appearance codes and a random background; a model that leaves the fused tail makes step() raise"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=4, img_wh=(20, 20), device=DEV)
    make = lambda **kw: _grid_buffers(ngp.networks.NGP(scale=0.5, **kw).to(DEV))
    model = make()              # (a refused construction leaves the model as it was: one model serves them all)
    refused = [dict(msk_model=implicit_mask().to(DEV)),
               dict(pose_refiner=PoseRefiner(scene.poses, scene.directions).to(DEV)),
               dict(semantic=True), dict(render_kwargs={"use_skybox": True}),
               dict(loss_kwargs={"normal_mono": True}), dict(loss_kwargs={"semantic": True}),
               dict(loss_kwargs={"depth_mono": True}), dict(loss_kwargs={"normal_ref": True})]
    for kw in refused:
        with pytest.raises(ValueError):
            NGPTrainer(model, normal_mono=True, **kw)
    assert model.differentiable_normals is False
    for model_kw in (dict(rgb_act="None"), dict(use_skybox=True)):
        with pytest.raises(ValueError):
            NGPTrainer(make(**model_kw), normal_mono=True)
    img, pix = scene.sample_batch(64)
    o, d = scene.rays(img, pix)
    gt = torch.rand(64, 3, device=DEV)
    some = torch.nn.functional.normalize(torch.randn(64, 3, device=DEV), dim=-1)
    plain = NGPTrainer(model)
    with pytest.raises(ValueError):
        plain.step(o, d, gt, normals=some)
    model = make(embed_a=True, embed_a_len=4)
    emb = torch.nn.Embedding(4, 4).to(DEV)
    tr = NGPTrainer(model, normal_mono=True, embedding_a=emb, exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img)
    for bad in (some[:5], some[:, :2], some.to(torch.int64), some.reshape(-1)):
        with pytest.raises(ValueError):
            tr.step(o, d, gt, img_idxs=img, normals=bad)
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, normals=some, target={"normal": None})
    before = N(model.norm_pred_header.params).copy()
    loss, _ = tr.step(o, d, gt, normals=torch.zeros(64, 3, device=DEV), img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all()
    assert np.array_equal(N(model.norm_pred_header.params), before)          # zero gradient, fresh Adam state: no move
    loss, res = tr.step(o, d, gt, normals=some, img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and not np.array_equal(N(model.norm_pred_header.params), before)
    # a model that leaves the fused tail after construction is an error, not a step on the default loss without normals
    model.differentiable_normals = True
    with pytest.raises(RuntimeError):
        tr.step(o, d, gt, normals=some, img_idxs=img)
    model.differentiable_normals = False


# ------------------------------------------------------------------------------------------- i. end to end
def test_train_dataset_with_normals_end_to_end(ngp, tmp_path):
    """the proxy scene with its analytic normal maps in the tnt layout (34 views of 80 x 80, every 8th held out),
    train_dataset.train(..., normal_mono=True) for 600 steps of 2048 rays, twice from the same seed: with
    lambda_normal_mono at NeRFLoss's 1e-3 and at 0, where the head stays untrained.  Held-out PSNR of the supervised run
    keeps test_train_from_other_dataset_formats' bar (mean > 20 dB); its mean held-out angle between predicted and target
    normals must lie below the unsupervised run's by more than that run's own max - min over the held-out images.
    Measured figures: profiles/normal_mono.txt."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    from ngp_amd.datasets import dataset_dict
    from ngp_amd.evaluation import evaluate_split, normal_summary
    from ngp_amd.synthetic import LegoProxy
    scene = LegoProxy(n_images=34, img_wh=(80, 80), device=DEV)
    root = td.make_proxy_with_normals(str(tmp_path / "scene"), scene, n_quad=128)
    assert len(os.listdir(os.path.join(root, "normal"))) == 34
    test_set = dataset_dict["tnt"](root, "test", 1.0, device=DEV, normal_mono=True)
    assert len(test_set) == 5 and tuple(test_set.normals.shape) == (5, 80 * 80, 3)
    share = float((test_set.normals != 0).any(-1).float().mean())
    assert 0.05 < share < 0.9
    runs = {}
    for tag, lam in (("supervised", None), ("lambda 0", 0.0)):
        train_set = dataset_dict["tnt"](root, "train", 1.0, device=DEV, normal_mono=True)
        assert tuple(train_set.normals.shape) == (29, 80 * 80, 3)
        torch.manual_seed(43)
        model = td.build_model(0.5, DEV)
        tr = td.train(model, train_set, num_epochs=3, steps_per_epoch=200, batch_size=2048, lr=1e-2, normal_mono=True,
                      lambda_normal_mono=lam)
        assert tr.global_step == 600 and tr.normal_mono and tr.loss_fn.lambda_normal_mono == (1e-3 if lam is None else 0.0)
        res = evaluate_split(model, test_set)
        assert len(res["normal_deg"]) == 5 and all(np.isfinite(res["normal_deg"]))
        runs[tag] = (sum(res["psnr"]) / 5, normal_summary(res), res["normal_deg"], res["psnr"])
        print(f"FIG end-to-end {tag}: psnr {runs[tag][0]:.2f} dB (per image {res['psnr']}), normal_deg mean {runs[tag][1]:.2f} "
              f"(per image {res['normal_deg']}), pixels with a normal {share:.3f}")
    sup, zero = runs["supervised"], runs["lambda 0"]
    spread = max(zero[2]) - min(zero[2])
    print(f"FIG end-to-end margin: {zero[1] - sup[1]:.2f} degrees, spread of the lambda 0 run {spread:.2f}")
    assert sup[0] > 20.0, sup[3]
    assert zero[1] - sup[1] > spread, (sup[1], zero[1], spread)
