"""The float64 restatement of the fused render + loss tail (tests/fused_tail_reference.py) is itself checked here, without a
GPU: against the C oracle's compositing, Ref-NeRF, distortion forward and backward (oracle/ngp_oracle.c follows the
reference project's kernels), against this package's NeRFLoss on CPU tensors, and the promises of the seeded inputs
that tests/test_fused_tail_gpu.py relies on.  The oracle is float32 C: it is held to the bars that
tests/test_gpu_parity.py holds the per-operation kernels to against it."""
import numpy as np
import pytest
import torch

import fused_tail_reference as R
import oracle

FW = dict(rtol=2e-5, atol=2e-6)            # test_composite_train_fw_bw / test_refloss_fw_bw, forward
DIST = dict(rtol=1e-3, atol=2e-6)          # test_distortion_loss_fw_bw: the loss is a cancellation of O(w * wt) products
BW_RTOL, BW_ATOL = 2e-4, 2e-5              # ... backward, for upstream gradients of order 1: scaled by 1 / n_rays here

BATCHES = {"crafted-1e-4": (lambda: R.make_crafted(0, 1e-4), 1e-2), "crafted-1e-2": (lambda: R.make_crafted(0, 1e-2), 1e-2),
           "random-300": (lambda: R.make_random(300), 1e-3)}
_CACHE = {}


def batch(name):
    if name not in _CACHE:
        make, rel = BATCHES[name]
        x = make()
        cfg = dict(T_thr=x["T_thr"], classes=7, use_bg=True, use_scale=True, masked=True, size_delta=6e-2)
        _CACHE[name] = (x, cfg, R.evaluate(x, **cfg), R.comparable(x, x["T_thr"], rel))
    return _CACHE[name]


@pytest.mark.parametrize("T_thr", [1e-4, 1e-2])
def test_crafted_stops_land_as_designed(T_thr):
    x = R.make_crafted(0, T_thr)
    assert sorted(x["cases"], key=str) == sorted(R.CASES, key=str) and len(x["rays_a"]) == 27
    assert (x["rays_a"][:, 0] != np.arange(27)).any() and sorted(x["rays_a"][:, 0]) == list(range(27))
    row, _ = R.owned(x)
    assert (row < 0).sum() == R.GAP and x["n"] == sum(n for n, _ in R.CASES) + R.GAP
    ref = R.evaluate(x, T_thr=T_thr)
    want = [-1 if stop is None else stop for _, stop in x["cases"]]
    assert ref["stops"].tolist() == want
    ok, ray_ok, smp_ok = R.comparable(x, T_thr, 1e-2)
    assert ok.all() and ray_ok.all() and smp_ok.sum() == x["n"] - R.GAP          # nothing is left out
    # without a designed stop the transmittance stays above 0.25; the stop sample takes it below 1e-8
    for (_, s, n), (_, stop) in zip(x["rays_a"], x["cases"]):
        T = np.cumprod(np.exp(-x["sig"][s:s + n].astype(np.float64) * x["deltas"][s:s + n]))
        assert (T[:stop] >= 0.25).all() and (stop is None or T[stop] < 1e-8)
    # the clamps of the three normalisations are exercised on live samples, the mask holds both ends
    live = np.nan_to_num(ref["ws"]) > 0
    for k in ("dsig", "nrm", "dirs"):
        assert (live & ~x[k].any(1)).sum() >= 2, k
    assert (x["mask"] == 0).sum() == 3 and (x["mask"] == 1).sum() == 3
    assert (np.isnan(ref["ws"]) == (row < 0)).all()
    # autograd on the truncated sum: exactly zero behind the stop
    behind = (row >= 0) & (R.owned(x)[1] > np.where(ref["stops"] >= 0, ref["stops"], 10 ** 6)[np.maximum(row, 0)])
    assert behind.sum() > 200
    assert not ref["ws"][behind].any() and not ref["d_sig"][behind].any() and not ref["d_rgb"][behind].any()


@pytest.mark.parametrize("n_rays", [300, 1500])
def test_random_batches_stay_under_the_cap(n_rays):
    x = R.make_random(n_rays)
    ok, _, _ = R.comparable(x, 1e-4, 1e-3)
    share = 1.0 - ok.mean()
    print(f"{n_rays} rays, {x['n']} samples: borderline share {share:.4f}")
    assert share <= R.MAX_BORDERLINE
    assert x["n"] <= 70000 and (x["rays_a"][::11, 2] == 0).all()
    stops = R.evaluate(x)["stops"] if n_rays == 300 else None
    if stops is not None:
        assert 0.2 < (stops >= 0).mean() < 0.9


@pytest.mark.parametrize("name", list(BATCHES))
def test_forward_matches_the_oracle(name):
    x, cfg, ref, (ok, ray_ok, smp_ok) = batch(name)
    T_thr, classes = cfg["T_thr"], cfg["classes"]
    total, opacity, depth, rgb, normal, sem, ws = oracle.composite_train_fw(
        x["sig"], x["rgbs"], ref["n_pred"], ref["prob"], x["deltas"], x["ts"], x["rays_a"], T_thr, classes)
    assert np.array_equal(total[ray_ok], ref["total"][ray_ok])
    for got, key in ((opacity, "opacity"), (depth, "depth"), (rgb, "rgb_fg"), (normal, "normal"), (sem, "sem")):
        np.testing.assert_allclose(got[ray_ok], ref[key][ray_ok], err_msg=key, **FW)
    np.testing.assert_allclose(ws[smp_ok], ref["ws"][smp_ok], **FW)
    lo, lp = oracle.composite_refloss_fw(x["sig"], ref["ndiff"], ref["nori"], x["deltas"], x["ts"], x["rays_a"], T_thr)
    np.testing.assert_allclose(lo[ray_ok], ref["Ro"][ray_ok], **FW)
    np.testing.assert_allclose(lp[ray_ok], ref["Rp"][ray_ok], **FW)
    dist, _, _ = oracle.distortion_loss_fw(np.nan_to_num(ref["ws"]), x["deltas"], x["ts"], x["rays_a"])      # (by ray)
    print(f"{name}: max |dist - ref| = {np.abs(dist - ref['dist'])[ray_ok].max():.3g}")
    np.testing.assert_allclose(dist[ray_ok], ref["dist"][ray_ok], **DIST)


@pytest.mark.parametrize("name", list(BATCHES))
def test_autograd_gradients_match_the_oracles_backward_chain(name):
    """distortion_loss_bw into composite_train_bw, seeded with the restatement's own dL/d rgb, dL/d opacity (which holds
    the background's share) and lambda_d / R, against autograd's d_sigmas and d_rgbs"""
    x, cfg, ref, (ok, ray_ok, smp_ok) = batch(name)
    n_rays, classes = x["n_rays"], cfg["classes"]
    rays = x["rays_a"][:, 0]
    ws = np.nan_to_num(ref["ws"]).astype(np.float32)
    np.testing.assert_allclose(ref["g_dist"], R.LAMBDA_D / n_rays, rtol=1e-12)
    _, wi, wti = oracle.distortion_loss_fw(ws, x["deltas"], x["ts"], x["rays_a"])
    d_ws = oracle.distortion_loss_bw(ref["g_dist"], wi, wti, ws, x["deltas"], x["ts"], x["rays_a"])

    def by_ray(v):
        out = np.zeros((n_rays,) + v.shape[1:])
        out[rays] = v
        return out

    zeros = lambda *s: np.zeros(s, np.float32)
    d_sig, d_rgb, _, _ = oracle.composite_train_bw(
        by_ray(ref["g_op"]), zeros(n_rays), by_ray(ref["g_rgb"]), zeros(n_rays, 3), zeros(n_rays, classes), d_ws, x["sig"],
        x["rgbs"], ref["n_pred"], ws, x["deltas"], x["ts"], x["rays_a"], ref["opacity"], ref["depth"], ref["rgb_fg"],
        ref["normal"], cfg["T_thr"], classes)
    err_s = np.abs(d_sig - ref["d_sig"])[smp_ok].max() * n_rays
    err_c = np.abs(d_rgb - ref["d_rgb"])[smp_ok].max() * n_rays
    print(f"{name}: n_rays * max |d_sigmas - ref| = {err_s:.3g}, n_rays * max |d_rgbs - ref| = {err_c:.3g}")
    assert np.abs(ref["d_sig"][smp_ok]).max() * n_rays > 1e-3
    np.testing.assert_allclose(d_sig[smp_ok] * n_rays, ref["d_sig"][smp_ok] * n_rays, rtol=BW_RTOL, atol=BW_ATOL)
    np.testing.assert_allclose(d_rgb[smp_ok] * n_rays, ref["d_rgb"][smp_ok] * n_rays, rtol=BW_RTOL, atol=BW_ATOL)


@pytest.mark.parametrize("name", list(BATCHES))
def test_loss_terms_match_nerfloss(ngp, name):
    """colour, opacity and mask terms from losses.NeRFLoss on float64 CPU tensors (exact up to rounding); the distortion
    term from the oracle; d_mask from autograd through NeRFLoss"""
    from ngp_amd.losses import NeRFLoss
    x, cfg, ref, (ok, ray_ok, smp_ok) = batch(name)
    rays = x["rays_a"][:, 0]
    loss_fn = NeRFLoss()
    assert (loss_fn.lambda_opa, loss_fn.lambda_distortion) == (R.LAMBDA_O, R.LAMBDA_D)
    res = {"rgb": torch.from_numpy(ref["rgb"][rays]), "opacity": torch.from_numpy(ref["opacity"][rays])}
    mask = torch.from_numpy(x["mask"][rays].astype(np.float64))[:, None].requires_grad_(True)
    colour = loss_fn._colour(res, {"rgb": torch.from_numpy(x["gt"][rays].astype(np.float64))}, mask).mean()
    r_ms, _ = loss_fn.mask_regularize(mask, cfg["size_delta"], 0)
    want = [float(colour.detach()), float(loss_fn._opacity_entropy(res).mean()), None, float(r_ms.detach())]
    dist, _, _ = oracle.distortion_loss_fw(np.nan_to_num(ref["ws"]), x["deltas"], x["ts"], x["rays_a"])
    want[2] = R.LAMBDA_D * float(dist.astype(np.float64).mean())
    got = ref["terms"]
    assert got.shape == (5,)
    for i in (0, 1, 3):
        np.testing.assert_allclose(got[1 + i], want[i], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[3], want[2], rtol=DIST['rtol'], atol=DIST['atol'] * R.LAMBDA_D)
    np.testing.assert_allclose(got[0], got[1:].sum(), rtol=1e-14)
    (colour + r_ms).backward()
    np.testing.assert_allclose(ref["d_mask"][rays], mask.grad.numpy()[:, 0], rtol=1e-10, atol=1e-18)
    # the unmasked entry: four terms, the plain colour mean
    plain = R.evaluate(x, **dict(cfg, masked=False, size_delta=0.0))
    assert plain["terms"].shape == (4,) and "d_mask" not in plain
    np.testing.assert_allclose(plain["terms"][1], float(loss_fn._colour(res, {"rgb": torch.from_numpy(x["gt"][rays].astype(np.float64))}).mean()), rtol=1e-12)
    np.testing.assert_array_equal(plain["terms"][2:4], got[2:4])


def test_options_of_the_restatement():
    """classes 0, 1 and 8, no background, no scale, lambda = 0, a subset of the rows: shapes, the identities that hold
    exactly, and the float32 run"""
    x = R.make_crafted(0, 1e-4)
    full = R.evaluate(x, classes=8, use_bg=False, lam_o=0.0, lam_d=0.0)
    assert full["sem"].shape == (27, 8) and full["terms"][2] == 0 and full["terms"][3] == 0
    np.testing.assert_array_equal(full["rgb"], full["rgb_fg"])
    np.testing.assert_allclose(full["sem"].sum(1), full["opacity"], rtol=1e-12)
    assert R.evaluate(x, classes=0)["sem"].shape == (27, 0)
    np.testing.assert_allclose(R.evaluate(x, classes=1)["sem"][:, 0], full["opacity"], rtol=1e-14)
    empty = x["rays_a"][x["rays_a"][:, 2] == 0, 0]
    bg = R.evaluate(x)
    assert (bg["opacity"][empty] == 0).all() and np.array_equal(bg["rgb"][empty], np.broadcast_to(x["bg"].astype(np.float64), (len(empty), 3)))
    part = R.evaluate(x, n_rays=9)
    rays = x["rays_a"][:9, 0]
    rest = np.setdiff1d(np.arange(27), rays)
    assert np.isnan(part["opacity"][rest]).all() and np.array_equal(part["opacity"][rays], bg["opacity"][rays])
    np.testing.assert_allclose(part["d_sig"][R.owned(x, 9)[0] >= 0] * 9, bg["d_sig"][R.owned(x, 9)[0] >= 0] * 27, rtol=1e-12, atol=1e-18)
    noise = R.fp32_error(x, ref=bg)
    print("float32 noise of the crafted batch:", {k: np.array2string(np.asarray(v), precision=3) for k, v in noise.items()})
    assert 0 < noise["opacity"] < 2e-6 and 0 < noise["d_sig"] * 27 < 2e-5 and noise["terms"].shape == (4,)


def test_layout_table_and_fused_tail(ngp):
    """rendering.TAIL_LAYOUT keeps every entry on its one-fill branch: vr_samples (an int64) 8-byte aligned behind the
    terms, the workspace right behind it and as large as the header says, the accumulator exactly that long (the semantic
    entry's workspace is an allocation of its own); and what FusedTail selects and refuses"""
    import os
    import re
    from ngp_amd.rendering import MULTI_TERMS, TAIL_LAYOUT, FusedTail
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ngp_hip.h")).read()
    ints = {k.lower(): int(v) for k, v in re.findall(r"#define NGP_(SEM|NRM|DEP|MULTI)_WS_INTS (\d+)", header)}
    assert sorted(ints) == ["dep", "multi", "nrm", "sem"]
    assert list(TAIL_LAYOUT) == ["default", "masked", "sem", "nrm", "dep", "multi"]
    for key, lay in TAIL_LAYOUT.items():
        assert lay.vr_at % 2 == 0 and lay.vr_at >= lay.n_terms, key
        assert lay.ws_ints == ints.get(key, 0), key
        if lay.ws_at is not None:
            assert lay.ws_ints > 0 and lay.ws_at == lay.vr_at + 2 and lay.acc == lay.ws_at + lay.ws_ints, key
        else:
            assert lay.acc == lay.vr_at + 2 and (lay.ws_ints == 0 or key == "sem"), key
    assert [TAIL_LAYOUT[k].n_terms for k in TAIL_LAYOUT] == [4, 5, 6, 5, 5, 8]
    gt, one = object(), {"depth_mono": (None, 1.0, 1.0)}
    two = dict(one, normal_mono=(None, 1.0))
    assert FusedTail(gt, 1.0, 2.0).entry == "default" and FusedTail(gt, 1.0, 2.0, mask=gt, size_delta=0.5).entry == "masked"
    assert [FusedTail(gt, 0, 0, terms={t: ()}, packed=True).entry for t in MULTI_TERMS] == ["sem", "nrm", "dep"]
    assert FusedTail(gt, 0, 0, terms=one).entry == "multi" and FusedTail(gt, 0, 0, terms=two).entry == "multi"
    assert FusedTail(gt, 0, 0).terms == {} and FusedTail(gt, 0, 0, terms=two).terms == two
    for bad in (dict(mask=gt, terms=one), dict(packed=True), dict(terms={}, packed=True), dict(terms=two, packed=True),
                dict(terms={}), dict(terms={"sky": ()}), dict(terms=dict(one, sky=()))):
        with pytest.raises(ValueError):
            FusedTail(gt, 0, 0, **bad)
