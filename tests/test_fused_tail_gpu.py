"""The fused render + loss tail on the GPU (render_loss_fused_kernel<8, 32, MASKED> behind ngp_render_loss_fused and
ngp_render_loss_fused_masked) against the float64 restatement of tests/fused_tail_reference.py, per ray and per sample,
on rays whose lengths and stop samples sit on the edges of the kernel's 32-sample chunks, and on random batches.  The
call, the restatement's cache and the comparer are those of tests/tail_harness.py (entries 'default' and 'masked').

Bars.  opacity, depth, rgb, normal_pred, semantic, ws: rtol 2e-5, atol 2e-6, and d_sigmas, d_rgbs: rtol 2e-4, atol
2e-5 / n_rays (tests/test_gpu_parity.py's bars of the per-operation kernels; their upstream gradients are of order 1,
the loss's seeds here of order 1 / n_rays).  Ro, Rp, the loss terms and d_mask have no earlier bar against a reference:
they are held to 8 times the error of the restatement run in float32 on the same inputs (fused_tail_reference.fp32_error;
8 for tree sums, __expf and float atomics in arbitrary order instead of serial sums), but not below the atol above — for
a loss term the atol times the term's weight (1, lambda_o, lambda_d, size_delta; the sum: 1), for d_mask 2e-5 / n_rays.
The measured figures are in profiles/fused_tail_reference.txt.  A failure names the ray's (length, stop) case and the
sample."""
import numpy as np
import pytest

import fused_tail_reference as R
from tail_harness import (FW_ATOL, FW_RTOL, PER_RAY, _same_launch, against_reference, batch, reference, run_entry,
                          wrapper_against_direct)

pytestmark = pytest.mark.gpu
ARGS = {"bg": dict(use_bg=True, use_scale=False, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D),
        "nobg-scale": dict(use_bg=False, use_scale=True, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D),
        "bg-scale-nolambda": dict(use_bg=True, use_scale=True, lam_o=0.0, lam_d=0.0),
        # at NeRFLoss's weights the distortion term's share of n_rays * d_sigmas is about 2e-6, a tenth of the bar: with
        # weights of order 1 the entropy and distortion gradients (passes B and C) are as large as the colour term's
        "bg-heavy-lambda": dict(use_bg=True, use_scale=False, lam_o=0.5, lam_d=1.0)}
PER_SAMPLE = ("ws", "d_sig", "d_rgb")
ENTRY = {False: "default", True: "masked"}


# ------------------------------------------------------------------------------------------- a. crafted edges
@pytest.mark.parametrize("args", list(ARGS))
@pytest.mark.parametrize("classes", [0, 1, 7, 8])
@pytest.mark.parametrize("T_thr", [1e-4, 1e-2])
def test_crafted_edges(ngp, T_thr, classes, args):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges; nothing is left out of the comparison"""
    x = batch("crafted")
    cfg = dict(T_thr=T_thr, classes=classes, **ARGS[args])
    ref, noise = reference("default", "crafted", **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    ok, _, _ = R.comparable(x, T_thr, 1e-2)
    assert ok.all()
    got = run_entry(ngp, "default", x, **cfg)
    against_reference("default", f"crafted T_thr={T_thr} classes={classes} {args}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- b. leading dimensions
@pytest.mark.parametrize("masked", [False, True])
def test_leading_dimensions(ngp, masked):
    """normal_head and sem_logits as the leading columns of 16-wide matrices whose other columns hold NaN"""
    x = batch("crafted")
    cfg = dict(classes=7, use_scale=True, size_delta=6e-2)
    a = run_entry(ngp, ENTRY[masked], x, **cfg)
    b = run_entry(ngp, ENTRY[masked], x, ld=16, **cfg)
    assert np.isfinite(a["terms"]).all() and np.isfinite(a["opacity"]).all()
    _same_launch(a, b, 4)


# ------------------------------------------------------------------------------------------- c. ownership
@pytest.mark.parametrize("classes", [0, 1, 7])
def test_ownership(ngp, classes):
    """the gap between two segments is not touched, everything behind a stop is exactly zero, empty rays give the
    background, and sem is written in all of its columns"""
    x = batch("crafted")
    got = run_entry(ngp, "default", x, classes=classes)
    row, k = R.owned(x)
    assert (row < 0).sum() == R.GAP
    stop_of_row = np.array([10 ** 6 if s is None else s for _, s in x["cases"]])
    behind = (row >= 0) & (k > stop_of_row[np.maximum(row, 0)])
    live = (row >= 0) & ~behind
    assert behind.sum() > 200
    for key in PER_SAMPLE:
        assert np.isnan(got[key][row < 0]).all(), key
        assert not got[key][behind].any() and not np.isnan(got[key][behind]).any(), key
        assert np.isfinite(got[key][live]).all(), key
    assert got["ws"][live].max() > 0.5 and np.count_nonzero(got["d_sig"][live]) > 0.6 * live.sum()
    empty = x["rays_a"][x["rays_a"][:, 2] == 0, 0]
    assert len(empty) == 1
    assert (got["opacity"][empty] == 0).all() and (got["total"][empty] == 0).all() and (got["depth"][empty] == 0).all()
    assert np.array_equal(got["rgb"][empty], np.broadcast_to(x["bg"], (1, 3)))
    assert got["sem"].shape == (27, classes) and not np.isnan(got["sem"]).any()
    if classes == 1:
        np.testing.assert_allclose(got["sem"][:, 0], got["opacity"], rtol=FW_RTOL, atol=FW_ATOL)
    for key in PER_RAY:
        assert np.isfinite(got[key]).all(), key


# ------------------------------------------------------------------------------------------- d. block edges
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8),
    a second workgroup with one ray (9).  What does not depend on the ray count equals the full launch bit for bit; the
    gradients and the terms (seeds scale with 1 / rows) are held to the restatement of the same rows; everything that
    belongs to the other rows is left alone."""
    x = batch("crafted")
    cfg = dict(classes=7, use_scale=True, n_rays=rows)
    full = run_entry(ngp, "default", x, classes=7, use_scale=True)
    got = run_entry(ngp, "default", x, **cfg)
    rays = x["rays_a"][:rows, 0]
    smp = R.owned(x, rows)[0] >= 0
    for key in ("opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "total"):
        assert np.array_equal(got[key][rays], full[key][rays]), key
    assert np.array_equal(got["ws"][smp], full["ws"][smp])
    ref, noise = reference("default", "crafted", **cfg)
    against_reference("default", f"crafted rows={rows}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- e. memset branches
@pytest.mark.parametrize("masked", [False, True])
def test_memset_branches(ngp, masked):
    """terms and vr_samples adjacent as rendering._RenderLossFn lays them out (one fill) and in separate allocations
    (two fills), both pre-filled with NaN / a large negative count"""
    x = batch("crafted")
    cfg = dict(classes=7, size_delta=6e-2)
    a = run_entry(ngp, ENTRY[masked], x, adjacent=True, **cfg)
    b = run_entry(ngp, ENTRY[masked], x, adjacent=False, **cfg)
    _same_launch(a, b, 4)
    ref, noise = reference(ENTRY[masked], "crafted", **cfg)
    for tag, got in (("adjacent", a), ("separate", b)):
        assert got["vr"][0] == ref["vr"][0]
        against_reference(ENTRY[masked], f"crafted masked={masked} {tag}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- f, g. mask, random batches
def _random_batch(ngp, entry, name, cfg, tag):
    """rays whose float64 transmittance comes within 1e-3 (relative) of T_threshold, and their samples, are left out of
    the per-ray and per-sample comparisons.  The loss terms are compared all the same: should such a ray stop one sample
    apart from the restatement, a weight below 1.001 * T_threshold = 1e-4 moves, and with it the ray's share of a mean by
    less than 2e-4 / n_rays of the term's weight.  For the 0.5 % of the rays that are flagged in these batches that is
    under 1e-6 of the weight, half the floor of the bars, even if every one of them did."""
    x = batch(name)
    ok, ray_ok, smp_ok = R.comparable(x, cfg.get("T_thr", 1e-4), 1e-3)
    left_out = 1.0 - ok.mean()
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}")
    assert left_out <= R.MAX_BORDERLINE
    ref, noise = reference(entry, name, **cfg)
    assert 0.2 < (ref["stops"] >= 0).mean() < 0.9
    got = run_entry(ngp, entry, x, **cfg)
    against_reference(entry, f"random-{name} {tag}", got, ref, noise, x, cfg, ray_ok, smp_ok)


@pytest.mark.parametrize("size_delta", [1.0, 6e-2])
@pytest.mark.parametrize("name", ["crafted", "1500"])
def test_masked_entry_with_a_real_mask(ngp, name, size_delta):
    """mask in (0, 1) with exact 0 and exact 1 on a few rays: d_mask, terms[4] and everything else"""
    cfg = dict(classes=7, size_delta=size_delta)
    x = batch(name)
    assert (x["mask"] == 0).any() and (x["mask"] == 1).any() and 0.3 < x["mask"].mean() < 0.7
    if name == "crafted":
        ref, noise = reference("masked", name, **cfg)
        assert ref["terms"][4] > 0 and np.abs(ref["d_mask"]).max() > 0
        against_reference("masked", f"crafted masked size_delta={size_delta}", run_entry(ngp, "masked", x, **cfg), ref, noise, x, cfg)
    else:
        _random_batch(ngp, "masked", name, cfg, f"classes=7 masked=True size_delta={size_delta}")


@pytest.mark.parametrize("name", ["300", "1500"])
def test_random_batch(ngp, name):
    _random_batch(ngp, "default", name, dict(classes=7), "classes=7")


# ------------------------------------------------------------------------------------------- h. the autograd wrappers
@pytest.mark.parametrize("masked", [False, True])
def test_wrapper_hands_back_the_direct_call(ngp, masked):
    """rendering._RenderLossFn (with and without a mask in its FusedTail) on the crafted batch: the outputs are those of the
    direct call, and back-propagating terms[0] with a unit seed hands back the launch's d_sigmas, d_rgbs (and d_mask) bit
    for bit"""
    from ngp_amd.rendering import FusedTail
    tail = lambda t, mask: FusedTail(t["gt"], R.LAMBDA_O, R.LAMBDA_D, **(dict(mask=mask, size_delta=6e-2) if masked else {}))
    wrapper_against_direct(ngp, ENTRY[masked], batch("crafted"), None, tail, classes=7, use_scale=True, size_delta=6e-2)
