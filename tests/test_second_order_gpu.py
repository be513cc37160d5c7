"""The second-order backward of the density field against a float64 autograd reference, element by element.

The route: a loss on normals_raw -> d(sigma)/dx -> the density table and xyz_net (`--normal_ref` trains through it).
Three levels, all against tests/second_order_reference.py (a torch float64 gather of 8 corners, every gradient from
torch.autograd; tests/test_second_order_host.py checks that reference itself against the C oracle without a GPU):

  (a) the kernels through the C ABI: ngp_grid_bwd_bwd_input, and with the same inputs ngp_grid_fwd, ngp_grid_bwd_input,
      ngp_grid_bwd_param and ngp_grid_bwd_param_scaled, on five layouts (F = 8, 2, 4, 1; dense and hashed levels; fewer
      threads than one workgroup) and four point sets (random, crafted onto cell faces, outside the cube, 64 copies of
      one point), then the variants of the double backward's call: padded dL_dy, either output NULL, a running sum in
      dtable, all-zero dL_dy rows, all-zero v rows.  Every output lies between guard bands.
  (b) the field: networks.NGP(scale).differentiable_normals, sigmas, normals_raw and the gradients of the density table
      and the four xyz_net tensors for random cotangents on sigma and on the normals, at scale 0.5 and 8.
  (c) the same with the encoder wired as the trainer wires it (params.grad a view of a flat buffer that is also
      enc.grad_buffer): the first-order scatter (behind autograd's back) and the second-order contribution (through
      autograd) must both land in the buffer, once each.

Bars.  Nothing is fixed in advance: for each compared tensor the FLOOR is the max-normalised distance between the
reference evaluated in float32 and in float64 on that same case (clamped from below at 2^-23), and the HIP result must
lie within 8 x floor of the float64 reference, max-normalised, over every element.  8, because the kernels sum the same
products in another order (atomics, fmaf contraction, rocBLAS for the MLP), which can cost a few times what one float32
order costs against exact but not orders of magnitude; a wrong sign, a missing scale, a wrong corner or a contribution
counted twice shows at 1e-2 and more.  Table gradients must be exactly zero on every row that no sample touches.

Measured on an MI355X (floor / HIP error, max-normalised; bar = 8 x floor):
  (a) kernels, floor/error per tensor in units of 1e-7:
  case                      y          dL_dx         dtable  dtable_scaled       dL_ddLdy        dtable2
  A-crafted         1.58/1.58      1.21/1.24      1.19/0.84      1.19/0.62      1.19/0.54      1.19/0.66
  A-dup             1.53/1.33      1.84/1.24      1.52/0.89      2.46/1.10      1.36/0.91      2.67/2.42
  A-outside         1.55/1.55      1.80/1.02      1.19/0.86      1.19/1.15      1.20/1.20      1.22/1.22
  A-random          1.61/1.59      1.52/1.31      1.19/0.74      1.19/0.93      1.19/0.93      1.19/0.79
  B-outside         1.23/1.46      1.19/0.97      1.19/0.53      1.19/0.47      1.65/1.17      1.19/1.04
  B-random          1.39/1.39      1.55/1.14      1.19/0.75      1.19/0.60      1.19/1.00      1.19/0.90
  C-dup             1.19/1.01      1.19/1.34      1.19/1.42      1.46/0.66      1.19/1.56      1.37/1.94
  C-random          1.21/1.15      1.19/0.64      1.19/0.94      1.19/1.02      1.19/0.86      1.19/0.78
  D-crafted         1.19/0.84      1.19/0.96      1.19/0.31      1.19/0.54      1.19/0.59      1.19/1.00
  D-one             1.19/0.24      1.19/0.49      1.19/0.12      1.19/1.00      1.19/0.61      1.19/0.65
  D-random          1.19/1.09      1.32/0.70      1.19/0.56      1.19/0.92      1.19/0.89      1.19/0.65
  E-random          1.75/1.75      1.47/1.30      1.19/1.25      1.27/1.79      1.19/0.55      1.19/1.28
  variants on A-random, the field (b) and the trainer's buffer (c):
  tensor                                       floor     error  x floor
  padded dL_ddLdy                           1.19e-07  9.26e-08     0.78
  padded dtable2                            1.19e-07  7.94e-08     0.67
  padded dL_dx                              1.52e-07  1.31e-07     0.86
  padded dtable                             1.19e-07  7.41e-08     0.62
  NULL dL_ddLdy: dtable2                    1.19e-07  7.94e-08     0.67
  prefilled dtable2                         1.19e-07  5.90e-08     0.50
  zero dL_dy rows: dtable2                  1.19e-07  7.63e-08     0.64
  zero dL_dy rows: dL_ddLdy                 1.19e-07  9.26e-08     0.78
  zero v rows: dL_ddLdy                     1.19e-07  9.97e-08     0.84
  zero v rows: dtable2                      1.19e-07  7.94e-08     0.67
  field s=0.5 sigma                         1.39e-07  2.63e-07     1.89
  field s=0.5 normals                       9.56e-07  1.04e-06     1.09
  field s=0.5 table                         1.86e-06  2.42e-06     1.30
  field s=0.5 W1                            1.09e-06  1.84e-06     1.68
  field s=0.5 b1                            4.86e-07  1.28e-06     2.63
  field s=0.5 W2                            7.17e-07  1.12e-06     1.56
  field s=0.5 b2                            1.28e-07  2.96e-08     0.23
  field s=8 sigma                           1.23e-07  2.49e-07     2.02
  field s=8 normals                         1.57e-06  1.99e-06     1.27
  field s=8 table                           1.99e-06  2.10e-06     1.05
  field s=8 W1                              7.78e-07  1.13e-06     1.45
  field s=8 b1                              5.76e-07  1.25e-06     2.18
  field s=8 W2                              9.14e-07  1.52e-06     1.66
  field s=8 b2                              1.19e-07  1.35e-07     1.13
  trainer buffer: table                     1.86e-06  2.55e-06     1.37
  trainer buffer: W1                        1.09e-06  1.84e-06     1.68
  trainer buffer: b1                        4.86e-07  1.28e-06     2.63
  trainer buffer: W2                        7.17e-07  1.12e-06     1.56
  trainer buffer: b2                        1.28e-07  2.96e-08     0.23
  trainer buffer, prefilled: table          2.05e-06  2.83e-06     1.38
  trainer buffer, prefilled: W1             1.09e-06  1.84e-06     1.68
  trainer buffer, prefilled: b1             4.86e-07  1.28e-06     2.63
  trainer buffer, prefilled: W2             7.17e-07  1.12e-06     1.56
  trainer buffer, prefilled: b2             1.28e-07  2.96e-08     0.23
  worst of the run: 2.63 x floor (trainer buffer: b1).
The table gradients are sums of atomics: their errors move by a few 1e-8 from run to run.  No tensor needed a factor of
its own (the b2 gradient at scale 8, whose floor can reach 1e-5 for other cotangents, sits at 1.1 x here).
"""
import numpy as np
import pytest
import torch

import second_order_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1 << 16          # floats before and after a table gradient
SENTINEL = 7.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _desc(ngp, c):
    gd = ngp._lib.GridDesc()
    assert ngp._lib.call_host("grid_layout", *c["args"], gd) == c["layout"].n_params
    return gd


class _Guarded:
    """a float32 device array of `n` values (`fill`, or a copy of `init`) between two bands of SENTINEL"""

    def __init__(self, n, before, after, fill=0.0, init=None):
        self.buf = torch.full((before + n + after,), SENTINEL, dtype=torch.float32, device=DEV)
        self.body = self.buf[before:before + n]
        if init is not None:
            self.body.copy_(T(init).reshape(-1))
        else:
            self.body.fill_(fill)
        self.before, self.n = before, n

    def result(self, what):
        torch.cuda.synchronize()
        out = N(self.buf)
        lo, hi = out[:self.before], out[self.before + self.n:]
        assert (lo == SENTINEL).all() and (hi == SENTINEL).all(), f"{what}: written outside its array"
        return out[self.before:self.before + self.n]


def _bwd_bwd(ngp, gd, c, dy, lddy, v, want_dtable=True, want_ddy=True, prefill=None):
    """one call of ngp_grid_bwd_bwd_input -> (dtable or None, dL_ddLdy or None) as numpy; dy is a device tensor (or a
    view with row stride lddy); 64 Ki floats guard dtable on both sides, L*F floats follow dL_ddLdy, which starts out
    full of SENTINEL: every value of it must be written"""
    lay, n = c["layout"], c["n"]
    dtab = _Guarded(lay.n_params, GUARD, GUARD, init=prefill) if want_dtable else None
    ddy = _Guarded(n * lay.width, 0, lay.width, fill=SENTINEL) if want_ddy else None
    ngp._lib.call("grid_bwd_bwd_input", gd, T(c["table"]), T(c["x"]), dy, lddy, T(v), n,
                  dtab.body if dtab else None, ddy.body if ddy else None)
    return (dtab.result("dtable") if dtab else None,
            ddy.result("dL_ddLdy").reshape(n, lay.width) if ddy else None)


# ---------------------------------------------------------------------------------------------- (a) kernels
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_grid_kernels_match_reference(ngp, name):
    c, r64, _, fl = R.case_reference(name)
    lay, n, rows = c["layout"], c["n"], r64["rows"]
    gd = _desc(ngp, c)
    call = ngp._lib.call
    table, x, dy = T(c["table"]), T(c["x"]), T(c["dy"])
    W = lay.width
    y = _Guarded(n * W, 64, 64, fill=SENTINEL)
    call("grid_fwd", gd, table, x, n, y.body, W)
    R.compare(y.result("y").reshape(n, W), r64["y"], fl["y"], name + " y")
    dx = _Guarded(n * 3, 64, 64, fill=SENTINEL)
    call("grid_bwd_input", gd, table, x, dy, W, n, dx.body)
    R.compare(dx.result("dL_dx").reshape(n, 3), r64["dL_dx"], fl["dL_dx"], name + " dL_dx")
    dt = _Guarded(lay.n_params, GUARD, GUARD)
    call("grid_bwd_param", gd, x, dy, W, n, dt.body)
    R.compare(dt.result("dtable"), r64["dtable"], fl["dtable"], name + " dtable", rows=rows)
    dts = _Guarded(lay.n_params, GUARD, GUARD)
    call("grid_bwd_param_scaled", gd, x, dy, W, T(c["row_scale"]), n, dts.body)
    R.compare(dts.result("dtable_scaled"), r64["dtable_scaled"], fl["dtable_scaled"], name + " dtable_scaled", rows=rows)
    d_tab, d_dy = _bwd_bwd(ngp, gd, c, dy, W, c["v"])
    R.compare(d_dy, r64["dL_ddLdy"], fl["dL_ddLdy"], name + " dL_ddLdy")
    R.compare(d_tab, r64["dtable2"], fl["dtable2"], name + " dtable2", rows=rows)


VARIANT = "A-random"


def test_double_backward_padded_dL_dy(ngp):
    """dL_dy as a column block of a wider matrix, row stride L*F + 8, NaN all around it: finite, unchanged results (the
    three kernels that read dL_dy)"""
    c, r64, _, fl = R.case_reference(VARIANT)
    lay, n, rows = c["layout"], c["n"], r64["rows"]
    gd = _desc(ngp, c)
    W, ld = lay.width, lay.width + 8
    wide = torch.full((n + 2, ld), float("nan"), device=DEV)
    block = wide[1:n + 1, 4:4 + W]                      # 16-byte aligned: what the first-order kernels ask of dL_dy
    block.copy_(T(c["dy"]))
    assert block.stride(0) == ld and block.data_ptr() % 16 == 0
    d_tab, d_dy = _bwd_bwd(ngp, gd, c, block, ld, c["v"])
    assert np.isfinite(d_tab).all() and np.isfinite(d_dy).all()
    R.compare(d_dy, r64["dL_ddLdy"], fl["dL_ddLdy"], "padded dL_ddLdy")
    R.compare(d_tab, r64["dtable2"], fl["dtable2"], "padded dtable2", rows=rows)
    _, d_dy_c = _bwd_bwd(ngp, gd, c, T(c["dy"]), W, c["v"], want_dtable=False)
    assert np.array_equal(d_dy, d_dy_c)                 # dL_ddLdy does not read dL_dy at all
    dx = _Guarded(n * 3, 64, 64, fill=SENTINEL)
    ngp._lib.call("grid_bwd_input", gd, T(c["table"]), T(c["x"]), block, ld, n, dx.body)
    R.compare(dx.result("dL_dx").reshape(n, 3), r64["dL_dx"], fl["dL_dx"], "padded dL_dx")
    dt = _Guarded(lay.n_params, GUARD, GUARD)
    ngp._lib.call("grid_bwd_param", gd, T(c["x"]), block, ld, n, dt.body)
    R.compare(dt.result("dtable"), r64["dtable"], fl["dtable"], "padded dtable", rows=rows)
    assert bool(torch.isnan(wide[0]).all()) and bool(torch.isnan(wide[:, :4]).all()) and bool(torch.isnan(wide[:, 4 + W:]).all())


def test_double_backward_with_one_output_null(ngp):
    c, r64, _, fl = R.case_reference(VARIANT)
    gd = _desc(ngp, c)
    W, dy = c["layout"].width, T(c["dy"])
    _, d_dy_both = _bwd_bwd(ngp, gd, c, dy, W, c["v"])
    d_tab, none = _bwd_bwd(ngp, gd, c, dy, W, c["v"], want_ddy=False)        # same stream
    _, d_dy = _bwd_bwd(ngp, gd, c, dy, W, c["v"], want_dtable=False)
    assert none is None and np.array_equal(d_dy, d_dy_both)                 # bit-identical
    R.compare(d_tab, r64["dtable2"], fl["dtable2"], "NULL dL_ddLdy: dtable2", rows=r64["rows"])


def test_double_backward_adds_to_a_running_sum(ngp):
    c, r64, r32, _ = R.case_reference(VARIANT)
    lay, rows = c["layout"], r64["rows"]
    gd = _desc(ngp, c)
    pre = np.random.default_rng(5407).standard_normal(lay.n_params).astype(np.float32)
    d_tab, _ = _bwd_bwd(ngp, gd, c, T(c["dy"]), lay.width, c["v"], want_ddy=False, prefill=pre)
    pre2, got2 = pre.reshape(-1, lay.n_features), d_tab.reshape(-1, lay.n_features)
    untouched = np.ones(lay.n_rows, bool)
    untouched[rows] = False
    assert np.array_equal(got2[untouched], pre2[untouched])                 # no other row moved
    want = pre2[rows].astype(np.float64) + r64["dtable2"]
    floor = R.floor_of(pre2[rows] + r32["dtable2"].astype(np.float32), want)  # the floor of the sum
    R.compare(got2[rows], want, floor, "prefilled dtable2")


def test_double_backward_zero_dL_dy_rows_add_nothing(ngp):
    """samples whose dL_dy row is all zero contribute exactly nothing to dtable: the result is the one of the batch
    without them, rows that only they touch stay exactly zero; their dL_ddLdy rows are written all the same"""
    c, r64, _, fl = R.case_reference(VARIANT)
    lay = c["layout"]
    gd = _desc(ngp, c)
    keep = np.ones(c["n"], bool)
    keep[100:180] = False
    dy = c["dy"].copy()
    dy[~keep] = 0
    sub64 = R.grid_orders(c["table"], c["x"][keep], lay, c["dy"][keep], c["v"][keep])
    sub32 = R.grid_orders(c["table"], c["x"][keep], lay, c["dy"][keep], c["v"][keep], dtype=torch.float32)
    assert len(sub64["rows"]) < len(r64["rows"])
    d_tab, d_dy = _bwd_bwd(ngp, gd, c, T(dy), lay.width, c["v"])
    R.compare(d_tab, sub64["dtable2"], R.floor_of(sub32["dtable2"], sub64["dtable2"]), "zero dL_dy rows: dtable2",
              rows=sub64["rows"])
    R.compare(d_dy, r64["dL_ddLdy"], fl["dL_ddLdy"], "zero dL_dy rows: dL_ddLdy")
    assert np.abs(d_dy[~keep]).max() > 0.1 * np.abs(r64["dL_ddLdy"]).max()


def test_double_backward_zero_v_rows_give_zero_rows(ngp):
    c, _, _, _ = R.case_reference(VARIANT)
    lay = c["layout"]
    gd = _desc(ngp, c)
    v = c["v"].copy()
    v[60:130] = 0
    z64 = R.grid_orders(c["table"], c["x"], lay, c["dy"], v)
    z32 = R.grid_orders(c["table"], c["x"], lay, c["dy"], v, dtype=torch.float32)
    d_tab, d_dy = _bwd_bwd(ngp, gd, c, T(c["dy"]), lay.width, v)
    assert not d_dy[60:130].any()                                            # exactly 0.0, and written (no SENTINEL left)
    R.compare(d_dy, z64["dL_ddLdy"], R.floor_of(z32["dL_ddLdy"], z64["dL_ddLdy"]), "zero v rows: dL_ddLdy")
    R.compare(d_tab, z64["dtable2"], R.floor_of(z32["dtable2"], z64["dtable2"]), "zero v rows: dtable2", rows=z64["rows"])


# ---------------------------------------------------------------------------------------------- (b), (c) the field
_FIELDS = {}


def _field(ngp, scale):
    """the model, its inputs on the device and the float64 reference of the case, built once"""
    if scale in _FIELDS:
        return _FIELDS[scale]
    torch.manual_seed(5)
    model = ngp.networks.NGP(scale=scale).to(DEV)
    with torch.no_grad():            # tcnn's 1e-4 init makes every feature ~0: an O(1) table for a real test
        model.xyz_encoder.params.uniform_(-0.3, 0.3)
    model.differentiable_normals = True
    pts = R.field_points(scale)
    lay = R.field_layout(scale)
    assert lay.n_params == model.xyz_encoder.params.numel()
    # input plumbing, not what is under test: the normalised positions are the device's, bit for bit
    lo, hi = np.float32(-scale), np.float32(scale)
    xn = (pts["x"] - lo) / (hi - lo)
    x = T(pts["x"])
    assert np.array_equal(N((x - model.xyz_min) / (model.xyz_max - model.xyz_min)), xn)
    assert xn.min() == 0 and xn.max() == 1
    span = N(model.xyz_max - model.xyz_min).reshape(3)
    lin1, lin2 = model.xyz_net[0], model.xyz_net[2]
    p = dict(table=N(model.xyz_encoder.params), W1=N(lin1.weight), b1=N(lin1.bias), W2=N(lin2.weight), b2=N(lin2.bias))
    args = (p, xn, span, pts["g_sigma"], pts["g_normals"], lay)
    r64, r32 = R.density_field(*args), R.density_field(*args, dtype=torch.float32)
    floors = {k: R.floor_of(r32[k], r64[k]) for k in R.FIELD_KEYS}
    _FIELDS[scale] = (model, pts, r64, r32, floors)
    return _FIELDS[scale]


def _field_loss(model, pts):
    sig, _, n_raw, _, _ = model(T(pts["x"]), T(pts["d"]))
    return sig, n_raw, (sig * T(pts["g_sigma"])).sum() + (n_raw * T(pts["g_normals"])).sum()


def _field_params(model):
    return [model.xyz_encoder.params, model.xyz_net[0].weight, model.xyz_net[0].bias, model.xyz_net[2].weight,
            model.xyz_net[2].bias]


@pytest.mark.parametrize("scale", [0.5, 8.0])
def test_field_second_order_matches_reference(ngp, scale):
    model, pts, r64, _, fl = _field(ngp, scale)
    sig, n_raw, loss = _field_loss(model, pts)
    grads = torch.autograd.grad(loss, _field_params(model))
    tag = f"field s={scale:g} "
    R.compare(N(sig), r64["sigma"], fl["sigma"], tag + "sigma")
    R.compare(N(n_raw), r64["normals"], fl["normals"], tag + "normals")
    R.compare(N(grads[0]), r64["table"], fl["table"], tag + "table", rows=r64["rows"])
    for k, g in zip(("W1", "b1", "W2", "b2"), grads[1:]):
        R.compare(N(g), r64[k], fl[k], tag + k)
    if scale != 0.5:
        del _FIELDS[scale]           # the tables of a model are 1.3 GB


@pytest.mark.parametrize("prefilled", [False, True])
def test_trainer_owned_gradient_buffer_gets_both_orders_once(ngp, prefilled):
    """params.grad is a view of the trainer's flat gradient and enc.grad_buffer is that view: the first-order scatter adds
    to it directly, the double backward's share arrives through autograd.  The buffer must end as (what it held) + the
    reference gradient: each share exactly once."""
    model, pts, r64, r32, fl = _field(ngp, 0.5)
    enc, rows = model.xyz_encoder, r64["rows"]
    Fd = enc.n_features
    flat = torch.zeros(enc.params.numel() + 256, device=DEV)                 # (a trainer's buffer holds more than one table)
    view = flat[128:128 + enc.params.numel()]
    if prefilled:
        view.copy_(torch.randn(view.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(11)))
    before = view.clone()
    small = _field_params(model)[1:]
    try:
        enc.params.grad = view
        enc.grad_buffer = enc.params.grad
        _, _, loss = _field_loss(model, pts)
        loss.backward()
        torch.cuda.synchronize()
        assert enc.params.grad.data_ptr() == view.data_ptr()                # autograd added in place
        moved = torch.nonzero((view != before).view(-1, Fd).any(1)).reshape(-1).cpu().numpy()
        assert np.isin(moved, rows).all(), "rows that no sample touches changed"
        got = N(view.view(-1, Fd)[T(rows)])
        pre = N(before.view(-1, Fd)[T(rows)])
        want = pre.astype(np.float64) + r64["table"]
        floor = R.floor_of(pre + r32["table"].astype(np.float32), want) if prefilled else fl["table"]
        tag = "trainer buffer, prefilled: " if prefilled else "trainer buffer: "
        R.compare(got, want, floor, tag + "table")
        assert not flat[:128].any() and not flat[-128:].any()
        for k, p in zip(("W1", "b1", "W2", "b2"), small):
            R.compare(N(p.grad), r64[k], fl[k], tag + k)
    finally:
        enc.grad_buffer = None
        enc.params.grad = None
        for p in small:
            p.grad = None

