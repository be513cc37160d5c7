"""The float64 reference of the grid and of the density field up to second order (tests/second_order_reference.py) is
itself checked here, without a GPU: its layout rule and cells against the C oracle's and the library's, its values
against the oracle's five grid functions on every case of tests/test_second_order_gpu.py, its comparison routine against
damaged copies of a result, and the argument checks of ngp_grid_bwd_bwd_input (which return before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
import second_order_reference as R

CASE_NAMES = sorted(R.CASES)


def _oracle_desc(args):
    return oracle.grid_layout(*args)


# ---------------------------------------------------------------------------------------------- layout and cells
@pytest.mark.parametrize("args", list(R.LAYOUTS.values()) + [
    (16, 8, 19, 16, float(np.exp(np.log(2048 * s / 16) / 15))) for s in (0.5, 8.0)])
def test_layout_matches_oracle_and_library(ngp, args):
    lay = R.grid_layout(*args)
    desc, n_params = _oracle_desc(args)
    gd = ngp._lib.GridDesc()
    assert ngp._lib.call_host("grid_layout", *args, gd) == n_params == lay.n_params
    L = lay.n_levels
    for d in (desc, gd):
        assert (d.n_levels, d.n_features) == (L, lay.n_features)
        assert list(d.offsets[:L + 1]) == list(lay.offset)
        assert list(d.resolution[:L]) == list(lay.res)
        assert np.array_equal(np.asarray(d.scale[:L], np.float32), np.asarray(lay.scale, np.float32))   # bit-equal


def test_layouts_cover_dense_and_hashed_levels():
    lay = {k: R.grid_layout(*a) for k, a in R.LAYOUTS.items()}
    assert any(lay["A"].hashed) and not all(lay["A"].hashed) and 1000 < lay["A"].scale[-1] < 1100
    assert not any(lay["E"].hashed)
    assert any(lay["B"].hashed) and any(lay["C"].hashed) and any(lay["D"].hashed)
    # the launch of ngp_grid_bwd_bwd_input has n * L * F threads: below one workgroup of 256 on D
    assert 77 * lay["D"].width == 231 and 1 * lay["D"].width == 3


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cells_identical_to_oracle(name):
    """(g, w) of every point on every level: the oracle's scatter of unit gradients adds the eight float32 corner weights
    of each cell to the eight rows of its corners, sample by sample.  The same sums made here from the reference's cells
    and rows, with the same float32 operations in the same order, must give the same table bit for bit."""
    c = R.make_case(name)
    lay = c["layout"]
    desc, n_params = _oracle_desc(c["args"])
    want = oracle.grid_bwd_param(desc, c["x"], np.ones((c["n"], lay.width), np.float32), n_params)
    g, w = R.cells(lay, c["x"])
    rows = R.corner_rows(lay, g)
    wt = np.ones(rows.shape, np.float32)
    for corner in range(8):
        for k in range(3):
            wt[:, :, corner] *= w[:, :, k] if (corner >> k) & 1 else np.float32(1) - w[:, :, k]
    mine = np.zeros(lay.n_rows, np.float32)
    np.add.at(mine, rows.reshape(-1), wt.reshape(-1))          # unbuffered: one float32 addition per corner, in order
    assert np.array_equal(want.reshape(lay.n_rows, lay.n_features), np.repeat(mine[:, None], lay.n_features, 1))


def test_crafted_points_sit_where_they_should():
    for name in ("A-crafted", "D-crafted"):
        c = R.make_case(name)
        lay, x = c["layout"], c["x"]
        g, w = R.cells(lay, x)
        assert x[0].tolist() == [0, 0, 0] and x[1].tolist() == [1, 1, 1] and x[2].tolist() == [0.5, 0.25, 0.75]
        # rows 3..6: exactly on faces of the coarsest level; rows 7..10: of the finest
        assert w[3, 0, 0] == 0 and w[4, 0, 1] == 0 and w[5, 0, 2] == 0 and not w[6, 0].any()
        assert w[7, -1, 0] == 0 and w[8, -1, 1] == 0 and w[9, -1, 2] == 0 and not w[10, -1].any()
        assert w[11, 0, 0] == 0 and w[11, -1, 1] == 0
        # rows 12.., one float32 below: the cell before, at its far end
        assert g[12, 0, 0] == g[3, 0, 0] - 1 and w[12, 0, 0] > 0.999
        assert g[14, -1, 0] == g[7, -1, 0] - 1 and w[14, -1, 0] > 0.9
    c = R.make_case("A-outside")
    inside = ((c["x"] >= 0) & (c["x"] <= 1)).all(1)
    assert inside[::5].all() and inside.sum() < 0.3 * c["n"] and c["x"].min() < -3 and c["x"].max() > 4
    for name in ("A-dup", "C-dup"):
        x = R.make_case(name)["x"]
        assert (x == x[np.argmax((x == np.float32(0.3137)).any(1))]).all(1).sum() == R.N_DUP


# ---------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_matches_oracle(name):
    """the oracle (float32 C, hand-derived first and second order) is one more float32 party here: within 8 x the floor"""
    c, r64, _, floors = R.case_reference(name)
    desc, n_params = _oracle_desc(c["args"])
    rows = r64["rows"]
    R.compare(oracle.grid_fwd(desc, c["table"], c["x"]), r64["y"], floors["y"], name + " y")
    R.compare(oracle.grid_bwd_input(desc, c["table"], c["x"], c["dy"]), r64["dL_dx"], floors["dL_dx"], name + " dL_dx")
    R.compare(oracle.grid_bwd_param(desc, c["x"], c["dy"], n_params), r64["dtable"], floors["dtable"], name + " dtable",
              rows=rows)
    d_tab, d_dy = oracle.grid_bwd_bwd_input(desc, c["table"], c["x"], c["dy"], c["v"])
    R.compare(d_dy, r64["dL_ddLdy"], floors["dL_ddLdy"], name + " dL_ddLdy")
    R.compare(d_tab, r64["dtable2"], floors["dtable2"], name + " dtable2", rows=rows)


def test_float32_evaluation_is_a_float32_distance_away():
    """the floors are float32 rounding, not something larger: below 1e-6 on every tensor of every kernel-level case"""
    for name in CASE_NAMES:
        floors = R.case_reference(name)[3]
        assert all(R.EPS32 <= f < 1e-6 for f in floors.values()), (name, floors)


def test_field_reference_runs_sparse_and_float32_stays_close():
    """density_field on the level geometry of NGP(scale = 0.5)'s density table (log2_T = 12 here, to keep the table small):
    it holds the touched rows only, its normals are unit vectors, every gradient is non-zero, and its float32 evaluation
    stays a float32 distance away (sums that cancel, such as the b2 gradient, reach 1e-5)."""
    lay = R.grid_layout(16, 8, 12, 16, float(np.exp(np.log(2048 * 0.5 / 16) / 15)))
    g = np.random.default_rng(7)
    p = dict(table=g.uniform(-0.3, 0.3, lay.n_params).astype(np.float32),
             W1=(g.standard_normal((128, 128)) * 0.1).astype(np.float32), b1=(g.standard_normal(128) * 0.1).astype(np.float32),
             W2=(g.standard_normal((1, 128)) * 0.1).astype(np.float32), b2=np.asarray([0.1], np.float32))
    pts = R.field_points(0.5)
    span = np.full(3, 1.0, np.float32)
    xn = (pts["x"] - np.float32(-0.5)) / span
    assert xn.min() == 0 and xn.max() == 1
    r64 = R.density_field(p, xn, span, pts["g_sigma"], pts["g_normals"], lay)
    r32 = R.density_field(p, xn, span, pts["g_sigma"], pts["g_normals"], lay, dtype=torch.float32)
    assert len(r64["rows"]) < 200 * 16 * 8 and r64["table"].shape == (len(r64["rows"]), 8)
    assert np.allclose(np.linalg.norm(r64["normals"], axis=1), 1, atol=1e-9)
    for k in R.FIELD_KEYS:
        assert r64[k].any() and R.floor_of(r32[k], r64[k]) < 2e-5, k


# ---------------------------------------------------------------------------------------------- compare() can fail
def test_compare_rejects_damaged_copies():
    c, r64, r32, floors = R.case_reference("A-random")
    lay, rows, Fd = c["layout"], r64["rows"], c["layout"].n_features
    fl = floors["dtable2"]

    def full(u):                                       # (U, F) rows -> the whole flat table gradient, float32
        t = np.zeros((lay.n_rows, Fd), np.float32)
        t[rows] = u
        return t.reshape(-1)

    # a float32 evaluation of the same thing is accepted
    R.compare(full(r32["dtable2"]), r64["dtable2"], fl, "float32 dtable2", rows=rows)
    R.compare(r32["dL_ddLdy"].astype(np.float32), r64["dL_ddLdy"], floors["dL_ddLdy"], "float32 dL_ddLdy")
    # one corner's sign flipped (corner 5 of level 9), one level's scale dropped from the second-order coefficient
    for damage in (dict(_flip=(9, 5)), dict(_slope={12: 1.0})):
        bad = R.grid_orders(c["table"], c["x"], lay, c["dy"], c["v"], **damage)
        assert np.array_equal(bad["rows"], rows)
        with pytest.raises(AssertionError, match="above"):
            R.compare(full(bad["dtable2"]), r64["dtable2"], fl, f"damaged dtable2 {damage}", rows=rows)
        with pytest.raises(AssertionError, match="above"):
            R.compare(bad["dL_ddLdy"], r64["dL_ddLdy"], floors["dL_ddLdy"], f"damaged dL_ddLdy {damage}")
    # one touched row missing: a row that carries at least 1 % of the largest entry
    strong = np.flatnonzero(np.abs(r64["dtable2"]).max(1) >= 0.01 * np.abs(r64["dtable2"]).max())
    missing = r64["dtable2"].copy()
    missing[strong[len(strong) // 2]] = 0
    with pytest.raises(AssertionError, match="above"):
        R.compare(full(missing), r64["dtable2"], fl, "a touched row missing", rows=rows)
    # one untouched row set to 1e-9
    stray = full(r64["dtable2"]).reshape(-1, Fd)
    untouched = np.setdiff1d(np.arange(lay.n_rows), rows)
    stray[untouched[len(untouched) // 3], Fd - 1] = 1e-9
    with pytest.raises(AssertionError, match="no sample touches"):
        R.compare(stray.reshape(-1), r64["dtable2"], fl, "an untouched row written", rows=rows)
    # a non-finite value anywhere
    nan = r64["dL_ddLdy"].copy()
    nan[3, 7] = np.nan
    with pytest.raises(AssertionError, match="above"):
        R.compare(nan, r64["dL_ddLdy"], floors["dL_ddLdy"], "a NaN")


# ---------------------------------------------------------------------------------------------- argument checks
def test_grid_bwd_bwd_input_rejects_bad_arguments(ngp):
    """none of these reaches a launch: every data pointer that is not NULL is a host address"""
    lib = ngp._lib.load()
    f = lib.ngp_grid_bwd_bwd_input
    L, Fd = 4, 4
    gd = ngp._lib.GridDesc()
    assert ngp._lib.call_host("grid_layout", L, Fd, 12, 8, 1.5, gd) > 0
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    ok = dict(desc=C.addressof(gd), table=p, x=p, dy=p, lddy=L * Fd, v=p, n=2, dtable=p, ddy=p)

    def run(**kw):
        a = dict(ok, **kw)
        return f(a["desc"], a["table"], a["x"], a["dy"], a["lddy"], a["v"], a["n"], a["dtable"], a["ddy"], None)
    EINVAL = -22
    assert run(lddy=L * Fd - 1) == EINVAL
    assert run(n=-1) == EINVAL
    for k in ("table", "x", "dy", "v", "desc"):
        assert run(**{k: None}) == EINVAL, k
    assert run(n=0) == 0
    assert run(n=0, table=None, x=None, dy=None, v=None, dtable=None, ddy=None) == 0
    gd3 = ngp._lib.GridDesc.from_buffer_copy(gd)
    gd3.n_features = 3
    assert run(desc=C.addressof(gd3)) == EINVAL
    assert run(desc=C.addressof(gd3), n=0) == EINVAL
