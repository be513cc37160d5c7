"""A plain reference of the hash grid and of the density field up to second order, for the tests of the route
loss(normals_raw) -> d(sigma)/dx -> density table and xyz_net (ngp_grid_bwd_bwd_input, NGP.differentiable_normals).

numpy and torch on the CPU only; the C oracle is not used here.  The forward is a gather of 8 corners with trilinear
weights written in torch; EVERY gradient comes from torch.autograd on it (first order with create_graph=True, second
order with a second autograd.grad): nothing is derived by hand.  Each function evaluates in float64 (the reference) or
in float32 (the same graph, used only to measure what one float32 evaluation order costs against exact: the floor the
bars of the tests are built on).

Layout rule (restated):
  scale_l = exp2(l * log2(per_level_scale)) * base - 1     in float32
  res_l   = ceil(scale_l) + 1
  size_l  = min(round_up_8(res_l^3), 2^log2_T)              rows of the level, the levels lie back to back
  hashed  iff size_l < stride, stride = the value reached by `stride = 1; for d in x, y, z while stride <= size_l:
          stride *= res_l`
  row     = (x + y * res + z * res^2) % size  (dense)   or   (x ^ y * 2654435761 ^ z * 805459861) % size  (hashed),
          both in uint32 arithmetic (wrap) before the modulo

Cell of a point (what every comparison hangs on): pos = float32(float64(scale) * float64(x) + 0.5), the one rounding
fmaf makes; g = (uint32)(int)floor(pos); w = pos - floor(pos) in float32.  w enters the graph as the constant
w + scale * (xvar - xvar.detach()): its value is the float32 cell's, its slope is `scale`, everything behind it runs in
the evaluation dtype.  No point is borderline under this rule and the tests leave none out.

The table is never built dense: a graph holds the unique rows its points touch (`rows`), gathered from the caller's
float32 table."""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23          # the floors are clamped here from below
FACTOR = 8.0                # bar = FACTOR * floor (tests/test_second_order_gpu.py says why)


# ---------------------------------------------------------------------------------------------- layout
@dataclass(frozen=True)
class Layout:
    n_levels: int
    n_features: int
    scale: tuple      # float32 values
    res: tuple
    size: tuple
    offset: tuple     # n_levels + 1 entries, in rows
    hashed: tuple

    @property
    def n_rows(self):
        return self.offset[-1]

    @property
    def n_params(self):
        return self.offset[-1] * self.n_features

    @property
    def width(self):
        return self.n_levels * self.n_features


def grid_layout(n_levels, n_features, log2_T, base, per_level_scale):
    l2 = np.float32(np.log2(np.float64(np.float32(per_level_scale))))
    scale, res, size, offset, hashed = [], [], [], [0], []
    for l in range(n_levels):
        e = np.float32(l) * l2                                                  # float32 product
        sc = np.float32(np.float32(np.exp2(np.float64(e))) * np.float32(base)) - np.float32(1.0)
        r = int(np.ceil(sc)) + 1
        s = min((r ** 3 + 7) // 8 * 8, 1 << log2_T)
        stride = 1
        for _ in range(3):
            if stride > s:
                break
            stride *= r
        scale.append(np.float32(sc))
        res.append(r)
        size.append(s)
        offset.append(offset[-1] + s)
        hashed.append(s < stride)
    return Layout(n_levels, n_features, tuple(scale), tuple(res), tuple(size), tuple(offset), tuple(hashed))


def cells(layout, x):
    """x (n, 3) float32 -> g (n, L, 3) uint32, w (n, L, 3) float32"""
    x = np.ascontiguousarray(x, np.float32)
    g = np.empty((len(x), layout.n_levels, 3), np.uint32)
    w = np.empty((len(x), layout.n_levels, 3), np.float32)
    for l, sc in enumerate(layout.scale):
        pos = (np.float64(sc) * x.astype(np.float64) + 0.5).astype(np.float32)
        fl = np.floor(pos)
        g[:, l] = fl.astype(np.int32).view(np.uint32)
        w[:, l] = pos - fl
    return g, w


def corner_rows(layout, g):
    """g (n, L, 3) uint32 -> rows (n, L, 8) int64 into the whole table; bit 0 / 1 / 2 of the corner number = the upper
    neighbour in x / y / z"""
    rows = np.empty(g.shape[:2] + (8,), np.int64)
    M = np.uint64(0xFFFFFFFF)
    for l in range(layout.n_levels):
        for c in range(8):
            q = [(g[:, l, k].astype(np.uint64) + np.uint64((c >> k) & 1)) & M for k in range(3)]
            if layout.hashed[l]:
                idx = q[0] ^ ((q[1] * np.uint64(2654435761)) & M) ^ ((q[2] * np.uint64(805459861)) & M)
            else:
                r = np.uint64(layout.res[l])
                idx = (q[0] + ((q[1] * r) & M) + ((((q[2] * r) & M) * r) & M)) & M
            rows[:, l, c] = layout.offset[l] + (idx % np.uint64(layout.size[l])).astype(np.int64)
    return rows


# ---------------------------------------------------------------------------------------------- the grid
def encode(table, x, layout, dtype=torch.float64, _flip=None, _slope=None):
    """table: the flat float32 table (numpy, n_params values); x (n, 3) float32.
    -> y (n, L*F) with its graph, tab (U, F) leaf: the touched rows, xvar (n, 3) leaf, rows (U,) int64 sorted.
    _flip = (level, corner) / _slope = {level: slope}: a wrong sign of one corner / a wrong slope of one level's
    weights, for the self-test of `compare` only."""
    x = np.ascontiguousarray(x, np.float32)
    g, w = cells(layout, x)
    rows_all = corner_rows(layout, g)
    rows, inv = np.unique(rows_all, return_inverse=True)
    inv = torch.from_numpy(inv.reshape(rows_all.shape))
    Fd = layout.n_features
    tab = torch.from_numpy(np.asarray(table, np.float32).reshape(-1, Fd)[rows]).to(dtype).requires_grad_(True)
    xvar = torch.from_numpy(x).to(dtype).requires_grad_(True)
    slide = xvar - xvar.detach()
    out = []
    for l in range(layout.n_levels):
        slope = float(layout.scale[l]) if _slope is None or l not in _slope else _slope[l]
        wv = torch.from_numpy(w[:, l]).to(dtype) + torch.tensor(slope, dtype=dtype) * slide
        acc = 0
        for c in range(8):
            wt = 1
            for k in range(3):
                wt = wt * (wv[:, k] if (c >> k) & 1 else 1 - wv[:, k])
            if _flip == (l, c):
                wt = -wt
            acc = acc + wt[:, None] * tab[inv[:, l, c]]
        out.append(acc)
    return torch.cat(out, 1), tab, xvar, rows


def grid_orders(table, x, layout, dL_dy, v, row_scale=None, dtype=torch.float64, **damage):
    """Everything the grid kernels compute, from autograd on encode():
      y, dL_dx = J^T dL_dy, dtable = d<y, dL_dy>/dtable (and dtable_scaled with dL_dy * row_scale[:, None]),
      dL_ddLdy, dtable2 = d<v, dL_dx>/d(dL_dy), /dtable.
    -> dict of numpy float64 arrays; the table gradients are (U, F) on `rows`."""
    y, tab, xvar, rows = encode(table, x, layout, dtype, **damage)
    dy = torch.from_numpy(np.ascontiguousarray(dL_dy, np.float32)).to(dtype).requires_grad_(True)
    vt = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dtype)
    dx, dtable = torch.autograd.grad(y, [xvar, tab], dy, create_graph=True)
    ddy, dtable2 = torch.autograd.grad(dx, [dy, tab], vt, retain_graph=True)
    out = dict(y=y, dL_dx=dx, dtable=dtable, dL_ddLdy=ddy, dtable2=dtable2)
    if row_scale is not None:
        rs = torch.from_numpy(np.ascontiguousarray(row_scale, np.float32)).to(dtype)
        (out["dtable_scaled"],) = torch.autograd.grad(y, tab, dy.detach() * rs[:, None], retain_graph=True)
    out = {k: t.detach().double().numpy() for k, t in out.items()}
    out["rows"] = rows
    return out


# ---------------------------------------------------------------------------------------------- the density field
FIELD_KEYS = ("sigma", "normals", "table", "W1", "b1", "W2", "b2")


def density_field(params, xn, span, g_sigma, g_normals, layout, dtype=torch.float64):
    """params: table (flat float32), W1 (128, L*F), b1 (128,), W2 (1, 128), b2 (1,) as numpy float32; xn (n, 3) float32
    in the unit cube; span (3,) = xyz_max - xyz_min.
      feat = encode; h = softplus(feat W1^T + b1); sigma = softplus(h W2^T + b2)[:, 0]
      grads = d(sum sigma)/dxn / span; normals = -normalize(grads, eps 1e-6)
      loss = sum(sigma * g_sigma) + sum(normals * g_normals)
    -> dict: sigma, normals, and d(loss)/d(table rows, W1, b1, W2, b2) as numpy float64; rows."""
    feat, tab, xvar, rows = encode(params["table"], xn, layout, dtype)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)
    W1, b1, W2, b2 = (t(params[k]).requires_grad_(True) for k in ("W1", "b1", "W2", "b2"))
    h = F.softplus(F.linear(feat, W1, b1))
    sigma = F.softplus(F.linear(h, W2, b2))[:, 0]
    (dxn,) = torch.autograd.grad(sigma, xvar, torch.ones_like(sigma), create_graph=True)
    grads = dxn / t(span).reshape(1, 3)
    normals = -F.normalize(grads, p=2, dim=-1, eps=1e-6)
    loss = (sigma * t(g_sigma)).sum() + (normals * t(g_normals)).sum()
    g = torch.autograd.grad(loss, [tab, W1, b1, W2, b2])
    out = dict(zip(FIELD_KEYS, (sigma, normals) + g))
    out = {k: v.detach().double().numpy() for k, v in out.items()}
    out["rows"] = rows
    return out


# ---------------------------------------------------------------------------------------------- comparison
def max_normalised(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def floor_of(ref32, ref64):
    """what one float32 evaluation order costs against exact on this case, clamped at 2^-23"""
    return max(max_normalised(ref32, ref64), EPS32)


def compare(got, want, floor, name, rows=None, factor=FACTOR):
    """max |got - want| / max |want| over every element must be within factor * max(floor, 2^-23).
    rows: `got` is a whole table gradient (n_rows * F values) and `want` its (U, F) rows: every other row of `got`
    must be exactly zero.  -> the error."""
    want = np.asarray(want, np.float64)
    got = np.asarray(got)
    if rows is not None:
        got2 = got.reshape(-1, want.shape[1])
        inside = got2[rows]
        stray = int(np.count_nonzero(got2)) - int(np.count_nonzero(inside))
        assert stray == 0, f"{name}: {stray} non-zero values in rows that no sample touches"
        got = inside
    floor = max(float(floor), EPS32)
    err = max_normalised(got.reshape(want.shape), want)
    print(f"[second-order] {name}: floor {floor:.2e}  error {err:.2e}  ({err / floor:.2f} x floor, bar {factor:g} x)")
    assert err <= factor * floor, f"{name}: error {err:.3e} above {factor:g} x floor {floor:.3e}"
    return err


# ---------------------------------------------------------------------------------------------- cases
#        L   F  log2_T base per_level_scale
LAYOUTS = {
    "A": (16, 8, 15, 16, 1.3195079107728942),     # dense and hashed levels, finest scale about 1000
    "B": (8, 2, 16, 16, 2.0),                     # the mask field's layout
    "C": (4, 4, 12, 8, 1.5),
    "D": (3, 1, 10, 4, 2.0),                      # n * L * F below one workgroup
    "E": (2, 8, 19, 4, 1.5),                      # dense levels only
}
#        name: (layout, point set, n)
CASES = {
    "A-random": ("A", "random", 257), "B-random": ("B", "random", 100), "C-random": ("C", "random", 65),
    "D-random": ("D", "random", 77), "D-one": ("D", "random", 1), "E-random": ("E", "random", 130),
    "A-crafted": ("A", "crafted", 40), "D-crafted": ("D", "crafted", 40),
    "A-outside": ("A", "outside", 130), "B-outside": ("B", "outside", 100),
    "A-dup": ("A", "dup", 130), "C-dup": ("C", "dup", 100),
}
N_DUP = 64


def faces_of(scale):
    """the x = (k - 0.5) / scale inside (0, 1) that float32 arithmetic puts exactly on a cell face: pos == k ..."""
    k = np.arange(1, min(int(scale), 4096) + 1)
    x = ((k - 0.5) / np.float64(scale)).astype(np.float32)
    at = lambda a: (np.float64(scale) * a.astype(np.float64) + 0.5).astype(np.float32)
    # ... and whose float32 neighbour below lies in the cell before (it may round back onto the face on a coarse level)
    x = x[(at(x) == k) & (x > 0) & (x < 1) & (at(np.nextafter(x, np.float32(-1))) < k)]
    assert len(x) >= 2, f"no exact faces for scale {scale}"
    return x


def crafted_points(layout, g, n):
    """(0,0,0), (1,1,1), (0.5,0.25,0.75), points exactly on cell faces of the coarsest and the finest level (one, two
    and three coordinates at once), the float32 value just below such a face, random points behind them"""
    c, f = faces_of(layout.scale[0]), faces_of(layout.scale[-1])
    f0, f0b, f1, f1b = c[0], c[-1], f[1], f[len(f) // 2]
    below = lambda a: np.nextafter(np.float32(a), np.float32(-1))
    r = lambda: np.float32(g.random())
    pts = [(0, 0, 0), (1, 1, 1), (0.5, 0.25, 0.75),
           (f0, r(), r()), (r(), f0b, r()), (r(), r(), f0), (f0, f0b, f0),
           (f1, r(), r()), (r(), f1b, r()), (r(), r(), f1), (f1, f1b, f1b), (f0, f1, r()),
           (below(f0), r(), r()), (r(), below(f0b), below(f0)), (below(f1), r(), r()), (r(), below(f1b), below(f1)),
           (below(f0), below(f1), below(f1b)), (below(1), below(1), below(1))]
    x = g.random((n, 3)).astype(np.float32)
    x[:len(pts)] = np.asarray(pts, np.float32)
    return x


def make_points(layout, kind, n, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        return g.random((n, 3)).astype(np.float32)
    if kind == "crafted":
        return crafted_points(layout, g, n)
    if kind == "outside":                          # [-3.7, 4.3]^3, every fifth inside the cube
        x = (g.random((n, 3)) * 8.0 - 3.7).astype(np.float32)
        x[::5] = g.random((len(x[::5]), 3)).astype(np.float32)
        return x
    if kind == "dup":                              # N_DUP copies of one interior point scattered among random ones
        x = g.random((n, 3)).astype(np.float32)
        x[g.permutation(n)[:N_DUP]] = np.asarray([0.3137, 0.4242, 0.5151], np.float32)
        return x
    raise KeyError(kind)


def make_case(name):
    """-> dict: layout args, Layout, and the seeded inputs of a kernel-level case (all float32)"""
    lname, kind, n = CASES[name]
    args = LAYOUTS[lname]
    layout = grid_layout(*args)
    seed = 52000 + sorted(CASES).index(name)
    g = np.random.default_rng(seed)
    return dict(name=name, args=args, layout=layout, n=n, x=make_points(layout, kind, n, seed + 500),
                table=g.uniform(-1, 1, layout.n_params).astype(np.float32),
                dy=g.standard_normal((n, layout.width)).astype(np.float32),
                v=g.standard_normal((n, 3)).astype(np.float32),
                row_scale=g.uniform(0.25, 2.0, n).astype(np.float32))


_REFS = {}


def case_reference(name):
    """(case, float64 reference, floors per tensor), computed once per process and left unchanged"""
    if name not in _REFS:
        c = make_case(name)
        r64 = grid_orders(c["table"], c["x"], c["layout"], c["dy"], c["v"], c["row_scale"])
        r32 = grid_orders(c["table"], c["x"], c["layout"], c["dy"], c["v"], c["row_scale"], dtype=torch.float32)
        floors = {k: floor_of(r32[k], r64[k]) for k in r64 if k != "rows"}
        _REFS[name] = (c, r64, r32, floors)
    return _REFS[name]


# ---------------------------------------------------------------------------------------------- field cases
def field_layout(scale):
    """the density table of networks.NGP(scale)"""
    b = np.exp(np.log(2048 * scale / 16) / 15)
    return grid_layout(16, 8, 19, 16, b)


def field_points(scale, n=200, seed=0):
    """n points of the box [-scale, scale]^3: N_DUP copies of one point, points on the box faces and corners, random ones"""
    g = np.random.default_rng(53000 + seed)
    s = np.float32(scale)
    x = ((g.random((n, 3)) * 2 - 1) * scale).astype(np.float32)
    faces = [(-s, 0.1 * s, 0.3 * s), (0.2 * s, s, -0.4 * s), (0.5 * s, -0.7 * s, -s), (s, s, s), (-s, -s, -s), (s, -s, 0)]
    x[g.permutation(n - len(faces))[:N_DUP]] = np.asarray([0.2274, -0.1516, 0.0303], np.float32) * (2 * s)
    x[n - len(faces):] = np.asarray(faces, np.float32)
    return dict(x=x, d=g.standard_normal((n, 3)).astype(np.float32), g_sigma=g.standard_normal(n).astype(np.float32),
                g_normals=g.standard_normal((n, 3)).astype(np.float32))
