"""Plain numpy restatement of the sampled occupancy-grid update (ngp_grid_sample_cells, ngp_density_grid_scatter_max,
ngp_density_grid_ema_threshold, ngp_packbits), written from include/ngp_hip.h and the kernel comments of
csrc/ray_kernels.hip.  Integers are uint64 with wrap-around, points are float64, the EMA is float32.

Every random quantity is a pure function of (seed, sample id, draw): hash64 is the SplitMix64 finaliser of
seed + 0x9E3779B97F4A7C15 * (id*8 + draw + 1), hash_u32 its top 32 bits, rand_below(n) = (hash_u32 * n) >> 32.
Draws 0..2 pick a uniform cell, draw 3 the occupied cell, draws 4..6 the jitter of the point.

The module also holds the cases of tests/test_grid_update_gpu.py (CASES, built by make_case) and the comparison of
a device result with the reference (check_samples), so that tests/test_grid_update_host.py can check both without
a GPU."""
import numpy as np

import oracle

GOLDEN = 0x9E3779B97F4A7C15
U64 = np.uint64
SORT_BITS = 21          # 8 bucket bits + 13 bits ordered inside a bucket


def _u64(v):
    return np.asarray(v).astype(np.int64).astype(U64) if np.asarray(v).dtype.kind == "i" else np.asarray(v, U64)


def hash64(seed, ids, draw):
    """seed: any Python int, taken modulo 2^64 (an int64 seed of -1 is 2^64 - 1); ids: integer array; draw: int"""
    with np.errstate(over="ignore"):
        ids = _u64(ids)
        z = U64(int(seed) % 2 ** 64) + U64(GOLDEN) * (ids * U64(8) + U64(int(draw) + 1))
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def hash_u32(seed, ids, draw):
    return hash64(seed, ids, draw) >> U64(32)


def rand_below(seed, ids, draw, n):
    return (hash_u32(seed, ids, draw) * U64(n)) >> U64(32)       # < 2^32 * 2^30: no wrap


def _spread3(v):
    v = v.astype(U64)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> U64(b)) & U64(1)) << U64(3 * b)
    return out


def morton(x, y, z):
    return _spread3(x) | (_spread3(y) << U64(1)) | (_spread3(z) << U64(2))


def morton_invert(keys):
    keys = np.asarray(keys).astype(U64)
    out = np.zeros(keys.shape + (3,), np.int64)
    for k in range(3):
        for b in range(10):
            out[..., k] |= (((keys >> U64(3 * b + k)) & U64(1)) << U64(b)).astype(np.int64)
    return out


def key_bits(G):
    bits = 3 * (int(G).bit_length() - 1)
    assert 2 <= G <= 1024 and 1 << (bits // 3) == G, "grid_size must be a power of two in 2..1024"
    return bits


def sort_shift(G):
    return max(0, key_bits(G) - SORT_BITS)


def occupied(grid, thr):
    """ascending list of the cells with grid > thr: strict, NaN is not occupied"""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.asarray(grid, np.float32) > np.float32(thr)).astype(np.int64)


def sample_cells(occ, G, m, seed, s):
    """-> (keys (2m,) int64, sids (2m,) int64, xyz (2m,3) float64) in sample order (the device orders its rows by
    keys >> sort_shift(G), see check_samples).  occ: occupied(grid, thr)."""
    key_bits(G)
    i = np.arange(2 * m, dtype=np.int64)
    sids = i.copy()
    if len(occ) == 0:
        sids[m:] -= m                                            # an exact repeat of the uniform half
    cell = [rand_below(seed, sids, k, G) for k in range(3)]
    keys = morton(*cell).astype(np.int64)
    if len(occ) > 0:
        keys[m:] = np.asarray(occ, np.int64)[rand_below(seed, i[m:], 3, len(occ)).astype(np.int64)]
    c = morton_invert(keys).astype(np.float64)
    s = float(s)
    u = np.stack([(hash_u32(seed, sids, 4 + k) >> U64(8)).astype(np.float64) / 2.0 ** 24 for k in range(3)], -1)
    xyz = (c / (G - 1) * 2 - 1) * (s - s / G) + (u * 2 - 1) * (s / G)
    return keys, sids, xyz


def point_tolerance(s):
    """Absolute, derived: roundings of c/(G-1), of (s - s/G) and of their product come to 4 * 2^-24 * s at most, the
    jitter term adds 2 * 2^-24 * s/G at most (u*2-1 is exact), the final add 2^-24 * s; contraction only lowers it."""
    return 8 * 2.0 ** -24 * float(s)


def check_samples(idx, xyz, ref, G, s):
    """Asserts that the device rows (idx (2m,), xyz (2m,3)) are the reference's rows `ref = sample_cells(...)` in a
    legal order.  Returns the number of keys that occur exactly once (the rows whose pairing is checked)."""
    keys, _, rxyz = ref
    idx = np.asarray(idx).astype(np.int64)
    xyz = np.asarray(xyz, np.float64)
    assert idx.shape == keys.shape and xyz.shape == rxyz.shape
    # 1. the multiset of cells: pins the count, the scan, the compaction and every draw
    od, orf = np.argsort(idx, kind="stable"), np.argsort(keys, kind="stable")
    bad = np.flatnonzero(idx[od] != keys[orf])
    assert bad.size == 0, f"multiset of indices differs at {bad.size} sorted positions, first: device " \
                          f"{idx[od][bad[:4]]} reference {keys[orf][bad[:4]]}"
    # 2. the order of the rows
    top = idx >> sort_shift(G)
    assert (np.diff(top) >= 0).all(), f"rows not ordered by idx >> {sort_shift(G)}"
    # 3. inside each group of equal key, each axis sorted on its own
    tol = point_tolerance(s)
    for k in range(3):
        a = xyz[np.lexsort((xyz[:, k], idx)), k]
        b = rxyz[np.lexsort((rxyz[:, k], keys)), k]
        err = np.abs(a - b)
        assert np.all(err <= tol), f"axis {k}: sorted-in-group values differ by {np.nanmax(err):.3e} > {tol:.3e}"
    # 4. keys that occur once: the whole row is the reference's row
    sk = idx[od]
    first = np.concatenate([[True], sk[1:] != sk[:-1]])
    last = np.concatenate([sk[1:] != sk[:-1], [True]])
    single = first & last
    err = np.abs(xyz[od][single] - rxyz[orf][single])
    assert np.all(err <= tol), f"singleton rows differ by {np.nanmax(err):.3e} > {tol:.3e}"
    return int(single.sum())


def singleton_share(keys, m):
    """share of the uniform samples (rows < m) whose key no other of the 2m rows has"""
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    return float((cnt[inv[:m]] == 1).mean())


# ---------------------------------------------------------------------------- scatter, EMA, threshold, packbits
def scatter_max(tmp0, idx, sigma):
    """tmp[j] = max(tmp0[j], the largest sigma > 0 written to j); sigmas that are 0, -0.0, negative or NaN are ignored"""
    tmp = np.array(tmp0, np.float32)
    sigma = np.asarray(sigma, np.float32)
    with np.errstate(invalid="ignore"):
        ok = sigma > 0
    np.maximum.at(tmp, np.asarray(idx, np.int64)[ok], sigma[ok])
    return tmp


def ema(grid, tmp, decay):
    """float32: g < 0 keeps g, otherwise fmax(fl32(g * decay), tmp) — a NaN cell becomes tmp"""
    g = np.asarray(grid, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(g < 0, g, np.fmax(g * np.float32(decay), np.asarray(tmp, np.float32))).astype(np.float32)


def mean_positive(grid):
    """float64 mean of the cells > 0; 0 when there is none"""
    g = np.asarray(grid, np.float32)
    with np.errstate(invalid="ignore"):
        pos = g[g > 0]
    return float(pos.astype(np.float64).mean()) if pos.size else 0.0


def threshold_rel_bound(n):
    """sequential float32 adds per lane of grid_ema_stats_kernel (512 blocks of 256 lanes) plus the shuffle, LDS and
    conversion steps; all terms are positive, so each rounding is a relative 2^-24 of the running sum at most"""
    per_block = -(-n // 512)
    return (-(-per_block // 256) + 10) * 2.0 ** -24


def packbits(grid, thr):
    return oracle.packbits(np.asarray(grid, np.float32), np.float32(thr))


# ---------------------------------------------------------------------------- the cases of the exact sampling test
def _ball(G):
    c = np.stack(np.meshgrid(*[np.arange(G, dtype=np.int64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    ctr = (c.astype(np.float32) + 0.5) / G - 0.5
    inside = (ctr ** 2).sum(-1) < 0.2 ** 2
    grid = np.zeros(G ** 3, np.float32)
    grid[morton(c[:, 0], c[:, 1], c[:, 2]).astype(np.int64)] = np.where(inside, 9.0, 0.3).astype(np.float32)
    return grid


def _grid_g2_none(G, thr):
    return np.array([thr, 0.0, -1.0, thr, np.nan, -0.0, thr, 0.25 * thr], np.float32)


def _grid_all(G, thr):
    return np.linspace(1.0, 2.0, G ** 3).astype(np.float32)


def _grid_cells(*cells):
    def make(G, thr):
        g = np.full(G ** 3, thr, np.float32)                     # equal to the threshold: not occupied
        g[1::3] = -1.0
        g[list(cells)] = np.float32(thr) + np.float32(1.0)
        return g
    return make


def _grid_random30(G, thr):
    r = np.random.default_rng(64)
    n = G ** 3
    kind = r.integers(0, 10, n)
    g = np.full(n, thr, np.float32)                              # kinds 3, 4: exactly the threshold
    occ = kind < 3
    g[occ] = np.float32(thr) + r.random(int(occ.sum()), dtype=np.float32) + np.float32(1e-3)
    g[kind == 5] = np.nextafter(np.float32(thr), np.float32(-np.inf))
    g[(kind == 6) | (kind == 7)] = -1.0
    g[kind == 8] = np.nan
    g[kind == 9] = 0.5 * thr
    g[r.integers(0, n, 50)] = np.inf                             # + inf > thr: occupied like any other
    g[r.integers(0, n, 50)] = -np.inf
    return g


def _grid_mod7(G, thr):
    n = G ** 3
    g = np.zeros(n, np.float32)
    g[5::7] = 2.0
    g[n - 1] = 2.0
    return g


# name: (G, m, s, thr, (seed of the first run, seed of the second run on the dirty workspace), grid builder).
# Measured on the reference (test_grid_update_host.py::test_reference_properties asserts > 0.5 for G >= 64), the share
# of the uniform samples that sit alone on their key, per seed:
#   G64-random30  0.866, 0.864      G128-ball  0.752, 0.752      G256-mod7  0.989, 0.987
SEED_MAX = (2 ** 47 - 1) + 1000003 * 3 + 7919 * 4                # the largest seed the model can form
CASES = {
    "G2-none": (2, 1, 0.5, 0.5, (11, 12), _grid_g2_none),
    "G2-all": (2, 5, 1.0, 0.01, (21, 2 ** 40 + 1), _grid_all),
    "G4-first-last": (4, 300, 2.0, 0.0, (31, 32), _grid_cells(0, 63)),
    "G16-block-edge": (16, 4097, 8.0, 1.5, (41, 42), _grid_cells(1023, 1024, 4095)),
    "G32-one-cell": (32, 4096, 0.5, 0.25, (51, 52), _grid_cells(12345)),
    "G64-random30": (64, 20000, 1.0, 3.0, (61, 62), _grid_random30),
    "G128-ball": (128, 128 ** 3 // 4, 0.5, 5.0, (SEED_MAX, 1234), lambda G, thr: _ball(G)),
    "G256-mod7": (256, 100000, 2.0, 1.0, (-1, 81), _grid_mod7),
}

_CACHE = {}


def make_case(name):
    """-> dict(G, m, s, thr, seeds, grid, occ, refs=[sample_cells(...) per seed]); computed once, shared, read-only"""
    if name not in _CACHE:
        G, m, s, thr, seeds, build = CASES[name]
        grid = build(G, thr)
        assert grid.shape == (G ** 3,) and grid.dtype == np.float32
        occ = occupied(grid, thr)
        refs = [sample_cells(occ, G, m, seed, s) for seed in seeds]
        for a in (grid, occ) + tuple(x for r in refs for x in r):
            a.setflags(write=False)
        _CACHE[name] = dict(G=G, m=m, s=s, thr=thr, seeds=seeds, grid=grid, occ=occ, refs=refs)
    return _CACHE[name]
