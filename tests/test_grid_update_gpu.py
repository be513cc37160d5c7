"""The sampled occupancy-grid update on the GPU against tests/grid_update_reference.py: ngp_grid_sample_cells row for
row (every output is a pure function of (seed, sample, draw)), ngp_density_grid_scatter_max and the grid after
ngp_density_grid_ema_threshold bit for bit, the mean threshold within the rounding of its float32 sums, ngp_packbits
with the threshold on the device byte for byte, and the cascade loop of NGP._update_density_grid_sampled at 3 cascades.

Bars.  Points: 8 * 2^-24 * s absolute (grid_update_reference.point_tolerance: the roundings of the float32 expression,
far below the jitter's span s/G).  Mean of the positive cells: relative (ceil(ceil(n/512)/256) + 10) * 2^-24
(grid_update_reference.threshold_rel_bound: the float32 adds one lane makes plus the reduction steps, all terms
positive).  Everything else is exact.  Every buffer a kernel writes carries sentinels past its end."""
import numpy as np
import pytest
import torch

import grid_update_reference as R
import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_I, SENT_F = -0x12345678, -7777.25
GARBAGE = 0x55555555


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # a copy: the shared references are read-only


def N(t):
    return t.detach().cpu().numpy()


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def padded(values, pad, sentinel):
    """device copy of `values` (1-d float32 / int32 / uint8) followed by `pad` sentinel elements"""
    values = np.ascontiguousarray(values)
    out = np.full(values.shape[0] + pad, sentinel, values.dtype)
    out[:values.shape[0]] = values
    return T(out)


def sample_twice(ngp, G, m, s, thr, grid_dev, seeds, refs):
    """two runs of ngp_grid_sample_cells on one workspace that starts as garbage and is never cleared; both must give
    the reference's rows and leave every sentinel alone"""
    from ngp_amd._lib import call, call_host
    n_ws = call_host("grid_sample_workspace", G, m)
    assert n_ws > 0
    work = torch.full((n_ws + 64,), GARBAGE, dtype=torch.int32, device=DEV)
    work[n_ws:] = SENT_I
    singles = []
    for seed, ref in zip(seeds, refs):
        idx = torch.full((2 * m + 8,), SENT_I, dtype=torch.int32, device=DEV)
        xyz = torch.full((2 * m + 8, 3), SENT_F, dtype=torch.float32, device=DEV)
        call("grid_sample_cells", grid_dev, G, float(thr), m, seed, float(s), work, idx, xyz)
        torch.cuda.synchronize()
        assert bool((work[n_ws:] == SENT_I).all()), "wrote past the workspace"
        assert bool((idx[2 * m:] == SENT_I).all()) and bool((xyz[2 * m:] == SENT_F).all()), "wrote past the outputs"
        singles.append(R.check_samples(N(idx[:2 * m]), N(xyz[:2 * m]), ref, G, s))
    return singles


# ---------------------------------------------------------------------------- ngp_grid_sample_cells, exact
@pytest.mark.parametrize("name", list(R.CASES))
def test_grid_sample_cells_rows_match_the_reference(ngp, name):
    """Per run: the multiset of indices is the reference's (the count, the scan, the compaction and each draw: an
    occupied sample is occ[rand_below(..)] of the ascending list), idx >> max(0, bits - 21) is non-decreasing, inside
    a key each axis' sorted values are the reference's, and rows alone on their key match in all three coordinates."""
    c = R.make_case(name)
    singles = sample_twice(ngp, c["G"], c["m"], c["s"], c["thr"], T(c["grid"]), c["seeds"], c["refs"])
    if c["G"] >= 64:
        assert min(singles) > c["m"] // 2          # the pairing check covers most of the uniform half


@pytest.mark.parametrize("G", [8, 512, 1024])
def test_grid_sample_cells_accepts_the_other_powers_of_two(ngp, G):
    """the sizes no case above uses, up to the largest the entry accepts (keys of 30 bits, 2^20 compaction blocks,
    1024 counts per scan thread): only the LAST cell occupied, so the reference needs no pass over the grid"""
    g3, m, s = G ** 3, 3, 1.0
    grid = torch.zeros(g3, dtype=torch.float32, device=DEV)
    grid[g3 - 1] = 2.0
    grid[g3 - 2] = 1.0                             # equal to the threshold
    occ = np.array([g3 - 1], np.int64)
    seeds = (G, -G)
    refs = [R.sample_cells(occ, G, m, seed, s) for seed in seeds]
    sample_twice(ngp, G, m, s, 1.0, grid, seeds, refs)
    grid[g3 - 1] = 1.0                             # nothing occupied: the uniform half twice
    refs = [R.sample_cells(occ[:0], G, m, seed, s) for seed in seeds]
    sample_twice(ngp, G, m, s, 1.0, grid, seeds, refs)


# ---------------------------------------------------------------------------- ngp_density_grid_scatter_max
SPECIAL_SIGMAS = np.array([0.0, -0.0, -2.5, np.nan, 1e-40, np.inf, -np.inf, 3.5], np.float32)


def _scatter_inputs(n):
    r = np.random.default_rng(1000 + n)
    cells = 4096
    tmp0 = (r.random(cells, dtype=np.float32) * 2 + np.float32(0.01)).astype(np.float32)      # non-zero everywhere
    tmp0[::5] = 0.25
    idx = r.integers(0, cells, n).astype(np.int32)
    hot = min(n // 2, 500)
    idx[r.permutation(n)[:hot]] = 777                                    # up to 500 duplicates on one cell
    sig = (r.random(n, dtype=np.float32) * 3).astype(np.float32)        # some below, some above tmp0
    k = np.arange(n)
    sel = k % 3 == 1
    sig[sel] = SPECIAL_SIGMAS[(k[sel] // 3) % len(SPECIAL_SIGMAS)]
    if n >= 255:
        idx[1] = idx[4] = 0                                              # 0.0 and -0.0 on the first cell
        idx[-1] = cells - 1
    return tmp0, idx, sig


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_scatter_max_bit_equal(ngp, n):
    from ngp_amd._lib import call
    runs = [_scatter_inputs(n)]
    if n == 1:                                                           # one sample: every special value in turn
        tmp0 = runs[0][0]
        runs = [(tmp0, np.array([c], np.int32), np.array([v], np.float32))
                for v in list(SPECIAL_SIGMAS) + [0.001, 9.0] for c in (0, 4095)]
    for tmp0, idx, sig in runs:
        if n > 1:
            assert (idx == 777).sum() >= min(n // 2, 500) - 3 and np.isin(sig, SPECIAL_SIGMAS).sum() >= 8
        want = R.scatter_max(tmp0, idx, sig)
        tmp = padded(tmp0, 8, SENT_F)
        call("density_grid_scatter_max", tmp, T(idx), T(sig), n)
        torch.cuda.synchronize()
        got = N(tmp)
        assert np.array_equal(bits_of(got[:4096]), bits_of(want)), np.flatnonzero(bits_of(got[:4096]) != bits_of(want))[:8]
        assert (got[4096:] == SENT_F).all()


# ---------------------------------------------------------------------------- ngp_density_grid_ema_threshold
def _ema_inputs(kind, n, decay):
    r = np.random.default_rng(7 * n + len(kind))
    f = np.float32
    if kind == "no-positive":                     # +0, negative and NaN cells over an empty tmp: nothing to count
        g = np.array([-1.0, 0.0, np.nan, -0.5], f)[r.integers(0, 4, n)]
        return g, np.zeros(n, f)
    if kind == "all-negative":                    # invisible cells stay as they are, whatever tmp holds
        return (-(r.random(n, dtype=f) + f(1e-3))).astype(f), (r.random(n, dtype=f) * 5).astype(f)
    k = r.integers(0, 8, n)
    k[:min(n, 8)] = [7, 3, 4, 5, 1, 0, 6, 2][:n]  # the smallest grids hold the kinds in this order
    g = (r.random(n, dtype=f) + f(0.5)).astype(f)
    tmp = np.zeros(n, f)                          # k == 7: a positive cell that only decays
    g[k == 0] = 0.0                               # + 0 over tmp 0: never counted
    g[(k == 1) | (k == 2)] = np.nan               # NaN becomes tmp: a positive one (1), zero (2)
    tmp[k == 1] = (r.random(int((k == 1).sum()), dtype=f) + f(0.1)).astype(f)
    tmp[k == 3] = g[k == 3] * f(2)                # tmp wins
    tmp[k == 4] = 0.1                             # g * decay wins
    tmp[k == 5] = g[k == 5] * f(decay)            # both equal
    g[k == 6] *= f(-1)                            # negative: kept, tmp ignored
    tmp[k == 6] = 4.0
    return g, tmp


@pytest.mark.parametrize("decay", [0.95, 1.0])
@pytest.mark.parametrize("n", [1, 7, 511, 512, 513, 1000, 128 ** 3 + 5])
def test_ema_threshold_grid_bit_equal_and_mean_within_rounding(ngp, n, decay):
    from ngp_amd._lib import call
    for kind in ("no-positive", "all-negative", "mix"):
        g0, tmp = _ema_inputs(kind, n, decay)
        want = R.ema(g0, tmp, decay)
        mean = R.mean_positive(want)
        if kind == "all-negative":
            assert np.array_equal(bits_of(want), bits_of(g0))
        if kind != "mix":
            assert mean == 0.0
        elif n >= 511:
            assert mean > 0 and np.isnan(g0).any() and (g0 == 0).any() and (g0 < 0).any()
        # density_threshold on both sides of the mean (no positive cell: of 0)
        for dthr in ((np.float32(0.5 * mean), np.float32(2 * mean)) if mean > 0 else (np.float32(-1.0), np.float32(1.0))):
            grid, tmp_d = padded(g0, 8, SENT_F), padded(tmp, 8, SENT_F)
            partials = padded(np.full(1024, np.nan, np.float32), 8, SENT_F)
            out = padded(np.full(2, np.nan, np.float32), 8, SENT_F)
            call("density_grid_ema_threshold", grid, tmp_d, n, float(decay), float(dthr), partials, out)
            torch.cuda.synchronize()
            got, o = N(grid), N(out)
            assert np.array_equal(bits_of(got[:n]), bits_of(want)), (kind, np.flatnonzero(bits_of(got[:n]) != bits_of(want))[:8])
            assert (got[n:] == SENT_F).all() and (o[2:] == SENT_F).all() and (N(partials)[1024:] == SENT_F).all()
            assert np.array_equal(bits_of(N(tmp_d)[:n]), bits_of(tmp))
            rel = abs(float(o[1]) - mean) / mean if mean > 0 else abs(float(o[1]))
            print(f"n {n} decay {decay} {kind}: mean {float(o[1])!r} reference {mean!r} relative error {rel:.3e} "
                  f"bound {R.threshold_rel_bound(n):.3e}")
            assert rel <= R.threshold_rel_bound(n), (kind, float(o[1]), mean)
            assert o[0] == min(o[1], dthr), (o, dthr)
            if mean > 0:
                assert (o[0] == dthr) == (dthr < o[1])


def test_ema_threshold_of_an_empty_grid_is_zero(ngp):
    from ngp_amd._lib import call
    partials = padded(np.full(1024, np.nan, np.float32), 8, SENT_F)
    for dthr in (5.0, -1.0):
        out = padded(np.full(2, np.nan, np.float32), 8, SENT_F)
        call("density_grid_ema_threshold", None, None, 0, 0.95, dthr, partials, out)
        torch.cuda.synchronize()
        o = N(out)
        assert o[1] == 0.0 and o[0] == min(0.0, dthr) and (o[2:] == SENT_F).all()
    assert (N(partials)[1024:] == SENT_F).all()


# ---------------------------------------------------------------------------- ngp_packbits, threshold on the device
@pytest.mark.parametrize("n_bytes", [1, 255, 257])
def test_packbits_device_threshold_byte_identical(ngp, n_bytes):
    from ngp_amd._lib import call
    r = np.random.default_rng(n_bytes)
    thr = np.float32(0.37)
    pool = np.array([thr, np.nan, -1.0, -0.0, 0.0, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0)), 2.0,
                     np.inf, -np.inf], np.float32)
    g = pool[r.integers(0, len(pool), 8 * n_bytes)]
    g[:8] = pool[:8]
    want = oracle.packbits(g, thr)
    assert want[0] == (1 << 5) | (1 << 7)
    grid = T(g)
    assert grid.data_ptr() % 16 == 0
    thr_dev = T(np.array([thr], np.float32))
    res = []
    for host_thr, dev in ((float(thr), None), (1e30, thr_dev), (-1e30, thr_dev)):      # the device value overrides the host's
        bits = padded(np.full(n_bytes, 0xAA, np.uint8), 8, 0x5C)
        call("packbits", grid, n_bytes, host_thr, dev, bits)
        torch.cuda.synchronize()
        b = N(bits)
        assert (b[n_bytes:] == 0x5C).all()
        res.append(b[:n_bytes])
    assert np.array_equal(res[0], want) and np.array_equal(res[1], want) and np.array_equal(res[2], want)


# ---------------------------------------------------------------------------- the cascade loop of the model
def _grid_model(ngp, scale, seed=3):
    torch.manual_seed(5)
    model = ngp.networks.NGP(scale=scale).to(DEV)
    with torch.no_grad():
        model.xyz_encoder.params.uniform_(-0.3, 0.3)
        model.rgb_encoder.params.uniform_(-0.3, 0.3)
        model.xyz_net[2].bias.fill_(1.5)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    c = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", c.reshape(-1, 3).contiguous())
    model.grid_rng = torch.Generator(device=DEV).manual_seed(seed)
    return model


def test_sampled_update_cascade_loop_matches_torch_formulas(ngp):
    """NGP._update_density_grid_sampled at scale 2.0 (3 cascades), two successive updates: per cascade the samples of
    s = min(2^(c-1), scale) and seed0 + 1000003*upd + 7919*c drawn from density_grid[c], density() on them, amax
    scatter and EMA in torch, on grids that differ per cascade (cascade 0 with cells far above the threshold, cascade
    1 with invisible cells, cascade 2 empty, hence sampled with no occupied cell) — the whole (3, G^3) grid bit for
    bit, and the bitfield against oracle.packbits at min(float64 mean over all cascades, thr0)."""
    from ngp_amd._lib import call, call_host
    model = _grid_model(ngp, 2.0)
    assert model.cascades == 3
    thr0 = 0.01 * 1024 / 3 ** 0.5
    model.update_density_grid(thr0, warmup=True)
    with torch.no_grad():
        model.density_grid[0, 5::11] = 50.0
        model.density_grid[1, 3::101] = 20.0
        model.density_grid[1, ::37] = -1.0
        model.density_grid[2].zero_()
    G, M = model.grid_size, model.grid_size ** 3 // 4
    seed0 = int(model.grid_rng.initial_seed()) & 0x7FFFFFFFFFFF
    work = torch.empty(call_host("grid_sample_workspace", G, M), dtype=torch.int32, device=DEV)
    idx = torch.empty(2 * M, dtype=torch.int32, device=DEV)
    xyz = torch.empty(2 * M, 3, dtype=torch.float32, device=DEV)
    for upd in range(2):
        before = model.density_grid.clone()
        n_occ = [int((before[c] > thr0).sum()) for c in range(3)]
        assert n_occ[0] != n_occ[1] > 0 and (upd > 0 or n_occ[2] == 0), n_occ   # a stale count from another cascade would show
        want = torch.empty_like(before)
        for c in range(3):
            s = min(2 ** (c - 1), model.scale)
            call("grid_sample_cells", before[c], G, float(thr0), M, seed0 + 1000003 * upd + 7919 * c, float(s), work, idx, xyz)
            assert float(xyz.abs().max()) <= s and float(xyz.abs().max()) > 0.9 * s
            with torch.no_grad():
                sig = model.density(xyz)
            tmp = torch.zeros_like(before[c]).scatter_reduce(0, idx.long(), sig, "amax", include_self=True)
            want[c] = torch.where(before[c] < 0, before[c], torch.maximum(before[c] * 0.95, tmp))
        model.update_density_grid(thr0, warmup=False)
        torch.cuda.synchronize()
        for c in range(3):
            assert torch.equal(model.density_grid[c], want[c]), (upd, c, int((model.density_grid[c] != want[c]).sum()))
        assert torch.equal(model.density_grid, want)
        w = N(want).reshape(-1)
        thr = min(float(w[w > 0].astype(np.float64).mean()), thr0)
        bits = oracle.packbits(w, np.float32(thr))
        mine = N(model.density_bitfield)
        assert mine.shape == bits.shape == (3 * G ** 3 // 8,)
        near = np.abs(w - thr) < 1e-5 * thr                              # cells within rounding of the threshold
        diff = np.unpackbits(mine ^ bits, bitorder="little").astype(bool)
        assert not (diff & ~near).any(), int((diff & ~near).sum())
        assert near.sum() < w.size // 100 and bits.any() and not bits.all()
        neg = w.reshape(3, -1)[1] < 0
        assert neg.sum() > 1000 and np.array_equal(N(model.density_grid[1])[neg], N(before[1])[neg])
        assert not (w.reshape(3, -1)[0] < 0).any() and not (w.reshape(3, -1)[2] < 0).any()
