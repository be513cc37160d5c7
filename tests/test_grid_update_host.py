"""CPU-only checks of tests/grid_update_reference.py (known answers of its hash, properties of its samples on every
case of tests/test_grid_update_gpu.py, its comparison routine against reordered and damaged copies of the reference)
and of the argument checks of the sampled grid update's entry points, none of which may reach a launch."""
import numpy as np
import pytest

import grid_update_reference as R

EINVAL = -22


def test_splitmix64_known_answers():
    """hash64(0, 0, d) is output d + 1 of SplitMix64 seeded with 0: state 0 + GOLDEN * (d + 1), then the finaliser.  The
    first two published outputs; the wrap of seed = -1 taken as uint64, worked out with Python integers."""
    assert int(R.hash64(0, 0, 0)) == 0xE220A8397B1DCDAF
    assert int(R.hash64(0, 0, 1)) == 0x6E789E6AA1B965F4
    assert int(R.hash_u32(0, 0, 0)) == 0xE220A839

    def plain(seed, i, draw):
        M = 2 ** 64 - 1
        z = (seed + R.GOLDEN * (i * 8 + draw + 1)) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    # seed -1 is 2^64 - 1: adding GOLDEN * 1 wraps to GOLDEN - 1
    assert int(R.hash64(-1, 0, 0)) == plain(2 ** 64 - 1, 0, 0) == plain(-1, 0, 0)
    assert int(R.hash64(-1, 0, 0)) != int(R.hash64(0, 0, 0))
    ids = np.array([0, 1, 7, 2 ** 20, 2 ** 31 - 1], np.int64)
    for seed in (-1, 0, R.SEED_MAX, 2 ** 63 + 5):
        for draw in range(7):
            assert [int(v) for v in R.hash64(seed, ids, draw)] == [plain(seed, int(i), draw) for i in ids]
    # rand_below: (h32 * n) >> 32 < n, and 0 for n = 1
    assert (R.rand_below(5, ids, 3, 1) == 0).all() and (R.rand_below(5, np.arange(1000), 3, 7) < 7).all()


def test_morton_matches_oracle_and_inverts():
    import oracle
    c = np.random.default_rng(0).integers(0, 1024, (2000, 3)).astype(np.int32)
    k = R.morton(c[:, 0], c[:, 1], c[:, 2]).astype(np.int64)
    assert np.array_equal(k, oracle.morton3D(c).astype(np.int64))
    assert np.array_equal(R.morton_invert(k), c)
    assert int(R.morton(np.array([99]), np.array([99]), np.array([99]))[0]) == 2064447     # the G = 100 example
    assert [R.key_bits(G) for G in (2, 4, 128, 256, 1024)] == [3, 6, 21, 24, 30]
    assert [R.sort_shift(G) for G in (2, 128, 256, 1024)] == [0, 0, 3, 9]


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_properties(name):
    c = R.make_case(name)
    G, m, s = c["G"], c["m"], c["s"]
    with np.errstate(invalid="ignore"):
        want_occ = [j for j in range(G ** 3) if c["grid"][j] > np.float32(c["thr"])] if G <= 16 else None
    if want_occ is not None:
        assert list(c["occ"]) == want_occ
    assert (np.diff(c["occ"]) > 0).all()
    for seed, (keys, sids, xyz) in zip(c["seeds"], c["refs"]):
        assert keys.shape == (2 * m,) and keys.min() >= 0 and keys.max() < G ** 3
        centre = (R.morton_invert(keys) / (G - 1) * 2 - 1) * (s - s / G)
        assert np.abs(xyz - centre).max() <= s / G
        assert np.abs(xyz - centre).mean() > 0.4 * s / G or m < 50          # jittered: E|U(-1,1)| = 0.5
        if len(c["occ"]):
            assert np.array_equal(sids, np.arange(2 * m))
            assert np.isin(keys[m:], c["occ"]).all()
            if m >= 300:                                                     # every occupied cell of a short list is drawn
                assert len(c["occ"]) > 300 or set(keys[m:]) == set(c["occ"])
        else:
            assert np.array_equal(keys[m:], keys[:m]) and np.array_equal(xyz[m:], xyz[:m])
            assert np.array_equal(sids[m:], np.arange(m))
        share = R.singleton_share(keys, m)
        print(f"{name} seed {seed}: singleton share of the uniform samples {share:.3f}, n_occ {len(c['occ'])}")
        if G >= 64:
            assert share > 0.5, share
    # the two seeds draw different samples
    assert not np.array_equal(c["refs"][0][0], c["refs"][1][0]) or G == 2


def test_case_list_reaches_what_it_claims():
    c = {n: R.make_case(n) for n in ("G2-none", "G2-all", "G4-first-last", "G16-block-edge", "G32-one-cell", "G64-random30",
                                     "G256-mod7")}
    assert len(c["G2-none"]["occ"]) == 0 and len(c["G2-all"]["occ"]) == 8
    assert list(c["G4-first-last"]["occ"]) == [0, 63] and list(c["G16-block-edge"]["occ"]) == [1023, 1024, 4095]
    assert list(c["G32-one-cell"]["occ"]) == [12345]
    k = c["G32-one-cell"]["refs"][0][0]
    assert (k == 12345).sum() >= 4096                                        # > 4096 rows in one bucket and one sub-bin
    g = c["G64-random30"]
    frac = len(g["occ"]) / 64 ** 3
    assert 0.28 < frac < 0.32
    rest = np.delete(g["grid"], g["occ"])
    assert (rest == np.float32(g["thr"])).sum() > 1000 and np.isnan(rest).sum() > 1000 and (rest < 0).sum() > 1000
    assert np.isinf(g["grid"]).sum() > 50 and np.isposinf(g["grid"][g["occ"]]).sum() > 10
    occ = c["G256-mod7"]["occ"]
    assert occ[-1] == 256 ** 3 - 1 and (occ[:-1] % 7 == 5).all() and len(occ) == 2396746
    assert c["G256-mod7"]["seeds"][0] == -1 and R.make_case("G128-ball")["seeds"][0] == 2 ** 47 - 1 + 3000009 + 31676
    assert sorted({v[2] for v in R.CASES.values()}) == [0.5, 1.0, 2.0, 8.0]


def test_check_samples_accepts_legal_orders_and_catches_damage():
    """check_samples on the reference itself: any order inside a sort key passes; the samples of another seed, one
    coordinate moved by a tenth of the jitter's half-width and two rows out of order do not."""
    for name in ("G16-block-edge", "G64-random30", "G256-mod7"):
        c = R.make_case(name)
        G, s, m = c["G"], c["s"], c["m"]
        ref = c["refs"][0]
        keys, _, xyz = ref
        r = np.random.default_rng(1)
        order = np.lexsort((r.random(2 * m), keys >> R.sort_shift(G)))       # random inside equal sort keys
        idx, pts = keys[order].astype(np.int32), xyz[order].astype(np.float32)
        n_single = R.check_samples(idx, pts, ref, G, s)
        assert n_single > 0
        if G == 256:
            assert (np.diff(idx.astype(np.int64)) < 0).any()                 # low 3 bits really are unsorted here
        # the reference of the other seed is another multiset
        with pytest.raises(AssertionError, match="multiset"):
            R.check_samples(idx, pts, c["refs"][1], G, s)
        # a point moved by a tenth of the jitter range
        bad = pts.copy()
        bad[m // 2, 1] += np.float32(0.1 * s / G)
        with pytest.raises(AssertionError, match="differ"):
            R.check_samples(idx, bad, ref, G, s)
        # two rows out of order
        a, b = 0, 2 * m - 1
        sw = np.arange(2 * m)
        sw[[a, b]] = [b, a]
        with pytest.raises(AssertionError, match="not ordered"):
            R.check_samples(idx[sw], pts[sw], ref, G, s)
        # the jitter of the neighbouring sample id: same cells, other points
        wrong = R.sample_cells(c["occ"], G, m, c["seeds"][0] + 1, s)
        assert not np.array_equal(wrong[0], keys)
    # the tolerance is far below the jitter's span s/G (>= s/256 = 65536 * 2^-24 * s): it separates any wrong draw
    for v in R.CASES.values():
        G, s = v[0], v[2]
        assert R.point_tolerance(s) * 8192 <= s / G


def test_scatter_ema_threshold_reference_edges():
    f = np.float32
    tmp = R.scatter_max(f([0.5, 0.5, 0, 0, 0, -0.0]), [0, 1, 2, 2, 3, 4, 5, 5], f([0.25, 0.75, 1e-40, np.nan, -3, 0.0, -0.0, np.inf]))
    assert tmp[0] == f(0.5) and tmp[1] == f(0.75) and tmp[2] == f(1e-40) and tmp[3] == 0 and tmp[4] == 0 and np.isposinf(tmp[5])
    g = R.ema(f([-1, np.nan, 0, 2, 2, 2]), f([9, 0.5, 0, 1, 3, 2]), 1.0)
    assert np.array_equal(g, f([-1, 0.5, 0, 2, 3, 2]))
    assert R.ema(f([2]), f([0]), 0.95)[0] == f(2) * f(0.95)
    assert R.mean_positive(f([-1, 0, np.nan, 1, 3])) == 2.0 and R.mean_positive(f([-1, 0, np.nan])) == 0.0
    assert R.threshold_rel_bound(1) == 11 * 2.0 ** -24 and R.threshold_rel_bound(128 ** 3 + 5) == (17 + 10) * 2.0 ** -24
    assert np.array_equal(R.packbits(f([1, 0.5, np.nan, -1, 0.6, 0.5, 2, 0]), 0.5), np.array([1 + 16 + 64], np.uint8))


# ---------------------------------------------------------------------------- argument checks, no launch
BAD_G = (3, 96, 100, 127, 129)
GOOD_G = tuple(2 ** k for k in range(1, 11))


def test_grid_size_must_be_a_power_of_two(ngp):
    """Morton keys of a G^3 grid span 3*ceil(log2 G) bits (G = 100: cell (99,99,99) has key 2064447 >= 2^20 >= G^3,
    bucket 504 of 256; G = 3: key 56 >= 27).  Both sampling entries refuse such a G before any launch: the pointers
    here are small dummy addresses, a launch on them would fault.  Accepted sizes are checked through the host-only
    workspace query here and by real calls in tests/test_grid_update_gpu.py."""
    lib = ngp._lib.load()
    dummy = 0x1000
    for G in BAD_G + (0, 1, -4, 1025, 2048):
        assert lib.ngp_grid_sample_workspace(G, 1) == EINVAL, G
        assert lib.ngp_grid_sample_cells(dummy, G, 0.5, 1, 7, 0.5, dummy, dummy, dummy, None) == EINVAL, G
    for G in GOOD_G:
        g3 = G ** 3
        nb = -(-g3 // 1024)
        assert lib.ngp_grid_sample_workspace(G, 5) == 2 * nb + 4 + g3 + 8 * 5 + 3 * 256, G
    assert lib.ngp_grid_sample_workspace(128, 0) == EINVAL
    assert lib.ngp_grid_sample_cells(dummy, 128, 0.5, 0, 7, 0.5, dummy, dummy, dummy, None) == EINVAL
    assert lib.ngp_grid_sample_cells(None, 128, 0.5, 1, 7, 0.5, dummy, dummy, dummy, None) == EINVAL


def test_marcher_entries_refuse_a_grid_size_that_is_no_power_of_two(ngp):
    """ngp_raymarching_train / _test index the bitfield by the Morton code of the cell, as the sampling does"""
    lib = ngp._lib.load()
    d = 0x1000
    for G in BAD_G + (0, -1, 2048):
        assert lib.ngp_raymarching_train(d, d, d, d, 1, 0.5, 0.0, d, G, 1024, 1, d, d, d, d, d, d, d, d, 1024, 0, None) == EINVAL, G
        assert lib.ngp_raymarching_test(d, d, d, d, d, 1, 0.5, 0.0, G, 1024, 1, 1, d, d, d, d, d, None) == EINVAL, G
    # accepted sizes get past the size check: an empty batch is NGP_OK without a launch (test entry only)
    for G in (1,) + GOOD_G:
        assert lib.ngp_raymarching_test(None, None, None, None, None, 1, 0.5, 0.0, G, 1024, 1, 0, None, None, None, None, None,
                                        None) == 0, G


def test_packbits_refuses_a_misaligned_grid(ngp):
    """packbits_kernel reads the grid as float4: a grid pointer that is not 16-byte aligned is NGP_EINVAL"""
    lib = ngp._lib.load()
    for off in (4, 8, 12, 1):
        assert lib.ngp_packbits(0x1000 + off, 1, 0.5, None, 0x2000, None) == EINVAL
    assert lib.ngp_packbits(0x1000 + 4, 0, 0.5, None, 0x2000, None) == 0         # empty: no pointer is looked at
    assert lib.ngp_packbits(None, 1, 0.5, None, 0x2000, None) == EINVAL
