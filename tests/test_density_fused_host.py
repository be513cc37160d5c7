"""Argument checks of ngp_density_field_fwd and its layout predicate: they return before any launch, so these run
without a GPU (all data pointers are NULL)."""
import ctypes as C


def _desc(ngp, levels, F, log2_T):
    d = ngp._lib.GridDesc()
    assert ngp._lib.call_host("grid_layout", levels, F, log2_T, 16, 1.3195079, d) > 0
    return d


def test_density_field_layout_predicate(ngp):
    ok = lambda d: ngp._lib.call_host("density_field_layout_ok", d)
    assert ok(_desc(ngp, 16, 8, 19)) == 1       # the density table of NGP
    assert ok(_desc(ngp, 16, 8, 14)) == 1       # more hashed levels
    assert ok(_desc(ngp, 8, 8, 19)) == 0        # not 16 levels
    assert ok(_desc(ngp, 16, 4, 19)) == 0       # not F = 8
    assert ok(_desc(ngp, 16, 8, 26)) == 0       # a table of 4 GiB and more: the tile kernels' 32-bit offsets
    assert ok(None) == 0


def test_density_field_fwd_rejects_bad_arguments(ngp):
    lib = ngp._lib.load()
    good, small = _desc(ngp, 16, 8, 19), _desc(ngp, 8, 8, 19)
    f = lib.ngp_density_field_fwd

    def run(desc, n):
        return f(C.addressof(desc) if desc is not None else None, None, None, n, None, None, None, None, None, None, None,
                 None, None, None)
    assert run(good, 0) == 0                    # empty batch: nothing to do
    assert run(good, -1) == -22
    assert run(good, 5) == -22                  # NULL pointers
    assert run(small, 5) == -22                 # not 16 levels
    assert run(small, 0) == -22
    assert run(None, 5) == -22
