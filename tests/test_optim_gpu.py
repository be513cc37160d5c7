"""The optimizer step (csrc/optim_kernels.hip) against the float64 restatement of tests/optim_reference.py, from a snapshot:
(p, g, m, v) as they are just before the step, one step, every output element under optim_reference.bars().  From a snapshot
one Adam step is perfectly conditioned (tests/tail_harness.py explains why a trajectory is not), so the bars are a few ulp.

  - ngp_adam_step_width through the C ABI, one step from arbitrary state: p', m' and v', the gradient buffer (cleared /
    untouched), at the sizes where its three loops hand over, at every argument combination the trainer uses;
  - the clip chain: ngp_clip_coef(_if), ngp_clip_decide(_rest) on misaligned and short operands, ngp_row_norm_sum;
  - NGPTrainer.optimizer_step as a whole on every route to the coefficient, on a sample of the 250 M entries that holds
    every border of the two-piece sweep, and NGPTrainer._pose_step.

The input builders are plain numpy: tests/test_optim_host.py imports them and holds the float32 restatements to half of
every bar, and a list of wrong Adams to missing them, on exactly these inputs."""
import functools

import numpy as np
import pytest
import torch

import optim_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8

# adam_kernel: 256 lanes, U = 2 quads per lane and trip, stride = blocks * 256 quads, blocks = min(ceil(n4 / 256), width or 512)
SMALL = (1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025)
MID = tuple(4 * 1317 + r for r in range(4))   # width 1: n4 = 2 * 512 + 256 + 37 (unrolled loop, single-quad loop, scalar tail)
BIG = 4 * (3 * 131072 + 37) + 3               # the default launch at its 512-workgroup cap, in the unrolled loop
SIZES = SMALL + MID + (BIG,)
WIDTHS = (1, 3, 0)
SWEEP_N = MID[3]
GRAD_SCALES = (None, 1.0, 0.37, 0.0)
DECAYS = (0.0, 0.01)
STEPS = (1, 2, 10, 1000, 100000, 2 ** 31 + 5)
LRS = (1e-2, 1e-6)


def args_of(grad_scale=None, weight_decay=0.0, step=1, lr=1e-2, zero_grad=1):
    return dict(grad_scale=grad_scale, weight_decay=weight_decay, step=step, lr=lr, zero_grad=zero_grad)


# what every size is run with: the trainer's call (a device coefficient, the gradient cleared) and the sharded / pose one
SIZE_ARGS = (args_of(0.37, 0.0, 10, 1e-2, 1), args_of(None, 0.01, 1, 1e-6, 0))


@functools.lru_cache(maxsize=None)
def adam_inputs(n, seed=0):
    """-> {p, g, m, v: float32 (n), still: g = m = v = 0, border: a quad-aligned cut with live quads on both sides}.
    m signed, 1e-12..1e3, a fifth exact zeros; v >= 0, 1e-24..1e6, a fifth exact zeros; p signed, 1e-4..10; g of m's range,
    30 % zeros (+0 and -0): single lanes, whole quads, quads with one live lane, runs where g = 0 and the state is not (p must
    move, the state decay), runs where g = m = v = 0 (nothing may change).  The first and last two quads, the ragged tail and
    the quads around `border` are live: g, m, v all nonzero."""
    r = np.random.default_rng(1000 + 7 * n + seed)

    def mag(lo, hi):
        return 10.0 ** r.uniform(lo, hi, n)

    def sign():
        return r.choice([-1.0, 1.0], n)

    p, g, m, v = sign() * mag(-4, 1), sign() * mag(-12, 3), sign() * mag(-12, 3), mag(-24, 6)
    n4 = n // 4
    kind = r.choice(5, n4, p=[0.76, 0.06, 0.06, 0.06, 0.06])
    if n4 >= 64:
        kind[n4 // 4:n4 // 4 + 8] = 3
        kind[3 * n4 // 4:3 * n4 // 4 + 8] = 4
    live = [q for q in (0, 1, n4 // 2 - 1, n4 // 2, n4 - 2, n4 - 1) if 0 <= q < n4]
    kind[live] = 5
    ek = np.full(n, 5)
    ek[:4 * n4] = np.repeat(kind, 4)
    lane = np.arange(n) % 4
    one = np.repeat(r.integers(0, 4, n4 + 1), 4)[:n]
    zm, zv, zg = r.random(n) < 0.2, r.random(n) < 0.2, r.random(n) < 0.1
    m[zm & (ek < 3)] = 0.0
    v[zv & (ek < 3)] = 0.0
    gz = (zg & (ek == 0)) | (ek == 1) | ((ek == 2) & (lane != one)) | (ek == 3) | (ek == 4)
    g[gz] = np.where(r.random(n) < 0.5, 0.0, -0.0)[gz]
    m[ek == 4] = 0.0
    v[ek == 4] = 0.0
    out = {k: a.astype(np.float32) for k, a in zip("pgmv", (p, g, m, v))}
    out["still"] = (out["g"] == 0) & (out["m"] == 0) & (out["v"] == 0)
    out["border"] = 4 * (n4 // 2)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def nonfinite_inputs():
    """SWEEP_N elements with a NaN and an infinite gradient in chosen quads (unrolled loop, single-quad loop, scalar tail)
    and gradients of 1e18 (float32 g^2 still finite) beside them"""
    x = {k: np.array(a) for k, a in adam_inputs(SWEEP_N, seed=5).items()}
    g = x["g"]
    g[4 * 10 + 1] = np.nan
    g[4 * 700:4 * 700 + 4] = np.inf
    g[4 * 1300 + 2] = -np.inf
    g[SWEEP_N - 1] = np.inf
    g[4 * 11:4 * 11 + 4] = [1e18, -1e18, 3e17, 0.0]
    g[4 * 1301] = -1e18
    x["still"] = (x["g"] == 0) & (x["m"] == 0) & (x["v"] == 0)
    return x


@functools.lru_cache(maxsize=None)
def subnormal_inputs():
    """SWEEP_N elements around float32's underflow, as a table entry is after one gradient of 1e-20: g of 1e-24..1e-17 (g^2 and
    its thousandth below 2^-126 or below 2^-149), m and v of 1e-45..1e-36, zeros among all three"""
    x = {k: np.array(a) for k, a in adam_inputs(SWEEP_N, seed=6).items()}
    r = np.random.default_rng(66)
    n = SWEEP_N
    x["g"] = np.where(x["g"] == 0, x["g"], np.sign(x["g"]) * 10.0 ** r.uniform(-24, -17, n)).astype(np.float32)
    x["m"] = np.where(x["m"] == 0, x["m"], np.sign(x["m"]) * 10.0 ** r.uniform(-45, -36, n)).astype(np.float32)
    x["v"] = np.where(x["v"] == 0, x["v"], 10.0 ** r.uniform(-45, -36, n)).astype(np.float32)
    x["still"] = (x["g"] == 0) & (x["m"] == 0) & (x["v"] == 0)
    return x


SUBNORMAL_ARGS = (args_of(0.37, 0.0, 3, 1e-2, 1), args_of(1.0, 0.0, 1000, 1e-2, 1), args_of(None, 0.0, 2 ** 31 + 5, 1e-6, 0))


def reference(x, a):
    """(adam_step64, bars) of the inputs x under the arguments a"""
    ref = R.adam_step64(x["p"], x["g"], x["m"], x["v"], a["lr"], BETA1, BETA2, EPS, a["weight_decay"], a["step"],
                        a["grad_scale"])
    return ref, R.bars(x["p"], x["m"], x["v"], ref, a["weight_decay"])


def sweep_args():
    for gs in GRAD_SCALES:
        for wd in DECAYS:
            for step in STEPS:
                for lr in LRS:
                    for zg in (1, 0):
                        yield args_of(gs, wd, step, lr, zg)


def all_cases():
    """every (name, inputs, arguments) the Adam tests of this module run: the host module measures the restatement on them"""
    for n in SIZES:
        for k, a in enumerate(SIZE_ARGS):
            yield f"n={n}/{k}", adam_inputs(n), a
    for a in sweep_args():
        yield "sweep/" + "/".join(str(v) for v in a.values()), adam_inputs(SWEEP_N), a
    yield "nonfinite", nonfinite_inputs(), args_of(0.37, 0.0, 10, 1e-2, 1)
    yield "slice", adam_inputs(SWEEP_N, seed=9), SIZE_ARGS[0]
    for k, a in enumerate(SUBNORMAL_ARGS):
        yield f"subnormal/{k}", subnormal_inputs(), a


# ---------------------------------------------------------------------------------------------------- the Adam kernel
def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.asarray(a).view(np.int32)


def launch(ngp, bufs, n, a, width):
    gs = None if a["grad_scale"] is None else torch.tensor([a["grad_scale"]], dtype=torch.float32, device=DEV)
    ngp._lib.call("adam_step_width", *bufs, n, a["lr"], BETA1, BETA2, EPS, a["weight_decay"], a["step"], gs,
                  a["zero_grad"], width)


def run_adam(ngp, x, a, width):
    bufs = [T(x[k]) for k in "pgmv"]
    launch(ngp, bufs, x["p"].size, a, width)
    torch.cuda.synchronize()
    return [N(b) for b in bufs]


def check(x, a, got, name):
    """p', m', v' under the bars, the gradient buffer cleared or untouched, and nothing moved where g = m = v = 0"""
    ref, bar = reference(x, a)
    p, g, m, v = got
    r = R.ratios((p, m, v), ref, bar)
    print(f"{name}: fractions of the bars p {r['p']:.3f} m {r['m']:.3f} v {r['v']:.3f}")
    assert R.within(r), (name, r)
    if a["zero_grad"]:
        assert (g == 0).all(), name
    else:
        assert np.array_equal(bits(g), bits(x["g"])), name
    if a["weight_decay"] == 0:
        s = x["still"]
        for k, b in zip("pmv", (p, m, v)):
            assert np.array_equal(bits(b)[s], bits(x[k])[s]), (name, k)
    return r


@pytest.mark.parametrize("n", SIZES)
def test_adam_sizes_against_float64(ngp, n):
    """every loop of adam_kernel and every hand-over between them, at launch widths 1, 3 and the default; the widths agree
    bit for bit"""
    x = adam_inputs(n)
    for k, a in enumerate(SIZE_ARGS):
        outs = [run_adam(ngp, x, a, w) for w in WIDTHS]
        check(x, a, outs[0], f"n={n}/{k}")
        for o in outs[1:]:
            assert all(np.array_equal(bits(u), bits(w)) for u, w in zip(o, outs[0])), (n, k)


@pytest.mark.parametrize("weight_decay", DECAYS)
@pytest.mark.parametrize("grad_scale", GRAD_SCALES)
def test_adam_arguments_against_float64(ngp, grad_scale, weight_decay):
    """step in {1, 2, 10, 1000, 100000, 2^31 + 5} x lr in {1e-2, 1e-6} x zero_grad in {1, 0}, from arbitrary state"""
    x = adam_inputs(SWEEP_N)
    for a in sweep_args():
        if a["grad_scale"] == grad_scale and a["weight_decay"] == weight_decay:
            check(x, a, run_adam(ngp, x, a, 0), "sweep/" + "/".join(str(v) for v in a.values()))


def test_adam_on_slices_leaves_the_neighbours_alone(ngp):
    """the kernel on [lo:hi] of larger buffers, cut at 16-byte bounds as the trainer cuts its two pieces: the elements on
    both sides keep their bits in all four buffers"""
    x, a = adam_inputs(SWEEP_N, seed=9), SIZE_ARGS[0]
    for lo, n, width in ((64, SWEEP_N, 0), (260, SWEEP_N - 3, 1), (4, 5, 0)):
        xs = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in x.items()}
        full = [torch.full((lo + n + 77,), s, dtype=torch.float32, device=DEV) for s in (11.0, 13.0, 17.0, 19.0)]
        for f, k in zip(full, "pgmv"):
            f[lo:lo + n] = T(xs[k])
        launch(ngp, [f[lo:lo + n] for f in full], n, a, width)
        torch.cuda.synchronize()
        check(xs, a, [N(f[lo:lo + n]) for f in full], f"slice[{lo}:{lo + n}]")
        for f, s in zip(full, (11.0, 13.0, 17.0, 19.0)):
            want = bits(np.float32(s))
            assert (bits(N(f[:lo])) == want).all() and (bits(N(f[lo + n:])) == want).all(), (lo, n, s)


def test_adam_nonfinite_gradients_stay_in_their_elements(ngp):
    """a NaN and an infinite gradient: those elements' p become non-finite as torch's do, every other element meets the bars"""
    x, a = nonfinite_inputs(), args_of(0.37, 0.0, 10, 1e-2, 1)
    got = run_adam(ngp, x, a, 0)
    bad = ~np.isfinite(x["g"])
    assert bad.sum() == 7 and not np.isfinite(got[0][bad]).any() and np.isfinite(got[0][~bad]).all()
    check(x, a, got, "nonfinite")


def test_adam_state_below_the_normal_range(ngp):
    """moments and squared gradients below 2^-126, where the trainer's tables spend their first steps: gradual underflow,
    nothing flushed to zero (the bars allow 4 spacings of 2^-149 there, a flush would be off by up to 2^-126)"""
    x = subnormal_inputs()
    assert (np.abs(x["v"][x["v"] != 0]) < 2.0 ** -126).mean() > 0.2
    for k, a in enumerate(SUBNORMAL_ARGS):
        got = run_adam(ngp, x, a, 0)
        check(x, a, got, f"subnormal/{k}")
        live = (x["v"] != 0) & (x["v"] > 2.0 ** -140)
        assert (got[3][live] != 0).all()


def test_adam_rejects_bad_arguments_and_writes_nothing(ngp):
    x = adam_inputs(1025)
    n = 1025
    a = SIZE_ARGS[1]

    def refused(bufs, n=n, step=1, width=0):
        keep = [b.clone() for b in bufs if b is not None]
        with pytest.raises(RuntimeError, match="ngp_adam_step_width failed"):
            ngp._lib.call("adam_step_width", *bufs, n, 1e-2, BETA1, BETA2, EPS, 0.0, step, None, 1, width)
        torch.cuda.synchronize()
        assert all(torch.equal(b.view(torch.int32), k.view(torch.int32)) for b, k in zip([b for b in bufs if b is not None], keep))

    bufs = [T(x[k]) for k in "pgmv"]
    refused(bufs, n=-1)
    refused(bufs, step=0)
    refused(bufs, step=-3)
    refused(bufs, width=-1)
    wide = [torch.cat([T(x[k]), torch.zeros(1, device=DEV)]) for k in "pgmv"]
    for k in range(4):
        refused([None if j == k else b for j, b in enumerate(bufs)])
        refused([w[1:] if j == k else w[:n] for j, w in enumerate(wide)])
    ngp._lib.call("adam_step_width", None, None, None, None, 0, 1e-2, BETA1, BETA2, EPS, 0.0, 1, None, 1, 0)   # n = 0: nothing to do
    ngp._lib.call("adam_step_width", *bufs, 0, 1e-2, BETA1, BETA2, EPS, 0.0, 1, None, 1, 0)
    torch.cuda.synchronize()
    assert all(np.array_equal(bits(N(b)), bits(x[k])) for b, k in zip(bufs, "pgmv"))
    launch(ngp, bufs, n, a, 0)                                   # and the same buffers are accepted as they are
    torch.cuda.synchronize()
    check(x, a, [N(b) for b in bufs], "after the refusals")


# ---------------------------------------------------------------------------------------------------- the clip chain
COEF_RTOL = 1e-5          # the bar of test_clip_decide_and_conditional_norm
SUM_RTOL = 1e-4           # its bar on a sum of squares
EXACT_MARGIN = 8 * R.E    # sqrtf, the product, the sum and the quotient of clip_coef_kernel round once each


def check_coef(got, sumsq, max_norm, extra, margin=EXACT_MARGIN):
    want, c = R.clip_coef64(sumsq, max_norm, extra)
    if np.isnan(want):
        assert np.isnan(got), (got, sumsq)
    elif c > 1.0 + margin:
        assert got == np.float32(extra), (got, sumsq, max_norm, extra)
    else:
        assert abs(got - want) <= COEF_RTOL * want, (got, want, sumsq, max_norm, extra)


@pytest.mark.parametrize("extra", [1.0, 0.5])
def test_clip_coef_edges(ngp, extra):
    call = ngp._lib.call
    for max_norm in (50.0, 1e-4):
        q = (max_norm / extra) ** 2
        for sumsq in (0.0, 1e-30, 0.25 * q, 0.99 * q, q, 1.01 * q, 4.0 * q, float("inf"), float("nan")):
            s = torch.tensor([sumsq], dtype=torch.float32, device=DEV)
            for flag in (None, 1, 5, 0):
                coef = torch.full((1,), -7.0, device=DEV)
                if flag is None:
                    call("clip_coef", s, max_norm, extra, coef)
                else:
                    call("clip_coef_if", s, max_norm, extra, coef, torch.tensor([flag], dtype=torch.int32, device=DEV))
                if flag == 0:
                    assert float(coef) == -7.0
                else:
                    check_coef(float(coef), float(s), max_norm, extra)
                assert np.array_equal(bits(N(s)), bits(np.float32([sumsq])))


def _misaligned(a):
    """the array on the device, one element past a 16-byte bound"""
    buf = torch.zeros(a.size + 5, dtype=torch.float32, device=DEV)
    buf[1:1 + a.size] = T(a)
    t = buf[1:1 + a.size]
    assert t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize("lens", [(1, 3, 4, 5), (5, 4, 3, 1), (4 * 33 + 1, 4 * 300 + 2, 4 * 7 + 3, 4 * 1025), (1000, 48, 777, 128)])
@pytest.mark.parametrize("aligned", [True, False])
def test_clip_decide_operand_shapes(ngp, lens, aligned):
    """ngp_clip_decide and ngp_clip_decide_rest with weight and rest pointers off the 16-byte grid (the kernel's scalar path),
    lengths around one quad, no rest at all, and a running sum that is not zero when the launch begins"""
    call = ngp._lib.call
    g = np.random.default_rng(sum(lens) + aligned)
    put = T if aligned else _misaligned
    w = [g.normal(size=k).astype(np.float32) for k in lens]
    wt = [put(a) for a in w]
    f = [np.linalg.norm(a.astype(np.float64)) for a in w]
    fa, fb = f[0] * f[1], f[2] * f[3]
    wargs = [z for t in wt for z in (t, t.numel())]
    for n_rest in (0, 1, 3, 4, 5, 4 * 2500 + 1):
        rest = (g.normal(size=max(n_rest, 1)) * 0.01).astype(np.float32)
        rest_t = put(rest)
        rest_sq = float((rest[:n_rest].astype(np.float64) ** 2).sum())
        for sa, sb, pre, max_norm, scale in ((3.0 / fa, 4.0 / fb, 144.0, 50.0, 1.0),           # bound 13 (+ rest)
                                              (30.0 / fa, 40.0 / fb, 0.0, 50.0, 1.0),         # bound 50: not below 50
                                              (30.0 / fa, 40.0 / fb, 2.5, 50.0, 0.5),         # halved: 25
                                              (float("nan"), 1.0 / fb, 0.0, 50.0, 1.0),
                                              (1.0 / fa, float("inf"), 1.0, 50.0, 1.0),
                                              (1e-3 / fa, 1e-3 / fb, 1e-8, 1e-4, 1.0)):
            sums = np.array([sa, sb], np.float32)
            for entry in ("clip_decide", "clip_decide_rest"):
                with_rest = entry == "clip_decide_rest"
                total = pre + (rest_sq if with_rest else 0.0)
                bound, safe = R.clip_bound64(sums, *w, total, max_norm, scale)
                assert not abs(bound * 1.001 + 1e-6 - max_norm) < 1e-4 * max_norm    # the case is not at the threshold
                acc = T(np.array([pre], np.float32))
                coef = torch.full((1,), -7.0, device=DEV)
                flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
                if with_rest:
                    call(entry, T(sums), *wargs, rest_t, n_rest, acc, max_norm, scale, coef, flag)
                else:
                    call(entry, T(sums), *wargs, acc, max_norm, scale, coef, flag)
                torch.cuda.synchronize()
                what = (entry, lens, aligned, n_rest, sa, sb, bound)
                assert int(flag) == (0 if safe else 1), what
                assert float(coef) == (np.float32(scale) if safe else -7.0), what
                if with_rest and n_rest:
                    assert abs(float(acc) - total) <= SUM_RTOL * total, what
                else:
                    assert float(acc) == np.float32(pre), what
    if aligned:    # ngp_clip_decide takes no running sum at all
        coef = torch.full((1,), -7.0, device=DEV)
        flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
        call("clip_decide", T(np.array([3.0 / fa, 4.0 / fb], np.float32)), *wargs, None, 50.0, 1.0, coef, flag)
        assert int(flag) == 0 and float(coef) == 1.0


@pytest.mark.parametrize("cols", [1, 3, 16])
def test_row_norm_sum_shapes(ngp, cols):
    """one lane per row: strided rows (ldx > cols), a row count on either side of one workgroup, rows of zeros, a sum that
    continues from what the accumulator holds"""
    call = ngp._lib.call
    g = np.random.default_rng(cols)
    ldx = cols + 3
    for n in (1, 255, 256, 257):
        rows = g.normal(size=(n, ldx)).astype(np.float32)
        rows[::3, :cols] = 0.0
        want = np.sqrt((rows[:, :cols].astype(np.float64) ** 2).sum(1)).sum()
        for pre in (0.0, 2.5):
            acc = torch.full((1,), pre, device=DEV)
            call("row_norm_sum", T(rows), ldx, n, cols, acc)
            assert abs(float(acc) - (pre + want)) <= 1e-5 * (pre + want), (n, cols, pre)
        rows[:, :cols] = 0.0                                   # the columns behind `cols` stay nonzero: they are not read
        acc = torch.full((1,), 2.5, device=DEV)
        call("row_norm_sum", T(rows), ldx, n, cols, acc)
        assert float(acc) == 2.5


# ---------------------------------------------------------------------------------------------------- the trainer's step
def _sample(tr, gen):
    """indices into the flat buffers: 64 on either side of every border of the sweep's two pieces, the whole MLP tail, and
    per table 2^19 seeded positions with a gradient and 2^19 drawn uniformly"""
    n, b0, lo = tr.flat_grad.numel(), tr.buckets.bounds[1], tr._mlp_lo
    assert 0 < b0 < lo < n and b0 % 4 == 0
    near = torch.cat([torch.arange(c - 64, c + 64, device=DEV) for c in (0, b0, lo, n)])
    parts = [near[(near >= 0) & (near < n)], torch.arange(lo, n, device=DEV)]
    for a, b in ((0, b0), (b0, lo)):
        nz = torch.nonzero(tr.flat_grad[a:b]).flatten()
        assert nz.numel() > 0
        parts.append(a + nz[torch.randint(nz.numel(), (2 ** 19,), device=DEV, generator=gen)])
        parts.append(torch.randint(a, b, (2 ** 19,), device=DEV, generator=gen))
    return torch.unique(torch.cat(parts))


def _watch_optimizer_step(tr, seen):
    """tr.optimizer_step between a snapshot of what it consumes and the comparison of what it leaves"""
    from ngp_amd import _lib
    orig = tr.optimizer_step
    gen = torch.Generator(device=DEV).manual_seed(17)

    def watched():
        torch.cuda.synchronize()
        n = tr.flat_grad.numel()
        idx = _sample(tr, gen)
        before = {k: N(b[idx]) for k, b in zip("pgmv", (tr.flat_param, tr.flat_grad, tr.exp_avg, tr.exp_avg_sq))}
        norm_sq = float((tr.flat_grad.double() ** 2).sum())
        still = (tr.flat_grad == 0) & (tr.exp_avg == 0) & (tr.exp_avg_sq == 0)
        p_before = tr.flat_param.clone()
        lr = tr.lr_at(min(tr.global_step // tr.steps_per_epoch, tr.num_epochs))
        early = bool(tr._norm_share_armed and tr._norm_share_fired == 1)
        _lib.CAPTURE = {"clip_decide_rest": [], "sumsq": [], "sumsq_if": [], "clip_coef": [], "clip_coef_if": [],
                        "adam_step_width": []}
        try:
            orig()
            calls = {k: [[a for a in args if isinstance(a, int)] for args in v] for k, v in _lib.CAPTURE.items()}
        finally:
            _lib.CAPTURE = None
        tr.wait()
        torch.cuda.synchronize()
        coef = float(tr.scalars[1])
        check_coef(coef, norm_sq, float(tr.clip_norm), 1.0, margin=2 * SUM_RTOL)   # (the device's own sum is within SUM_RTOL)
        a = args_of(coef, 0.0, tr.global_step, lr, 1)
        x = dict(before, still=(before["g"] == 0) & (before["m"] == 0) & (before["v"] == 0))
        got = [N(b[idx]) for b in (tr.flat_param, tr.flat_grad, tr.exp_avg, tr.exp_avg_sq)]
        r = check(x, a, got, f"step {tr.global_step}, {idx.numel()} of {n} entries, coef {coef:.6g}, lr {lr:.6g}")
        assert not tr.flat_grad.any()
        assert float(tr.scalars[0]) == 0.0 and not tr.norm_acc.any()
        same = tr.flat_param.view(torch.int32) == p_before.view(torch.int32)
        assert not (still & ~(same & (tr.exp_avg.view(torch.int32) == 0) & (tr.exp_avg_sq.view(torch.int32) == 0))).any()
        seen.append(dict(coef=coef, lr=lr, step=tr.global_step, need_exact=int(tr.need_exact), norm=norm_sq ** 0.5,
                         moved=int((~same).sum()), ratios=r, state=float(np.abs(before["m"]).max()), early=early,
                         calls=calls))
    tr.optimizer_step = watched


ROUTES = {
    # name: (norm_bound, clip_norm, armed, steps, steps_per_epoch)
    "bound": (True, 50.0, True, 2, 1000),           # need_exact == 0; the second step starts from nonzero moments
    "bound_fallback": (True, 1e-4, True, 1, 1000),  # the bound cannot clear 1e-4: the device takes the exact norm, coef < 1
    "early_share": (False, 50.0, True, 2, 2),       # the colour table's share summed behind its scatter; step 2 opens epoch 2
    "full_sum": (False, 50.0, False, 1, 1000),      # no share was armed: one sum over the whole buffer
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_trainer_optimizer_step_against_float64(ngp, route):
    """clip_grad_norm_(clip_norm) + Adam at the schedule's lr, as NGPTrainer.step runs them on 2048 rays: the coefficient
    against the float64 norm of the gradient, p, m and v on the sample against adam_step64 with that coefficient, the
    gradient and both accumulators zero afterwards, untouched entries untouched"""
    import test_gpu_parity as parity
    from helpers import make_rays
    from ngp_amd.trainer import NGPTrainer
    bound, clip, armed, steps, spe = ROUTES[route]
    o, d = make_rays(2048, scale=1.0, seed=93)
    o, d = T(o), T(d)
    gt = torch.rand(2048, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    model = parity._grid_model(ngp, seed=4)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    tr = NGPTrainer(model, lr=1e-2, clip_norm=clip, num_epochs=4, steps_per_epoch=spe)
    assert tr.norm_bound
    tr.norm_bound = bound
    tr.global_step = 1
    if not armed:      # a backward that step() did not announce: the early share does not fire, the sum is the plain full one
        assert model.rgb_encoder.on_grad_ready == tr._early_norm_share

        def unannounced():
            tr._norm_share_armed = False
            tr._early_norm_share()
        model.rgb_encoder.on_grad_ready = unannounced
    seen = []
    _watch_optimizer_step(tr, seen)
    for _ in range(steps):
        tr.step(o, d, gt)
    print(route, seen)
    assert len(seen) == steps and [s["step"] for s in seen] == list(range(2, 2 + steps))
    n, b0, lo = tr.flat_grad.numel(), tr.buckets.bounds[1], tr._mlp_lo
    for s in seen:
        c = s["calls"]
        assert s["moved"] > 0 and s["norm"] > 0
        assert [a[0] for a in c["adam_step_width"]] == [n - b0, b0] and all(a[1] == s["step"] for a in c["adam_step_width"])
        if bound:
            assert not s["early"] and len(c["clip_decide_rest"]) == 1 and c["sumsq_if"] == [[lo]] and len(c["clip_coef_if"]) == 1
            assert not c["sumsq"] and not c["clip_coef"]
        else:
            assert s["early"] == armed and not c["clip_decide_rest"] and len(c["clip_coef"]) == 1
            assert c["sumsq"] == ([[n - b0]] if armed else [[n]])
    if route == "bound":
        assert all(s["need_exact"] == 0 and s["coef"] == 1.0 and s["lr"] == tr.lr_at(0) for s in seen) and seen[1]["state"] > 0
    elif route == "bound_fallback":
        assert seen[0]["need_exact"] == 1 and 0 < seen[0]["coef"] < 0.5
    elif route == "early_share":
        assert all(s["coef"] == 1.0 for s in seen) and seen[1]["state"] > 0
        assert seen[0]["lr"] == tr.lr_at(0) and seen[1]["lr"] == tr.lr_at(1) < 0.9 * tr.lr_at(0)
    else:
        assert seen[0]["coef"] == 1.0


def test_pose_step_against_float64(ngp):
    """NGPTrainer._pose_step: clip_grad_norm_(clip_norm) + Adam(pose_lr) over [dR | dT], steps in a row (pose_steps counts),
    without clipping and with it"""
    import test_gpu_parity as parity
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    model = parity._grid_model(ngp, seed=4)
    scene = LegoProxy(n_images=3, img_wh=(24, 24), device=DEV)
    ref = PoseRefiner(scene.poses, scene.directions).to(DEV)
    g = np.random.default_rng(23)
    tr = NGPTrainer(model, lr=1e-2, pose_refiner=ref, pose_lr=1e-6)
    n = tr.pose_grad.numel()
    assert tr.pose_lr == 1e-6 and n % 4 == 0 and tr.pose_param.data_ptr() % 16 == 0 and tr.pose_steps == 0
    with torch.no_grad():
        tr.pose_param.copy_(T((g.normal(size=n) * 0.02).astype(np.float32)))
    for k, clip in enumerate((50.0, 50.0, 0.5, 0.5), start=1):
        tr.clip_norm = clip
        grad = (g.normal(size=n) * 10.0 ** g.uniform(-9, 0, n)).astype(np.float32)
        grad[g.random(n) < 0.3] = 0.0
        grad[0] = 2.0                                            # the norm lies between the two thresholds
        tr.pose_grad.copy_(T(grad))
        bufs = (tr.pose_param, tr.pose_grad, tr.pose_exp_avg, tr.pose_exp_avg_sq)
        x = {name: N(b).copy() for name, b in zip("pgmv", bufs)}
        x["still"] = (x["g"] == 0) & (x["m"] == 0) & (x["v"] == 0)
        tr._pose_step()
        torch.cuda.synchronize()
        assert tr.pose_steps == k
        coef = float(tr.pose_scalars[1])
        check_coef(coef, float((grad.astype(np.float64) ** 2).sum()), clip, 1.0, margin=2 * SUM_RTOL)
        assert (coef == 1.0) == (clip == 50.0)
        check(x, args_of(coef, 0.0, k, 1e-6, 1), [N(b) for b in bufs], f"pose step {k}, clip {clip}")
