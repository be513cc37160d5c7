"""Restatement of the transient mask field (models/implicit_mask.py) and of the masked loss (losses.py:85-94, 142-151)
for the tests: the encoder is the C oracle's (oracle.grid_fwd / oracle.grid_bwd_param, float32 like tiny-cuda-nn), the
MLP, the sigmoid, the loss and their gradients are float64 numpy.  Also the seeded inputs of tests/test_mask_gpu.py, so
that the host suite can check their selection rule without a GPU."""
import math

import numpy as np

import oracle

L, F, LOG2_T, N_MIN = 8, 2, 16, 16
PER_LEVEL_SCALE = math.exp(math.log(2048 / N_MIN) / (L - 1))
KEYS = ("mask_encoder.params", "mask_net.0.weight", "mask_net.0.bias", "mask_net.2.weight", "mask_net.2.bias")
SHAPES = {"mask_encoder.params": (860160,), "mask_net.0.weight": (64, 16), "mask_net.0.bias": (64,),
          "mask_net.2.weight": (1, 64), "mask_net.2.bias": (1,)}
RELU_MARGIN = 1e-5      # rows with a first-layer pre-activation closer to zero than this are left out of backward tests
MAX_DROPPED = 0.02      # ... and at most this share of a batch may go

_LAYOUT = None


def layout():
    global _LAYOUT
    if _LAYOUT is None:
        _LAYOUT = oracle.grid_layout(L, F, LOG2_T, N_MIN, PER_LEVEL_SCALE)
    return _LAYOUT


def forward(p, uvi):
    """p: {key: array}; uvi (n, 3) float32 -> dict(feat float32 (n,16), z1, a1 (n,64), z2, mask (n,) float64)"""
    desc, _ = layout()
    uvi = np.ascontiguousarray(uvi, np.float32)
    feat = oracle.grid_fwd(desc, np.ascontiguousarray(p["mask_encoder.params"], np.float32), uvi)
    W1, b1 = p["mask_net.0.weight"].astype(np.float64), p["mask_net.0.bias"].astype(np.float64)
    W2, b2 = p["mask_net.2.weight"].astype(np.float64), p["mask_net.2.bias"].astype(np.float64)
    z1 = feat.astype(np.float64) @ W1.T + b1
    a1 = np.maximum(z1, 0.0)
    z2 = (a1 @ W2.T + b2)[:, 0]
    return {"feat": feat, "z1": z1, "a1": a1, "z2": z2, "mask": 1.0 / (1.0 + np.exp(-z2))}


def backward(p, uvi, dL_dmask, fwd=None):
    """gradients of sum(dL_dmask * mask) -> {key: array}: float64 for the MLP; the table gradient is the oracle's float32
    scatter of the float32-rounded d feat.  Also 'dfeat' (n,16) float64."""
    desc, n_params = layout()
    fwd = forward(p, uvi) if fwd is None else fwd
    g = np.asarray(dL_dmask, np.float64).reshape(-1)
    m = fwd["mask"]
    dz2 = (g * m * (1.0 - m))[:, None]
    W1, W2 = p["mask_net.0.weight"].astype(np.float64), p["mask_net.2.weight"].astype(np.float64)
    dz1 = (dz2 @ W2) * (fwd["z1"] > 0)
    dfeat = dz1 @ W1
    out = {"mask_net.2.weight": dz2.T @ fwd["a1"], "mask_net.2.bias": dz2.sum(0),
           "mask_net.0.weight": dz1.T @ fwd["feat"].astype(np.float64), "mask_net.0.bias": dz1.sum(0), "dfeat": dfeat}
    out["mask_encoder.params"] = oracle.grid_bwd_param(desc, np.ascontiguousarray(uvi, np.float32),
                                                       np.ascontiguousarray(dfeat, np.float32), n_params)
    return out


def masked_loss(rgb, gt, mask, size_delta):
    """NeRFLoss(embed_msk=True)'s two mask-dependent terms and the gradient of sum(term.mean()) w.r.t. the mask (n,):
    -> r_ms (scalar), rgb term (n,3), d_mask (n,), d_rgb (n,3)"""
    rgb, gt = np.asarray(rgb, np.float64), np.asarray(gt, np.float64)
    m = np.asarray(mask, np.float64).reshape(-1)
    n = len(m)
    e = rgb - gt
    r_ms = size_delta * np.mean(m * m)
    term = (1.0 - m)[:, None] * e * e
    d_mask = 2.0 * size_delta * m / n - (e * e).sum(1) / (3.0 * n)
    d_rgb = 2.0 * (1.0 - m)[:, None] * e / (3.0 * n)
    return r_ms, term, d_mask, d_rgb


# ------------------------------------------------------------------ seeded inputs of the GPU tests
SIZES = (1, 63, 64, 65, 257, 4099)   # below, at and just over a wave; a ragged last workgroup; more than one workgroup


W2_GAIN = 10.0
PARAM_SEED = 1


def make_params(seed=PARAM_SEED):
    """table uniform +-0.3, W1 / b1 / b2 normal * 0.3, W2 normal * 0.3 * W2_GAIN.  With W2 at normal * 0.3 as well the
    interpolated features (|f| ~ 0.1) move the output pre-activation by a few tenths only and the float64 mask stays
    within 0.26 .. 0.71 for every seed tried: the tests' own requirement "min < 0.2 and max > 0.8" could not hold.  The
    gain and the seed were chosen on the float64 reference alone; at this seed every batch of 63 rows and more reaches
    both tails and none saturates to 0 or 1 in float32."""
    g = np.random.default_rng(1700 + seed)
    p = {}
    for k in KEYS:
        if k == "mask_encoder.params":
            p[k] = g.uniform(-0.3, 0.3, SHAPES[k]).astype(np.float32)
        else:
            p[k] = (g.standard_normal(SHAPES[k]) * 0.3).astype(np.float32)
    p["mask_net.2.weight"] = p["mask_net.2.weight"] * np.float32(W2_GAIN)
    return p


def special_rows():
    """-0.5 and 0 exactly; points on cell faces (scale_l * x + 0.5 an integer) of levels 0-2: the two dense levels and the
    first hashed one; the largest float32 below 0.5"""
    desc, _ = layout()
    rows = [[-0.5, -0.5, -0.5], [0.0, 0.0, 0.0], [-0.5, 0.0, 0.25], [0.49999997, 0.49999997, 0.49999997],
            [0.49999997, -0.5, 0.0]]
    for l in range(3):
        sc = float(desc.scale[l])
        for k in (-3, 1, 5):
            x = (k - 0.5) / sc
            rows.append([x, 0.1, -0.2])
            rows.append([0.3, x, x])
    return np.array(rows, np.float32)


def make_uvi(n, seed=PARAM_SEED):
    g = np.random.default_rng(1800 + seed + n)
    uvi = g.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    uvi = np.minimum(uvi, np.float32(0.49999997))   # (float32 rounding of a float64 draw may reach 0.5)
    s = special_rows()
    k = min(len(s), n - 1)
    uvi[:k] = s[:k]
    return uvi


def select_rows(p, uvi):
    """rows kept for the backward tests: every first-layer pre-activation at least RELU_MARGIN away from zero in the
    float64 reference (a ReLU decided the other way in float32 would change a whole row's contribution)"""
    z1 = forward(p, uvi)["z1"]
    return np.abs(z1).min(1) >= RELU_MARGIN
