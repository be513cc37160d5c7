"""float64 numpy restatement of the HDR tone-mappers (NGP(rgb_act='None'): per colour channel a tinycudann.Network
1 -> 64 (ReLU) -> 1 (Sigmoid), bias-free, whose one input tcnn pads to 16 columns with ones), forward and backward, written
with the padded matrices as they stand: nothing is folded, so the kernels' folding of the 15 ones-columns is checked too.

params: three arrays of 2048 floats, W1 (64, 16) row-major, then W2 (16, 64).
    x = [log_radiance + ln(exposure), 1, ..., 1]   z = x W1^T   h = relu(z)   y = sigmoid(h W2[0])
The backward also returns, for every parameter-gradient sum, the sum of the ABSOLUTE contributions: the scale an error of a
float32 sum is measured against (a sum of terms of both signs may cancel to far less than its rounding error).
"""
import numpy as np

H, IN, N_PARAMS = 64, 16, 2048
CHUNK = 32768


def split(params):
    """-> W1 (64, 16), W2 (16, 64) as float64"""
    p = np.asarray(params, dtype=np.float64).reshape(-1)
    assert p.size == N_PARAMS
    return p[:H * IN].reshape(H, IN), p[H * IN:].reshape(IN, H)


def _log_exposure(exposure, n):
    if exposure is None:
        return np.zeros(n)
    e = np.asarray(exposure, dtype=np.float64).reshape(-1)
    assert e.size in (1, n)
    return np.broadcast_to(np.log(e), (n,))


def _hidden(W1, u):
    x = np.ones((u.shape[0], IN))
    x[:, 0] = u
    return x, x @ W1.T


def forward(params3, log_radiance, exposure=None):
    """rgb (n, 3) float64"""
    lr = np.asarray(log_radiance, dtype=np.float64)
    n = lr.shape[0]
    le = _log_exposure(exposure, n)
    out = np.empty((n, 3))
    for c in range(3):
        W1, W2 = split(params3[c])
        for a in range(0, n, CHUNK):
            _, z = _hidden(W1, lr[a:a + CHUNK, c] + le[a:a + CHUNK])
            with np.errstate(over="ignore"):
                out[a:a + CHUNK, c] = 1.0 / (1.0 + np.exp(-(np.maximum(z, 0.0) @ W2[0])))
    return out


def backward(params3, log_radiance, exposure, dL_drgb):
    """-> d_log_radiance (n, 3), dparams (3, 2048), scale (3, 2048): the gradients of sum(rgb * dL_drgb) and, per parameter,
    the sum over the samples of |contribution|.  ReLU derivative: z > 0 (0 at z = 0); rows 1..15 of W2 get nothing."""
    lr = np.asarray(log_radiance, dtype=np.float64)
    dy = np.asarray(dL_drgb, dtype=np.float64)
    n = lr.shape[0]
    le = _log_exposure(exposure, n)
    dlr = np.empty((n, 3))
    dparams, scale = np.zeros((3, N_PARAMS)), np.zeros((3, N_PARAMS))
    for c in range(3):
        W1, W2 = split(params3[c])
        dW1, sW1 = np.zeros((H, IN)), np.zeros((H, IN))
        dW2, sW2 = np.zeros((IN, H)), np.zeros((IN, H))
        for a in range(0, n, CHUNK):
            x, z = _hidden(W1, lr[a:a + CHUNK, c] + le[a:a + CHUNK])
            h = np.maximum(z, 0.0)
            e = np.exp(-np.abs(h @ W2[0]))                  # sigmoid' = e^-|s| / (1 + e^-|s|)^2: y (1 - y) without the
            dt = dy[a:a + CHUNK, c] * (e / (1.0 + e) ** 2)    # cancellation of 1 - y next to saturation
            dz = (dt[:, None] * W2[0][None, :]) * (z > 0)
            dW2[0] += dt @ h
            sW2[0] += np.abs(dt) @ h
            dW1 += dz.T @ x
            sW1 += np.abs(dz).T @ np.abs(x)
            dlr[a:a + CHUNK, c] = dz @ W1[:, 0]
        dparams[c] = np.concatenate([dW1.reshape(-1), dW2.reshape(-1)])
        scale[c] = np.concatenate([sW1.reshape(-1), sW2.reshape(-1)])
    return dlr, dparams, scale


def loss(params3, log_radiance, exposure, dL_drgb):
    """sum(rgb * dL_drgb): what backward() differentiates"""
    return float((forward(params3, log_radiance, exposure) * np.asarray(dL_drgb, dtype=np.float64)).sum())
