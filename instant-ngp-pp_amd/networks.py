"""NGP field of the reference (models/networks.py:13-420) on the MI355X library.

Same constructor, buffers (`center, xyz_min, xyz_max, half_size, density_bitfield`; the trainer
adds `density_grid`, `grid_coords`), attributes (`cascades, scale, grid_size`), methods
(`density, grad, forward, forward_test, forward_skybox, get_all_cells,
sample_uniform_and_occupied_cells, mark_invisible_cells, update_density_grid`) and state-dict
keys (`xyz_encoder.params`, `xyz_net.0.weight`, `rgb_net.params`, ...), so reference
checkpoints map one to one.

Differences, all deliberate:
  * by default d(sigma)/dx is computed analytically in the forward pass (sigmoid-gated
    back-substitution through the 2-layer density MLP + the grid input-gradient kernel) instead of
    torch.autograd.grad(create_graph=True) (networks.py:186-196).  The values are identical; the
    result is detached, i.e. normals_raw carries no gradient — which is what every recipe without
    --normal_ref needs.  Setting `model.differentiable_normals = True` switches forward() to the
    reference's own formulation, with the grid double backward (H4) on ngp_grid_bwd_bwd_input.
    `model.second_order_normals = True` keeps the fused node instead and makes its d(sigma)/dx differentiable: the second
    order then runs on ngp_grid_bwd_bwd_input, ngp_density_head_bwd2 and four existing products (what
    NGPTrainer(normal_ref=True) trains through).
"""
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function

from . import tinycudann as tcnn
from . import vren
from ._lib import call, call_host
from .appearance import RayCodes
from .custom_functions import TruncExp
from .link import FieldLink
from .rendering import NEAR_DISTANCE

_f32 = torch.float32
_SOFTPLUS = 3


class _LinearAct(Function):
    """y = act(x W^T + b) with nn.Linear parameter layout; also returns the pre-activation
    (non-differentiable output, needed by Softplus' backward and by the analytic d(sigma)/dx)."""

    @staticmethod
    def forward(ctx, x, W, b, act):
        x = x.contiguous()
        n, ni = x.shape
        no = W.shape[0]
        y = torch.empty(n, no, dtype=_f32, device=x.device)
        z = torch.empty(n, no, dtype=_f32, device=x.device)
        call("linear_fwd", x, ni, W, ni, b, n, ni, no, act, y, no, z)
        ctx.save_for_backward(x, W, y, z)
        ctx.act = act
        ctx.has_bias = b is not None
        ctx.mark_non_differentiable(z)
        return y, z

    @staticmethod
    def backward(ctx, dy, _dz):
        x, W, y, z = ctx.saved_tensors
        n, ni = x.shape
        no = W.shape[0]
        act = ctx.act
        dz = dy.contiguous()
        if act != 0:
            dz = torch.empty_like(dz)
            call("act_bwd", dy.contiguous(), y, dz.numel(), act, dz)
        dx = dW = db = None
        if ctx.needs_input_grad[1]:
            dW = torch.zeros_like(W)
            db = torch.zeros(no, dtype=_f32, device=x.device) if ctx.has_bias else None
            call("linear_bwd_weight", dz, no, x, ni, n, ni, no, dW, ni, db)
        if ctx.needs_input_grad[0]:
            dx = torch.empty(n, ni, dtype=_f32, device=x.device)
            call("linear_bwd_input", dz, no, W, ni, n, ni, no, dx, ni, 0)
        return dx, dW, db, None


_RELU, _NONE = 1, 0

# widest second layer that takes the fused route (tools/mlp_bwd_microbench.py, n = 433 k, MI355X):
# density head 0.54 -> 0.49 ms, rgb_net 0.60 -> 0.57 ms, 32-wide headers 0.22 -> 0.22 ms
_FUSED_BWD_MAX_OUT = 3
# Per-device default streams of the field, by role: "colour" (the colour branch of the forward), "scatter" (the backward's
# table scatters) and "heads" (the two 32-wide heads of the forward).
_STREAMS = {}


def _stream(role, dev, own=None):
    """`own` (the stream a trainer put on the model's link) if there is one, else the device's default for the role"""
    key = (role, torch.device(dev).index)
    if own is None and key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device=dev)
    return _STREAMS[key] if own is None else own


class _Mlp2(NamedTuple):
    """A 2-layer MLP as the kernels see it: hidden (H) = act1(x W1^T + b1), out (n_out) = act2(hidden W2^T + b2).  W1 is
    (H, n_in) with leading dimension ldw1, W2 (>= n_out, H) with leading dimension H; either may be a flat slice."""
    W1: torch.Tensor
    ldw1: int
    b1: Optional[torch.Tensor]
    W2: torch.Tensor
    b2: Optional[torch.Tensor]
    n_in: int
    H: int
    n_out: int
    act1: int
    act2: int

    @classmethod
    def tcnn(cls, params, n_in, H, n_out, act2):
        """a bias-free tinycudann.Network with one ReLU hidden layer: params = [W1 (H, n_in) | W2 (padded n_out, H)]"""
        return cls(params, n_in, None, params[H * n_in:], None, n_in, H, n_out, _RELU, act2)

    def grad_slices(self, flat):
        """(dW1, dW2, db1, db2) inside `flat`, the gradient of a tcnn() net's params"""
        return flat, flat[self.H * self.n_in:], None, None

    def forward(self, x, ldx, n, hidden, out, dact=None):
        """both layers in one launch, the second in the MFMA epilogue; dact (n, n_out): the launch also leaves act2'(z2)"""
        args = (x, ldx, self.W1, self.ldw1, self.b1, self.act1, self.W2, self.H, self.b2, self.act2, n, self.n_in, self.H,
                self.n_out, hidden, self.H, out, self.n_out)
        if dact is None:
            call("mlp2_fwd", *args)
        else:
            call("mlp2_fwd_dact", *args, dact)


class _Mlp2Bwd:
    """Backward of a 2-layer MLP (x_in -> H hidden with act1 -> n_out with act2) on the library, in three stages
    the caller can interleave with other work: the constructor runs the elementwise stage (dz2, on the plain route
    also dz1), input_product() the data gradient dz1 . W1[:, cols], weight_products() dW1 / dW2 / db1 / db2.
    On the fused route dz1 = act1'(hidden) * (dz2 . W2) is formed inside the two first-layer products."""

    def __init__(self, mlp, grads, acts, norm_acc=None):
        """mlp: the _Mlp2; grads = (dW1, dW2, db1, db2), the destinations the weight products add to; acts = (d_out, out,
        hidden, x_in, ld_in), the loss gradient and what the forward left, x_in with its leading dimension
        norm_acc: device scalar that takes sum_s ||dz2[s]|| (the trainer's norm-bound sums), accumulated by the pass
        that forms dz2 when that pass is the elementwise one (self.norm_noted says whether it was)"""
        self.mlp = mlp
        self.dW1, self.dW2, self.db1, self.db2 = grads
        d_out, out, self.hidden, self.x_in, self.ld_in = acts
        H, n_out = mlp.H, mlp.n_out
        self.norm_noted = False
        n = self.n = self.hidden.shape[0]
        dev = self.hidden.device
        ld_out = out.stride(0)
        self.fused = bool(n_out <= _FUSED_BWD_MAX_OUT and d_out.stride(0) == n_out and ld_out == n_out)
        self.dz1 = None
        self.dw2_done = False
        if self.fused:
            self.dz2 = torch.empty(n, n_out, dtype=_f32, device=dev)
            if norm_acc is not None and n_out <= 4:
                call("act_bwd_rows", d_out, out, n, n_out, mlp.act2, self.dz2, norm_acc)
                self.norm_noted = True
            else:
                call("act_bwd", d_out, out, n * n_out, mlp.act2, self.dz2)
            return
        self.dz2 = torch.empty(n, 16 if n_out > 4 else 4, dtype=_f32, device=dev)
        self.dz1 = torch.empty(n, H, dtype=_f32, device=dev)
        if n_out <= 4:   # dW2 / db2 come out of the same pass over the hidden activations
            call("mlp_hidden_bwd", d_out, d_out.stride(0), out, ld_out, mlp.act2, mlp.W2, H, self.hidden, H, mlp.act1, n, H,
                 n_out, None, 0, self.dz1, H, self.dW2, H, self.db2)
            self.dw2_done = True
        else:
            call("mlp_hidden_bwd", d_out, d_out.stride(0), out, ld_out, mlp.act2, mlp.W2, H, self.hidden, H, mlp.act1, n, H,
                 n_out, self.dz2, self.dz2.shape[1], self.dz1, H, None, 0, None)

    def input_product(self, dx, ld_dx, dx_cols, w1_col0, accumulate):
        """dx (+)= dz1 . W1[:, w1_col0 : w1_col0 + dx_cols] (the input columns that need a gradient)"""
        mlp = self.mlp
        w1_dx = mlp.W1[w1_col0:] if mlp.W1.dim() == 1 else mlp.W1
        if self.fused:
            call("mlp_bwd_input", self.dz2, mlp.n_out, mlp.W2, mlp.H, self.hidden, mlp.H, mlp.act1, w1_dx, mlp.ldw1, self.n,
                 dx_cols, mlp.H, mlp.n_out, dx, ld_dx, 1 if accumulate else 0)
        else:
            call("linear_bwd_input", self.dz1, mlp.H, w1_dx, mlp.ldw1, self.n, dx_cols, mlp.H, dx, ld_dx,
                 1 if accumulate else 0)

    def weight_products(self):
        # One launch per product whatever n_in: rgb_net's 144 / 160 columns go through the streaming kernel in one pass,
        # and every other first layer is at most 128 columns wide.
        mlp, n = self.mlp, self.n
        H, n_out = mlp.H, mlp.n_out
        if self.fused:
            # the first-layer weight product streams dz2 and hidden anyway: it also leaves dW2 / db2
            call("mlp_bwd_weight", self.dz2, n_out, mlp.W2, H, self.hidden, H, mlp.act1, self.x_in, self.ld_in, n, mlp.n_in, H,
                 n_out, self.dW1, mlp.ldw1, self.db1, self.dW2, H, self.db2)
            return
        if not self.dw2_done:
            call("linear_bwd_weight", self.dz2, self.dz2.shape[1], self.hidden, H, n, H, n_out, self.dW2, H, self.db2)
        call("linear_bwd_weight", self.dz1, H, self.x_in, self.ld_in, n, mlp.n_in, H, self.dW1, mlp.ldw1, self.db1)


def _density_mlp(W1, b1, W2, b2):
    """the density head 128 -> 128 -> 1, Softplus on both layers, with nn.Linear parameters"""
    return _Mlp2(W1, 128, b1, W2, b2, 128, 128, 1, _SOFTPLUS, _SOFTPLUS)


def _field_mlps(model, W1, b1, W2, b2, rgb_p, nrm_p, sem_p):
    """the four MLPs of the field node -> (density head, rgb_net, normal head, semantic head)"""
    net = model.rgb_net
    return (_density_mlp(W1, b1, W2, b2),
            _Mlp2.tcnn(rgb_p, net.padded_in, 128, 3, net.output_activation),
            _Mlp2.tcnn(nrm_p, 128, 32, 3, _NONE),
            _Mlp2.tcnn(sem_p, 128, 32, model.semantic_header.n_output_dims, _NONE))


class _NegNormalize(Function):
    """y = -F.normalize(x * scale3, p=2, dim=-1, eps=1e-6) on (N,3) rows, one launch each way."""

    @staticmethod
    def forward(ctx, x, scale3):
        x = x.contiguous()
        y = torch.empty(x.shape[0], 3, dtype=_f32, device=x.device)
        call("neg_normalize", x, 3, scale3, x.shape[0], y)
        if scale3 is None:
            ctx.save_for_backward(x)
        elif ctx.needs_input_grad[0]:   # (second-order normals: d(sigma)/dx carries a graph)
            ctx.save_for_backward(x, scale3)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        x, *scale3 = ctx.saved_tensors
        if scale3:   # the chain rule around the scaling: the kernel differentiates -normalize at x * scale3
            x = x * scale3[0]
        dx = torch.empty_like(x)
        call("neg_normalize_bwd", x, 3, g.contiguous(), x.shape[0], dx)
        return (dx * scale3[0] if scale3 else dx), None


def _density_fused_ok(enc, W1, b1, W2, b2):
    """whether ngp_density_field_fwd takes the density path: a 16-level F = 8 table the tile kernels take and the
    128 -> 128 -> 1 head with contiguous (W1 16-byte aligned) parameters; anything else keeps the four launches"""
    ok = getattr(enc, "_density_fused_layout", None)
    if ok is None:
        ok = enc._density_fused_layout = bool(enc.n_levels == 16 and enc.n_features == 8 and
                                              call_host("density_field_layout_ok", enc.desc) == 1)
    return (ok and W1.is_cuda and tuple(W1.shape) == (128, 128) and W1.is_contiguous() and W1.data_ptr() % 16 == 0
            and W2.numel() == 128 and W2.is_contiguous() and (b1 is None or (b1.numel() == 128 and b1.is_contiguous()))
            and (b2 is None or b2.numel() == 1))


# The inputs of _FieldFn.forward (and so of NGP._field's apply), in order: backward looks up which of them need a gradient
# and hands its gradients back under these names.
_FIELD_INPUTS = ("model", "x", "d", "embed_a", "xyz_table", "W1", "b1", "W2", "b2", "rgb_table", "rgb_p", "nrm_p", "sem_p",
                 "ray_codes", "second_order")


class _Saved(NamedTuple):
    """What _FieldFn.forward keeps for backward, in save_for_backward's order."""
    xn: torch.Tensor            # (n, 3) normalised positions
    feat: torch.Tensor          # density path: grid features (n, 128), hidden layer a1 (n, 128), sigma (n, 1) and
    a1: torch.Tensor            # dsig_dfeat = d(sigma)/d(features) (n, 128)
    sig: torch.Tensor
    dsig_dfeat: torch.Tensor
    rgb_o: torch.Tensor         # colour branch: the three outputs (n, 3) (n, 3) (n, C), rgb_net's input matrix (n, Kp) and
    np_o: torch.Tensor          # the three hidden layers (n, 128) (n, 32) (n, 32)
    sem_o: torch.Tensor
    rgb_in: torch.Tensor
    a_r: torch.Tensor
    a_n: torch.Tensor
    a_s: torch.Tensor
    xyz_table: torch.Tensor
    W1: torch.Tensor
    W2: torch.Tensor
    rgb_table: torch.Tensor
    rgb_p: torch.Tensor
    nrm_p: torch.Tensor
    sem_p: torch.Tensor
    d: Optional[torch.Tensor]   # the view directions, kept only when they need a gradient (pose refinement: its kernel
                                # reads them again)


def _forward_buffers(n, C, Kp, dev):
    """Every buffer of one forward -> (d(sigma)/dxn (n, 3), the eleven of _Saved from feat to a_s).  They come from the
    caller's stream (the allocator then knows them as that stream's; the colour stream only launches into them and is
    joined before anything is returned)."""
    feat = torch.empty(n, 128, dtype=_f32, device=dev)
    a1 = torch.empty(n, 128, dtype=_f32, device=dev)
    sig = torch.empty(n, 1, dtype=_f32, device=dev)
    dfeat = torch.empty(n, 128, dtype=_f32, device=dev)
    grads = torch.empty(n, 3, dtype=_f32, device=dev)   # d sigma / d xn (normalised coordinates)
    rgb_o = torch.empty(n, 3, dtype=_f32, device=dev)
    np_o = torch.empty(n, 3, dtype=_f32, device=dev)
    sem_o = torch.empty(n, C, dtype=_f32, device=dev)
    rgb_in = torch.empty(n, Kp, dtype=_f32, device=dev)
    a_r = torch.empty(n, 128, dtype=_f32, device=dev)
    a_n = torch.empty(n, 32, dtype=_f32, device=dev)
    a_s = torch.empty(n, 32, dtype=_f32, device=dev)
    return grads, (feat, a1, sig, dfeat, rgb_o, np_o, sem_o, rgb_in, a_r, a_n, a_s)


class _FieldCall:
    """One forward or one backward of the field node: what its stages share, and the stages.  _FieldFn.forward and
    _FieldFn.backward hold the schedule (which stage runs when, on which stream); a stage launches on the current stream."""

    def __init__(self, model, saved, E, side, b1=None, b2=None, need=None):
        """saved: the _Saved; E: length of the appearance codes; side: the stream fork() launches on; need: name of
        _FIELD_INPUTS -> whether it needs a gradient (backward)"""
        s = self.s = saved
        self.model, self.link = model, model.link
        self.xe, self.re = model.xyz_encoder, model.rgb_encoder
        self.n, self.dev = s.xn.shape[0], s.xn.device
        self.E, self.K, self.Kp, self.C = E, 144 + E, s.rgb_in.shape[1], s.sem_o.shape[1]
        self.W_cols = 128 + E       # [grid features | appearance code]: the columns of dfeat_rgb
        self.density_mlp, self.rgb_mlp, self.nrm_mlp, self.sem_mlp = _field_mlps(model, s.W1, b1, s.W2, b2, s.rgb_p, s.nrm_p,
                                                                                 s.sem_p)
        self.main, self.side, self.forked = torch.cuda.current_stream(), side, False
        self.need, self.grads = need, {}        # grads: name of _FIELD_INPUTS -> what autograd gets (absent: None)
        self.dfeat_rgb = None                   # backward: dL/d[grid features | appearance code] (n, W_cols)

    def fork(self, stage, *args):
        """stage(*args) on the side stream, behind everything the main stream holds so far"""
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            stage(*args)
        self.forked = True

    def join(self):
        if self.forked:
            self.main.wait_stream(self.side)

    def sink(self, name, like, acc):
        """Where the gradient of input `name` accumulates.  `acc`: the storage a trainer owns for it (NGPTrainer: views of
        one flat buffer, zeroed by its Adam launch), which the launches add straight into while autograd gets None — no
        zeros_like fill, no AccumulateGrad add per parameter.  Without one: a fresh zero buffer shaped as `like` (a tensor
        or a shape), which is also what autograd gets."""
        if acc is None:
            acc = self.grads[name] = (torch.zeros(like, dtype=_f32, device=self.dev) if isinstance(like, tuple)
                                      else torch.zeros_like(like))
        return acc

    def density_head_sinks(self):
        """-> (dW1, dW2, db1, db2) of the density head, for either of its backwards"""
        s, sinks = self.s, self.link.grad_sinks
        return tuple(self.sink(k, like, sinks.get(k)) for k, like in (("W1", s.W1), ("W2", s.W2), ("b1", (128,)), ("b2", (1,))))

    # ---- forward stages
    def colour_forward(self, d, embed_a, ray_codes, second_order, ev_p, ev_c):
        """[SH(16) | rgb grid features (128) | appearance code (E) | ones-padding] -> rgb_net and the two heads (the heads on
        their own stream when the fused kernel takes them), for the forward's colour stream"""
        s, n, E, K, Kp, C = self.s, self.n, self.E, self.K, self.Kp, self.C
        rgb_in = s.rgb_in
        feat_rgb = rgb_in[:, 16:144]
        if second_order:
            # The module route's own direction encoding, op for op (F.normalize, the [0,1] remap, ngp_sh_fwd), so that
            # both normal_ref routes hand rgb_net the same bits.  ngp_sh_fwd_dirs multiplies by a rounded reciprocal
            # and fuses the remap's add: 14 % of its basis values differ from these by up to 4e-7, which is enough to
            # move a ReLU pre-activation that lies within 1e-8 of zero across it and with it one sample's whole term of
            # dW1 (the reference's normal_ref step, G10, has such a sample: 5.5e-5 of rgb_net's gradient)
            dn = F.normalize(d, p=2, dim=-1, eps=1e-6)
            call("sh_fwd", ((dn + 1) / 2).contiguous(), n, 4, rgb_in, Kp)
        else:
            call("sh_fwd_dirs", d, n, 4, rgb_in, Kp)
        if ev_c is not None:
            ev_c.wait()   # the colour table's piece (the stream this runs on waits for it)
        call("grid_fwd", self.re.desc, s.rgb_table, s.xn, n, rgb_in[:, 16:], Kp)
        if ev_p is not None:
            ev_p.wait()   # the MLPs' piece
        if ray_codes is not None:
            img_idxs, rays_a = ray_codes
            if not getattr(rays_a, "_ngp_full_cover", False):   # rows outside every segment: finite inputs
                rgb_in[:, 144:K] = 0.0
                rgb_in[:, K:] = 1.0
            # codes and ones-padding of every sample in one launch
            call("embed_a_fwd", embed_a, embed_a.shape[0], E, img_idxs, rays_a, rays_a.shape[0], rgb_in[:, 144:], Kp,
                 Kp - 144)
        else:
            if E:
                rgb_in[:, 144:K] = embed_a
            if Kp > K:
                rgb_in[:, K:] = 1.0
        if C <= 8:
            # the two 32-wide heads read the same rows as rgb_net: on a stream of their own their 256-thread
            # workgroups (72 registers) fit beside the 8-wave rgb_net workgroup on every CU (-0.03 ms/step)
            cur = torch.cuda.current_stream()
            heads = _stream("heads", self.dev, self.link.heads_stream)
            heads.wait_stream(cur)
            with torch.cuda.stream(heads):
                self.nrm_mlp.forward(feat_rgb, Kp, n, s.a_n, s.np_o)
                self.sem_mlp.forward(feat_rgb, Kp, n, s.a_s, s.sem_o)
            self.rgb_mlp.forward(rgb_in, Kp, n, s.a_r, s.rgb_o)
            cur.wait_stream(heads)
        else:   # (the fused forward's epilogue takes at most 8 outputs)
            self.rgb_mlp.forward(rgb_in, Kp, n, s.a_r, s.rgb_o)
            self.nrm_mlp.forward(feat_rgb, Kp, n, s.a_n, s.np_o)
            call("linear_fwd", feat_rgb, Kp, self.sem_mlp.W1, 128, None, n, 128, 32, _RELU, s.a_s, 32, None)
            call("linear_fwd", s.a_s, 32, self.sem_mlp.W2, 32, None, n, 32, C, _NONE, s.sem_o, C, None)

    def density_forward(self, grads):
        """encoder, density head, d(sigma)/d(features) and d(sigma)/dxn (into grads), for the forward's main stream"""
        s, n, xe, mlp = self.s, self.n, self.xe, self.density_mlp
        if _density_fused_ok(xe, mlp.W1, mlp.b1, mlp.W2, mlp.b2):
            # encoder, both layers, d(sigma)/d(features) and d(sigma)/dx in one launch: feat, a1, sig and dfeat bitwise
            # those of the four launches below, grads within 128 ulps of the row's largest component
            call("density_field_fwd", xe.desc, s.xyz_table, s.xn, n, mlp.W1, mlp.b1, mlp.W2, mlp.b2, s.feat, s.a1, s.sig,
                 s.dsig_dfeat, grads)
        else:
            dz2 = torch.empty(n, 1, dtype=_f32, device=self.dev)
            call("grid_fwd", xe.desc, s.xyz_table, s.xn, n, s.feat, 128)
            # both layers in one launch, the 1-wide second layer in the MFMA epilogue, which also leaves
            # dz2 = softplus'(z2) = 1 - exp(-sigma): the start of the d(sigma)/dx pass below (no act_bwd launch)
            mlp.forward(s.feat, 128, n, s.a1, s.sig, dact=dz2)
            # analytic d(sigma)/dx: back-substitute ones through the head, then the grid input gradient
            call("mlp_bwd_input", dz2, 1, mlp.W2, 128, s.a1, 128, _SOFTPLUS, mlp.W1, 128, n, 128, 128, 1, s.dsig_dfeat, 128, 0)
            call("grid_bwd_input", xe.desc, s.xyz_table, s.xn, s.dsig_dfeat, 128, n, grads)
        # dsig_dfeat = d(sigma)/d(features) is kept: the density head has ONE output, so the gradient the backward
        # sends into the density encoder is d_sigma[s] * dsig_dfeat[s] — no second data-gradient product there

    # ---- backward stages
    def density_scatter(self, d_sig_c, buf):
        """the density table's scatter of d_sig[s] * d(sigma)/d(features)[s] into buf, for the backward's scatter stream"""
        call("grid_bwd_param_scaled", self.xe.desc, self.s.xn, self.s.dsig_dfeat, 128, d_sig_c, self.n, buf)
        self.xe.grad_ready()

    def rgb_net_data_grad(self, d_rgb):
        """rgb_net's elementwise stage and its data gradient w.r.t. [grid features | appearance code], which creates
        dfeat_rgb; for pose refinement also w.r.t. the 16 SH columns and on to dL/dd -> rgb_net's _Mlp2Bwd"""
        s, n, dev, W_cols = self.s, self.n, self.dev, self.W_cols
        acc = self.sink("rgb_p", s.rgb_p, self.link.grad_sinks.get("rgb_p"))
        self.dfeat_rgb = torch.empty(n, W_cols, dtype=_f32, device=dev)
        nb_acc = self.link.norm_acc
        st = _Mlp2Bwd(self.rgb_mlp, self.rgb_mlp.grad_slices(acc), (d_rgb.contiguous(), s.rgb_o, s.a_r, s.rgb_in, self.Kp),
                      norm_acc=None if nb_acc is None else nb_acc[0:1])
        st.input_product(self.dfeat_rgb, W_cols, W_cols, 16, False)
        if self.need["d"]:
            # dL/dd: rgb_net's data gradient for the 16 SH columns, then the adjoint of the direction encoding
            d_sh = torch.empty(n, 16, dtype=_f32, device=dev)
            st.input_product(d_sh, 16, 16, 0, False)
            g_d = self.grads["d"] = torch.empty(n, 3, dtype=_f32, device=dev)
            call("sh_bwd_dirs", s.d, d_sh, 16, n, g_d)
        return st

    def head_data_grads(self, d_np, d_sem):
        """the elementwise stages of the seeded 32-wide heads and their data gradients, added to dfeat_rgb (the first
        creates it when rgb_net has not) -> their _Mlp2Bwds"""
        s, n, dev, W_cols = self.s, self.n, self.dev, self.W_cols
        stages = []
        for d_o, name, mlp, a_h, out in ((d_np, "nrm_p", self.nrm_mlp, s.a_n, s.np_o),
                                         (d_sem, "sem_p", self.sem_mlp, s.a_s, s.sem_o)):
            if d_o is None:
                continue
            self.link.bound_spoiled()    # a head adds to the colour features' gradient: outside the norm bound
            acc = self.sink(name, getattr(s, name), self.link.grad_sinks.get(name))
            first = self.dfeat_rgb is None
            if first:
                self.dfeat_rgb = (torch.zeros(n, W_cols, dtype=_f32, device=dev) if self.E
                                  else torch.empty(n, W_cols, dtype=_f32, device=dev))
            st = _Mlp2Bwd(mlp, mlp.grad_slices(acc), (d_o.contiguous(), out, a_h, s.rgb_in[:, 16:], self.Kp))
            st.input_product(self.dfeat_rgb, W_cols, 128, 0, not first)
            stages.append(st)
        return stages

    def colour_scatter(self, buf):
        """the colour table's scatter of dfeat_rgb into buf, for the scatter stream (the main one without a density scatter)"""
        call("grid_bwd_param", self.re.desc, self.s.xn, self.dfeat_rgb, self.W_cols, self.n, buf)
        self.re.grad_ready()

    def code_and_position_grads(self, ray_codes, codes_shape):
        """what dfeat_rgb gives the node's inputs: the appearance codes' gradient (RayCodes: summed per image) and the
        colour table's share of dL/dx, for the backward's main stream"""
        n, E, W_cols, need = self.n, self.E, self.W_cols, self.need
        if E and need["embed_a"] and ray_codes is not None:
            # per-image sums of the code columns, one launch: into the trainer's sink when its shape is the table's
            img_idxs, rays_a = ray_codes
            acc = self.link.grad_sinks.get("embedding_a")
            acc = self.sink("embed_a", codes_shape, acc if acc is not None and tuple(acc.shape) == codes_shape else None)
            call("embed_a_bwd", self.dfeat_rgb[:, 128:], W_cols, E, img_idxs, rays_a, rays_a.shape[0], codes_shape[0], acc)
        elif E and need["embed_a"]:
            self.grads["embed_a"] = self.dfeat_rgb[:, 128:]
        if need["x"]:
            g_x = self.grads["x"] = torch.empty(n, 3, dtype=_f32, device=self.dev)
            call("grid_bwd_input", self.re.desc, self.s.rgb_table, self.s.xn, self.dfeat_rgb, W_cols, n, g_x)

    def colour_weight_products(self, stages):
        """dW1 / dW2 of rgb_net and the seeded heads into their sinks, for the main stream beside the scatters"""
        for st in stages:
            st.weight_products()

    def density_head(self, d_sig, reuse):
        """the density head's first-order backward into its sinks, for the main stream; reuse: the density table's share
        went out with density_scatter (or is not asked for), else the data gradient, its scatter and dL/dx run here"""
        s, n, xe = self.s, self.n, self.xe
        sinks = self.density_head_sinks()
        nb_acc = self.link.norm_acc
        st = _Mlp2Bwd(self.density_mlp, sinks, (d_sig.contiguous().view(n, 1), s.sig, s.a1, s.feat, 128),
                      norm_acc=None if nb_acc is None else nb_acc[1:2])
        if not reuse:
            dfeat = torch.empty(n, 128, dtype=_f32, device=self.dev)
            st.input_product(dfeat, 128, 128, 0, False)
        st.weight_products()
        self.link.bound_note(st, 1, 1, n)
        if not reuse:
            if self.need["xyz_table"]:
                buf = self.sink("xyz_table", s.xyz_table, xe.grad_buffer)
                call("grid_bwd_param", xe.desc, s.xn, dfeat, 128, n, buf)
                xe.grad_ready()
            if self.need["x"]:
                gx2 = torch.empty(n, 3, dtype=_f32, device=self.dev)
                call("grid_bwd_input", xe.desc, s.xyz_table, s.xn, dfeat, 128, n, gx2)
                self.grads["x"] = gx2 if "x" not in self.grads else self.grads["x"] + gx2

    def density_head_second_order(self, d_sig, v):
        """Both orders of the density path in one pass, for the main stream (include/ngp_hip.h, D2): v becomes
        u = dL/d(dfeat) and the table's second-order share in the grid's double backward, r = u W1^T, and
        ngp_density_head_bwd2 leaves m (dW1 += m^T u), e1 = dL/dz1 with the first-order share of d_sig inside it
        (dW1 += e1^T feat, db1, dL/dfeat = e1 W1) and dW2 / db2.  The d_sig-scaled scatter and the first-order weight
        products are not run: each share lands once."""
        s, n, dev, xe = self.s, self.n, self.dev, self.xe
        self.link.bound_spoiled()    # the norm bound is not shown to hold for these contributions
        acc_W1, acc_W2, acc_b1, acc_b2 = self.density_head_sinks()
        buf = self.sink("xyz_table", s.xyz_table, xe.grad_buffer) if self.need["xyz_table"] else None
        u = torch.empty(n, 128, dtype=_f32, device=dev)
        call("grid_bwd_bwd_input", xe.desc, s.xyz_table, s.xn, s.dsig_dfeat, 128, v.contiguous(), n, buf, u)
        r = torch.empty(n, 128, dtype=_f32, device=dev)
        call("linear_fwd", u, 128, s.W1, 128, None, n, 128, 128, _NONE, r, 128, None)
        m = torch.empty(n, 128, dtype=_f32, device=dev)
        call("density_head_bwd2", s.a1, s.sig, r, s.W2, None if d_sig is None else d_sig.contiguous(), n, m, r, acc_W2, acc_b2,
             _workspace("density_head_bwd2", dev))
        call("linear_bwd_weight", m, 128, u, 128, n, 128, 128, acc_W1, 128, None)
        call("linear_bwd_weight", r, 128, s.feat, 128, n, 128, 128, acc_W1, 128, acc_b1)      # (r holds e1 now)
        if buf is not None:
            call("linear_bwd_input", r, 128, s.W1, 128, n, 128, 128, m, 128, 0)               # (m is free: dL/dfeat)
            call("grid_bwd_param", xe.desc, s.xn, m, 128, n, buf)
            xe.grad_ready()


class _FieldFn(Function):
    """The whole NGP field (networks.py:198-240) as one autograd node: explicit kernel launches on
    preallocated buffers, no concat (both encoders write straight into rgb_net's input matrix),
    analytic d(sigma)/dx, and a backward that runs only the branches whose outputs received a
    gradient (normal / semantic heads are skipped when the loss does not use them).  forward and backward hold the
    schedule; the stages they order are _FieldCall's methods.

    inputs : _FIELD_INPUTS: x (N,3) world, d (N,3), embed_a (N,E) or None, then the 9 parameter tensors
    outputs: sigma (N), rgb (N,3) [after rgb_net's output activation], dsigma/dxn (N,3) w.r.t. the
             normalised position (no grad; divide by xyz_max-xyz_min for world units),
             normal head (N,3) raw, semantic logits (N,C)
    """

    @staticmethod
    def forward(ctx, model, x, d, embed_a, xyz_table, W1, b1, W2, b2, rgb_table, rgb_p, nrm_p, sem_p, ray_codes=None,
                second_order=False):
        # second_order: d(sigma)/dxn is a differentiable output (NGP.second_order_normals): a gradient on it reaches the
        # density table and xyz_net through ngp_grid_bwd_bwd_input and ngp_density_head_bwd2 in backward
        # ray_codes = (img_idxs (n_rays) i64, rays_a (n_rays, 3) i64) of appearance.RayCodes: embed_a is then the
        # (n_imgs, E) embedding TABLE, broadcast per sample by ngp_embed_a_fwd and summed back by ngp_embed_a_bwd
        #
        # Schedule.  The colour branch needs the positions and the colour table, nothing of the density path: it runs on a
        # stream of its own from the moment the colour table's Adam piece is done, beside the rest of the density
        # path and the analytic normals (which are stretched beyond that piece's end on one stream).
        #   main  : xn, buffers -> (fork) -> wait MLP piece -> density path ------------------------------------> join
        #   colour:                 SH -> wait colour piece -> colour gather -> wait MLP piece -> codes -> rgb_net -> join
        #   heads :                                                     (C <= 8, forked behind the codes)  two heads -^
        # ev_p, ev_c: the two pieces of the trainer's Adam sweep (or of the sharded optimizer's all-gather): every stream
        # waits for a piece where it first reads that piece's parameters
        E = 0 if embed_a is None else embed_a.shape[1]
        xn = (x - model.xyz_min).div_(model._span())   # (before the waits: it reads no parameter and runs under the Adam sweep)
        ev_p, ev_c = model.link.take_param_events()
        keep_d = ctx.needs_input_grad[_FIELD_INPUTS.index("d")]
        grads, buffers = _forward_buffers(x.shape[0], model.semantic_header.n_output_dims, model.rgb_net.padded_in, x.device)
        saved = _Saved(xn, *buffers, xyz_table, W1, W2, rgb_table, rgb_p, nrm_p, sem_p, d if keep_d else None)
        c = _FieldCall(model, saved, E, _stream("colour", x.device), b1, b2)
        c.fork(c.colour_forward, d, embed_a, ray_codes, second_order, ev_p, ev_c)
        if ev_p is not None:
            ev_p.wait()
        c.density_forward(grads)
        c.join()

        ctx.model, ctx.E = model, E
        ctx.ray_codes = ray_codes
        ctx.codes_shape = None if ray_codes is None else tuple(embed_a.shape)
        ctx.save_for_backward(*saved)
        if not second_order:
            ctx.mark_non_differentiable(grads)
        ctx.set_materialize_grads(False)
        return saved.sig[:, 0], saved.rgb_o, grads, saved.np_o, saved.sem_o

    @staticmethod
    def backward(ctx, d_sig, d_rgb, v, d_np, d_sem):
        # v = dL/d(d sigma/dxn) (n,3): only a node built with second_order=True can receive one
        #
        # Schedule.  The two table scatters are bound by memory-side atomic requests, the MLP products by the
        # matrix pipe: the scatters go to a side stream, one behind the other, and the products run beside them.
        #   side: [density scatter] -> [colour scatter (+ its share of the gradient norm / its reduce-scatter)]
        #   main: colour data gradients -> (fork) -> codes, dL/dx -> colour weight gradients -> density head -> join
        # The density scatter can start at once: its input is d_sigma[s] * d(sigma)/d(features)[s], and the second
        # factor was computed (and kept) by the forward pass for the analytic normals.  It runs when that product is the
        # table's whole share: not with dL/dx asked for (the density head then forms its data gradient anyway and scatters
        # it) and not with v (density_head_second_order scatters both orders' shares at once).
        need = dict(zip(_FIELD_INPUTS, ctx.needs_input_grad))
        saved = _Saved(*ctx.saved_tensors)
        c = _FieldCall(ctx.model, saved, ctx.E, _stream("scatter", saved.xn.device, ctx.model.link.side_stream), need=need)
        ev = c.link.take_acc_zeroed()   # the trainer clears its norm accumulators behind the Adam launches
        if ev is not None:
            ev.wait()
        if v is not None and need["x"]:
            raise RuntimeError("second-order normals with sample positions that require a gradient (pose refinement): the "
                               "field's second order has no dL/dx")
        reuse = d_sig is not None and not need["x"]
        scaled = reuse and need["xyz_table"] and v is None
        if scaled:
            scatter_args = d_sig.contiguous(), c.sink("xyz_table", saved.xyz_table, c.xe.grad_buffer)
        # Does the density scatter lead or follow on the side stream?
        # Data parallel: the colour table's gradient (77 % of the bytes) goes into its reduce-scatter the moment
        # its scatter is enqueued, so there the colour scatter leads on the side stream and the density scatter
        # follows it — the collective then runs under the density scatter and the weight products.
        # One GPU: the density scatter leads on the side stream and is let loose at once.  It becomes ready together
        # with the colour branch's data gradient, and whichever reaches the CUs first keeps them (the product takes
        # 0.15 ms when its 256 large workgroups are placed first, 0.4-0.6 ms behind the scatter's thousands of
        # small ones).  Holding the scatter back behind the product makes that deterministic and is the slower
        # schedule: +0.04 ms/step (3 alternations of 100 steps), the scatters are the longer path and every
        # microsecond they start later is lost.
        follows = scaled and c.re.grad_ready_is_collective and d_rgb is not None and need["rgb_table"]
        if scaled and not follows:
            c.fork(c.density_scatter, *scatter_args)
        stages = ([c.rgb_net_data_grad(d_rgb)] if d_rgb is not None else []) + c.head_data_grads(d_np, d_sem)
        if c.dfeat_rgb is not None and need["rgb_table"]:
            buf = c.sink("rgb_table", saved.rgb_table, c.re.grad_buffer)
            if d_sig is not None:
                c.fork(c.colour_scatter, buf)
            else:
                c.colour_scatter(buf)
        if follows:
            c.fork(c.density_scatter, *scatter_args)
        if c.dfeat_rgb is not None:
            c.code_and_position_grads(ctx.ray_codes, ctx.codes_shape)
        c.colour_weight_products(stages)
        if v is not None:
            c.density_head_second_order(d_sig, v)
        elif d_sig is not None:
            c.density_head(d_sig, reuse)
        # the norm-bound sums feed the optimizer's clip decision only: behind the weight products, where they fill the
        # wait for the scatters instead of sitting between the data gradient and the weight gradient (67 us there)
        if d_rgb is not None:
            c.link.bound_note(stages[0], 0, 3, c.n)
        if "x" in c.grads:
            c.grads["x"] = c.grads["x"] / c.model._span()
        c.join()
        return tuple(c.grads.get(k) for k in _FIELD_INPUTS)


_WORKSPACES = {}


def _workspace(entry, dev):
    """scratch of a backward entry point that sums in two passes (the workgroups' partial sums, as doubles), sized for any
    n by the host call `entry`_workspace.  One per entry, device AND stream: two backwards on one stream run one behind
    the other (a step's render and its unit-exposure term do), backwards on two streams may overlap and must not share
    their partial sums.  entry: density_head_bwd2 (at most 1024 x 129 doubles), tonemap_bwd (512 x 576), skybox_bwd (256 x 416)"""
    key = (entry, torch.device(dev).index, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = torch.empty(call_host(entry + "_workspace", 1 << 40), dtype=_f32, device=dev)
    return _WORKSPACES[key]


class _ToneMapFn(Function):
    """rgb (n,3) = the three tone-mappers of log_radiance (n,3) + ln(exposure), one launch each way (ngp_tonemap_fwd /
    ngp_tonemap_bwd).  exposure: None, one value (every sample's) or (n) values; it takes no gradient.  Parameter
    gradients: into the owner's `link.grad_sinks` (tone_0..2: a trainer's flat gradient views, autograd gets None, as
    _FieldFn does) or, without sinks, handed to autograd."""

    @staticmethod
    def forward(ctx, log_radiance, exposure, p0, p1, p2, owner):
        n = log_radiance.shape[0]
        rgb = torch.empty(n, 3, dtype=_f32, device=log_radiance.device)
        stride = 0 if exposure is None or exposure.numel() == 1 else 1
        call("tonemap_fwd", p0, p1, p2, log_radiance, exposure, stride, n, rgb)
        ctx.save_for_backward(log_radiance, exposure, p0, p1, p2)
        ctx.owner, ctx.stride = owner, stride
        return rgb

    @staticmethod
    def backward(ctx, g):
        log_radiance, exposure, p0, p1, p2 = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[0], any(ctx.needs_input_grad[2:5])
        if not (need_x or need_p):
            return (None,) * 6
        sinks = ctx.owner.link.grad_sinks
        to_sinks = need_p and "tone_0" in sinks
        if to_sinks:
            out = [sinks[f"tone_{i}"] for i in range(3)]
        else:
            out = [torch.zeros_like(p) for p in (p0, p1, p2)]
        dx = torch.empty_like(log_radiance) if need_x else None
        call("tonemap_bwd", p0, p1, p2, log_radiance, exposure, ctx.stride, g.contiguous(), log_radiance.shape[0], dx,
             *out, _workspace("tonemap_bwd", g.device))
        if to_sinks or not need_p:
            return (dx,) + (None,) * 5
        return (dx, None) + tuple(t if need else None for t, need in zip(out, ctx.needs_input_grad[2:5])) + (None,)


class _SkyFn(Function):
    """rgb_bg (n,3) = the skybox's colour of rays_d (n,3), one launch each way (ngp_skybox_fwd / ngp_skybox_bwd); rays_d
    takes no gradient.  Parameter gradient: into the owner's `link.grad_sinks['sky']` (a trainer's flat gradient view,
    autograd gets None, as _ToneMapFn does) or, without a sink, handed to autograd."""

    @staticmethod
    def forward(ctx, rays_d, params, owner):
        n = rays_d.shape[0]
        rgb_bg = torch.empty(n, 3, dtype=_f32, device=rays_d.device)
        call("skybox_fwd", params, rays_d, n, rgb_bg)
        ctx.save_for_backward(rays_d, params)
        ctx.owner = owner
        return rgb_bg

    @staticmethod
    def backward(ctx, g):
        rays_d, params = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None
        sink = ctx.owner.link.grad_sinks.get("sky")
        out = sink if sink is not None else torch.zeros_like(params)
        call("skybox_bwd", params, rays_d, g.contiguous(), rays_d.shape[0], out, _workspace("skybox_bwd", g.device))
        return None, (None if sink is not None else out), None


class NGP(nn.Module):
    def __init__(self, scale, rgb_act='Sigmoid', use_skybox=False, embed_a=False, embed_a_len=12, classes=7):
        super().__init__()
        self.rgb_act = rgb_act
        self.scale = scale
        self.use_skybox = use_skybox
        self.embed_a = embed_a
        self.link = FieldLink()               # what a trainer and the field's autograd node agree on (link.py)
        self.grid_rng = None                  # set from outside: a shared-seed generator keeps DDP ranks' grids identical
        self.differentiable_normals = False   # True: forward() takes the reference's own formulation (module docstring)
        # True: with grad enabled the fused field node hands out d(sigma)/dx WITH a graph (second order on ngp_grid_bwd_bwd_input
        # and ngp_density_head_bwd2), so normals_raw reaches the density table and xyz_net; NGPTrainer(normal_ref=True) sets it
        self.second_order_normals = False
        self.register_buffer('center', torch.zeros(1, 3))
        self.register_buffer('xyz_min', -torch.ones(1, 3) * scale)
        self.register_buffer('xyz_max', torch.ones(1, 3) * scale)
        self.register_buffer('half_size', (self.xyz_max - self.xyz_min) / 2)

        # cascade k of the occupancy grid covers [-2^(k-1), 2^(k-1)]^3
        self.cascades = max(1 + int(np.ceil(np.log2(2 * scale))), 1)
        self.grid_size = 128
        self.register_buffer('density_bitfield',
                             torch.zeros(self.cascades * self.grid_size ** 3 // 8, dtype=torch.uint8))

        L, Fdim, log2_T, N_min = 16, 8, 19, 16
        b = np.exp(np.log(2048 * scale / N_min) / (L - 1))
        self.xyz_encoder = tcnn.Encoding(3, {
            "otype": "Grid", "type": "Hash", "n_levels": L, "n_features_per_level": Fdim,
            "log2_hashmap_size": log2_T, "base_resolution": N_min, "per_level_scale": b,
            "interpolation": "Linear"})
        self.xyz_net = nn.Sequential(
            nn.Linear(self.xyz_encoder.n_output_dims, 128),
            nn.Softplus(),
            nn.Linear(128, 1))
        self.sigma_act = nn.Softplus()

        L_, F_, log2_T_, N_min_ = 16, 8, 21, 16
        b_ = np.exp(np.log(2048 * scale / N_min_) / (L_ - 1))
        self.rgb_encoder = tcnn.Encoding(3, {
            "otype": "HashGrid", "n_levels": L_, "n_features_per_level": F_,
            "log2_hashmap_size": log2_T_, "base_resolution": N_min_, "per_level_scale": b_,
            "interpolation": "Linear"}, seed=1338)
        self.dir_encoder = tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 4})

        rgb_input_dim = self.rgb_encoder.n_output_dims + self.dir_encoder.n_output_dims
        self.rgb_net = tcnn.Network(
            n_input_dims=rgb_input_dim + embed_a_len if embed_a else rgb_input_dim, n_output_dims=3,
            network_config={"otype": "CutlassMLP", "activation": "ReLU", "output_activation": rgb_act,
                            "n_neurons": 128, "n_hidden_layers": 1}, seed=1339)
        self.norm_pred_header = tcnn.Network(
            n_input_dims=self.rgb_encoder.n_output_dims, n_output_dims=3,
            network_config={"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None",
                            "n_neurons": 32, "n_hidden_layers": 1}, seed=1340)
        self.semantic_header = tcnn.Network(
            n_input_dims=self.rgb_encoder.n_output_dims, n_output_dims=classes,
            network_config={"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None",
                            "n_neurons": 32, "n_hidden_layers": 1}, seed=1341)
        self.semantic_act = nn.Softmax(dim=-1)

        if use_skybox:
            self.skybox_dir_encoder = tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 3})
            self.skybox_rgb_net = tcnn.Network(
                n_input_dims=9, n_output_dims=3,
                network_config={"otype": "CutlassMLP", "activation": "ReLU", "output_activation": rgb_act,
                                "n_neurons": 32, "n_hidden_layers": 1}, seed=1342)

        if self.rgb_act == 'None':  # rgb_net outputs log-radiance: one tonemapper per channel
            for i in range(3):
                setattr(self, f'tonemapper_net_{i}', tcnn.Network(
                    n_input_dims=1, n_output_dims=1,
                    network_config={"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "Sigmoid",
                                    "n_neurons": 64, "n_hidden_layers": 1}, seed=1343 + i))

    def add_occupancy_grid(self):
        """registers the two buffers a trainer adds to the model (the reference's train.py:128-132): density_grid
        (cascades, G^3) float32 zeros and grid_coords (G^3, 3) int32, on the device the model is on.  -> self"""
        G, dev = self.grid_size, self.density_bitfield.device
        self.register_buffer("density_grid", torch.zeros(self.cascades, G ** 3, device=dev))
        coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=dev)] * 3, indexing="ij"), -1)
        self.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
        return self

    # ------------------------------------------------------------------ density / normals
    def _density_head(self, feat):
        """feat (N,128) -> sigma (N) through autograd-visible layers (used when a caller wants
        gradients of density() alone)."""
        lin1, lin2 = self.xyz_net[0], self.xyz_net[2]
        a1, _ = _LinearAct.apply(feat, lin1.weight, lin1.bias, _SOFTPLUS)
        s, _ = _LinearAct.apply(a1, lin2.weight, lin2.bias, _SOFTPLUS)
        return s[:, 0]

    def density(self, x, return_feat=False, grad=True, grad_feat=True):
        """x (N,3) in [-scale, scale] -> sigmas (N) [, feat_rgb (N,128)]"""
        x = ((x - self.xyz_min) / (self.xyz_max - self.xyz_min)).contiguous()
        self.link.wait_params(rgb_table=return_feat)
        if not (grad and torch.is_grad_enabled()):
            # inference (update_density_grid runs this on 1-2 M points): three launches, no graph
            with torch.no_grad():
                n = x.shape[0]
                lin1, lin2 = self.xyz_net[0], self.xyz_net[2]
                feat = torch.empty(n, 128, dtype=_f32, device=x.device)
                call("grid_fwd", self.xyz_encoder.desc, self.xyz_encoder.params, x, n, feat, 128)
                a1 = torch.empty(n, 128, dtype=_f32, device=x.device)
                sig = torch.empty(n, 1, dtype=_f32, device=x.device)
                _density_mlp(lin1.weight, lin1.bias, lin2.weight, lin2.bias).forward(feat, 128, n, a1, sig)
                sigmas = sig[:, 0]
        else:
            sigmas = self._density_head(self.xyz_encoder(x))
        if return_feat:
            with torch.set_grad_enabled(grad_feat and torch.is_grad_enabled()):
                feat_rgb = self.rgb_encoder(x)
            return sigmas, feat_rgb
        return sigmas

    def _field(self, x, d, kwargs):
        """-> sigmas, rgbs (after rgb_net's own output activation), dsigma/dx, raw normal head, semantic logits"""
        embed_a = ray_codes = None
        if self.embed_a:
            embed_a = kwargs['embedding_a']
            if isinstance(embed_a, RayCodes):
                # the table itself enters the node (its gradient is the per-image sum); the rays' images and segments
                # travel beside it
                if embed_a.rays_a is None:
                    raise ValueError("RayCodes is not bound to a ray batch: pass it to render(), which binds rays_a")
                if embed_a.weight.shape[1] != self.rgb_net.n_input_dims - 144:
                    raise ValueError(f"codes of length {embed_a.weight.shape[1]} for a model built with embed_a_len="
                                     f"{self.rgb_net.n_input_dims - 144}")
                ray_codes = (embed_a.img_idxs, embed_a.rays_a.contiguous())
                if getattr(embed_a.rays_a, "_ngp_full_cover", False):
                    ray_codes[1]._ngp_full_cover = True
                embed_a = embed_a.weight if embed_a.weight.is_contiguous() else embed_a.weight.contiguous()
            else:
                if embed_a.size(0) < x.size(0):
                    embed_a = torch.repeat_interleave(embed_a, int(x.size(0) / embed_a.size(0)), 0)
                embed_a = embed_a.contiguous()
        lin1, lin2 = self.xyz_net[0], self.xyz_net[2]
        second = bool(self.second_order_normals and torch.is_grad_enabled())
        if second:
            if not (x.is_cuda and _density_fused_ok(self.xyz_encoder, lin1.weight, lin1.bias, lin2.weight, lin2.bias)
                    and lin1.bias is not None and lin2.bias is not None):
                raise RuntimeError("second_order_normals needs the density path ngp_density_field_fwd takes (a 16-level F = 8 "
                                   "table and the 128 -> 128 -> 1 head with biases, contiguous, on the GPU): "
                                   "differentiable_normals = True is the route for any other field")
            if x.requires_grad:
                raise RuntimeError("second_order_normals with sample positions that require a gradient (pose refinement): "
                                   "the field's second order has no dL/dx")
        if not x.is_cuda:   # (every launch of the node takes device pointers)
            raise RuntimeError("x must be a CUDA tensor")
        return _FieldFn.apply(self, x.contiguous(), d.contiguous(), embed_a,
                              self.xyz_encoder.params, lin1.weight, lin1.bias, lin2.weight, lin2.bias,
                              self.rgb_encoder.params, self.rgb_net.params, self.norm_pred_header.params,
                              self.semantic_header.params, ray_codes, second)

    def grad(self, x):
        """-> sigmas (N), feat_rgb (N,128), d(sigma)/dx (N,3) (detached, see module docstring).
        Kept for API parity (networks.py:186-196); forward()/forward_test() use the fused node."""
        sigmas, _, grads, _, _ = self._field(x, torch.zeros_like(x), {'embedding_a': torch.zeros(
            x.shape[0], self.rgb_net.n_input_dims - 144, device=x.device)} if self.embed_a else {})
        span = self.xyz_max - self.xyz_min
        feat_rgb = self.rgb_encoder(((x - self.xyz_min) / span).contiguous())
        return sigmas, feat_rgb, grads / span

    # ------------------------------------------------------------------ full field
    def _span(self):
        sp = getattr(self, '_span_t', None)
        if sp is None or sp.device != self.xyz_min.device:
            sp = self._span_t = self.xyz_max - self.xyz_min
        return sp

    def _inv_span(self):
        inv = getattr(self, '_inv_span_t', None)
        if inv is None or inv.device != self.xyz_min.device:
            inv = self._inv_span_t = (1.0 / (self.xyz_max - self.xyz_min)).reshape(3).contiguous()
        return inv

    def _tone(self, rgbs, kwargs):
        if self.rgb_act == 'None':  # rgb_net outputs log-radiance
            if kwargs.get('output_radiance', False):
                rgbs = TruncExp.apply(rgbs)
            else:
                rgbs = self.log_radiance_to_rgb(rgbs, **kwargs)
        return rgbs

    def _forward_differentiable_normals(self, x, d, kwargs):
        """The reference's own formulation (networks.py:186-240): d(sigma)/dx by
        torch.autograd.grad(create_graph=True), so that normals_raw carries gradients back into the
        density table and MLP (H4, needed by --normal_ref).  The grid's double backward runs on
        ngp_grid_bwd_bwd_input; the 17 k-parameter density MLP uses torch ops here."""
        self.link.wait_params()
        x = x.detach().clone().requires_grad_(True)
        xn = (x - self.xyz_min) / (self.xyz_max - self.xyz_min)
        with torch.enable_grad():
            h = self.xyz_net(self.xyz_encoder(xn))
            sigmas = self.sigma_act(h[:, 0])
            # this walk wants d(sigma)/dx only: without the flag the encoder's backward would also scatter d(sum sigma)/dtable,
            # into a table-sized scratch array or, under a trainer, into the flat gradient itself
            self.xyz_encoder.input_grad_only = True
            try:
                grads = torch.autograd.grad(sigmas, x, torch.ones_like(sigmas), create_graph=True)[0]
            finally:
                self.xyz_encoder.input_grad_only = False
        feat_rgb = self.rgb_encoder(xn.detach())
        dn = F.normalize(d, p=2, dim=-1, eps=1e-6)
        cols = [self.dir_encoder((dn + 1) / 2), feat_rgb]
        if self.embed_a:
            embed_a = kwargs['embedding_a']
            if isinstance(embed_a, RayCodes):
                embed_a = embed_a.expand()
            if embed_a.size(0) < feat_rgb.size(0):
                embed_a = torch.repeat_interleave(embed_a, int(feat_rgb.size(0) / embed_a.size(0)), 0)
            cols.append(embed_a)
        rgbs = self.rgb_net(torch.cat(cols, 1))
        return sigmas, rgbs, grads, self.norm_pred_header(feat_rgb), self.semantic_header(feat_rgb)

    def forward(self, x, d, **kwargs):
        """x, d (N,3) -> sigmas (N), rgbs (N,3), normals_raw (N,3), normals_pred (N,3), semantic (N,C)"""
        if self.differentiable_normals and torch.is_grad_enabled():
            sigmas, rgbs, grads, np_raw, sem_logits = self._forward_differentiable_normals(x, d, kwargs)
            normals_raw = -F.normalize(grads, p=2, dim=-1, eps=1e-6)
        else:
            sigmas, rgbs, grads, np_raw, sem_logits = self._field(x, d, kwargs)
            normals_raw = _NegNormalize.apply(grads, self._inv_span())
        normals_pred = _NegNormalize.apply(np_raw, None)
        semantic = self.semantic_act(sem_logits)
        return sigmas, self._tone(rgbs, kwargs), normals_raw, normals_pred, semantic

    def forward_test(self, x, d, **kwargs):
        """same as forward but returns (sigmas, rgbs, normals_pred, normals_raw, semantic) — the
        reference's test path swaps the two normals (networks.py:282) and detaches the heads."""
        sigmas, rgbs, grads, np_raw, sem_logits = self._field(x, d, kwargs)
        normals_raw = _NegNormalize.apply(grads, self._inv_span())
        normals_pred = _NegNormalize.apply(np_raw.detach(), None)
        semantic = self.semantic_act(sem_logits.detach())
        return sigmas, self._tone(rgbs, kwargs), normals_pred, normals_raw, semantic

    def forward_skybox(self, d):
        if not self.use_skybox:
            return None
        d = d / torch.norm(d, dim=1, keepdim=True)
        d = self.skybox_dir_encoder((d + 1) / 2)
        return self.skybox_rgb_net(d)

    def skybox_rgb(self, rays_d):
        """forward_skybox(rays_d) as one launch each way (_SkyFn: ngp_skybox_fwd / ngp_skybox_bwd), what the fused training
        tail composites over; rays_d takes no gradient.  forward_skybox stays the module-by-module route (the test-time
        renderer's, and render(use_skybox=True)'s without a fused tail)."""
        if not self._stock_skybox():
            raise RuntimeError("skybox_rgb needs the skybox as the constructor builds it with rgb_act='Sigmoid' (SH degree 3 "
                               "-> 32 -> 3, Sigmoid): the sky kernels are written for nothing else")
        if not rays_d.is_cuda:
            raise RuntimeError("rays_d must be a CUDA tensor")
        # the sky parameters sit in the Adam sweep's first piece, as every MLP's do
        self.link.join_params(rgb_table=False)
        return _SkyFn.apply(rays_d.detach().to(_f32).contiguous(), self.skybox_rgb_net.params, self)

    def _stock_skybox(self):
        """the skybox as the constructor builds it for sigmoid colours (what ngp_skybox_fwd / _bwd are written for)"""
        enc, net = getattr(self, 'skybox_dir_encoder', None), getattr(self, 'skybox_rgb_net', None)
        return bool(self.use_skybox and isinstance(enc, tcnn.Encoding) and enc.otype == "SphericalHarmonics" and enc.n_output_dims == 9
                    and isinstance(net, tcnn.Network) and net.layer_shapes == [(32, 16), (16, 32)] and net.n_input_dims == 9
                    and net.n_output_dims == 3 and net.activation == _RELU and net.output_activation == 2
                    and net.params.is_contiguous())

    def log_radiance_to_rgb(self, log_radiances, **kwargs):
        """HDR -> LDR with the per-channel tonemappers (models/networks_noCUDA.py:238-251; the
        reference's CUDA model calls this without defining it, networks.py:238).  With the constructor's tone-mappers
        the three channels run as one launch each way (_ToneMapFn); `exposure` is absent, one value ((1,1) or 0-dim:
        every sample's) or (n,1): one per sample, and takes no gradient."""
        nets = self._stock_tonemappers()
        if nets is None:   # tone-mappers put there from outside: composed module by module
            out = []
            for i in range(3):
                inp = log_radiances[:, i:i + 1]
                if 'exposure' in kwargs:
                    inp = inp + torch.log(kwargs['exposure'])
                out.append(getattr(self, f'tonemapper_net_{i}')(inp))
            return torch.cat(out, 1)
        if not log_radiances.is_cuda:
            raise RuntimeError("log_radiances must be a CUDA tensor")
        n = log_radiances.shape[0]
        exposure = kwargs.get('exposure')
        if exposure is not None:
            if not exposure.is_cuda:
                raise RuntimeError("exposure must be a CUDA tensor")
            if exposure.requires_grad:
                raise ValueError("exposure takes no gradient: the tone-mapper kernels have none for it")
            if exposure.numel() not in (1, n):
                raise ValueError(f"exposure holds one value or one per sample ({n}), got {tuple(exposure.shape)}")
            exposure = exposure.detach().to(_f32).reshape(-1).contiguous()
        return _ToneMapFn.apply(log_radiances.to(_f32).contiguous(), exposure, *[t.params for t in nets], self)

    def _stock_tonemappers(self):
        """the three networks as the constructor builds them (what ngp_tonemap_fwd / _bwd are written for), or None"""
        nets = [getattr(self, f'tonemapper_net_{i}', None) for i in range(3)]
        for t in nets:
            if not (isinstance(t, tcnn.Network) and t.layer_shapes == [(64, 16), (16, 64)] and t.n_input_dims == 1
                    and t.n_output_dims == 1 and t.activation == _RELU and t.output_activation == 2
                    and t.params.is_contiguous()):
                return None
        return nets

    # ------------------------------------------------------------------ occupancy grid
    @torch.no_grad()
    def get_all_cells(self):
        indices = vren.morton3D(self.grid_coords).long()
        return [(indices, self.grid_coords)] * self.cascades

    @torch.no_grad()
    def sample_uniform_and_occupied_cells(self, M, density_threshold):
        cells = []
        for c in range(self.cascades):
            gen = self.grid_rng  # shared-seed generator keeps DDP ranks' grids identical
            coords1 = torch.randint(self.grid_size, (M, 3), dtype=torch.int32, device=self.density_grid.device,
                                    generator=gen)
            indices1 = vren.morton3D(coords1).long()
            # M random occupied cells without a host round trip (the reference's nonzero() +
            # randint(len) syncs): rank r ~ U[0, n_occ) is mapped to the r-th occupied cell through
            # the running count of the occupancy mask.  With no occupied cell at all the reference
            # samples none; here those M draws fall back onto the uniform cells (same coverage).
            occ = self.density_grid[c] > density_threshold
            csum = torch.cumsum(occ, 0, dtype=torch.int32)
            n_occ = csum[-1]
            u = torch.rand(M, device=occ.device, generator=gen)
            rank = torch.clamp((u * n_occ).to(torch.int32), max=n_occ - 1) + 1
            pos = torch.searchsorted(csum, rank.clamp(min=1), right=False)
            indices2 = torch.where(n_occ > 0, pos.clamp(max=occ.numel() - 1), indices1)
            coords2 = vren.morton3D_invert(indices2.int())
            indices, coords = torch.cat([indices1, indices2]), torch.cat([coords1, coords2])
            # Morton order: neighbouring points share hash-grid cells at the coarse levels, so the 1 M
            # point gather of density() runs out of L2 instead of HBM (which cell receives which jitter
            # draw changes, their distribution does not)
            indices, perm = torch.sort(indices)
            coords = coords[perm]
            cells += [(indices, coords)]
        return cells

    @torch.no_grad()
    def mark_invisible_cells(self, K, poses, img_wh, chunk=64 ** 3):
        """Cells that no camera sees, or that lie in front of a camera but closer than NEAR_DISTANCE,
        get density -1 and are never updated again; `count_grid` keeps the fraction of cameras that
        see each cell (networks.py:336-377).  Run once before training.
        K (3,3) intrinsics, poses (N,3,4) camera-to-world, img_wh (w, h)."""
        n_cams = poses.shape[0]
        w, h = img_wh
        rot_t = poses[:, :3, :3].transpose(1, 2)                       # world -> camera rotations
        # one 3x4 projection per camera: pixel-homogeneous coordinates = proj @ [x_world; 1]
        proj = K @ torch.cat([rot_t, -rot_t @ poses[:, :3, 3:]], 2)
        self.count_grid = torch.zeros_like(self.density_grid)
        for c, (indices, coords) in enumerate(self.get_all_cells()):
            s = min(2 ** (c - 1), self.scale)
            centres = (coords.to(_f32) / (self.grid_size - 1) * 2 - 1) * (s - s / self.grid_size)
            for lo in range(0, len(indices), chunk):
                sel = indices[lo:lo + chunk]
                uvd = torch.einsum('nij,mj->nim', proj[:, :, :3], centres[lo:lo + chunk]) + proj[:, :, 3:]
                depth = uvd[:, 2]
                u, v = uvd[:, 0] / depth, uvd[:, 1] / depth
                inside = (depth >= 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
                seen = (inside & (depth >= NEAR_DISTANCE)).sum(0) / n_cams
                too_close = (inside & (depth < NEAR_DISTANCE)).any(0)
                self.count_grid[c, sel] = seen
                self.density_grid[c, sel] = torch.where((seen > 0) & ~too_close, 0.0, -1.0)

    @torch.no_grad()
    def _update_density_grid_sampled(self, density_threshold, decay):
        """The sampled branch of update_density_grid on the fused kernels (ngp_grid_sample_cells ->
        density() -> ngp_density_grid_scatter_max -> ngp_density_grid_ema_threshold -> ngp_packbits): per
        cascade M = G^3/4 uniform cells + M occupied ones, jittered, evaluated, max-combined into the grid; EMA,
        mean threshold and bit packing.  The draws are a counter-based hash of (seed, update number, cascade):
        identical on every data-parallel rank (the seed comes from `grid_rng` when the trainer set one)."""
        G = self.grid_size
        M = G ** 3 // 4
        dev = self.density_grid.device
        ws = getattr(self, '_grid_ws', None)
        if ws is None or ws[0].device != dev:
            n_ws = call_host("grid_sample_workspace", G, M)
            ws = self._grid_ws = (torch.empty(n_ws, dtype=torch.int32, device=dev),
                                  torch.empty(2 * M, dtype=torch.int32, device=dev),
                                  torch.empty(2 * M, 3, dtype=_f32, device=dev),
                                  torch.empty(1024, dtype=_f32, device=dev), torch.empty(2, dtype=_f32, device=dev))
            gen = self.grid_rng
            self._grid_seed = int(gen.initial_seed() if gen is not None else torch.initial_seed()) & 0x7FFFFFFFFFFF
            self._grid_updates = 0
        work, indices, xyzs_w, partials, thr = ws
        density_grid_tmp = torch.zeros_like(self.density_grid)
        for c in range(self.cascades):
            s = min(2 ** (c - 1), self.scale)
            seed = self._grid_seed + 1000003 * self._grid_updates + 7919 * c
            call("grid_sample_cells", self.density_grid[c], G, float(density_threshold), M, seed, float(s), work, indices,
                 xyzs_w)
            sig = self.density(xyzs_w)
            call("density_grid_scatter_max", density_grid_tmp[c], indices, sig.contiguous(), 2 * M)
        self._grid_updates += 1
        call("density_grid_ema_threshold", self.density_grid, density_grid_tmp, self.density_grid.numel(), float(decay),
             float(density_threshold), partials, thr)
        call("packbits", self.density_grid.view(-1), self.density_bitfield.shape[0], 0.0, thr, self.density_bitfield)

    @torch.no_grad()
    def update_density_grid(self, density_threshold, warmup=False, decay=0.95, erode=False):
        if not warmup and not erode and self.density_grid.is_cuda:
            return self._update_density_grid_sampled(density_threshold, decay)
        density_grid_tmp = torch.zeros_like(self.density_grid)
        if warmup:
            cells = self.get_all_cells()
        else:
            cells = self.sample_uniform_and_occupied_cells(self.grid_size ** 3 // 4, density_threshold)
        for c in range(self.cascades):
            indices, coords = cells[c]
            s = min(2 ** (c - 1), self.scale)
            noise = torch.rand(coords.shape[0], 3, dtype=_f32, device=coords.device,
                               generator=self.grid_rng)
            xyzs_w = torch.empty(coords.shape[0], 3, dtype=_f32, device=coords.device)
            call("grid_cell_points", coords.contiguous(), noise, coords.shape[0], self.grid_size, float(s), xyzs_w)
            density_grid_tmp[c, indices] = self.density(xyzs_w)
        if erode:
            if not hasattr(self, 'count_grid'):
                raise RuntimeError("erode=True needs mark_invisible_cells() to have been called "
                                   "(the reference crashes here too: networks.py:399)")
            decay_t = torch.clamp(decay ** (1 / self.count_grid), 0.1, 0.95)
            self.density_grid = torch.where(self.density_grid < 0, self.density_grid,
                                            torch.maximum(self.density_grid * decay_t, density_grid_tmp))
        else:
            call("density_grid_ema", self.density_grid, density_grid_tmp, self.density_grid.numel(), float(decay))
        # threshold = min(mean of the positive cells, density_threshold), kept on the device
        pos = self.density_grid > 0
        mean_density = (self.density_grid * pos).sum() / pos.sum().clamp(min=1)
        thr = torch.clamp(mean_density, max=density_threshold).reshape(1)
        call("packbits", self.density_grid.view(-1), self.density_bitfield.shape[0], 0.0, thr, self.density_bitfield)

    def uniform_sample(self, resolution=128):
        half_grid_size = self.scale / resolution
        lin = torch.linspace(0, 1 - half_grid_size, resolution, device=self.xyz_min.device)
        samples = torch.stack(torch.meshgrid(lin, lin, lin, indexing='ij'), -1)
        dense_xyz = self.xyz_min * (1 - samples) + self.xyz_max * samples
        dense_xyz += half_grid_size * torch.rand_like(dense_xyz)
        return self.density(dense_xyz.view(-1, 3))
