"""FLowHigh vector-field network, ConvNeXt backbone (`FLowHigh(architecture='convnext')`), on the HIP kernels.

Mirrors models/flow.py:124-139,185-261 of the reference (paths under its src/flowhigh/) (`FLowHigh.forward` at inference with
architecture = 'convnext') and models/convnext.py:9-93 (`ConvNeXtBlock`, `AdaLayerNorm`).  Everything in front of the blocks is
the transformer path's (flow.py:232-242) and runs on the same kernels as `flow.FlowNet`; behind them come a plain
LayerNorm(eps = 1e-6) and `to_pred`.

The backbone is local by construction: 15 frames a side from ConvPositionEmbed + 8 blocks x 3 = 39 frames a side, O(N), no
attention.  One block, rows token-major [B*n, dim]:

    u = dwconv7(x)                                        zero padded at the clip's ends
    y = LayerNorm(u, eps 1e-6) * scale(temb) + shift(temb)         one launch: fh_dwconv_ln_f32 (csrc/convnext.hip)
    h = gelu(W1 y + b1)                                   the fp32 / bf16 x 6 GEMM + fh_gelu_f32
    x = x + gamma * (W2 h + b2)                           the GEMM's LINEAR epilogue with R = x: gamma is folded into W2, b2

One vector-field evaluation = 39 launches for the reference's 8 blocks.  Fusions beside the transformer path's:
  * all 16 scale / shift projections of an evaluation are one GEMV over the stacked [2 * blocks * dim, hidden] rows;
  * `gamma` (layer scale) is folded into pwconv2 at pack time: W2' = diag(gamma) W2, b2' = gamma * b2, formed in float64 and
    rounded once (`fold_gamma`); a checkpoint without gamma keys (layer_scale_init_value <= 0) skips the fold.

`ConvNextNet` has `FlowNet`'s interface, so the ODE steppers, classifier-free guidance, generate_many (both `ends`), sample_many
and capture of flowhighsr.py run it unchanged.
"""
import re

import torch

from . import hip
from .field import FieldNet, across
from .flow import FH, _pad_rows

DWLN_ROWS = 16          # rows of one clip a block of fh_dwconv_ln_f32 owns (csrc/convnext.hip: LN_ROWS)
LN_EPS = 1e-6           # AdaLayerNorm(eps=1e-6) and final_layer_norm (convnext.py:32, flow.py:139)
_BLOCK_KEY = re.compile(r"^" + re.escape(FH) + r"convnext\.(\d+)\.")


def is_convnext_state_dict(sd):
    """The checkpoint holds the ConvNeXt backbone's tensors (any `flowhigh.convnext.*` key)."""
    return any(_BLOCK_KEY.match(k) for k in sd)


def n_blocks(sd):
    """Number of ConvNeXt blocks of a state dict: indices 0 .. max, read from the keys."""
    idx = [int(m.group(1)) for m in map(_BLOCK_KEY.match, sd) if m]
    return max(idx) + 1 if idx else 0


def block_keys(i, gamma=True):
    """State-dict keys of block i under `flowhigh.` (convnext.py:29-42)."""
    p = f"{FH}convnext.{i}."
    names = ["dwconv.weight", "dwconv.bias", "norm.scale.weight", "norm.scale.bias", "norm.shift.weight", "norm.shift.bias",
             "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias"] + (["gamma"] if gamma else [])
    return [p + n for n in names]


def fold_gamma64(w2, b2, gamma):
    """gamma * (W2 h + b2) = (diag(gamma) W2) h + gamma * b2: W2' and b2' in float64 (products of two float32 values: exact)."""
    g = gamma.double()
    return g[:, None] * w2.double(), g * b2.double()


def fold_gamma(w2, b2, gamma):
    """fold_gamma64 rounded to float32, once: what the block's second GEMM reads."""
    w, b = fold_gamma64(w2, b2, gamma)
    return w.float(), b.float()


class ConvNextNet(FieldNet):
    grouped_field = False          # (the time-conditioned LayerNorm takes one time: no forward(groups=))

    def __init__(self, sd, device, bf=False):
        self.device = hip.norm_device(device)
        dev = self.device
        g = lambda name: sd[FH + name].detach().float().cpu()
        up = lambda t: t.contiguous().to(dev)
        # bf: the linears in the bf16 x 6 form, as FlowNet's (conv_form = 'bf16x6' / 'direct_bf16x6' / 'direct_bf16x3')
        self.bf = bool(bf)
        if self.bf:
            from .packing import pack_gemm_bf_weight
            up_w = lambda t: up(pack_gemm_bf_weight(_pad_rows(t)))
        else:
            up_w = lambda t: up(_pad_rows(t))
        w_embed = g("to_embed.weight")
        self.dim, self.dim_in = w_embed.shape[0], w_embed.shape[1] // 2
        self.dw_k = g("conv_embed.dw_conv1d.0.weight").shape[-1]
        self.hidden = g("sinu_pos_emb.1.weight").shape[0]
        self.blocks = n_blocks(sd)
        if self.dim % 256 or self.dim > 4096 or self.dim_in % 32 or self.blocks < 1:
            raise NotImplementedError("unsupported convnext dims")
        self.w_x = up_w(w_embed[:, :self.dim_in])
        self.w_c = up_w(w_embed[:, self.dim_in:])
        self.b_embed = up(g("to_embed.bias"))
        self.null_cond = up(g("null_cond").reshape(1, -1))
        self._e_null = None
        self.dw_w = up(g("conv_embed.dw_conv1d.0.weight").reshape(self.dim, self.dw_k).t())      # [ksz, dim], tap-major
        self.dw_b = up(g("conv_embed.dw_conv1d.0.bias"))
        self.sinu_w = up(g("sinu_pos_emb.0.weights"))
        self.t_w = up(g("sinu_pos_emb.1.weight"))
        self.t_b = up(g("sinu_pos_emb.1.bias"))
        self.layers, ss_w, ss_b = [], [], []
        for i in range(self.blocks):
            p = f"convnext.{i}."
            cw = g(p + "dwconv.weight")
            w1, w2, b2 = g(p + "pwconv1.weight"), g(p + "pwconv2.weight"), g(p + "pwconv2.bias")
            if FH + p + "gamma" in sd:
                w2, b2 = fold_gamma(w2, b2, g(p + "gamma"))
            if w1.shape[0] % 32 or w2.shape != (self.dim, w1.shape[0]) or cw.shape[-1] > 7 or cw.shape[-1] % 2 == 0:
                raise NotImplementedError(f"unsupported convnext block {i}: pwconv1 {tuple(w1.shape)}, dwconv {tuple(cw.shape)}")
            self.layers.append(dict(
                cw=up(cw.reshape(self.dim, cw.shape[-1]).t()), cb=up(g(p + "dwconv.bias")), ksz=cw.shape[-1],    # [ksz, dim]
                w1=up_w(w1), b1=up(g(p + "pwconv1.bias")), w2=up_w(w2), b2=up(b2), inner=w1.shape[0]))
            for which in ("scale", "shift"):
                ss_w.append(g(p + f"norm.{which}.weight"))
                ss_b.append(g(p + f"norm.{which}.bias"))
        self.ss_w = up(torch.cat(ss_w, 0))            # [2 * blocks * dim, hidden]: block i's scale rows, then its shift rows
        self.ss_b = up(torch.cat(ss_b, 0))
        self.ln_w = up(g("final_layer_norm.weight"))
        self.ln_b = up(g("final_layer_norm.bias"))
        self.w_pred = up_w(g("to_pred.weight"))
        self.inner = self.layers[0]["inner"]
        if any(l["inner"] != self.inner for l in self.layers):      # (the GELU between the linears runs over contiguous rows)
            raise NotImplementedError("convnext blocks of different inner widths")
        self._ws = hip.ShapeCache()

    @hip.on_device
    def workspace(self, batch, n):
        key = (batch, n)
        if key in self._ws:
            return self._ws[key]
        dev, M, D = self.device, batch * n, self.dim
        f32 = dict(dtype=torch.float32, device=dev)
        ws = dict(e_cond=torch.empty(M, D, **f32), h=torch.empty(M, D, **f32), h2=torch.empty(M, D, **f32),
                  a=torch.empty(M, D, **f32), g=torch.empty(M, self.inner, **f32),
                  four=torch.empty(self.sinu_w.shape[0] * 2, **f32), temb=torch.empty(self.hidden, **f32),
                  ss=torch.empty(2 * self.blocks * D, **f32))
        self._ws[key] = ws
        return ws

    def _dwconv_ln(self, x, w, b, ksz, scale, shift, y, rows):
        across("fh_dwconv_ln", (x.data_ptr(), hip.ptr(w), hip.ptr(b), scale.data_ptr(), shift.data_ptr(), y.data_ptr()), rows,
               (self.dim, ksz, LN_EPS))

    @hip.on_device
    def forward(self, x, t, out, batch, n, alpha=1.0, res=None, null_cond=False, ragged=None):
        """out = alpha * v(x, t) + res  with v the vector field; x/out/res [B*n, dim_in]: FlowNet.forward's contract, ragged
        included (the convs stop at every clip's ends: the segment forms of the two operators that look across rows)."""
        L, st = hip.lib(), hip.stream()
        ws = ragged if ragged is not None else self.workspace(batch, n)
        M, D = (ragged["rows"] if ragged is not None else batch * n), self.dim
        rows = (batch, n) if ragged is None else (ragged["seg"].data_ptr(), len(ragged["frames"]), ragged["max_n"])
        h, h2, a, gbuf, ss = ws["h"], ws["h2"], ws["a"], ws["g"], ws["ss"]
        self._embed(x, ws, M, rows, null_cond)
        self._time_path(t, ws, self.sinu_w.shape[0], self.hidden, self.ss_w, self.ss_b, ss)
        cur, other = h2, h
        for i, lay in enumerate(self.layers):
            o = 2 * i * D
            self._dwconv_ln(cur, lay["cw"], lay["cb"], lay["ksz"], ss[o:o + D], ss[o + D:o + 2 * D], a, rows)
            inner = lay["inner"]
            self.gemm(a, lay["w1"], gbuf, M, inner, D, bias=lay["b1"])
            hip.check(L.fh_gelu_f32(gbuf.data_ptr(), gbuf.data_ptr(), M * inner, st), "fh_gelu_f32")
            self.gemm(gbuf, lay["w2"], other, M, D, inner, bias=lay["b2"], R=cur)
            cur, other = other, cur
        self._dwconv_ln(cur, None, None, 1, self.ln_w, self.ln_b, a, rows)
        return self._predict(a, out, M, alpha, res)
