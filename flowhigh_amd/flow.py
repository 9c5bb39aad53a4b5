"""FLowHigh vector-field network (transformer backbone) on the HIP kernels.

Mirrors /root/reference/src/flowhigh/models/flow.py:185-261 (`FLowHigh.forward` at inference:
cond_drop_prob = 0, no masks, architecture = 'transformer'), transformer.py:167-234,
attend.py:153-189 and pos_emb.py.  The reference's tensor-to-string INFO logging and NaN
`.any()` host syncs (flow.py:256-267) are deliberately not reproduced.

One vector-field evaluation = 21 kernel launches for depth 2 (the reference issues 1 882 aten
calls).  Fusions:
  * cat(x, cond) @ W_embed^T  ->  x @ W_x^T + (cond @ W_c^T + b), the second term computed once
    per generate() because cond does not change across ODE evaluations (flow.py:234-239);
  * bias / residual / ODE axpy ("y + dt * f") in GEMM epilogues; GEGLU in the FF1 epilogue;
  * all eight adaptive-norm gamma/beta projections of a forward in one GEMV (the time embedding
    is identical for every clip, flow.py:208-211).
"""
import ctypes

import torch

from . import hip
from .field import FieldNet, across, entry_pair
from .tables import rotary_tables

FH = "flowhigh."


def _pad_rows(w, mult=128):
    n = w.shape[0]
    n_pad = (n + mult - 1) // mult * mult
    if n_pad == n:
        return w.contiguous()
    out = torch.zeros((n_pad,) + tuple(w.shape[1:]), dtype=w.dtype)
    out[:n] = w
    return out


def pack_geglu(w, b):
    """FF1 weight [2*inner, K], bias [2*inner] -> packed blocks of 64 rows = 32 value + 32 gate
    (transformer.py:92-95: x, gate = chunk(2)).  Returns (W' [nblk*64, K], b' [nblk*64], inner_pad)."""
    two_inner, k = w.shape
    inner = two_inner // 2
    nblk = (inner + 31) // 32
    wp = torch.zeros(nblk, 2, 32, k, dtype=torch.float32)
    bp = torch.zeros(nblk, 2, 32, dtype=torch.float32)
    val, gate = w[:inner], w[inner:]
    vpad = torch.zeros(nblk * 32, k)
    gpad = torch.zeros(nblk * 32, k)
    vpad[:inner], gpad[:inner] = val, gate
    wp[:, 0], wp[:, 1] = vpad.view(nblk, 32, k), gpad.view(nblk, 32, k)
    bv = torch.zeros(nblk * 32)
    bg = torch.zeros(nblk * 32)
    bv[:inner], bg[:inner] = b[:inner], b[inner:]
    bp[:, 0], bp[:, 1] = bv.view(nblk, 32), bg.view(nblk, 32)
    return _pad_rows(wp.view(nblk * 64, k)), bp.view(-1).contiguous(), nblk * 32


class FlowNet(FieldNet):
    grouped_field = True           # forward(groups=): a time per group of rows, for clips of different step counts in one sequence

    def __init__(self, sd, device, depth=2, heads=16, dim_head=64, store=None, bf=False, attn_form="f32", attn_window=None):
        if dim_head != 64:
            raise NotImplementedError("dim_head must be 64")
        self.device = hip.norm_device(device)
        dev = self.device
        # (device tensors come through the weight store: packed from `sd`, or taken from an uploaded weight blob: weights.py)
        from .weights import WeightStore
        W = store if store is not None else WeightStore(dev)
        g = lambda name: sd[FH + name].detach().float().cpu()
        self.depth, self.heads = depth, heads
        # bf: the linears run in the bf16 x 6 form (gemm_bf.hip: six bf16 MFMAs per product over exact three-piece splits,
        # fp32-grade; the model's conv_form = 'bf16x6', 'direct_bf16x6' or 'direct_bf16x3'): their weights are stored split (6 bytes per weight)
        self.bf = bool(bf)
        # attn_form: 'f32' (attention.hip) | 'bf16x6' (attention_bf.hip: the two products of attention in the same six-MFMA form,
        # the softmax unchanged).  The entry pair is picked here, once; a missing entry is an error at the first forward.
        from .planner import resolve_attn_form
        self.attn_form = resolve_attn_form(attn_form)
        stem = "fh_attention_bf16x6" if self.attn_form == "bf16x6" else "fh_attention"
        self._attn, self._attn_seg = entry_pair(stem)
        # attn_window: None (full attention: the pair above, as always) | W >= 0: frame i attends to the frames j of its clip with
        # |i - j| <= W (frames of 10 ms: 500 = +-5 s) -- the banded pair of the same form, with W as their radius
        from .planner import resolve_attn_window
        self.attn_window = resolve_attn_window(attn_window)
        self._attn_band, self._attn_band_seg = entry_pair(stem + "_band")
        self._radius = None if self.attn_window is None else min(self.attn_window, 2 ** 31 - 1)      # (the entries take a C int)
        self._attn_stem, self._attn_tail = (stem, (10.0,)) if self._radius is None else (stem + "_band", (self._radius, 10.0))
        from .planner import use_gemm_bf16x6
        if getattr(W, "form", None) is not None and use_gemm_bf16x6(W.form) != self.bf:
            # (a blob holds the linears in ONE form: asking it for the other would fail on the first missing key)
            raise ValueError(f"the weight blob was packed for conv_form={W.form!r}: its linears are "
                             f"{'split into bf16 pieces' if use_gemm_bf16x6(W.form) else 'fp32'}, this model asks for the other form")
        if self.bf:
            from .packing import pack_gemm_bf_weight
            dev_w = lambda key, make: W.dev(key + ".bf3", lambda: pack_gemm_bf_weight(make()))
        else:
            dev_w = W.dev
        w_embed = lambda: g("to_embed.weight")
        dims = W.host("f.dims", lambda: torch.tensor([w_embed().shape[0], w_embed().shape[1] // 2,
                                                      g("conv_embed.dw_conv1d.0.weight").shape[-1]], dtype=torch.int32)).tolist()
        self.dim, self.dim_in, self.dw_k = dims
        if self.dim % 256 or self.dim_in % 32 or heads * dim_head != self.dim:
            raise NotImplementedError("unsupported transformer dims")
        self.w_x = dev_w("f.w_x", lambda: _pad_rows(w_embed()[:, :self.dim_in]))
        self.w_c = dev_w("f.w_c", lambda: _pad_rows(w_embed()[:, self.dim_in:]))
        self.b_embed = W.dev("f.b_embed", lambda: g("to_embed.bias"))
        self.null_cond = W.dev("f.null_cond", lambda: g("null_cond").reshape(1, -1))
        self._e_null = None
        self.dw_w = W.dev("f.dw_w", lambda: g("conv_embed.dw_conv1d.0.weight").reshape(self.dim, self.dw_k).t())   # [ksz, dim], tap-major
        self.dw_b = W.dev("f.dw_b", lambda: g("conv_embed.dw_conv1d.0.bias"))
        self.sinu_w = W.dev("f.sinu_w", lambda: g("sinu_pos_emb.0.weights"))
        self.t_w = W.dev("f.t_w", lambda: g("sinu_pos_emb.1.weight"))
        self.t_b = W.dev("f.t_b", lambda: g("sinu_pos_emb.1.bias"))
        self.layers = []
        for layer in range(depth):
            p = f"transformer.layers.{layer}."
            ff = {}

            def ff1(p=p, ff=ff):
                if not ff:
                    ff["w1"], ff["b1"], ff["inner_pad"] = pack_geglu(g(p + "5.0.weight"), g(p + "5.0.bias"))
                return ff

            def w2_padded(p=p):
                w2 = g(p + "5.3.weight")
                w2p = torch.zeros(w2.shape[0], ff1()["inner_pad"])
                w2p[:, :w2.shape[1]] = w2
                return _pad_rows(w2p)
            k = f"f.layer{layer}."
            self.layers.append(dict(
                gq=W.dev(k + "gq", lambda: g(p + "3.q_norm.gamma").reshape(heads, 64)),
                gk=W.dev(k + "gk", lambda: g(p + "3.k_norm.gamma").reshape(heads, 64)),
                w_qkv=dev_w(k + "w_qkv", lambda: _pad_rows(g(p + "3.to_qkv.weight"))),
                w_out=dev_w(k + "w_out", lambda: _pad_rows(g(p + "3.to_out.weight"))),
                w1=dev_w(k + "w1", lambda: ff1()["w1"]), b1=W.dev(k + "b1", lambda: ff1()["b1"]),
                w2=dev_w(k + "w2", w2_padded), b2=W.dev(k + "b2", lambda: g(p + "5.3.bias")),
                inner_pad=int(W.host(k + "inner_pad", lambda: torch.tensor([ff1()["inner_pad"]], dtype=torch.int32))[0])))

        def gamma_beta(which_tensor):
            out = []
            for layer in range(depth):
                for nidx in ("2", "4"):
                    for which in ("to_gamma", "to_beta"):
                        out.append(g(f"transformer.layers.{layer}.{nidx}.{which}.{which_tensor}"))
            return torch.cat(out, 0)
        self.gb_w = W.dev("f.gb_w", lambda: gamma_beta("weight"))      # [depth*4*dim, dim]
        self.gb_b = W.dev("f.gb_b", lambda: gamma_beta("bias"))
        self.final_gamma = W.dev("f.final_gamma", lambda: g("transformer.final_norm.gamma"))
        self.w_pred = dev_w("f.w_pred", lambda: _pad_rows(g("to_pred.weight")))
        self.inv_freq = W.host("f.inv_freq", lambda: g("transformer.rotary_emb.inv_freq"))
        self._ws = hip.ShapeCache()
        self._group_ws = {}

    @hip.on_device
    def workspace(self, batch, n):
        key = (batch, n)
        if key in self._ws:
            return self._ws[key]
        dev, M, D = self.device, batch * n, self.dim
        f32 = dict(dtype=torch.float32, device=dev)
        cos_t, sin_t = rotary_tables(self.inv_freq, n)
        ws = dict(
            e_cond=torch.empty(M, D, **f32), h=torch.empty(M, D, **f32), h2=torch.empty(M, D, **f32),
            a=torch.empty(M, D, **f32), att=torch.empty(M, D, **f32), qkv=torch.empty(M, 3 * D, **f32),
            g=torch.empty(M, max(l["inner_pad"] for l in self.layers), **f32),
            four=torch.empty(D, **f32), temb=torch.empty(D, **f32),
            gb=torch.empty(self.depth * 4 * D, **f32), cos=cos_t.to(dev), sin=sin_t.to(dev))
        self._ws[key] = ws
        return ws

    def _ragged_tables(self, max_n):
        cos_t, sin_t = rotary_tables(self.inv_freq, max_n)      # positions restart in every clip
        return dict(cos=cos_t.to(self.device), sin=sin_t.to(self.device))

    @hip.on_device
    def _group_buffers(self, n_groups):
        """four [G, D], temb [G, D], gb [G, depth*4*D] of the grouped forward: a few KB to a few hundred KB, kept per G."""
        bufs = self._group_ws.get(n_groups)
        if bufs is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            bufs = self._group_ws[n_groups] = dict(four=torch.empty(n_groups, self.dim, **f32), temb=torch.empty(n_groups, self.dim, **f32),
                                                   gb=torch.empty(n_groups, self.depth * 4 * self.dim, **f32))
        return bufs

    @hip.on_device
    def forward(self, x, t, out, batch, n, alpha=1.0, res=None, null_cond=False, ragged=None, groups=None, n_seg=None):
        """out = alpha * v(x, t) + res  with v the vector field; x/out/res [B*n, dim_in].
        null_cond=True evaluates v with every frame's condition replaced by `null_cond`
        (the cond_drop_prob = 1 pass of forward_with_cond_scale, flow.py:174-178,222-230).
        ragged: a ragged_workspace -- the rows are clips of different lengths packed back to back; everything
        row-wise runs as for one long clip, the three operators that look across rows (ConvPositionEmbed, rotary
        positions, attention) take the segment table: the reference's mask paths (transformer.py:35-44,
        attend.py:127-128) without the padding rows.
        groups = (row_ends, times) with ragged, n_seg = k: a time per GROUP of rows (csrc/steps.hip; ode.mixed_schedule).  The
        first k segments of the workspace run, row_ends[-1] rows in all; group g is the rows row_ends[g - 1] .. row_ends[g] - 1
        and is evaluated at times[g] (at most 8 groups).  The time path is three grouped launches, the five norms take a gamma /
        beta per group, the segment kernels take the prefix of the table.  The field is written raw in this form (t, alpha and
        res are not read: the caller applies the update, fh_axpy_groups_f32); a row has the bits of a ragged forward of its
        group's clips alone at that group's time."""
        if groups is not None and ragged is None:
            raise ValueError("groups= goes with a ragged workspace")
        L, st = hip.lib(), hip.stream()
        ws = ragged if ragged is not None else self.workspace(batch, n)
        M, D = (ragged["rows"] if ragged is not None else batch * n), self.dim
        n_seg_all, max_n = (len(ragged["frames"]), ragged["max_n"]) if ragged is not None else (0, 0)
        grp = None
        if groups is not None:
            row_ends, times = groups
            n_seg = n_seg_all if n_seg is None else int(n_seg)
            if not 1 <= n_seg <= n_seg_all or sum(ragged["frames"][:n_seg]) != row_ends[-1] or len(times) != len(row_ends):
                raise ValueError(f"groups ending at rows {tuple(row_ends)} with {len(times)} times do not fit the first {n_seg} "
                                 f"segments of frames {ragged['frames']}")
            grp, M, max_n = hip.row_groups(row_ends), int(row_ends[-1]), max(ragged["frames"][:n_seg])
            alpha, res = 1.0, None
        else:
            n_seg = n_seg_all
        rows = (batch, n) if ragged is None else (ragged["seg"].data_ptr(), n_seg, max_n)
        h, h2, a, att, qkv = ws["h"], ws["h2"], ws["a"], ws["att"], ws["qkv"]
        self._embed(x, ws, M, rows, null_cond)
        if grp is None:
            gb = ws["gb"]
            self._time_path(t, ws, D // 2, D, self.gb_w, self.gb_b, gb)

            def norm(x_, gamma, beta):
                hip.check(L.fh_rmsnorm_f32(x_.data_ptr(), gamma.data_ptr(), hip.ptr(beta), a.data_ptr(), M, D, st), "fh_rmsnorm_f32")
        else:
            G, gw = grp.n, self._group_buffers(grp.n)
            gb = gw["gb"][0]                      # (group 0's vector: group g's lies g * gb_stride floats behind it)
            gb_stride = gw["gb"].shape[1]
            hip.check(L.fh_time_fourier_groups_f32(self.sinu_w.data_ptr(), hip.group_floats(times), gw["four"].data_ptr(), D // 2, G, st),
                      "fh_time_fourier_groups_f32")
            hip.check(L.fh_gemv_rows_f32(self.t_w.data_ptr(), gw["four"].data_ptr(), D, self.t_b.data_ptr(), gw["temb"].data_ptr(), D,
                                         D, D, G, 1, st), "fh_gemv_rows_f32")
            hip.check(L.fh_gemv_rows_f32(self.gb_w.data_ptr(), gw["temb"].data_ptr(), D, self.gb_b.data_ptr(), gw["gb"].data_ptr(),
                                         gb_stride, self.gb_w.shape[0], D, G, 0, st), "fh_gemv_rows_f32")

            def norm(x_, gamma, beta):            # (the final norm's gamma is a weight, the same for every group: stride 0)
                hip.check(L.fh_rmsnorm_groups_f32(x_.data_ptr(), gamma.data_ptr(), hip.ptr(beta), gb_stride if beta is not None else 0,
                                                  a.data_ptr(), M, D, ctypes.byref(grp), st), "fh_rmsnorm_groups_f32")
        cur, other = h2, h
        for li, lay in enumerate(self.layers):
            o = li * 4 * D
            g1, b1, g2, b2 = (gb[o + i * D: o + (i + 1) * D] for i in range(4))
            norm(cur, g1, b1)
            self.gemm(a, lay["w_qkv"], qkv, M, 3 * D, D)
            across("fh_qknorm_rope", (qkv.data_ptr(), lay["gq"].data_ptr(), lay["gk"].data_ptr(), ws["cos"].data_ptr(), ws["sin"].data_ptr()),
                   rows, (self.heads,))
            across(self._attn_stem, (qkv.data_ptr(), att.data_ptr()), rows, (self.heads, *self._attn_tail))
            self.gemm(att, lay["w_out"], other, M, D, D, R=cur)
            cur, other = other, cur
            norm(cur, g2, b2)
            ip = lay["inner_pad"]
            self.gemm(a, lay["w1"], ws["g"], M, 2 * ip, D, bias=lay["b1"], epilogue=hip.EPI_GEGLU, ldc=ws["g"].shape[1])
            self.gemm(ws["g"], lay["w2"], other, M, D, ip, bias=lay["b2"], R=cur, lda=ws["g"].shape[1])
            cur, other = other, cur
        norm(cur, self.final_gamma, None)
        return self._predict(a, out, M, alpha, res)
