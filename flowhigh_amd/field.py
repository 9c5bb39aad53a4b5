"""What the two vector fields (`flow.FlowNet`, `convnext.ConvNextNet`) do identically, once: everything in front of the
backbone (flow.py:232-242 of the reference: the embedding, ConvPositionEmbed, the time embedding), `to_pred` behind it, the
segment table of a ragged batch, and the one place that picks the batched or the segment entry of an operator that looks
across rows."""
import torch

from . import hip


def entry_pair(stem):
    """The batched and the segment entry of an operator that looks across rows: `<stem>_f32`, `<stem>_seg_f32`."""
    return stem + "_f32", stem + "_seg_f32"


def across(stem, lead, rows, trail):
    """One launch of such an operator.  rows = (batch, n): `<stem>_f32(*lead, batch, n, *trail, stream)`; rows = (seg, n_seg,
    max_n) with seg the device segment table: `<stem>_seg_f32(*lead, seg, n_seg, max_n, *trail, stream)`."""
    name = entry_pair(stem)[len(rows) - 2]
    hip.check(getattr(hip.lib(), name)(*lead, *rows, *trail, hip.stream()), name)


class FieldNet:
    """Base of the vector fields.  A subclass sets device, bf, dim, dim_in, dw_k, w_x, w_c, b_embed, null_cond, dw_w, dw_b,
    sinu_w, t_w, t_b, w_pred, _e_null = None and _ws = hip.ShapeCache(), and has workspace(batch, n)."""

    def gemm(self, A, W, C_out, M, N, K, **kw):
        return hip.gemm(A, W, C_out, M, N, K, bf=self.bf, **kw)

    def _ragged_tables(self, max_n):
        """Device tables a ragged entry owns beside the segment table (positions restart in every clip)."""
        return {}

    @hip.on_device
    def ragged_workspace(self, frames):
        """Workspace for a ragged batch: clips of `frames` frames each packed back to back (M = sum rows, no padding).
        Carries the device segment table [n_seg][2] = (first row, rows) the seg kernels take."""
        frames = tuple(int(n) for n in frames)
        key = ("ragged",) + frames
        M, max_n = sum(frames), max(frames)
        if key in self._ws:
            small = self._ws[key]
        else:
            starts = [0]
            for n in frames[:-1]:
                starts.append(starts[-1] + n)
            small = dict(self._ragged_tables(max_n),
                         seg=torch.tensor([[s_, n] for s_, n in zip(starts, frames)], dtype=torch.int32).to(self.device),
                         frames=frames, rows=M, max_n=max_n)
            self._ws[key] = small           # (accounted with what it owns: the tables)
        # The row buffers are the ones of ONE clip of >= M frames, looked up on every call and never held by the
        # cached entry (an entry that kept them would pin workspace(1, M) for every mix of lengths, outside the byte
        # bound of the cache); M is rounded up so that mixes of similar total length share them.
        ws = dict(self.workspace(1, -(-M // 256) * 256))
        ws.update(small)
        return ws

    @hip.on_device
    def set_cond(self, cond, batch, n, ragged=None):
        """cond [B*n, dim_in] (log-mel of the low-res clip): e_cond = cond @ W_c^T + b."""
        ws = ragged if ragged is not None else self.workspace(batch, n)
        M = ragged["rows"] if ragged is not None else batch * n
        self.gemm(cond, self.w_c, ws["e_cond"], M, self.dim, self.dim_in, bias=self.b_embed)

    def _embed(self, x, ws, M, rows, null_cond):
        """h = x @ W_x^T + e_cond (or + the null condition's row), h2 = h + ConvPositionEmbed(h): ws['h'], ws['h2']."""
        D, h = self.dim, ws["h"]
        if null_cond:
            if self._e_null is None:            # null_cond @ W_c^T + b: one row, broadcast with ldr = 0
                self._e_null = torch.empty(1, D, dtype=torch.float32, device=self.device)
                self.gemm(self.null_cond, self.w_c, self._e_null, 1, D, self.dim_in, bias=self.b_embed)
            self.gemm(x, self.w_x, h, M, D, self.dim_in, R=self._e_null, ldr=0)
        else:
            self.gemm(x, self.w_x, h, M, D, self.dim_in, R=ws["e_cond"])
        across("fh_dwconv_gelu_res", (h.data_ptr(), self.dw_w.data_ptr(), self.dw_b.data_ptr(), ws["h2"].data_ptr()), rows, (D, self.dw_k))

    def _time_path(self, t, ws, half, hidden, w, b, out):
        """One time for all rows: out = W silu(t_w fourier(t) + t_b) + b, with fourier [2 half], the embedding [hidden]."""
        L, st = hip.lib(), hip.stream()
        hip.check(L.fh_time_fourier_f32(self.sinu_w.data_ptr(), float(t), ws["four"].data_ptr(), half, st), "fh_time_fourier_f32")
        hip.check(L.fh_gemv_f32(self.t_w.data_ptr(), ws["four"].data_ptr(), self.t_b.data_ptr(), ws["temb"].data_ptr(), hidden,
                                self.t_w.shape[1], 1, st), "fh_gemv_f32")
        hip.check(L.fh_gemv_f32(w.data_ptr(), ws["temb"].data_ptr(), b.data_ptr(), out.data_ptr(), w.shape[0], hidden, 0, st),
                  "fh_gemv_f32")

    def _predict(self, a, out, M, alpha, res):
        """out = alpha * (a @ W_pred^T) + res."""
        self.gemm(a, self.w_pred, out, M, self.dim_in, self.dim, R=res, alpha=alpha)
        return out
