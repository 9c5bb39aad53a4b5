"""CPU restatement of the ConvNeXt vector field (TEST HELPER, not collected): plain torch in the dtype of its inputs, driven by
a state dict under the reference's key names.  Restates flow.py:185-261 with architecture = 'convnext' and convnext.py:44-93 of
the reference's src/flowhigh/models/; no reference code is imported.  tests/test_convnext_cpu.py pins it against the live
reference; the GPU tests take it in float64 as the truth and in float32 as the measure of what float32 can do.

The front end, the ODE stepper, the vocoder and the post-processing around the field are the oracle's (oracle/ref_cpu.py)."""
import torch
import torch.nn.functional as F

from oracle import ref_cpu

FH = "flowhigh."
EPS = 1e-6


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def n_blocks(sd):
    i = 0
    while f"{FH}convnext.{i}.dwconv.weight" in sd:
        i += 1
    return i


def dwconv_ln(x, w, b, scale, shift, eps=EPS):
    """x [B, n, dim]; w [dim, 1, k] or None (no conv); scale / shift [dim]: the operator of fh_dwconv_ln_f32."""
    u = x
    if w is not None:
        u = F.conv1d(x.transpose(1, 2), w, b, padding=w.shape[-1] // 2, groups=w.shape[0]).transpose(1, 2)
    return F.layer_norm(u, (u.shape[-1],), eps=eps) * scale + shift


def block(sd, p, x, t_emb):
    """convnext.py:44-61 on [B, n, dim]; t_emb [B, hidden]."""
    scale = F.linear(t_emb, sd[p + "norm.scale.weight"], sd[p + "norm.scale.bias"])[:, None, :]      # convnext.py:87-93
    shift = F.linear(t_emb, sd[p + "norm.shift.weight"], sd[p + "norm.shift.bias"])[:, None, :]
    y = dwconv_ln(x, sd[p + "dwconv.weight"], sd[p + "dwconv.bias"], scale, shift)
    y = F.linear(F.gelu(F.linear(y, sd[p + "pwconv1.weight"], sd[p + "pwconv1.bias"])), sd[p + "pwconv2.weight"], sd[p + "pwconv2.bias"])
    if p + "gamma" in sd:
        y = sd[p + "gamma"] * y
    return x + y


def convnext_forward(sd, x, cond, t, return_stages=False):
    """flow.py:185-261 with cond_drop_prob = 0, masks None, architecture = 'convnext'.  x, cond [B, N, dim_in]; t scalar / [B]."""
    times = torch.as_tensor(t, dtype=x.dtype)
    if times.ndim == 0:
        times = times.repeat(cond.shape[0])
    h = F.linear(torch.cat((x, cond), dim=-1), sd[FH + "to_embed.weight"], sd[FH + "to_embed.bias"])
    w = sd[FH + "conv_embed.dw_conv1d.0.weight"]
    pe = F.conv1d(h.transpose(1, 2), w, sd[FH + "conv_embed.dw_conv1d.0.bias"], padding=w.shape[-1] // 2, groups=w.shape[0])
    h = F.gelu(pe).transpose(1, 2) + h
    t_emb = ref_cpu.time_embedding(sd, times)
    stages = {"conv_embed": h}
    for i in range(n_blocks(sd)):
        h = block(sd, f"{FH}convnext.{i}.", h, t_emb)
        stages[f"block{i}"] = h
    h = F.layer_norm(h, (h.shape[-1],), sd[FH + "final_layer_norm.weight"], sd[FH + "final_layer_norm.bias"], eps=EPS)
    out = F.linear(h, sd[FH + "to_pred.weight"])
    return (out, stages) if return_stages else out


def vector_field(sd, y, cond_mel, t, cond_scale=1.0):
    """flow.py:165-178 forward_with_cond_scale."""
    logits = convnext_forward(sd, y, cond_mel, t)
    if cond_scale == 1.0:
        return logits
    null_logits = convnext_forward(sd, y, sd[FH + "null_cond"].to(cond_mel.dtype).expand_as(cond_mel), t)
    return null_logits + (logits - null_logits) * cond_scale


@torch.no_grad()
def sample(sd, h, cond48, noise, time_steps=1, method="euler", cond_scale=1.0, decode=True):
    """oracle.ref_cpu.sample (basic_cfm) around the restated field, in the dtype of `cond48` (sd already cast)."""
    cond_mel = ref_cpu.logmel(cond48)
    t = torch.linspace(0, 1, time_steps + 1, dtype=cond48.dtype)
    mel = ref_cpu.odeint_fixed(lambda tt, y: vector_field(sd, y, cond_mel, tt, cond_scale), noise.to(cond48.dtype), t, method)
    return ref_cpu.bigvgan_forward(sd, h, mel.transpose(1, 2)) if decode else mel


@torch.no_grad()
def generate(sd, h, audio, sr, noise, timestep=1, method="euler", dtype=torch.float32):
    """oracle.ref_cpu.generate around the restated field -> (out [1, T48], cr).  dtype float64: everything behind the
    (float32) resampled clip in double."""
    cond = ref_cpu.preprocess(audio, sr).to(dtype)
    wav = sample(cast(sd, dtype), h, cond, noise, timestep, method).squeeze(1)
    return ref_cpu.post_processing(wav, cond, cond.size(-1), return_cr=True)
