"""`FlowHighSR` -- drop-in host class for the reference's public API on MI355X.

Mirrors flowhighsr.py:21-149 of the reference's src/flowhigh/ (`FlowHighSR`: ctor kwargs,
`generate`, `set_cfm_method`, `from_local`, `from_pretrained`) and the inference half of
cfm_superresolution.py:94-284 (`ConditionalFlowMatcherWrapper`:
`sample`, `load`, `device`, `odeint_kwargs`, `sigma`, `cfm_method`).  torchdiffeq's fixed-grid
steppers (call site cfm:243; euler, midpoint, heun2, heun3, rk4) are tableaus in ode.py, run by integrate.py.

Everything numerical runs in the HIP kernels of libflowhigh_hip.so; this file only moves
tensors, picks shapes and sequences launches.  There is no CPU path: constructing the model on
a non-CUDA device, or without the built library, raises.

Extensions over the reference (all keyword-only, defaults keep reference behaviour):
  generate(..., noise=, generator=)   explicit prior draw / CPU generator (parity hook)
  prior='device', generate(..., seed=) the prior drawn on the device from (seed, stream) keys (csrc/prior.hip, prior.py)
  sample(..., cond_scale=, mel_pp=)    as in the reference, evaluated on the device (no python bin loops)
  generate_batch(clips, sr, ...)      B equal-length clips, every per-clip normalisation kept per clip
  upsampling_method='hip'             resample_poly on the device instead of scipy on the host
  generate*(..., channels=, level=)   multichannel clips ([C, T] / [T, C], one prior per clip) and output at the input's own
                                      level instead of 0.99 peak (csrc/level.hip; DESIGN.md "Channels and level")
  generate*(..., output_rate=, pcm=, dither=, dither_seed=, interleaved=)   the result delivered on the device: resampled to
                                      another rate, as int16 PCM (TPDF dither), interleaved [T, C] (delivery.py, csrc/pcm.hip)
  generate*(..., loudness=L)          the result at L LUFS (ITU-R BS.1770-4) on the device; measure_loudness reads it back
                                     (loudness.py is the definition, csrc/loudness.hip the kernels; DESIGN.md "Loudness")
  generate*(..., true_peak=T, limiter=)   the result under T dBTP, by one gain or by a look-ahead limiter; measure_true_peak reads it
                                     back (truepeak.py is the definition, csrc/truepeak.hip the kernels; DESIGN.md "True peak and limiter")
  stream(sr, ...) -> push / flush, stream_push(sessions, blocks), generate_long(audio, sr, ...)   streaming sessions: overlapping
                                     windows that share one keyed prior at their absolute frames, cross-faded on the device
                                     (stream.py is the definition, streaming.py the host side, csrc/stream.hip the seam; DESIGN.md "Streaming")
"""
import json
from pathlib import Path

import os

import numpy as np
import torch

from . import hip, integrate, ode
from .flow import FlowNet
from .delivery import Delivery, resolve_delivery
from .frontend import LogMel, PostProcessor, Resampler, _starts, _views, clip_rates
from .grouping import pack_ragged, plan_buckets
from .prior import expand_seed, normalize_key
from .tables import HOP, resample_out_len
from .vocoder import VOC, Vocoder, fold_weight_norm

REPO_ID = "ResembleAI/FlowHigh"
# the checkpoint files from_local reads (flowhighsr.py:110-137 of the reference); a weight blob records their digests
CKPT_FILES = ("bigvgan_48khz_256band.json", "bigvgan_48khz_256band.pt", "FLowHigh_basic_400k.pt")


def weights_conv_form():
    """The conv form the environment asks for ('auto' resolved to the default form): what convert.py packs."""
    from .planner import resolve_conv_form
    return resolve_conv_form()[0]


def read_checkpoints(ckpt_dir, architecture=None):
    """(state dict with the wrapper's keys, vocoder JSON) from the reference's three checkpoint files: weight norm folded
    (init_vocoder.py:13-17), key sets checked as load_state_dict(strict=True) would (flowhighsr.py:135).
    architecture: None = the backbone the model file's keys show (detect_architecture), else the one they must be of."""
    ckpt_dir = Path(ckpt_dir)
    cfg = json.loads((ckpt_dir / "bigvgan_48khz_256band.json").read_text())
    gen = _load_checkpoint(ckpt_dir / "bigvgan_48khz_256band.pt")['generator']
    sd = {VOC + k: v for k, v in fold_weight_norm(gen).items()}            # init_vocoder.py:13-17
    model = _load_checkpoint(ckpt_dir / "FLowHigh_basic_400k.pt")['model']
    check_state_dict_keys(sd, cfg, only_prefix=VOC)                        # vocoder.load_state_dict (init_vocoder.py:16)
    # load_state_dict(strict=True), flowhighsr.py:135
    check_state_dict_keys(model, cfg, architecture=resolve_architecture(architecture, model))
    sd.update(model)                                                       # wrapper checkpoint wins
    return sd, cfg
_CFM_METHODS = ("basic_cfm", "independent_cfm_adaptive", "independent_cfm_constant", "independent_cfm_mix")
# where the flow-matching prior eps ~ N(0, 1) of a call without noise= comes from.  'reference': torch's CPU stream, drawn on the
# host (reference_prior_draw below; the default).  'device': this project's own counter-based stream, drawn by fh_prior_normal_f32
# from one (seed, stream) key per clip (prior.py restates it on the host)
_PRIORS = ("reference", "device")
# how a ragged generate_many call runs what surrounds its one transformer + vocoder launch sequence (resampling, peak
# normalisation, log-mel, the vocoder's input copies, post-processing).  'per_clip': once per clip, the batched entries on
# batches of one (the default).  'ragged': the segment forms of the same entries (fh_*_seg_f32, csrc/frontend.hip), one launch per step
# for the whole list; same bits per clip
_ENDS = ("per_clip", "ragged")


def resolve_ends(ends=None):
    """ends= of generate_many / BatchingServer: the keyword, else FH_RAGGED_ENDS, else 'per_clip'."""
    if ends is None:
        ends = os.environ.get("FH_RAGGED_ENDS") or "per_clip"
    if ends not in _ENDS:
        raise ValueError(f"ends must be one of {_ENDS}, got {ends!r}")
    return ends


def resolve_rates(sr, n_clips):
    """sr= of generate_many as one input rate per clip: an int holds for every clip, a sequence gives one positive integer
    rate per clip.  Anything else is a ValueError (a wrong length names both counts), raised before any GPU work."""
    return clip_rates(sr, n_clips)


# channels= of generate / generate_batch / generate_many / BatchingServer: the layout of a clip.  None: mono, 1-D or [1, T] (the
# reference's contract).  'first': [C, T].  'last': [T, C] (gradio, soundfile).  Every channel runs as the mono path runs a clip;
# the clip's channels share one prior draw and, at level='peak', one peak.
_CHANNELS = (None, "first", "last")
MAX_CHANNELS = 8
# level= of the same entries: what the output is scaled to.  'peak' (default): 0.99 of the clip's own peak, as the reference.
# 'input': the level of what came in -- the input's band as it was sent plus the generated high band beside it
_LEVELS = ("peak", "input")


def resolve_level(level):
    if level not in _LEVELS:
        raise ValueError(f"level must be one of {_LEVELS}, got {level!r}")
    return level


def resolve_channels(audio, channels=None):
    """One clip as planar [C, T] (a numpy view where the input allows one; dtype and values untouched), 1 <= C <= 8.
    channels=None: 1-D or [1, T].  'first': [C, T].  'last': [T, C].  A 1-D clip is one channel under every value.
    Everything else is a ValueError: a 2-D clip without the keyword, more than 8 channels, an empty clip, 0-D or 3-D input."""
    if channels not in _CHANNELS:
        raise ValueError(f"channels must be one of {_CHANNELS}, got {channels!r}")
    if isinstance(audio, torch.Tensor):
        audio = audio.detach().cpu().numpy()
    a = np.asarray(audio)
    if a.ndim == 1:
        a = a[None]
    elif a.ndim != 2:
        raise ValueError(f"a clip is 1-D, or 2-D with channels='first' ([C, T]) or channels='last' ([T, C]); got shape {a.shape}")
    elif channels is None:
        if a.shape[0] != 1:
            raise ValueError(f"a clip of shape {a.shape} needs channels='first' ([C, T]) or channels='last' ([T, C]): "
                             "without the channels keyword a clip is 1-D or [1, T]")
    elif channels == "last":
        a = a.T
    if a.shape[1] < 1:
        raise ValueError("empty clip")
    if a.shape[0] > MAX_CHANNELS:
        raise ValueError(f"channels={channels!r}: {a.shape[0]} channels, at most {MAX_CHANNELS} (is the layout the other one?)")
    return a


def channel_noise(noise, n_channels):
    """noise= of one clip of n_channels channels as [C, N, n_mels]: [1, N, n_mels] is shared by the channels (a view), [C, N,
    n_mels] is one draw per channel.  Any other leading dimension is a ValueError."""
    if noise.ndim != 3 or noise.shape[0] not in (1, n_channels):
        raise ValueError(f"noise of shape {tuple(noise.shape)} for a clip of {n_channels} channels: [1, N, n_mels] "
                         f"(shared) or [{n_channels}, N, n_mels] (one per channel)")
    return noise.expand(n_channels, -1, -1)


def clip_noises(noise, chans):
    """noise= of a call over clips of chans[i] channels as a list of [C_i, N, n_mels] (channel_noise): a list holds one tensor
    per clip; a tensor is the one clip's, or [B, N, n_mels] with one shared draw per clip."""
    if noise is None:
        return None
    if isinstance(noise, (list, tuple)):
        noises = list(noise)
    elif len(chans) == 1:
        noises = [noise]
    else:
        noises = [noise[i:i + 1] for i in range(noise.shape[0])]
    if len(noises) != len(chans):
        raise ValueError(f"one noise tensor per clip: {len(noises)} for {len(chans)} clips")
    return [channel_noise(z, c) for z, c in zip(noises, chans)]


def resolve_clips(clips, channels=None, level="peak"):
    """The clips of a call, layouts checked (resolve_channels; a ValueError before any GPU work) ->
      (clips, None)     mono clips at level='peak', a plain call (FlowHighSR._planar): as they came, or [1, T] views
      (None, planar)    anything else: float [C_i, T_i] arrays, the int16 rule (max > 1 -> / 32768) applied once per clip."""
    level = resolve_level(level)
    planar = [resolve_channels(a, channels) for a in clips]
    if level == "peak" and all(a.shape[0] == 1 for a in planar):
        return (clips if channels is None else planar), None
    return None, [a / 32768.0 if a.max() > 1 else a for a in planar]


def reference_prior_draw(n_frames, n_mels=256, generator=None):
    """What `torch.randn_like(cond)` yields in the reference on CPU (cfm_superresolution.py:220):
    `cond` is the 'b d n -> b n d' *view* of the mel (melvoco.py:85); randn_like keeps its strides
    and torch's CPU normal_() takes the scalar path for non-contiguous outputs, so both the fill
    order and the values differ from a contiguous torch.randn(1, N, 256)."""
    t = torch.empty_strided((1, n_frames, n_mels), (n_frames * n_mels, 1, n_frames))
    return t.normal_(generator=generator)


def _load_checkpoint(path):
    """torch.load of a reference checkpoint file.  Only plain state-dict entries are read ('generator', 'model'), so
    the safe unpickler is enough (`weights_only=True`: a downloaded file cannot run code); a checkpoint that carries
    arbitrary pickled objects needs the explicit opt-in FH_UNSAFE_LOAD=1."""
    try:
        return torch.load(str(path), map_location='cpu', weights_only=True)
    except Exception as e:                         # noqa: BLE001  (torch raises pickle.UnpicklingError subclasses)
        if os.environ.get("FH_UNSAFE_LOAD", "0") != "1":
            raise RuntimeError(f"{path}: cannot be read with weights_only=True ({type(e).__name__}: {e}); "
                               "set FH_UNSAFE_LOAD=1 to unpickle it anyway (executes code from the file)") from e
        return torch.load(str(path), map_location='cpu', weights_only=False)


# the vector field's backbone (the reference's FLowHigh(architecture=), models/flow.py:74-139): the published checkpoint is a
# transformer (flow.py: FlowNet); 'convnext' is the reference's second one (convnext.py: ConvNextNet)
ARCHITECTURES = ("transformer", "convnext")
CONVNEXT_BLOCKS = 8            # num_layers of the reference's convnext backbone (flow.py:126)


def detect_architecture(sd):
    """The backbone a state dict holds: 'convnext' if it has any `flowhigh.convnext.*` key, else 'transformer'."""
    from .convnext import is_convnext_state_dict
    return "convnext" if is_convnext_state_dict(sd) else "transformer"


def resolve_architecture(architecture, sd=None):
    """architecture= of FLowHigh / from_local / load: None = what the keys of `sd` show ('transformer' without a state dict),
    else one of ARCHITECTURES (anything else is a ValueError)."""
    if architecture is None:
        return detect_architecture(sd) if sd is not None else "transformer"
    if architecture not in ARCHITECTURES:
        raise ValueError(f"architecture must be None or one of {ARCHITECTURES}, got {architecture!r}")
    return architecture


def expected_state_keys(vocoder_cfg, depth=2, architecture="transformer", blocks=CONVNEXT_BLOCKS):
    """Key set of the reference module's state_dict (SURVEY.md 8a "State-dict contract"): what
    `load_state_dict(strict=True)` (flowhighsr.py:135, cfm_superresolution.py:125-131) accepts, no more, no less.
    architecture='convnext': the module built with that backbone (flow.py:124-139; `depth` is then unused, `blocks` is the
    reference's 8): the same keys without any `transformer.*` one, the blocks' and `final_layer_norm`'s instead."""
    resolve_architecture(architecture)
    fh = "flowhigh."
    keys = [fh + k for k in ("null_cond", "sinu_pos_emb.0.weights", "sinu_pos_emb.1.weight", "sinu_pos_emb.1.bias",
                             "to_embed.weight", "to_embed.bias", "conv_embed.dw_conv1d.0.weight",
                             "conv_embed.dw_conv1d.0.bias", "transformer.rotary_emb.inv_freq",
                             "transformer.final_norm.gamma", "to_pred.weight")]
    if architecture == "convnext":
        from .convnext import block_keys
        keys = [k for k in keys if not k.startswith(fh + "transformer.")]
        for i in range(blocks):
            keys += block_keys(i)
        keys += [fh + "final_layer_norm.weight", fh + "final_layer_norm.bias"]
        depth = 0
    for layer in range(depth):
        p = f"{fh}transformer.layers.{layer}."
        for nidx in ("2", "4"):
            keys += [p + f"{nidx}.{w}.{t}" for w in ("to_gamma", "to_beta") for t in ("weight", "bias")]
        keys += [p + "3.q_norm.gamma", p + "3.k_norm.gamma", p + "3.to_qkv.weight", p + "3.to_out.weight",
                 p + "5.0.weight", p + "5.0.bias", p + "5.3.weight", p + "5.3.bias"]
    cfg = vocoder_cfg
    beta = cfg["activation"] == "snakebeta"

    def act(name):
        return [name + "act.alpha"] + ([name + "act.beta"] if beta else []) + \
               [name + "upsample.filter", name + "downsample.lowpass.filter"]

    keys += [VOC + "conv_pre.weight", VOC + "conv_pre.bias", VOC + "conv_post.weight", VOC + "conv_post.bias"]
    keys += [VOC + k for k in act("activation_post.")]
    nk, nm = len(cfg["resblock_kernel_sizes"]), len(cfg["resblock_dilation_sizes"][0])
    for i in range(len(cfg["upsample_rates"])):
        keys += [VOC + f"ups.{i}.0.weight", VOC + f"ups.{i}.0.bias"]
        for j in range(nk):
            r = VOC + f"resblocks.{i * nk + j}."
            if str(cfg["resblock"]) == "1":
                keys += [r + f"{c}.{m}.{t}" for c in ("convs1", "convs2") for m in range(nm) for t in ("weight", "bias")]
                nact = 2 * nm
            else:
                keys += [r + f"convs.{m}.{t}" for m in range(nm) for t in ("weight", "bias")]
                nact = nm
            for a in range(nact):
                keys += [k for k in act(r + f"activations.{a}.")]
    return keys


def check_state_dict_keys(sd, vocoder_cfg, depth=2, only_prefix=None, architecture="transformer", skip_prefix=None):
    """load_state_dict(strict=True) semantics on the key set: missing AND unexpected keys raise RuntimeError.
    skip_prefix: keys under it, wanted or present, are left out of the comparison."""
    want = expected_state_keys(vocoder_cfg, depth, architecture)
    if only_prefix is not None:
        want = [k for k in want if k.startswith(only_prefix)]
    if skip_prefix is not None:
        want = [k for k in want if not k.startswith(skip_prefix)]
        sd = [k for k in sd if not k.startswith(skip_prefix)]
    have = set(sd)
    missing = [k for k in want if k not in have]
    wset = set(want)
    unexpected = [k for k in sd if k not in wset]
    if missing or unexpected:
        def short(v):
            return f"{v[:8]}{' ...' if len(v) > 8 else ''}"
        msg = "Error(s) in loading state_dict:"
        if missing:
            msg += f" Missing key(s) in state_dict: {short(missing)}."
        if unexpected:
            msg += f" Unexpected key(s) in state_dict: {short(unexpected)}."
        raise RuntimeError(msg)


class GraphedGenerate:
    """One captured generate_from_device call (FlowHighSR.capture)."""

    def __init__(self, model, batch, n_in, sr, timestep):
        self.device = dev = model.device
        with hip.device_guard(dev):
            self._capture(model, batch, n_in, sr, timestep, dev)

    def _capture(self, model, batch, n_in, sr, timestep, dev):
        self.x = torch.zeros(batch, n_in, dtype=torch.float32, device=dev)
        t48 = -(-n_in * 48000 // sr)
        # the prior: a static noise buffer, or on a prior='device' model the keys the recorded prior launch reads at every replay
        if model.prior == 'device':
            self.keys = torch.zeros(batch, 2, dtype=torch.int64, device=dev)
            prior = dict(keys=self.keys)
        else:
            self.noise = torch.zeros(batch * (t48 // 480), model.flowhigh.n_mels, dtype=torch.float32, device=dev)
            prior = dict(noise=self.noise)
        self.x[:, 0] = 1.0                                  # any non-silent clip: the peak normalisation divides by max |x|
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                       # warm-up outside the capture: plans, workspaces, LDS opt-in
            for _ in range(2):
                model._generate_from_device(self.x, sr, timestep, **prior)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = model._generate_from_device(self.x, sr, timestep, **prior)
        # The graph holds raw pointers into the per-shape plans / workspaces of the model (vocoder pool and
        # descriptor arrays, transformer / front-end / post-processing buffers).  Those live in byte-bounded LRU
        # caches (hip.ShapeCache): keep a strong reference to every entry of this shape, so that an eviction only
        # drops the cache's reference and replay() never touches memory that went back to the allocator.
        fh = model.flowhigh
        n = t48 // 480
        # (PostProcessor keys its workspace on the vocoder's output length: hop * n, or a few samples more when some
        # upsampler has an odd k - u: Vocoder.out_len)
        self._keep = [c.get(k) for c, k in ((fh.net._ws, (batch, n)), (fh.logmel._ws, (batch, t48)),
                                            (model.postproc._ws, (batch, fh.vocoder.out_len(n), t48, t48)))]
        # vocoder: the plan of the clip, or the plans of its time chunks (key (batch, chunk frames, clip frames))
        voc_plans = [v for k, v in dict.items(fh.vocoder._plans) if k[0] == batch and k[-1] == n]
        self._keep += voc_plans if voc_plans else [None]
        if any(v is None for v in self._keep):
            raise hip.HipError("capture: a workspace of the captured shape is not in its cache (cache bound too small "
                               "for this shape: raise FH_CACHE_GB)")
        self._keep.append(model)

    @hip.on_device
    def replay(self):
        self.graph.replay()
        return self.out


class FLowHigh:
    """Device-resident weights of the vector-field net + its mel codec (the reference's
    `FLowHigh` with `audio_enc_dec = MelVoco`, models/flow.py:54-142, models/melvoco.py:16-46).
    conv_form: 'auto' | 'winograd' | 'bf16x6' | 'direct' | 'direct_bf16x6' | 'direct_bf16x3' (planner.resolve_conv_form; the last one
    is the Winograd-free plan on two bf16 pieces per operand: at most 3 2^-16 per product, not fp32-grade, never chosen by 'auto')."""

    def __init__(self, state_dict, vocoder_config, device="cuda", depth=2, conv_bf16x6=None, store=None, conv_form=None,
                 attn_form=None, attn_window=None, architecture=None):
        from .planner import resolve_attn_form, resolve_attn_window
        # architecture: None (what the state dict's keys show; a weight blob holds a transformer) | 'transformer' | 'convnext'.
        # A named architecture that the keys contradict fails as load_state_dict(strict=True) does.  The convnext backbone has
        # no attention: an explicit attn_form='bf16x6' or attn_window= with it is a ValueError
        named = architecture
        architecture = resolve_architecture(architecture, state_dict)
        if architecture == "convnext" and (attn_window is not None or attn_form == "bf16x6"):
            raise ValueError("attn_form='bf16x6' / attn_window= choose a kernel of the transformer's attention: "
                             "the convnext backbone has none")
        attn_form = resolve_attn_form(attn_form)          # (a wrong keyword is a ValueError before anything is loaded)
        attn_window = resolve_attn_window(attn_window)
        if architecture == "convnext" and state_dict is None:
            raise ValueError("architecture='convnext' needs the checkpoint's state dict: weight blobs hold the transformer backbone only")
        if named is not None and state_dict is not None and detect_architecture(state_dict) != named:
            check_state_dict_keys(state_dict, vocoder_config, depth, architecture=named, skip_prefix=VOC)
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.HipError(f"flowhigh_amd runs on MI355X only (got device '{device}'); there is no CPU path")
        hip.lib()                                   # fail loudly if the extension is not built
        if not torch.cuda.is_available():
            raise hip.HipError("no HIP device visible")
        # 'cuda' = the device current NOW; the model then stays on that ordinal whatever the caller makes current
        # later: every public entry below runs under hip.on_device (the reference's from_local(ckpt_dir, device),
        # flowhighsr.py:110-137)
        self.device = device = hip.norm_device(device)
        self.architecture = architecture
        self.vocoder_config = dict(vocoder_config)
        # store: a weights.WeightStore opened on a weight blob (state_dict may then be None), or a recording one (convert.py)
        if store is None or state_dict is not None:
            missing = [k for k in ("flowhigh.to_embed.weight", VOC + "conv_pre.weight") if k not in state_dict]
            if missing:
                raise RuntimeError(f"Missing key(s) in state_dict: {missing}")
        with hip.device_guard(device):
            # (the transformer's linears follow the REQUESTED form -- bf16 x 6 linears have no Winograd transform to be ill-conditioned,
            # so a probe that moves the vocoder to the direct form below leaves them as they are)
            # attn_form: None | 'f32' (default) | 'bf16x6' -- the arithmetic form of the two products of attention
            # (planner.resolve_attn_form; independent of conv_form, touches no weight).  fp32 kernel's time / bf16 x 6 kernel's at
            # (B, N) = (1, 50) (1, 1000) (8, 1000) (32, 1000) (1, 3000) (8, 3000): 1.00 1.02 1.41 1.36 1.23 1.44 (profiles/attention_bf16x6.md)
            # attn_window: None (default: full attention, the reference's) | W >= 0 -- frame i attends to the frames j of its clip with
            # |i - j| <= W.  The unit is frames of 10 ms: attn_window=500 is +-5 s.  O(N W) instead of O(N^2) for long clips
            # (planner.resolve_attn_window; touches no weight, no part of a blob's format tag; profiles/attention_band.md)
            from .planner import resolve_conv_form, use_gemm_bf16x6
            bf = use_gemm_bf16x6(resolve_conv_form(conv_form, conv_bf16x6)[0])
            if architecture == "convnext":
                # (blocks and inner width are read from the state dict; its linears follow conv_form as the transformer's do)
                from .convnext import ConvNextNet
                self.net = ConvNextNet(state_dict, device, bf=bf)
            else:
                self.net = FlowNet(state_dict, device, depth=depth, store=store, bf=bf, attn_form=attn_form, attn_window=attn_window)
            # conv_form: the arithmetic form of the vocoder's convs, 'auto' | 'winograd' | 'bf16x6' | 'direct' | 'direct_bf16x6' | 'direct_bf16x3'
            # (planner.resolve_conv_form; None: FH_CONV_FORM / the older switches, else 'auto'.  conv_bf16x6: the boolean keyword
            # of rounds 2-5.)  'auto' = the default form, checked once against the direct form through THESE weights when the
            # checkpoint is at hand (probe_conv_form below): a model whose weights amplify the Winograd transforms' rounding is
            # rebuilt in the direct form.
            self.vocoder = Vocoder(self.vocoder_config, state_dict, device, bf16x6=conv_bf16x6, store=store, conv_form=conv_form)
            self.conv_form_probe = None
            if self.vocoder.form_auto and state_dict is not None and os.environ.get("FH_CONV_PROBE", "1") != "0":
                self.probe_conv_form(state_dict)
            self.logmel = LogMel(device)
        self.n_mels = self.net.dim_in

    @property
    def conv_form(self):
        return self.vocoder.form

    @property
    def attn_form(self):
        return getattr(self.net, "attn_form", None)       # (None: the convnext backbone, which has no attention)

    @property
    def attn_window(self):
        """None (full attention) or the band's radius in frames (10 ms each): frame i attends to |i - j| <= attn_window."""
        return getattr(self.net, "attn_window", None)

    def probe_conv_form(self, state_dict, frames=20, limit=None):
        """The load-time estimate behind conv_form='auto': the vocoder in its default form against the direct form (no Winograd
        transform anywhere: its distance to a float64 run is the reference's own fp32 noise, profiles/r05_regime_sweep.txt), both
        through the loaded weights on a `frames`-frame random mel.  max |difference| is logged and kept (conv_form_probe); above
        `limit` (planner.PROBE_LIMIT = 3e-5: a third of the 1e-4 bar) the model keeps the direct-form vocoder instead.
        Oracle-free; costs one packing of the direct-form weights (a reshape) and two 0.2 s forwards."""
        import logging
        from .planner import PROBE_LIMIT
        limit = PROBE_LIMIT if limit is None else limit
        g = torch.Generator().manual_seed(175)
        mel = (torch.randn(1, frames, self.vocoder.true_mels, generator=g) * 2.0 - 3.0).to(self.device)
        direct = Vocoder(self.vocoder_config, state_dict, self.device, conv_form="direct", act_blocks=self.vocoder.act_blocks)
        a = self.vocoder.forward(mel).clone()
        b = direct.forward(mel)
        est = float((a - b).abs().max())
        peak = float(b.abs().max())
        self.conv_form_probe = dict(estimate=est, peak=peak, limit=limit, default=self.vocoder.form, frames=frames)
        log = logging.getLogger("flowhigh_amd")
        if est > limit:
            log.warning("conv_form='auto': the %s form is %.2e from the direct form on a %d-frame probe (|wav| <= %.2f; limit %.0e): "
                        "using the direct form", self.vocoder.form, est, frames, peak, limit)
            self.vocoder = direct
            self.conv_form_probe["chosen"] = "direct"
        else:
            log.info("conv_form='auto': the %s form is %.2e from the direct form on a %d-frame probe (|wav| <= %.2f; limit %.0e): kept",
                     self.vocoder.form, est, frames, peak, limit)
            self.conv_form_probe["chosen"] = self.vocoder.form
            del direct
        return self.conv_form_probe


class FlowHighSR:
    def __init__(
        self,
        flowhigh: FLowHigh,
        sigma=0.,
        ode_atol=1e-5,
        ode_rtol=1e-5,
        use_torchode=False,
        cfm_method='basic_cfm',
        torchdiffeq_ode_method='midpoint',   # ode.ODE_METHODS: [euler, midpoint, heun2, heun3, rk4]
        torchode_method_klass=None,
        cond_drop_prob=0.,
        #
        upsampling_method='scipy',
        prior='reference',                   # [reference, device]: _PRIORS above
    ):
        if prior not in _PRIORS:
            raise ValueError(f"prior must be one of {_PRIORS}, got {prior!r}")
        self.prior = prior
        if use_torchode:
            raise NotImplementedError("the torchode adaptive solver path is out of scope (SURVEY.md 8a row 2)")
        self.flowhigh = flowhigh
        self.sigma = sigma
        self.cond_drop_prob = cond_drop_prob
        self.use_torchode = use_torchode
        self.torchode_method_klass = torchode_method_klass
        self.cfm_method = cfm_method
        self.odeint_kwargs = dict(atol=ode_atol, rtol=ode_rtol, method=torchdiffeq_ode_method)
        self.upsampling_method = upsampling_method
        self.postproc = PostProcessor(flowhigh.device)
        self.resampler = Resampler(flowhigh.device)
        self.delivery = Delivery(flowhigh.device, self.resampler)

    # ---- reference surface -----------------------------------------------------------------
    @property
    def device(self):
        return self.flowhigh.device

    def set_cfm_method(self, cfm_method):
        self.cfm_method = cfm_method

    def eval(self):
        return self

    @hip.on_device
    def load(self, path, strict=True, architecture=None):
        """architecture: None = the backbone the checkpoint's keys show, else the one they must be of (FLowHigh)."""
        path = Path(path)
        assert path.exists()
        pkg = _load_checkpoint(path)
        arch = resolve_architecture(architecture, pkg['model'])
        if strict:
            check_state_dict_keys(pkg['model'], self.flowhigh.vocoder_config, architecture=arch)
        attn = dict(attn_form=self.flowhigh.attn_form, attn_window=self.flowhigh.attn_window) if arch == "transformer" else {}
        self.flowhigh = FLowHigh(pkg['model'], self.flowhigh.vocoder_config, self.device, architecture=arch, **attn)
        return pkg

    @classmethod
    def from_local(cls, ckpt_dir, device='cuda', conv_form=None, attn_form=None, attn_window=None, architecture=None,
                   **kwargs) -> 'FlowHighSR':
        """from_local of the reference (flowhighsr.py:110-137) + conv_form = 'auto' (default) | 'winograd' | 'bf16x6' | 'direct' | 'direct_bf16x6' | 'direct_bf16x3': the
        arithmetic form of the vocoder's convs (planner.resolve_conv_form; the environment's
        FH_CONV_FORM overrides nothing a caller passes here); attn_form = None | 'f32' (default) | 'bf16x6': the form of the two
        products of attention (planner.resolve_attn_form; no part of a weight blob); attn_window = None (default: full attention, as
        the reference) | W >= 0: every frame attends to the frames within W of it, in frames of 10 ms -- attn_window=500 is +-5 s
        (planner.resolve_attn_window; no part of a weight blob either); architecture = None (default: the backbone the
        checkpoint's keys show) | 'transformer' | 'convnext' (the reference's --architecture; FLowHigh).  Weight blobs hold the
        transformer backbone only: a convnext checkpoint is always read from its files."""
        from .planner import resolve_attn_form, resolve_attn_window, resolve_conv_form
        form, form_auto = resolve_conv_form(conv_form)
        if architecture is not None:
            resolve_architecture(architecture)
        if architecture == "convnext" and (attn_window is not None or attn_form == "bf16x6"):
            raise ValueError("attn_form='bf16x6' / attn_window= choose a kernel of the transformer's attention: "
                             "the convnext backbone has none")
        explicit_attn = dict(attn_form=attn_form, attn_window=attn_window)
        attn_form = resolve_attn_form(attn_form)
        attn_window = resolve_attn_window(attn_window)
        ckpt_dir = Path(ckpt_dir)
        dev = device if torch.device(device).type == 'cuda' else 'cuda'        # the reference always .cuda()s
        # A weight blob next to the checkpoints (python -m flowhigh_amd.convert <ckpt_dir>; FH_BLOB = another path, FH_BLOB=0 =
        # ignore): the packed device weights in one file, mapped and uploaded with one copy -- if it was made from THESE
        # checkpoint files (content digests) under the current layout switches.  Otherwise the checkpoints are read as always.
        from . import weights
        blob = os.environ.get("FH_BLOB", str(ckpt_dir / weights.BLOB_NAME))
        if blob != "0" and Path(blob).exists() and architecture != "convnext":
            srcs = {f: weights.file_digest(ckpt_dir / f) for f in CKPT_FILES} if os.environ.get("FH_BLOB_VERIFY", "1") != "0" else None
            # ('auto': a blob of the default form is taken as it is -- the probe needs the checkpoint; a blob written by
            # `python -m flowhigh_amd.convert --probe` on a GPU box already holds the form the probe chose)
            tags = [weights.format_tag(form)] + ([weights.format_tag("direct")] if form_auto else [])
            store, why = None, None
            for tag in tags:
                store = weights.WeightStore.open(blob, hip.norm_device(dev), expect_format=tag, sources=srcs)
                if store is not None:
                    form = json.loads(tag)["form"]
                    break
                why = why or weights.WeightStore.why          # (the reason the blob is not one of the FIRST form asked for)
            if store is None:
                weights.WeightStore.why = why
            if store is not None:
                try:
                    return cls(flowhigh=FLowHigh(None, store.cfg, dev, store=store, conv_form=form, attn_form=attn_form, attn_window=attn_window),
                               **kwargs)
                except (RuntimeError, KeyError, ValueError) as e:          # a damaged or stale blob must not stop the load
                    weights.WeightStore.why = f"{type(e).__name__}: {e}"
            import logging
            logging.getLogger("flowhigh_amd").warning("weight blob %s not used (%s): reading the checkpoints", blob, weights.WeightStore.why)
        sd, cfg = read_checkpoints(ckpt_dir, architecture)
        # (the keywords as the caller gave them: with a convnext checkpoint an explicit attention keyword is FLowHigh's ValueError)
        return cls(flowhigh=FLowHigh(sd, cfg, dev, conv_form="auto" if form_auto else form, architecture=architecture, **explicit_attn),
                   **kwargs)

    @classmethod
    def from_pretrained(cls, device='cuda', conv_form=None, attn_form=None, attn_window=None, architecture=None,
                        **kwargs) -> 'FlowHighSR':
        """from_local on the published checkpoint.  conv_form = 'auto' (default) | 'winograd' | 'bf16x6' | 'direct' | 'direct_bf16x6' |
        'direct_bf16x3' (from_local).  attn_window = None (full attention) | W >= 0 frames of 10 ms (from_local)."""
        from .planner import resolve_attn_window
        attn_window = resolve_attn_window(attn_window)          # (a wrong keyword is a ValueError before anything is fetched)
        from huggingface_hub import hf_hub_download
        for fpath in ["FLowHigh_basic_400k.json", "bigvgan_48khz_256band.json",
                      "FLowHigh_basic_400k.pt", "bigvgan_48khz_256band.pt"]:
            local_path = hf_hub_download(repo_id=REPO_ID, filename=fpath)
        return cls.from_local(Path(local_path).parent, device, conv_form=conv_form, attn_form=attn_form, attn_window=attn_window,
                              architecture=architecture, **kwargs)

    # ---- host pre-step (flowhighsr.py:59-86) -----------------------------------------------------
    def _upload(self, t):
        """Host tensor -> device through pinned staging, asynchronously: a pageable .to(device) blocks the host
        until everything queued before it on the stream has run, which serialises the host work of the next
        request with the GPU work of the current one (generate_many / the batching server)."""
        if t.device.type != "cpu" or self.device.type != "cuda":
            return t.to(self.device)
        return t.pin_memory().to(self.device, non_blocking=True)

    @staticmethod
    def _host_clips(clips):
        prepared = []
        for audio in clips:
            if isinstance(audio, torch.Tensor):
                audio = audio.detach().cpu().numpy()
            audio = np.asarray(audio)
            if len(audio.shape) == 2:
                audio = audio.squeeze(0)
            if audio.max() > 1:
                audio = audio / 32768.0
            prepared.append(audio)
        return prepared

    def _planar(self, clips, channels, level):
        """The clips of a call -> (float [C_i, T_i] arrays, the int16 rule (max > 1 -> / 32768) applied once per clip; plain).
        plain: every clip mono and level='peak' (what resolve_clips hands back as it came).  It is read by the front end
        (_prepare_rows) and by the post-processor's level arguments (_level_args); nothing else asks whether a clip is mono."""
        clips, planar = resolve_clips(clips, channels, level)
        if planar is None:
            return [a[None] for a in self._host_clips(clips)], True
        return planar, False

    def _prepare_rows(self, rows, sr, plain, ragged=False):
        """The front end: 1-D float rows (one per channel of every clip, the int16 rule applied already; equal lengths, one
        rate) -> (cond [R, T48] float32 on the device, every row divided by its peak p; gains float32 [R] on the device: p).
        ragged: rows of different lengths, sr one input rate or one per row -> (list of [T48_i] views of one packed device
        buffer, gains), every row the bits of the batched form on that row alone.  'hip': the resampler's launches (their
        segment forms with ragged); 'scipy': resampled and normalised on the host per row, one upload.
        A silent row is divided by 1 and has gain 0: 'hip' keeps the peaks on the device (fh_channel_peaks_f32), 'scipy' uploads
        the host's np.max(np.abs(.)).  plain: the default path's front end -- the peak as it is (a silent clip is 0 / 0), no
        fh_channel_peaks_f32, gains None."""
        if self.upsampling_method == 'scipy':
            import scipy.signal
            conds, peaks = [], []
            for audio, sr_i in zip(rows, resolve_rates(sr, len(rows)) if ragged else [sr] * len(rows)):
                cond = scipy.signal.resample_poly(audio, 48000, sr_i)
                p = np.max(np.abs(cond))
                peaks.append(p)
                conds.append(cond / p if plain or p > 0 else cond)
            gains = None if plain else self._upload(torch.from_numpy(np.array(peaks, dtype=np.float32)))
            if ragged:
                return self.resampler.upload_packed(conds)[1], gains
            return self._upload(torch.stack([torch.tensor(cond).float() for cond in conds])), gains
        if self.upsampling_method == 'hip':
            if ragged:
                out = self.resampler.ragged(rows, sr, 48000, gains=not plain)
                return out[1], (None if plain else out[2])
            x = self._upload(torch.from_numpy(np.stack([np.asarray(a, dtype=np.float32) for a in rows])))
            out = self.resampler(x, sr, 48000, gains=not plain)
            return (out, None) if plain else out
        raise UnboundLocalError(f"cond: unsupported upsampling_method '{self.upsampling_method}'")

    def _level_args(self, chans, level, gains, plain):
        """The post-processor's gains= and groups= for rows that are chans[i] channels per clip.  plain: none, it ends with
        the per-row 0.99 peak.  level='input': the rows' gains, no groups.  level='peak': every clip is a group; a mono clip
        among them takes gain 1, which makes its row gain and its group peak the identity (w * 1, fl(q * 1)): it keeps the bits
        of a plain call."""
        if plain:
            return {}
        if level != "peak":
            return dict(gains=gains, groups=None)
        group = np.repeat(np.arange(len(chans), dtype=np.int32), chans)
        if 1 in chans:
            mono = self._upload(torch.from_numpy(np.repeat(np.array(chans) == 1, chans)))
            gains = gains.masked_fill(mono, 1.0)
        return dict(gains=gains, groups=self._upload(torch.from_numpy(group)))

    def _prior_scale(self):
        """std_2 = 1 of independent_cfm_adaptive as _sample's keyword (flowhighsr.py:88-96 of the reference)."""
        return dict(std_2=1.) if self.cfm_method == 'independent_cfm_adaptive' else {}

    def _generate_rows(self, planar, sr, timestep, noises, keys, generator, level, plain, return_stages=False, first_frames=None):
        """The batch body of every entry: clips of equal length and one rate as planar float [C_i, T] arrays with their plain
        flag (_planar), noises = None or one [C_i, N, n_mels] per clip (clip_noises), keys = None or one key per clip.  Every
        channel is a row of the batch and runs as a mono clip does; the rows of a clip share its prior (first_frames, with
        keys: the absolute frame every clip's prior starts at, _device_prior).  -> [sum C_i, T48] (rows in clip order; a fresh
        tensor), with return_stages also the stages of the rows (and, unless plain, their gains)."""
        chans = [a.shape[0] for a in planar]
        noise = row_keys = None
        if keys is not None:
            row_keys = [k for k, c in zip(keys, chans) for _ in range(c)]
            if first_frames is not None:
                first_frames = [f for f, c in zip(first_frames, chans) for _ in range(c)]
        else:
            if noises is None:                               # one draw per CLIP, in clip order, whatever its channels
                n = resample_out_len(planar[0].shape[1], 48000, sr) // 480
                noises = [channel_noise(self._draw_noise(1, n, generator), c) for c in chans]
            noise = torch.cat(list(noises), 0)
        cond, gains = self._prepare_rows([row for a in planar for row in a], sr, plain)
        wav = self._sample(cond=cond, time_steps=timestep, cfm_method=self.cfm_method, noise=noise, keys=row_keys,
                           first_frames=first_frames if keys is not None else None, **self._prior_scale()).squeeze(1)
        out = self.postproc(wav, cond, cond.size(-1), return_cr=return_stages, **self._level_args(chans, level, gains, plain))
        if return_stages:                                    # (wav and cr are plan- and workspace-owned buffers)
            return out[0], dict(cond=cond, wav=wav.clone(), cr=out[1].clone(), **({} if gains is None else dict(gains=gains)))
        return out

    # ---- sampler (cfm_superresolution.py:162-284) ------------------------------------------------
    def _draw_noise(self, batch, n_frames, generator):
        n_mels = self.flowhigh.n_mels
        return torch.cat([reference_prior_draw(n_frames, n_mels, generator) for _ in range(batch)], 0)

    def _prior_keys(self, seed, n_clips, generator=None, noise=None):
        """The (seed, stream) key of every clip of a call, or None where the call does not draw on the device (a
        prior='reference' model, or an explicit noise=, which always wins).  seed=: prior.expand_seed.  No seed=: one
        torch.randint per clip from `generator` (torch's global one when None), in clip order, stream 0 -- so
        torch.manual_seed / generator= make runs reproducible and a list consumes the generator as a loop over its clips does."""
        if self.prior != 'device':
            if seed is not None:
                raise ValueError("seed= names a key of the device prior: construct the model with prior='device' "
                                 "(a prior='reference' model draws from generator=)")
            return None
        keys = expand_seed(seed, n_clips) if seed is not None else None
        if noise is not None:
            return None
        if keys is None:
            keys = [normalize_key(int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator)), 0) for _ in range(n_clips)]
        return keys

    def _device_prior(self, keys, n_seg, n, seg=None, rows=None, first_frames=None):
        """fh_prior_normal_f32: [n_seg * n, n_mels] noise rows of the keys (a list of (seed, stream), or a device int64
        [n_seg, 2]); seg: the ragged segment table, rows = its total.  first_frames (a list of ints, or a device int64 [n_seg]):
        clip b's rows are rows first_frames[b] .. of its key's stream (fh_prior_normal_at_f32; the windows of a streaming session)."""
        if not isinstance(keys, torch.Tensor):
            host = np.array([[k[0], k[1]] for k in keys], dtype=np.uint64).view(np.int64)
            keys = self._upload(torch.from_numpy(host))
        if keys.shape != (n_seg, 2) or keys.dtype != torch.int64 or not keys.is_contiguous():
            raise ValueError(f"keys must be a contiguous int64 [{n_seg}, 2], got {keys.dtype} {tuple(keys.shape)}")
        d = self.flowhigh.n_mels
        out = torch.empty(n_seg * n if rows is None else rows, d, dtype=torch.float32, device=self.device)
        if first_frames is None:
            hip.check(hip.lib().fh_prior_normal_f32(out.data_ptr(), keys.data_ptr(), hip.ptr(seg), n_seg, n, d, hip.stream()),
                      "fh_prior_normal_f32")
            return out
        if not isinstance(first_frames, torch.Tensor):
            if min(int(f) for f in first_frames) < 0:
                raise ValueError(f"first_frames must be non-negative, got {list(first_frames)}")
            first_frames = self._upload(torch.tensor([int(f) for f in first_frames], dtype=torch.int64))
        if first_frames.shape != (n_seg,) or first_frames.dtype != torch.int64 or not first_frames.is_contiguous():
            raise ValueError(f"first_frames must be a contiguous int64 [{n_seg}], got {first_frames.dtype} {tuple(first_frames.shape)}")
        hip.check(hip.lib().fh_prior_normal_at_f32(out.data_ptr(), keys.data_ptr(), first_frames.data_ptr(), hip.ptr(seg), n_seg, n, d,
                                                   hip.stream()), "fh_prior_normal_at_f32")
        return out

    @torch.no_grad()
    @hip.on_device
    def draw_prior(self, frames, seed, *, stream=0, first_frame=0):
        """The noise a prior='device' call with that key uses, as a device tensor (read it back to rebuild a call with noise=,
        or to hand it to the oracle; prior.prior_normal_host gives the same values without a GPU).
        frames = N, seed = s            -> [1, N, n_mels]: key (s, stream)
        frames = N, seed = [s_0, ...]   -> [len(seed), N, n_mels]: clip i's key (an int s_i = (s_i, stream), or a pair)
        frames = [N_0, N_1, ...]        -> a list of [1, N_i, n_mels] (the ragged form, one launch); seed an int s = keys
                                           (s, stream + i) as seed=s gives a call over the list, or one item per clip.
        first_frame = f (the uniform forms): rows f .. f + N of the keys' streams, what window i of a streaming session draws
        at f = its first absolute frame (stream.py)."""
        ragged = not isinstance(frames, (int, np.integer))
        count = len(frames) if ragged else (1 if isinstance(seed, (int, np.integer)) else len(seed))
        if isinstance(seed, (int, np.integer)):
            keys = [normalize_key(seed, stream + i) for i in range(count)]
        else:
            keys = [normalize_key(s_, stream) if isinstance(s_, (int, np.integer)) else k
                    for k, s_ in zip(expand_seed(seed, count), seed)]
        if not ragged:
            at = None if not first_frame else [int(first_frame)] * count
            return self._device_prior(keys, count, int(frames), first_frames=at).view(count, int(frames), -1)
        if first_frame:
            raise ValueError("first_frame= goes with one frame count, not with a list of them")
        frames = [int(n) for n in frames]
        seg = self.flowhigh.net.ragged_workspace(frames)["seg"]
        z = self._device_prior(keys, count, max(frames), seg=seg, rows=sum(frames))
        return [v[None] for v in _views(z, _starts(frames), frames)]

    def _cutoff_bins(self, cond_mel, n_seg, n, seg=None):
        """int32 [n_seg] cutoff bin of every clip, two launches: n_seg clips of n rows, or (seg: the device segment table)
        clips of different lengths packed back to back."""
        L, st = hip.lib(), hip.stream()
        d = cond_mel.shape[-1]
        energy = torch.empty(n_seg, d, dtype=torch.float32, device=self.device)
        cut = torch.empty(n_seg, dtype=torch.int32, device=self.device)
        if seg is None:
            hip.check(L.fh_mel_energy_f32(cond_mel.data_ptr(), energy.data_ptr(), n_seg, n, d, st), "fh_mel_energy_f32")
        else:
            hip.check(L.fh_mel_energy_seg_f32(cond_mel.data_ptr(), energy.data_ptr(), seg.data_ptr(), n_seg, d, st),
                      "fh_mel_energy_seg_f32")
        hip.check(L.fh_cutoff_index_f32(energy.data_ptr(), cut.data_ptr(), n_seg, d, 0.9995, st), "fh_cutoff_index_f32")
        return cut

    @hip.on_device
    def mel_cutoff_bins(self, cond_mel, batch, n):
        """Device version of mel_cutoff_bins (cfm:134-159): int32 [B], no host loop, no sync."""
        return self._cutoff_bins(cond_mel, batch, n)

    def _mel_replace(self, high, low, cut, n_seg, n, seg=None):
        """out = bins below cut[clip] from low, the others from high; seg as in _cutoff_bins (n: then the longest clip's rows)."""
        L, st = hip.lib(), hip.stream()
        out = torch.empty_like(high)
        args = (low.data_ptr(), high.data_ptr(), cut.data_ptr(), out.data_ptr())
        if seg is None:
            hip.check(L.fh_mel_splice_f32(*args, n_seg, n, high.shape[-1], st), "fh_mel_splice_f32")
        else:
            hip.check(L.fh_mel_splice_seg_f32(*args, seg.data_ptr(), n_seg, n, high.shape[-1], st), "fh_mel_splice_seg_f32")
        return out

    def _sample_rows(self, cond_mel, noise, keys, n_seg, n, time_steps, cfm_method, std_1, std_2, cond_scale, mel_pp, ragged=None,
                     first_frames=None):
        """The sampler behind the log-mel (cfm:176-279) on token-major rows: n_seg clips of n rows, or (ragged: the net's
        ragged workspace) clips of different lengths packed back to back, n = the longest.  cond_mel, noise [rows, n_mels] on
        the device; noise None: drawn on the device from the clips' keys (first_frames: _device_prior).  Returns the mel rows."""
        if cfm_method in _CFM_METHODS[1:]:
            if std_1 is None or std_2 is None:          # cfm:180-183 (resets BOTH; generate() never passes std_1)
                std_1, std_2 = 1.0, self.sigma
        seg = ragged["seg"] if ragged is not None else None
        if noise is None:                               # prior='device': drawn where it is used
            noise = self._device_prior(keys, n_seg, n, seg=seg, rows=cond_mel.shape[0], first_frames=first_frames)
        cut = None
        if cfm_method == 'basic_cfm':
            y0 = noise
        else:
            y0 = torch.empty_like(noise)                # cond * std_1 + eps * std_2
            hip.check(hip.lib().fh_axpby_f32(cond_mel.data_ptr(), float(std_1), noise.data_ptr(), float(std_2),
                                             y0.data_ptr(), y0.numel(), hip.stream()), "fh_axpby_f32")
            if cfm_method == 'independent_cfm_mix':     # cfm:231-237, cutoff bins per clip
                cut = self._cutoff_bins(cond_mel, n_seg, n, seg)
                y0 = self._mel_replace(noise, y0, cut, n_seg, n, seg)
        mel = integrate.solve(self.flowhigh.net, self.odeint_kwargs['method'], y0, cond_mel, n_seg, n, time_steps, float(cond_scale),
                              ragged=ragged)
        if mel_pp:                                      # cfm:278-279, per clip
            cut = cut if cut is not None else self._cutoff_bins(cond_mel, n_seg, n, seg)
            mel = self._mel_replace(mel, cond_mel, cut, n_seg, n, seg)
        return mel

    @torch.no_grad()
    @hip.on_device
    def sample(self, *, cond=None, cond_mask=None, time_steps=4, cond_scale=1., decode_to_audio=True,
               std_1=None, std_2=None, mel_pp=False, cfm_method=None, noise=None, generator=None, seed=None):
        """The reference's `sample` (cfm:162-284).  The returned tensor is the caller's own (the vocoder's output
        buffer belongs to a per-shape launch plan and is overwritten by the next call of the same shape, so the
        public entry hands out a copy; `generate*` read the plan's buffer in place).  seed=: _prior_keys."""
        keys = self._prior_keys(seed, cond.shape[0], generator, noise)
        out = self._sample(cond=cond, cond_mask=cond_mask, time_steps=time_steps, cond_scale=cond_scale,
                           decode_to_audio=decode_to_audio, std_1=std_1, std_2=std_2, mel_pp=mel_pp,
                           cfm_method=cfm_method, noise=noise, generator=generator, keys=keys)
        return out.clone() if decode_to_audio else out

    def _sample(self, *, cond=None, cond_mask=None, time_steps=4, cond_scale=1., decode_to_audio=True,
                std_1=None, std_2=None, mel_pp=False, cfm_method=None, noise=None, generator=None, keys=None, first_frames=None):
        if cfm_method not in _CFM_METHODS:
            cfm_method = self.cfm_method
        if cond_mask is not None:
            raise NotImplementedError("cond_mask is a training-time option (SURVEY.md 8a row 2)")
        fh = self.flowhigh
        cond = cond.to(self.device, torch.float32)
        if cond.ndim == 2 or (cond.ndim == 3 and cond.shape[1] == 1):      # raw audio (cfm:91-92,185)
            if cond.ndim == 3:
                cond = cond.squeeze(1)
            batch = cond.shape[0]
            cond_mel = fh.logmel(cond)
            n = cond_mel.shape[0] // batch
        else:
            batch, n, _ = cond.shape
            cond_mel = cond.reshape(batch * n, -1).contiguous()
        if noise is not None or keys is None:
            if noise is None:
                noise = self._draw_noise(batch, n, generator)
            noise = self._upload(noise.to(torch.float32)).reshape(batch * n, -1).contiguous()
        mel = self._sample_rows(cond_mel, noise, keys, batch, n, time_steps, cfm_method, std_1, std_2, cond_scale, mel_pp,
                                first_frames=first_frames)
        mel = mel.view(batch, n, -1)
        if not decode_to_audio:
            return mel
        return fh.vocoder.forward(mel).unsqueeze(1)           # [B, 1, hop * n]

    def _sample_ragged(self, conds, time_steps, cfm_method, noises=None, std_1=None, std_2=None, mels=None, cond_scale=1.,
                       mel_pp=False, decode_to_audio=True, keys=None, cond_mel=None):
        """`sample()` (cfm:162-284, incl. cond_scale != 1 and mel_pp, cfm:162-175,278-279) for clips of DIFFERENT
        lengths as one launch sequence.
        conds: list of [T48_i] device tensors (peak-normalised), noises: list of [1, N_i, n_mels] host tensors, or None and
        keys = the clips' (seed, stream) keys: the prior is then drawn on the device, one launch over the segment table.
        time_steps: one count, or a list of one count per clip, sorted descending (at most 8 distinct: integrate.solve).
        Returns the vocoder's waveforms, a list of [1, 480 N_i] (plan-owned buffers; decode_to_audio=False: the mels,
        a list of [N_i, n_mels]), each what _sample gives for that clip alone: the log-mels are made per clip, every
        row-wise operator runs on the packed rows, the operators that look across rows take the clip boundaries (the
        mel cutoff bins are per clip: fh_mel_*_seg_f32), the vocoder runs its merged plan.
        cond_mel (with mels = its per-clip views; ends='ragged'): the clips' log-mels packed already (LogMel.ragged); nothing
        is concatenated and the vocoder takes the packed result (forward_ragged_packed)."""
        fh = self.flowhigh
        if mels is None:
            mels = [fh.logmel(c[None]) for c in conds]       # [N_i, n_mels] each
        frames = [m.shape[0] for m in mels]
        packed = cond_mel is not None
        if not packed:
            cond_mel = torch.cat(mels, 0)
        noise = None
        if noises is not None:
            noise = self._upload(torch.cat([z.reshape(-1, z.shape[-1]).to(torch.float32) for z in noises], 0)).contiguous()
            if noise.shape != cond_mel.shape:
                raise ValueError(f"noise rows {tuple(noise.shape)} do not match the clips' frames {tuple(cond_mel.shape)}")
        mel = self._sample_rows(cond_mel, noise, keys, len(frames), max(frames), time_steps, cfm_method, std_1, std_2, cond_scale,
                                mel_pp, ragged=fh.net.ragged_workspace(frames))
        if packed and decode_to_audio:
            return fh.vocoder.forward_ragged_packed(mel, frames)
        out = _views(mel, _starts(frames), frames)
        return fh.vocoder.forward_ragged(out) if decode_to_audio else out

    @torch.no_grad()
    @hip.on_device
    def sample_many(self, conds, *, time_steps=4, cond_scale=1., decode_to_audio=True, std_1=None, std_2=None, mel_pp=False,
                    cfm_method=None, noise=None, generator=None, seed=None):
        """`sample()` for a LIST of conditioning clips of different lengths (each [T48_i], 48 kHz, peak-normalised) as
        one masked / ragged launch sequence, with the reference's sampler options (cond_scale: classifier-free
        guidance against null_cond, mel_pp: low-band replacement with per-clip cutoff bins, std_1 / std_2: prior scales of the
        independent_cfm_* paths, both reset unless both are given; cfm:162-183,278-279).
        Every result is bit-identical to `sample(cond=clip[None], ...)` on that clip alone.  Returns a list of
        [1, 1, 480 N_i] waveforms (or [1, N_i, n_mels] mels).
        time_steps: one count, or one count per clip (generate_many's timestep=): clip i is then `sample(..., time_steps=steps[i])`."""
        if cfm_method not in _CFM_METHODS:
            cfm_method = self.cfm_method
        conds = list(conds)
        time_steps = ode.check_steps(time_steps, len(conds), "time_steps")
        keys = self._prior_keys(seed, len(conds), generator, noise)
        conds = [c.to(self.device, torch.float32).reshape(-1) for c in conds]
        frames = [c.shape[0] // 480 for c in conds]
        if noise is None and keys is None:
            noise = [self._draw_noise(1, n, generator) for n in frames]
        if isinstance(time_steps, list):
            # one step count per clip: the clips sorted by count (descending, stable) into sequences of at most 8 distinct counts
            # (one count each on the convnext backbone, which has no grouped form), the results put back in list order
            limit = ode.MAX_STEP_GROUPS if self.flowhigh.net.grouped_field else 1
            seqs = ode.step_sequences(list(range(len(conds))), time_steps, limit)
        else:
            seqs = [(list(range(len(conds))), time_steps)]
        result = [None] * len(conds)
        for idx, steps in seqs:
            outs = self._sample_ragged([conds[i] for i in idx], steps, cfm_method, noises=None if noise is None else [noise[i] for i in idx],
                                       std_1=std_1, std_2=std_2, cond_scale=cond_scale, mel_pp=mel_pp, decode_to_audio=decode_to_audio,
                                       keys=None if keys is None else [keys[i] for i in idx])
            for i, o in zip(idx, outs):
                result[i] = o.clone().unsqueeze(1) if decode_to_audio else o.clone()[None]
        return result

    @torch.no_grad()
    @hip.on_device
    def generate_batch(self, clips, sr, target_sampling_rate=48000, timestep=1, *, noise=None,
                       generator=None, return_stages=False, seed=None, channels=None, level='peak',
                       output_rate=None, pcm=None, dither=None, dither_seed=0, interleaved=False, loudness=None,
                       true_peak=None, limiter=None):
        """B clips of equal length as one batch -> [B, T48], every clip what generate() returns for it alone.
        timestep: one step count, or one per clip (generate_many); mixed counts run one batch per distinct count.
        channels=, level= (generate): with channels= every clip may have its own number of channels and the result is a list
        of [C_i, T48]; noise= is then one tensor per clip in a list ([1, N, n_mels] shared by the clip's channels, or
        [C_i, N, n_mels]), or [B, N, n_mels]: one shared draw per clip.
        output_rate=, pcm=, dither=, dither_seed=, interleaved= (generate): the same shapes at the output rate, int16 with
        pcm=; interleaved=True gives [B, T, 1] without channels=, a list of [T, C_i] with it.  loudness= (generate): every clip
        at that many LUFS, each by its own gain.  true_peak=, limiter= (generate): every clip under that ceiling in dBTP, each by
        its own gain or its own limiter gain."""
        planar, plain = self._planar(list(clips), channels, level)
        n_clips, chans = len(planar), [a.shape[0] for a in planar]
        opt = resolve_delivery(n_clips, output_rate, pcm, dither, dither_seed, interleaved, loudness=loudness, level=level,
                               true_peak=true_peak, limiter=limiter)
        if opt is not None and return_stages:
            raise ValueError("return_stages=True returns the 48 kHz stages: it does not go with output_rate= / pcm= / loudness= / "
                             "true_peak=")
        timestep = ode.check_steps(timestep, n_clips)
        if isinstance(timestep, list) and return_stages:
            raise ValueError("return_stages=True returns the stages of one batch: it does not go with one step count per clip")
        keys = self._prior_keys(seed, n_clips, generator, noise)
        if target_sampling_rate != 48000:
            raise NotImplementedError("the mel codec is fixed at 48 kHz")
        if isinstance(timestep, list):
            # one step count per clip: one batch per distinct count (the clips are of one shape), the rows put back in clip
            # order; the host prior is drawn first, in clip order, as the one batch draws it
            noises = clip_noises(noise, chans)
            if noises is None and keys is None:
                n = resample_out_len(planar[0].shape[1], 48000, sr) // 480
                noises = [channel_noise(self._draw_noise(1, n, generator), c) for c in chans]
            parts = [None] * n_clips
            for count in sorted(set(timestep)):
                idx = [i for i, s in enumerate(timestep) if s == count]
                y = self._generate_rows([planar[i] for i in idx], sr, count, None if noises is None else [noises[i] for i in idx],
                                        None if keys is None else [keys[i] for i in idx], None, level, plain)
                for i, rows_i in zip(idx, y.split([chans[i] for i in idx])):
                    parts[i] = rows_i
            out = torch.cat(parts, 0)
        else:
            out = self._generate_rows(planar, sr, timestep, clip_noises(noise, chans), keys, generator, level, plain, return_stages)
        rows, stages = out if return_stages else (out, None)
        if opt is not None:
            # (without channels= every clip is one row: the delivered buffer itself is the [B, T] result)
            return self.delivery.batch(rows, chans, level, opt, range(n_clips), packed=channels is None)
        if channels is not None:
            rows = list(rows.split(chans))
        return (rows, stages) if return_stages else rows

    @torch.no_grad()
    @hip.on_device
    def generate_many(self, clips, sr, target_sampling_rate=48000, timestep=1, *, noise=None, generator=None,
                      max_batch=64, streams=None, ragged=None, max_frames=None, seed=None, ends=None, channels=None,
                      level='peak', output_rate=None, pcm=None, dither=None, dither_seed=0, interleaved=False, loudness=None,
                      true_peak=None, limiter=None):
        """Serving-side entry (the gradio caller of app.py:8-26, many requests at once): clips of ANY lengths,
        int16 or float.  Clips of equal length run as one batch (at most max_batch rows), so every result is
        what generate() returns for that clip alone; the prior noise is drawn in the order of `clips`, as a loop
        over generate() would.  noise: optional list of [1, N_i, n_mels] tensors.  Returns a list of [1, T48_i].
        sr: the input rate of every clip, or a sequence of one rate per clip (resolve_rates): clips of different input rates run
        in the same launch sequences (everything behind the resampler works at 48 kHz), every result what generate(clip_i, sr_i)
        returns; two clips are one shape when length AND rate agree.  With ends='ragged' the resampling of a group is one launch
        with a polyphase filter per clip (fh_resample_poly_rates_seg_f32); profiles/mixed_rates.md has the measurement.
        On a prior='device' model nothing is drawn on the host: every clip has a (seed, stream) key (seed=, or one
        torch.randint per clip from the generator, in the order of `clips`: _prior_keys) and the launch sequences draw from them.
        ragged (default on, FH_RAGGED=0 switches it off): clips of different lengths run as ONE launch sequence
        (masked / ragged batch, the reference's mask paths transformer.py:35-44, attend.py:127-128): ~120 launches for
        the whole list instead of ~120 per distinct length; at most max_frames (FH_RAGGED_MAX_FRAMES, default 12 000 =
        120 s of audio) frames per sequence; clips too long for that (or for the unchunked vocoder) run alone.
        Results are bit-identical to generate() per clip either way.
        ends ('per_clip' | 'ragged'; None: FH_RAGGED_ENDS, else 'per_clip'): what surrounds the launch sequence of a ragged
        group of two or more clips -- resampling and peak normalisation, log-mel, the vocoder's input copies, post-processing.
        'per_clip' runs them once per clip (~18 launches each); 'ragged' runs their segment forms (fh_*_seg_f32, csrc/frontend.hip), one
        launch per step for the whole group, out of workspaces kept per mix of lengths; same bits per clip.
        streams (ragged off): batches of different FRAME COUNTS can be enqueued round-robin on several HIP streams (FH_SERVE_STREAMS,
        default 1), so that the launches of a short clip - a few dozen blocks each, a fraction of the 256 CUs - overlap
        with those of the next one.  The per-shape workspaces are keyed by (batch, frames): two input lengths with the
        same frame count (6000 and 6001 samples at 12 kHz: 50 frames both) share them, so every bucket of one frame
        count runs on the same stream, in order; results do not depend on `streams`.  Measured on a
        mix of 0.5-4 s clips: between -15 % and +40 % of the single-stream time from run to run (the host enqueues
        ~120 launches per clip and is the bottleneck either way), hence off by default.
        channels=, level= (generate): every clip may have its own number of channels; the result list then holds one [C_i, T48_i]
        per clip.  A clip's channels are rows of the same batch or ragged sequence (a clip of C channels costs what C clips
        cost), share the clip's prior -- noise[i] is [1, N_i, n_mels], or [C_i, N_i, n_mels] for a draw per channel -- and a
        clip gives the same bits alone, in a batch, in a ragged group and under either `ends`.
        output_rate=, pcm=, dither=, dither_seed=, interleaved= (generate): every result delivered at the output rate / as
        int16 ([C_i, T_i], or [T_i, C_i] interleaved).  A batch of equal clips goes through the batched entries, a ragged group
        through their segment forms, one launch per step over the group, reading the rows where the post-processor left
        them; dither_seed=s gives clip i the key (s, i), or it holds one int / (seed, stream) pair per clip.  A clip's result
        does not depend on how it ran.
        loudness= (generate): every clip at that many LUFS at the delivered rate, each by its own gain; a batch of equal clips
        through the batched entries of csrc/loudness.hip, a ragged group through their segment forms, the same bits either way.
        true_peak=, limiter= (generate): every clip under that ceiling in dBTP, through the batched entries of csrc/truepeak.hip or
        their segment forms, the same bits either way.
        timestep: one step count for the list, or ONE COUNT PER CLIP -- generate_many(clips, sr, 48000, [1, 4, 2, ...]); a list of
        another length than `clips`, or an entry that is no int >= 1 (a bool, a float, 0) is a ValueError before any GPU work
        (ode.check_steps).  A list of equal counts is the int, and an int runs what it always ran.  Mixed counts run as ragged
        sequences with a time and a step size per clip (integrate.py, csrc/steps.hip): the clips of a ragged group sorted by
        count, descending and stable, max(steps) passes over a shrinking prefix of the rows, at most 8 distinct counts per
        sequence (a group with more is cut into several), the results back in list order; priors, keys and dither keys stay
        tied to a clip's place in the list.  Clip i is bit for bit generate(clip_i, sr_i, timestep=steps[i]), with every option
        above.  One batch per (length, rate, noise shape, step count) instead: ragged=False / FH_RAGGED=0, the convnext
        backbone, a vocoder configuration whose plan cannot be merged.  profiles/mixed_steps.md has the measurement."""
        clips = list(clips)
        ends = resolve_ends(ends)
        timestep = ode.check_steps(timestep, len(clips))      # (an int, or a list of one count per clip that are not all equal)
        mixed = isinstance(timestep, list)
        rates = resolve_rates(sr, len(clips))
        opt = resolve_delivery(len(clips), output_rate, pcm, dither, dither_seed, interleaved, loudness=loudness, level=level,
                               true_peak=true_peak, limiter=limiter)
        planar, plain = self._planar(clips, channels, level)
        chans, lengths = [a.shape[0] for a in planar], [a.shape[1] for a in planar]
        if target_sampling_rate != 48000:
            raise NotImplementedError("the mel codec is fixed at 48 kHz")
        if noise is not None:
            for z, c in zip(noise, chans):
                channel_noise(z, c)                      # (a wrong leading dimension: a ValueError before any GPU work)
        keys = self._prior_keys(seed, len(clips), generator, noise)
        if noise is None:
            frames = [resample_out_len(n_in, 48000, sr_i) // 480 for n_in, sr_i in zip(lengths, rates)]
            if keys is None:
                noise = [self._draw_noise(1, n, generator) for n in frames]
        if noise is not None and len(noise) != len(clips):
            raise ValueError("one noise tensor per clip")
        # the shape of every clip's noise: given or drawn on the host, or what the device draws from the clip's key
        shapes = [tuple(z.shape) for z in noise] if noise is not None else [(1, n, self.flowhigh.n_mels) for n in frames]
        if ragged is None:
            ragged = os.environ.get("FH_RAGGED", "1") != "0"
        # mixed step counts run as ragged sequences with a time per clip (integrate.py) -- clips of one shape included -- where
        # the vector field has the grouped form; the convnext backbone (its time-conditioned LayerNorm takes one time), ragged
        # off and an unmergeable vocoder plan run one batch per (shape, step count) below
        if ragged and (len(set(zip(lengths, rates))) > 1 if not mixed else self.flowhigh.net.grouped_field):
            try:
                return self._generate_many_ragged(planar, rates, timestep, noise, max_frames, keys, [sh[1] for sh in shapes], ends,
                                                  level, plain, opt)
            except NotImplementedError as e:
                # a vocoder configuration whose launch positions cannot be merged: one batch per length (said once)
                if not getattr(self, "_ragged_fallback_logged", False):
                    self._ragged_fallback_logged = True
                    import logging
                    logging.getLogger("flowhigh_amd").warning("generate_many: ragged launch sequence not available (%s); "
                                                              "running one batch per clip length", e)
        if streams is None:
            streams = int(os.environ.get("FH_SERVE_STREAMS", "1"))
        n_streams, parts = plan_buckets(lengths, rates, shapes, streams, max_batch, steps=timestep if mixed else None)
        main = torch.cuda.current_stream(self.device)
        side = self._serve_streams(n_streams) if n_streams > 1 else [main]
        for s_ in side:
            if s_ is not main:
                s_.wait_stream(main)
        out = [None] * len(clips)
        for s_, rate, part in parts:                         # (max_batch counts clips: a clip's channels stay in one batch)
            with torch.cuda.stream(side[s_]):
                steps = timestep[part[0]] if mixed else timestep          # (a bucket holds one step count)
                for i, y in zip(part, self._run_clips(planar, part, rate, steps, noise, keys, level, plain, opt)):
                    out[i] = y.clone() if opt is None else y
                    if side[s_] is not main:
                        out[i].record_stream(main)
        for s_ in side:
            if s_ is not main:
                main.wait_stream(s_)
        return out

    def _run_clips(self, planar, idx, rate, timestep, noise, keys, level, plain, opt):
        """The clips idx of a generate_many call (equal lengths, one rate) as one batch, delivered if opt says so -> one
        [C_i, T] result per clip: views of the batch's fresh rows, or what Delivery.batch returns."""
        chans = [planar[i].shape[0] for i in idx]
        y = self._generate_rows([planar[i] for i in idx], rate, timestep,
                                clip_noises([noise[i] for i in idx], chans) if keys is None else None,
                                [keys[i] for i in idx] if keys is not None else None, None, level, plain)
        return y.split(chans) if opt is None else self.delivery.batch(y, chans, level, opt, idx)

    def _generate_many_ragged(self, planar, rates, timestep, noise, max_frames, keys, frames, ends, level, plain, opt):
        """generate_many's ragged path.  planar, plain: _planar's pair; rates: the input rate of every clip (resolve_rates);
        frames: every clip's frame count; clip i is C_i rows of frames[i] frames in its sequence.  opt: resolve_delivery's
        result; a clip that runs alone is delivered by the batched entries, a group by the segment forms."""
        if max_frames is None:
            max_frames = int(os.environ.get("FH_RAGGED_MAX_FRAMES", "12000"))
        chunk_limit = int(os.environ.get("FH_VOCODER_CHUNK_FRAMES", "6000"))
        # greedy packing in list order; a clip that does not fit a sequence, or has one to itself, runs as a batch of one
        groups, alone = pack_ragged(frames, [a.shape[0] for a in planar], max_frames, chunk_limit)
        steps_of = (lambda i: timestep[i]) if isinstance(timestep, list) else (lambda i: timestep)
        # mixed step counts in a group: its clips sorted by count, descending and stable, cut into sequences of at most 8 distinct
        # counts (one launch of csrc/steps.hip takes 8 groups).  idx carries the clips' places in the caller's list through the
        # run and the delivery: priors, keys and dither keys stay tied to them, the results go back by them
        seqs = [seq for idx in groups for seq in ode.step_sequences(idx, [steps_of(i) for i in idx])]
        out = [None] * len(planar)
        for idx, steps in [([i], steps_of(i)) for i in alone] + seqs:
            if len(idx) == 1:
                (out[idx[0]],) = self._run_clips(planar, idx, rates[idx[0]], steps, noise, keys, level, plain, opt)
                continue
            # a group's 48 kHz results are the caller's own without delivery, else still workspace-owned where delivery reads them
            ys = self._ragged_group_rows([planar[i] for i in idx], [rates[i] for i in idx], steps,
                                         [noise[i] for i in idx] if keys is None else None,
                                         [keys[i] for i in idx] if keys is not None else None, ends, level, plain, own=opt is None)
            if opt is not None:
                ys = self.delivery.ragged(ys, level, opt, idx)
            for i, y in zip(idx, ys):
                out[i] = y
        return out

    def _ragged_group_rows(self, planar, rates, timestep, noises, keys, ends, level, plain, own=True):
        """One ragged group: every channel of every clip is a row of the sequence, the rows of a clip are adjacent and share
        its prior, and unless plain the post-processor gets the rows' gains and (level='peak') their clip as their group.
        -> list of [C_i, T48_i], each the bits of _generate_rows on that clip alone.  ends='ragged': front and back end as
        segment-form launches over the group, the results views of the post-processor's workspace (own: of one copy of it);
        'per_clip': the batched entries once per clip (on up to 4 side streams they measured 121.5 ms against 121.3 ms on one
        for a 24-clip mix: not worth the cross-stream bookkeeping), the results fresh tensors."""
        chans = [a.shape[0] for a in planar]
        if isinstance(timestep, (list, tuple)):              # (one count per clip, sorted descending: a clip's rows share its count)
            timestep = [s for s, c in zip(timestep, chans) for _ in range(c)]
        if keys is not None:
            prior = dict(keys=[k for k, c in zip(keys, chans) for _ in range(c)], **self._prior_scale())
        else:
            prior = dict(noises=[z[None] for zs, c in zip(noises, chans) for z in channel_noise(zs, c)], **self._prior_scale())
        if ends == "ragged":
            rows = [row for a in planar for row in a]
            conds, gains = self._prepare_rows(rows, [r for r, c in zip(rates, chans) for _ in range(c)], plain, ragged=True)
            cond_mel, mels = self.flowhigh.logmel.ragged(conds)
            wavs = self._sample_ragged(conds, timestep, self.cfm_method, mels=mels, cond_mel=cond_mel, **prior)
            packed, _ = self.postproc.ragged(wavs, conds, [c.shape[0] for c in conds], **self._level_args(chans, level, gains, plain))
            if own:
                packed = packed.clone()                      # (the caller's own: one copy for the group, handed out as views)
            # (a clip's rows are adjacent and of one length)
            lens = [c * conds[r].shape[0] for c, r in zip(chans, _starts(chans))]
            return [v.view(c, -1) for v, c in zip(_views(packed, _starts(lens), lens), chans)]
        prepared = [self._prepare_rows(list(a), rate, plain) for a, rate in zip(planar, rates)]      # (cond [C_i, T48_i], gains [C_i])
        wavs = self._sample_ragged([row for cond, _ in prepared for row in cond], timestep, self.cfm_method, **prior)
        # (the vocoder's [1, Tp] buffers: one is read where it lies, a clip's several become its [C_i, Tp] rows)
        return [self.postproc(wavs[r] if c == 1 else torch.cat(list(wavs[r:r + c]), 0), cond, cond.shape[1],
                              **self._level_args([c], level, gains, plain))
                for (cond, gains), c, r in zip(prepared, chans, _starts(chans))]

    # ---- streaming sessions (stream.py is the definition, streaming.py the host side, csrc/stream.hip the seam) ------------------
    def stream(self, sr, *, window_ms=1000, overlap_ms=200, guard_ms=50, timestep=1, seed=None, stream=0, pcm=None,
               channels=None, dither=None, output_rate=None, loudness=None, true_peak=None, delivery=None, n_channels=None):
        """A streaming session at the input rate `sr` (prior='device' models): push(block) returns the samples that block made
        final, float32 [1, n] on the device at 48 kHz (n may be 0), flush() the rest; the blocks of a stream of T input samples
        add up to tables.resample_out_len(T, 48000, sr) samples, equal to stream.stitch of its windows' results bit for bit.
        window_ms / overlap_ms / guard_ms: the StreamPlan (multiples of stream.grain_ms(sr): 10 ms at most rates; overlap >= 20 ms,
        2 overlap <= window, 2 guard < overlap).  Window i is what generate(window_i, sr, level='input') returns with the noise
        of the session's key (seed, stream) at rows i * hop frames on (draw_prior(first_frame=)): consecutive windows share
        their prior where they overlap and are cross-faded there (fh_xfade_seg_f32).  seed=None draws one from torch's generator.
        Latency: a sample is final once the window that holds it left of its right overlap has arrived, at most window_ms after it
        came in, plus one batched run.  The sample format is fixed by the session's first block: an integer dtype is divided by
        32768, a float dtype taken as it is.  pcm='int16' | 's24' | 's24in32' encodes every emitted block (no dither: the encoding is
        stateless; 's24' blocks are uint8 [1, n, 3]).
        delivery=dict(output_rate=, pcm=, dither=, dither_seed=, true_peak=, limiter='lookahead'): what the session emits goes
        through a DeliveryStream (delivery_stream()): the keywords mean what they mean to generate(level='input'), and the blocks
        of the stream add up to the bits of that delivery of the whole 48 kHz stream, delivery.delivered_len(T48, output_rate)
        samples.  The resampler withholds about 10 max(up, down) / up samples at 48 kHz and the limiter 2 H + 10 delivered
        samples (about 10.2 ms) until the flush.  The dither's key is (dither_seed, 0).  delivery= excludes the session's own pcm=;
        it does not take loudness= (a statistic of the whole stream), true_peak= without the limiter (the same), channels=, or,
        in a mono session, interleaved=; a dict of defaults is None.  meter=True in it: the DeliveryStream owns a loudness meter
        (loudness_meter()) fed the float32 samples it makes final, session.delivery.loudness() reads it; the blocks are those of
        the same session without the meter.
        n_channels=C (an int 1 .. 8; None: one mono stream): the stream has C channels, fixed here and never read from a block's
        shape.  Blocks are [C, n] (a block of another row count is a ValueError that leaves the session as it was), push() and
        flush() return [C, m].  Window i is what generate(window_i [C, n], sr, channels='first', level='input') returns under
        the session's prior: the channels share it, each is cross-faded on its own with the one ramp.  pcm='int16' encodes
        planar.  delivery= then delivers C channels (delivery_stream(n_channels=C)): the limiter is channel-linked, channel c
        takes its own dither, and delivery=dict(interleaved=True, pcm='int16', ...) returns sample frames, int16 [m, C].
        n_channels=1 gives [1, n] blocks with the bits of the mono session.
        Not built as keywords of their own, each a ValueError: channels= (the count goes by n_channels=), dither=, output_rate=,
        loudness=, true_peak=."""
        from .streaming import open_session
        return open_session(self, sr, window_ms, overlap_ms, guard_ms, timestep, seed, stream, pcm,
                            dict(channels=channels, dither=dither, output_rate=output_rate, loudness=loudness, true_peak=true_peak),
                            delivery, n_channels)

    def stream_push(self, sessions, blocks):
        """One block per session -> one output block per session (StreamSession.push).  Every window that became runnable, of
        every session with the same (sr, window, overlap, guard, timestep), goes through ONE batched run and one
        fh_xfade_seg_f32 launch -- several windows of one session included; sessions with other plans form further batches.
        A session's output does not depend on what it was pushed with."""
        sessions, blocks = list(sessions), list(blocks)
        if len(sessions) != len(blocks):
            raise ValueError(f"one block per session: {len(blocks)} blocks for {len(sessions)} sessions")
        from .streaming import check_sessions
        check_sessions(self, sessions)                      # (before any block is taken: a refused push leaves every session as it was)
        for s, b in zip(sessions, blocks):
            s._take(b)
        return self._stream_run(sessions, final=False)

    @torch.no_grad()
    @hip.on_device
    def _stream_run(self, sessions, final):
        from .streaming import run
        return run(self, sessions, final)

    def delivery_stream(self, n_channels=None, **keywords):
        """The delivery of a stream on its own: output_rate=, pcm=, dither=, dither_seed=, true_peak=, limiter= as stream(delivery=)
        takes them -> a DeliveryStream: push(block48) takes float32 [1, n] on the device at 48 kHz and returns the delivered
        samples it made final, flush() the rest.  The blocks add up to Delivery.batch of the whole stream at level='input'.
        n_channels=C (an int 1 .. 8; None: the mono stream): push takes [C, n] and returns [C, m], the blocks add up to
        Delivery.batch of the whole [C, T] stream as one clip: the limiter's envelope and gain are one for all channels, channel c
        takes its own dither.  interleaved=True (with n_channels and pcm): int16 sample frames [m, C].  meter=True: the stream owns a
        LoudnessMeter (loudness_meter()) at the delivered rate, fed the float32 samples the stream makes final -- behind the
        resampler and the limiter, in front of the encoder --; loudness() returns its read().  The blocks have the bits of the same
        stream without the meter; with nothing but meter=True they are returned as they came.  Refused: channels= (the
        count goes by n_channels=), loudness=, true_peak= without limiter='lookahead', and interleaved= without n_channels."""
        from .delivery_stream import DeliveryStream, resolve
        return DeliveryStream(resolve(keywords, None, n_channels), self)

    @torch.no_grad()
    def delivery_push(self, streams, blocks, final=False):
        """One 48 kHz block per DeliveryStream (None: nothing) -> one delivered block per stream; every stage is one launch for
        all the streams that share a plan, whatever their channel counts (streams opened with n_channels= form one plan, mono
        streams opened without it another).  final: the streams end here."""
        from .delivery_stream import push
        return push(self.delivery, streams, blocks, final)

    def generate_long(self, audio, sr, **stream_keywords):
        """A clip of any length through a streaming session: push everything, then flush -> [1, T48] (int16 with pcm='int16');
        with delivery=: [1, delivery.delivered_len(T48, output_rate)] at the delivered rate, int16 with delivery's pcm.
        Keywords: those of stream().  Memory and attention cost are those of one push's windows, whatever the clip's length.
        With n_channels=C: audio is [C, T], the result [C, T48] (or what delivery= makes of it: [C, n], int16 [n, C] with its
        interleaved=)."""
        s = self.stream(sr, **stream_keywords)
        first = s.push(audio)
        frames = s.delivery is not None and s.delivery.interleaved
        return torch.cat([first, s.flush()], 0 if frames else 1)

    @torch.no_grad()
    def measure_loudness(self, rows, chans=None, rate=48000):
        """Integrated loudness on the device: rows = float32 [R, T] on the model's device (chans: channels per clip, summing to
        R; None: every row is a clip) or a list of [C_i, T_i] tensors; rate: their sample rate -> float32 [n_clips] LUFS on the
        device, -inf for a clip no block of which passes the gates.  The kernels of loudness= with no target: it reads what a
        loudness= call delivered, and whether the peak cap bound (flowhigh_amd/loudness.py is the definition)."""
        return self.delivery.measure(rows, chans, rate)

    @torch.no_grad()
    def measure_loudness_report(self, rows, chans=None, rate=48000):
        """EBU R128's figures on the device: rows, chans and rate as measure_loudness takes them -> float32 [n_clips, 6] on the
        device: the integrated loudness (the bits of measure_loudness), the maximum momentary (400 ms) and the maximum
        short-term (3 s) loudness in LUFS, the loudness range (EBU Tech 3342) in LU, and the last momentary and short-term
        value; -inf for an empty series (a clip shorter than 3 s has no short-term value) and a range of 0 when no window passes
        its gates (flowhigh_amd/meter.py is the definition).  At most 2^20 sub-blocks of 100 ms per clip."""
        return self.delivery.measure_report(rows, chans, rate)

    def loudness_meter(self, rate=48000, n_channels=None, log_capacity=None):
        """The meter of a stream at `rate`: push(block) takes float32 [1, n] / [n] on the model's device ([C, n] with
        n_channels=C, an int 1 .. 8), n may be 0, and returns nothing; read() -> float32 [6] on the device, the row
        measure_loudness_report(x[:, :m.measured]) gives for the stream x so far, bit for bit (m.measured, a host int: the
        complete 100 ms sub-blocks among the whole spans of 4096 samples pushed; all -inf with a range of 0 while it is 0);
        flush() processes the rest and closes the meter: read() is then the report of all of x.  read() costs one launch; nothing
        is read back by any of them.  log_capacity: the sub-blocks the energy log holds at first (it grows by doubling, to 2^20
        at most: a push that would begin one more is a RuntimeError that leaves the meter as it was)."""
        from .loudness_meter import LOG_CAPACITY, LoudnessMeter
        return LoudnessMeter(self, rate, n_channels, LOG_CAPACITY if log_capacity is None else log_capacity)

    @torch.no_grad()
    def meter_push(self, meters, blocks, final=False):
        """One block per LoudnessMeter (None: nothing): ONE launch for all rows of all meters of one rate and one table upload.
        final: the meters end here.  A meter's result does not depend on its company."""
        from .loudness_meter import push
        push(self.delivery, meters, blocks, final)

    @torch.no_grad()
    def measure_true_peak(self, rows, chans=None, rate=48000):
        """True peak on the device: rows, chans and rate as measure_loudness takes them -> float32 [n_clips] dBTP on the device,
        -inf for a silent clip: the largest of the samples and of their 4x oversampling (81 taps, the same at every rate) over
        the clip's channels.  The kernels of true_peak=: it reads what a true_peak= call delivered (flowhigh_amd/truepeak.py is
        the definition)."""
        return self.delivery.measure_true_peak(rows, chans, rate)

    @torch.no_grad()
    def measure_quality(self, rows, ref_rows, chans=None, rate=48000, cutoff_hz=None):
        """Spectral quality report on the device: an estimate against a full-band reference.  rows, ref_rows = float32 [R, T] on
        the model's device (chans: channels per clip, summing to R; None: every row is a clip), or two lists of [C_i, T_i] tensors
        of equal shapes pair by pair (no chans=; one launch sequence for all of them).  cutoff_hz: None, one positive number, or
        one per clip -- for a clip generated from sr_in it is sr_in / 2; rate turns it into a bin and does nothing else
        -> float32 [n_clips, 4] on the device, nothing is read back: the log-spectral distance over all bins, below and above the
        cutoff (NaN for an empty band, and for both without a cutoff), and the SNR in dB (+inf for identical rows).  STFT of
        2048 / 480 with the post-processor's window; flowhigh_amd/quality.py is the definition.  Synthetic-weight models give
        distances between computations, not perceptual quality."""
        return self.delivery.measure_quality(rows, ref_rows, chans, rate, cutoff_hz)

    def _serve_streams(self, n):
        pool = getattr(self, "_side_streams", None)
        if pool is None or len(pool) < n:
            pool = self._side_streams = [torch.cuda.Stream(self.device) for _ in range(n)]
        return pool[:n]

    @torch.no_grad()
    @hip.on_device
    def generate_from_device(self, x, sr, timestep=1, *, noise=None, seed=None, generator=None):
        """Device-resident variant (no host work, no sync; graph-capturable): x [B, T_in] float32
        low-rate clips already in HBM (|x| <= 1), noise [B, N, n_mels] -> [B, T48].  Same
        arithmetic as generate_batch with upsampling_method='hip'.  Mono clips at 0.99 peak only: channels= and level= are
        keywords of generate / generate_batch / generate_many (a multichannel clip can go in as its channels, [C, T_in]; they
        then come back as C independent clips).  On a prior='device' model `noise` may be left out:
        the prior is drawn on the device from seed= (or from keys taken from the generator: _prior_keys); a
        prior='reference' model has no device-side draw and needs `noise`."""
        keys = self._prior_keys(seed, x.shape[0], generator, noise)
        if noise is None and keys is None:
            raise ValueError("generate_from_device: a prior='reference' model needs noise= (its prior is drawn on the host); "
                             "construct the model with prior='device' to draw it on the device")
        return self._generate_from_device(x, sr, timestep, noise=noise, keys=keys)

    def _generate_from_device(self, x, sr, timestep=1, *, noise=None, keys=None):
        cond = self.resampler(x, sr, 48000)
        wav = self._sample(cond=cond, time_steps=timestep, cfm_method=self.cfm_method, noise=noise, keys=keys,
                           **self._prior_scale()).squeeze(1)
        return self.postproc(wav, cond, cond.size(-1))

    @torch.no_grad()
    @hip.on_device
    def capture(self, batch, n_in, sr, timestep=1):
        """HIP-graph form of generate_from_device for one input shape: the ~150 launches of a call are recorded once
        and replayed with a single enqueue (short clips are launch-bound from Python).  Returns a `GraphedGenerate`
        with static buffers `.x` [batch, n_in] and `.noise` [batch * N, n_mels]; fill them and call `.replay()`.
        On a prior='device' model the graph records the prior launch and has `.keys` (device int64 [batch, 2] = the clips'
        (seed, stream)) in place of `.noise`: a replay draws from the keys that are there.
        The captured call is generate_from_device: mono [batch, n_in] clips at 0.99 peak, no channels= or level=."""
        return GraphedGenerate(self, batch, n_in, sr, timestep)

    @torch.no_grad()
    @hip.on_device
    def generate(self, audio, sr: int, target_sampling_rate=48000, timestep=1, *, noise=None, generator=None, seed=None,
                 channels=None, level='peak', output_rate=None, pcm=None, dither=None, dither_seed=0, interleaved=False,
                 loudness=None, true_peak=None, limiter=None):
        """One clip, reference contract: returns float32 [1, T48] on the model device.  seed= (prior='device' models): the
        clip's noise is that of the key (seed, 0), or of a (seed, stream) pair given as [(seed, stream)].
        channels = None (default: a mono clip, 1-D or [1, T]; a 2-D clip is then a ValueError) | 'first' ([C, T]) | 'last'
        ([T, C], what gradio and soundfile hand over), 1 <= C <= 8: returns [C, T48] in every layout.  Each channel runs as a
        mono clip does (resampled, divided by its own peak p_c, its own cutoff); the channels share ONE prior draw (noise=
        [1, N, n_mels]; [C, N, n_mels] gives every channel its own) or the clip's one (seed, stream) key, and one final
        scaling, so the balance between them is kept.  A silent channel comes back as exact zeros.
        level = 'peak' (default: 0.99 of the clip's peak -- over all its channels --, as the reference) | 'input': the
        output at the level of the input, w_c * p_c: below the cutoff it is the 48 kHz input itself, not its normalised copy.
        A mono clip with neither keyword runs what it always ran (DESIGN.md "Channels and level").
        Delivery (DESIGN.md "Delivery"; all on the device, every default leaves the call as it was):
        output_rate = None | 48000 (as it is) | R, a positive integer whose reduced R / 48000 has no term above 640 (8000, 11025,
        12000, 16000, 22050, 24000, 32000, 44100, 88200, 96000; anything else is a ValueError): the result is
        scipy.signal.resample_poly(y48, R, 48000) of every row, tables.resample_out_len(T48, R, 48000) samples; at level='peak'
        it is put at 0.99 of its own peak (over the clip's channels) again, at level='input' it is left as resampled.
        target_sampling_rate keeps its meaning (the rate of the mel codec: 48000 or NotImplementedError).
        pcm = None | 'int16': torch.int16 in the float result's shape, pcm.py's encoding of it (round to nearest even, clamp).
        pcm = 's24': packed signed 24-bit little-endian (a WAV's pcm_s24le layout) as torch.uint8 with a last axis of 3 bytes,
        [C, T, 3] ([1, T, 3] mono), [T, C, 3] interleaved -- .reshape(-1) of that is the data chunk of a 24-bit WAV file;
        pcm = 's24in32': the same integer sign-extended in a torch.int32, shaped like the int16 result (pcm.py: encode24).
        dither = None | 'tpdf' (pcm only): +-1 LSB triangular dither from the key (dither_seed, 0) -- dither_seed an int, or
        [(seed, stream)]; a function of the key, the channel and the sample index alone.
        interleaved = True (pcm only): [T, C] ([T, 1] for a mono clip), written in that order by the kernel.
        loudness = None | L, a finite target in LUFS, -70 <= L <= 0 (-16: streaming and podcasts, -23: EBU R 128): the clip at
        that integrated loudness (ITU-R BS.1770-4 as loudness.py states it: K-weighting in float64, 400 ms blocks, both gates),
        measured at the delivered rate after the resampling and before the PCM encoding, one gain for all channels:
        g = min(10^((L - measured) / 20), 0.99 / peak).  The peak stays at or below 0.99, so without limiter= a clip
        that would need more comes out below the target (measure_loudness reads what was delivered).  A clip shorter than
        400 ms is measured as one block of its own length; channel weights are 1 (exact for mono and stereo).  It goes with
        level='peak' only (level='input' is a ValueError: two rules for one gain); a silent clip stays zeros.
        true_peak = None | T, a finite ceiling in dBTP, -20 <= T <= 0 (-1: the usual delivery spec): the true peak of the result --
        the largest of its samples and of their 4x oversampling (ITU-R BS.1770-4 Annex 2 as truepeak.py states it: 81 taps, factor
        4 at every rate), over the clip's channels, at the delivered rate -- is held at or under T, behind the resampling and the
        loudness measurement and before the PCM encoding.  It only attenuates, so it goes with either level=.
        limiter = None: one gain for the clip, g = min(g_L, 10^(T / 20) / TP), g_L the gain of loudness= (1 without it) |
        'lookahead' (with true_peak= only): a zero-delay look-ahead limiter, 5 ms either side, one gain curve for all channels
        (the stereo image stays), no sample above the ceiling; with loudness= the loudness gain is then NOT capped at the 0.99
        peak, the limiter takes what is over, and the delivered loudness ends slightly under the target (nothing iterates;
        measure_loudness reads it).  A delivered rate above 102 499 Hz is a ValueError (the limiter's window).  Non-finite samples
        are outside the contract.  measure_true_peak reads what was delivered."""
        out = self.generate_batch([audio], sr, target_sampling_rate, timestep, noise=noise, generator=generator, seed=seed,
                                  channels=channels, level=level, output_rate=output_rate, pcm=pcm, dither=dither,
                                  dither_seed=dither_seed, interleaved=interleaved, loudness=loudness, true_peak=true_peak,
                                  limiter=limiter)
        if channels is not None or (interleaved and pcm is not None):
            return out[0]
        return out
