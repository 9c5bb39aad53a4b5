"""Enqueueing: one-off launchers of the conv / activation entry points (tests, tools), the per-device occupancy setting of
the activation launches, and the dispatch a plan is run with: step kind (planner.STEP_TYPES, plain and ragged) -> enqueueing function.
(Split out of vocoder.py in round 5; `flowhigh_amd.vocoder` re-exports every name.)
"""
import ctypes as C
import os

import torch

from . import hip
from .planner import (AMP_BF16X3, AMP_DIRECT, WINO_BF16X6, WINO_F54, WINO_FRAG_ORDER, WINO_NOVL, act_ragged_groups, amp_max_center, amp_tile_list, make_act_group,
                      make_wino_group, make_wino_seg, pick_wino54_tile, pick_wino_tile, use_wino54, wino_packer, wino_run_map, wino_weight_flags)

def amp_actconv(groups, batch, channels, dilation, device, direct=False, bf3=False):
    """Upload descriptors and enqueue one narrow-stage launch (test / one-off use).  direct: the bf16 x 6 form (groups made with
    make_amp_seg / make_amp_group(..., direct=True), weights from pack_narrow_bf_weight); bf3 beside it: the bf16 x 3 form
    (fh_narrow_conv_bf16x3_f32, weights from pack_narrow_bf3_weight)."""
    tiles = amp_tile_list([g.len for g in groups], batch, dilation, direct=direct).to(device)
    d = hip.to_device_struct_array(groups, device)
    name, tail = narrow_entry(int(all(g.len % 4 == 0 for g in groups)) | (AMP_DIRECT if direct else 2) | (AMP_BF16X3 if direct and bf3 else 0),
                              amp_max_center(groups, direct))
    enqueue(getattr(hip.lib(), name), (d.data_ptr(), len(groups), tiles.data_ptr(), tiles.shape[0], channels, dilation, *tail, hip.stream()))
    return d, tiles


def conv_wino(groups, batch, cout_pad, length, dilation, device, tile_cfg=0, phase_major=False):
    """Upload descriptors and enqueue one Winograd conv launch (test / one-off use)."""
    d = hip.to_device_struct_array(groups, device)
    # (F(5,4) kernel: the groups' weights are pack_wino54_weight, ngrp = ceil(k / 4))
    if tile_cfg & WINO_F54 and any(g.out_stride > 1 or g.out_len or g.seg[i].ngrp > 3 or g.seg[i].xlen for g in groups for i in range(g.nseg)):
        raise NotImplementedError("the F(5,4) kernel takes plain convs of at most 12 taps (no strided outputs, xlen, out_len)")
    name, cfg = wino_entry(tile_cfg, tile_cfg & (WINO_BF16X6 | WINO_FRAG_ORDER))           # (a caller's weight-format flags stay)
    enqueue(getattr(hip.lib(), name), (d.data_ptr(), len(groups), batch, cout_pad, length, dilation, int(phase_major), cfg, hip.stream()))
    return d


def conv_wino_ragged(groups, lengths, cout_pad, dilation, device, tile_cfg=0, phase_major=False):
    """Upload descriptors and run map and enqueue one ragged Winograd conv launch (test / one-off use): group i is one clip's
    [C, lengths[i]] tensors (g.len = lengths[i], batch 1), the groups in launch order.  tile_cfg: plan tile id, F(4,3) or
    WINO_F54 | id, | WINO_BF16X6 for three-piece weights (| WINO_FRAG_ORDER: in fragment order); the vector loader is ruled out as planner._merge_wino does it.
    -> (descriptors, run map): keep both until the launch has run."""
    if any(g.len != n for g, n in zip(groups, lengths)) or len(groups) != len(lengths):
        raise ValueError("conv_wino_ragged: lengths must be the groups' own")
    if tile_cfg & WINO_F54 and any(g.out_stride > 1 or g.out_len or g.seg[i].ngrp > 3 or g.seg[i].xlen for g in groups for i in range(g.nseg)):
        raise NotImplementedError("the F(5,4) kernel takes plain convs of at most 12 taps (no strided outputs, xlen, out_len)")
    wcfg = tile_cfg & (15 | WINO_F54)
    novl = 0 if ((phase_major or all(n % 4 == 0 for n in lengths)) and not tile_cfg & WINO_NOVL) else 2
    runs = torch.tensor(wino_run_map(list(lengths), wcfg, cout_pad, dilation, bool(phase_major)), dtype=torch.int32).to(device)
    d = hip.to_device_struct_array(groups, device)
    name, cfg = wino_entry(wcfg, tile_cfg & (WINO_BF16X6 | WINO_FRAG_ORDER), ragged=True)
    enqueue(getattr(hip.lib(), name), (d.data_ptr(), len(groups), cout_pad, max(lengths), dilation, int(bool(phase_major)) | novl, cfg,
                                       runs.data_ptr(), runs.numel(), hip.stream()))
    return d, runs


def conv_grouped(groups, batch, cout_pad, n_len, tile_cfg, device, ck=8, bf=False):
    """Upload descriptors and enqueue one grouped conv launch (test / one-off use).  bf: 1 / True = the bf16 x 6 entry (the groups' weights
    are pack_conv_bf_weight's; every cin a multiple of 16), 2 = the bf16 x 3 entry (pack_conv_bf3_weight's)."""
    d = hip.to_device_struct_array(groups, device)
    name, tail = conv_entry(bf, ck)
    enqueue(getattr(hip.lib(), name), (d.data_ptr(), len(groups), batch, cout_pad, n_len, tile_cfg, *tail, hip.stream()))
    return d


def act1d_grouped(groups, batch, channels, length, device, din=1, dout=1):
    d = hip.to_device_struct_array(groups, device)
    enqueue(hip.lib().fh_act1d_grouped_pm_f32, (d.data_ptr(), len(groups), batch, channels, length, din, dout, hip.stream()))
    return d


def act1d_ragged(groups, lengths, channels, device, din=1, dout=1):
    """Upload descriptors and enqueue one ragged activation launch (test / one-off use): group i (make_act_group) is one clip's
    [channels, lengths[i]] tensors, in launch order; length, tile prefix and the mult4 flag as planner._merge_act makes them."""
    ragged, tiles, mult4 = act_ragged_groups(groups, lengths, channels)
    d = hip.to_device_struct_array(ragged, device)
    enqueue(hip.lib().fh_act1d_ragged_f32, (d.data_ptr(), len(ragged), channels, din, dout, tiles, mult4, hip.stream()))
    return d


# ---- occupancy of the activation launches (fh_act_set_blocks_per_cu) --------------------------------------------------
# On some MI355X boxes an uncapped activation launch (7 blocks = 28 waves per CU: vector ALUs, LDS and HBM busy at once)
# makes the power management drop the shader clock for the duration of the NEXT launch: a Winograd launch that follows
# one runs at 2.11 instead of 2.38 GHz (tools/clock_dip_probe.py, tools/box_probe.sh; a device copy of the same bytes does
# not do it).  With 3 blocks per CU the dip is mostly gone (on such a box the capped activation is 10-15 % slower, the convs
# 10 % faster); on boxes without the dip the cap would only cost the activation 25 %.  So the setting is measured once per device and process.
# (tools/exp/occ_ab.sh on both kinds of affected boxes: 4 blocks help on one kind only (bench 500 -> 527) and do nothing on the
# other (the clock is clamped as before); 3 blocks help on both (488 -> 522, 500 -> 524); 2 blocks: the activation itself
# is too slow then (512))
ACT_BLOCKS_CHOICES = (0, 3, 4)          # 0 = no cap; 4 is enough on one kind of affected box (and costs the activation less), 3 on both
_act_blocks = {}                        # device ordinal -> setting in force
_act_choice = {}                        # (device ordinal, bf16 x 6 convs?) -> setting chosen for models of that form


def pick_act_blocks(pair_us, slack=0.98):
    """The decision rule: no cap unless a capped setting makes the (activation + conv) pair at least 2 % faster -- in EVERY
    measurement pass (pair_us: one {blocks: us} dict, or a list of them, one per pass): a single noisy pass on a shared
    or busy GPU must not flip the setting."""
    passes = [pair_us] if isinstance(pair_us, dict) else list(pair_us)
    wins = [b for b in passes[0] if b != 0 and all(p[b] < slack * p[0] for p in passes)]
    if not wins:
        return 0
    return min(wins, key=lambda b: sorted(p[b] for p in passes)[len(passes) // 2])


def parse_act_blocks(value):
    """FH_ACT_BLOCKS / Vocoder(act_blocks=): None, '' or 'auto' -> None (measure); 0 or 2..5 -> that setting."""
    if value is None or str(value).strip().lower() in ("", "auto"):
        return None
    try:
        v = int(str(value).strip())
    except ValueError:
        v = -1
    if v != 0 and not 2 <= v <= 5:
        raise ValueError(f"FH_ACT_BLOCKS / act_blocks must be 'auto', 0 (no cap) or 2..5 blocks per CU, got {value!r}")
    return v


def decide_act_blocks(measure, group=None, collective=False):
    """(choice, passes) from `measure()` (-> list of per-pass {blocks: us}).
    collective=False (what a constructor does): measured by the calling process, no communication -- a constructor must never
    enter a collective: whether a rank gets here depends on per-process state (the per-device cache, FH_ACT_BLOCKS, a second
    model on one rank), and the ranks that wait would hang.
    collective=True (sync_act_blocks: an explicit call that EVERY rank of `group` makes at the same point of the program): rank 0
    of the group alone measures -- eight ranks timing launch pairs while their neighbours load models under one power budget
    would each measure something else -- and broadcasts its choice, or the error it hit (a failing rank 0 must not leave the
    others waiting: they raise too)."""
    if not collective:
        passes = measure()
        return pick_act_blocks(passes), passes
    import torch.distributed as dist
    box = [None]
    if dist.get_rank(group) == 0:
        try:
            passes = measure()
            box[0] = ("ok", pick_act_blocks(passes), passes)
        except Exception as e:                            # noqa: BLE001  (reported on every rank)
            box[0] = ("error", f"{type(e).__name__}: {e}", None)
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if box[0][0] != "ok":
        raise RuntimeError(f"activation occupancy calibration failed on rank 0 of the group: {box[0][1]}")
    return box[0][1], box[0][2]


def sync_act_blocks(device, group=None, bf=None):
    """One setting for all ranks of `group` (default: the world; pass a per-node group when the nodes differ): call it on EVERY
    rank, before the models are built; it returns the setting and puts it in force (and in the per-device cache, so that the
    constructors measure nothing).  FH_ACT_BLOCKS still overrides.  Without an initialised process group: the local calibration."""
    import torch.distributed as dist
    dev = hip.norm_device(device)
    if bf is None:                                   # (the conv form the environment's models will have)
        from .planner import use_bf16x6
        bf = use_bf16x6()
    fixed = parse_act_blocks(os.environ.get("FH_ACT_BLOCKS"))
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return calibrate_act_occupancy(dev, bf=bf)

    # EVERY rank enters the collective, whatever its own FH_ACT_BLOCKS says (a variable exported on some ranks only must not
    # leave the others waiting in the broadcast: ADVICE r05): rank 0 of the group decides -- its FH_ACT_BLOCKS if it has one,
    # else its measurement -- and every rank takes that.
    def measure():
        if fixed is not None:
            return [{0: 1.0, fixed: 0.5}] * 2 if fixed != 0 else [{0: 1.0}] * 2        # (pick_act_blocks -> `fixed`)
        return [{b: measure_act_conv_pair(dev, b, bf=bf) for b in ACT_BLOCKS_CHOICES} for _ in range(2)]
    choice, passes = decide_act_blocks(measure, group=group, collective=True)
    if fixed is not None and fixed != choice:
        import logging
        logging.getLogger("flowhigh_amd").warning("FH_ACT_BLOCKS=%s on this rank, rank 0 of the group chose %s: taking rank 0's", fixed, choice)
    calibrate_act_occupancy.last_measurement = passes
    return calibrate_act_occupancy(dev, force=True, act_blocks=choice, bf=bf)


def measure_act_conv_pair(device, blocks, c=192, length=60000, warm=60, reps=100, bf=False):
    """Average us of one (activation launch, Winograd launch) pair of a mid-network stage's size with the activation capped
    at `blocks` per CU (synthetic tensors; the launches are the model's: 3 groups, k = 11 / 7 / 3)."""
    dev = hip.norm_device(device)
    with hip.device_guard(dev):
        g = torch.Generator().manual_seed(0)
        ks = (11, 7, 3)
        xs = [torch.randn(1, c, length, generator=g).to(dev) for _ in ks]
        ys = [torch.empty(1, c, length, device=dev) for _ in ks]
        outs = [torch.empty(1, c, length, device=dev) for _ in ks]
        bias = torch.zeros(c, device=dev)
        # (the conv launch of the model at this width: the F(5,4) kernel unless it is switched off)
        # (bf: the conv of the pair in the bf16 x 6 form -- the cap exists for what the activation launch does to the clock of the
        # conv launch behind it, and that differs between the fp32 and the bf16 matrix instructions: round 6 measured a cap that
        # pays in front of fp32-MFMA convs and costs in front of bf16 x 6 ones on the same box)
        f54 = use_wino54(c, "bf16x6" if bf else "winograd")
        wcfg, wpad = pick_wino54_tile(c, bf) if f54 else pick_wino_tile(c)
        pack = wino_packer(wcfg, bf)
        name, cfg = wino_entry(wcfg, wino_weight_flags(wcfg, bf))
        us = [pack(torch.randn(c, c, k, generator=g) * 0.02, wpad).to(dev) for k in ks]
        gw = hip.to_device_struct_array([make_wino_group([make_wino_seg(ys[i], us[i], c, k, taps=4 if f54 else 3)], bias, [],
                                                         outs[i], c, wpad, length) for i, k in enumerate(ks)], dev)
        filt = [0.0] * 5 + [0.5, 0.5] + [0.0] * 5
        p = dict(alpha=torch.ones(c, device=dev), inv_beta=torch.ones(c, device=dev), up=filt, down=filt)
        ga = hip.to_device_struct_array([make_act_group(xs[i], ys[i], p) for i in range(len(ks))], dev)
        lib, st = hip.lib(), hip.stream()
        before = lib.fh_act_get_blocks_per_cu()
        hip.check(lib.fh_act_set_blocks_per_cu(blocks), "fh_act_set_blocks_per_cu")
        try:
            def pair():
                enqueue(lib.fh_act1d_grouped_pm_f32, (ga.data_ptr(), len(ks), 1, c, length, 1, 1, st))
                enqueue(getattr(lib, name), (gw.data_ptr(), len(ks), 1, wpad, length, 1, 0, cfg, st))
            for _ in range(warm):
                pair()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                pair()
            e1.record()
            torch.cuda.synchronize(dev)
        finally:
            hip.check(lib.fh_act_set_blocks_per_cu(before), "fh_act_set_blocks_per_cu")
        return e0.elapsed_time(e1) * 1e3 / reps


def calibrate_act_occupancy(device, force=False, act_blocks=None, bf=False):
    """Choose and set the activation launches' blocks per CU on `device` (once per device and process).
    act_blocks (Vocoder(act_blocks=)) or FH_ACT_BLOCKS = auto | 0 | 2..5 override the measurement -- a deployment that
    knows its boxes, or a launcher that wants every rank alike, passes the number.  No communication here: ranks that want one
    setting call sync_act_blocks() before they build their models (bench.py does).  The measured pair times are logged
    (logger 'flowhigh_amd').  Returns the setting.  Results do not depend on it, only launch times."""
    dev = hip.norm_device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        return 0
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, bool(bf))                            # one measured choice per device and conv form (bf: see measure_act_conv_pair)
    fixed = parse_act_blocks(act_blocks)
    if fixed is None:
        fixed = parse_act_blocks(os.environ.get("FH_ACT_BLOCKS"))
    if key in _act_choice and not force and (fixed is None or fixed == _act_choice[key]):
        choice = _act_choice[key]
    elif fixed is not None:
        choice = fixed
    else:
        def measure():                               # two alternating passes: the chip's state drifts over the first 100 ms
            return [{b: measure_act_conv_pair(dev, b, bf=bf) for b in ACT_BLOCKS_CHOICES} for _ in range(2)]
        choice, passes = decide_act_blocks(measure)
        calibrate_act_occupancy.last_measurement = passes
        import logging
        logging.getLogger("flowhigh_amd").info("activation occupancy on cuda:%d (%s convs): %s blocks per CU; (activation, conv) pair us per pass: %s",
                                               idx, "bf16 x 6" if bf else "fp32-MFMA", choice or "uncapped (7)", passes)
    _act_choice[key] = choice
    ensure_act_blocks(dev, choice)
    return choice


def ensure_act_blocks(device, choice):
    """Put `choice` in force on `device` if another one is (the library holds ONE setting per device; models of both conv forms
    in one process -- bench.py builds both -- each ask for theirs in front of their launches: a host-side integer, no GPU work)."""
    dev = hip.norm_device(device)
    if dev.type != "cuda":
        return
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if _act_blocks.get(idx) != choice:
        with hip.device_guard(dev):
            hip.check(hip.lib().fh_act_set_blocks_per_cu(choice), "fh_act_set_blocks_per_cu")
        _act_blocks[idx] = choice


calibrate_act_occupancy.last_measurement = None


def wino_entry(wcfg, flag, ragged=False):
    """(library entry's name, its tile_cfg argument) of a Winograd launch with plan tile id `wcfg` (| mapping / alignment flags): the
    F(5,4) kernel takes the tile in the low four bits, the F(4,3) kernel the whole id; flag: the weight-format flags
    (planner.wino_weight_flags: FH_WINO_BF16X6, FH_WINO_FRAG_ORDER) or 0."""
    f54 = wcfg & WINO_F54
    return ("fh_conv_wino54" if f54 else "fh_conv_wino") + ("_ragged_f32" if ragged else "_f32"), ((wcfg & 15) if f54 else wcfg) | flag


def conv_entry(bf, ck):
    """(library entry's name, its arguments behind tile_cfg) of a direct-kernel launch whose record has `bf` (planner.direct_bf_pieces:
    0 fp32, 1 bf16 x 6, 2 bf16 x 3): the bf16 entries take no channel chunk."""
    return (("fh_conv_grouped_bf16x3_f32" if bf == 2 else "fh_conv_grouped_bf16x6_f32"), ()) if bf else ("fh_conv_grouped_f32", (ck,))


def narrow_entry(flags, cmax):
    """(library entry's name, its arguments behind the dilation) of a narrow-stage launch with plan flags `flags`."""
    if flags & AMP_DIRECT:
        return ("fh_narrow_conv_bf16x3_f32" if flags & AMP_BF16X3 else "fh_narrow_conv_bf16x6_f32"), (flags & 1,)
    return "fh_amp_actconv_f32", (cmax, flags)


def enqueue(fn, args, timing=None):
    """One call of the library entry `fn` on the stream in `args`.  timing: None, or the list that receives the launch's (start, end) events."""
    if timing is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = fn(*args)
    if rc:
        hip.check(rc, fn.__name__)
    if timing is not None:
        e1.record()
        timing.append((e0, e1))


# ---- one function per step kind (planner's records): (library, voc, step, batch, stream, address of the ragged plan's descriptor blob).
# voc.conv_timing / voc.act_timing, when lists, receive one event pair per conv / convt / wino / amp and per act launch, in launch
# order (bench.py zips them with plan["conv_launches"]); the ragged kinds record nothing.  Enqueue only: graph-capturable. -----------
def _conv(L, voc, s, B, st, base):
    name, tail = conv_entry(s.bf, s.ck)
    enqueue(getattr(L, name), (s.desc.data_ptr(), s.ng, B, s.cpad, s.n_len, s.tcfg, *tail, st), voc.conv_timing)

def _convt(L, voc, s, B, st, base):
    enqueue(L.fh_conv_transpose_fused_f32, (s.desc.data_ptr(), s.ng, B, s.cpad, s.n_len, s.tcfg, s.phases, st), voc.conv_timing)

def _wino(L, voc, s, B, st, base):
    name, cfg = wino_entry(s.wcfg, wino_weight_flags(s.wcfg, voc.bf))
    enqueue(getattr(L, name), (s.desc.data_ptr(), s.ng, s.batch, s.wpad, s.length, s.dil, s.pm, cfg, st), voc.conv_timing)

def _amp(L, voc, s, B, st, base):
    name, tail = narrow_entry(s.flags, s.cmax)
    enqueue(getattr(L, name), (s.desc.data_ptr(), s.ng, s.tiles.data_ptr(), s.n_tiles, s.c, s.dil, *tail, st), voc.conv_timing)

def _act(L, voc, s, B, st, base):
    enqueue(L.fh_act1d_grouped_pm_f32, (s.desc.data_ptr(), s.ng, B, s.c, s.length, s.din, s.dout, st), voc.act_timing)

def _mean(L, voc, s, B, st, base):
    enqueue(L.fh_mean_f32, (s.a.data_ptr(), s.b.data_ptr(), s.c.data_ptr() if s.c is not None else None, s.out.data_ptr(), s.n, s.scale, st))

def _sum(L, voc, s, B, st, base):
    arr = (C.c_void_p * len(s.srcs))(*[t.data_ptr() for t in s.srcs])
    enqueue(L.fh_sum_f32, (arr, len(s.srcs), s.out.data_ptr(), s.n, s.scale, st))

def _post(L, voc, s, B, st, base):
    enqueue(L.fh_conv_post_tanh_f32, (s.x.data_ptr(), voc.post_w.data_ptr(), voc.post_b.data_ptr(), s.wav.data_ptr(), B, s.c, s.length, voc.post_k, st))

def _rwino(L, voc, s, B, st, base):
    name, cfg = wino_entry(s.wcfg, wino_weight_flags(s.wcfg, voc.bf), ragged=True)
    enqueue(getattr(L, name), (base + s.off, s.ng, s.wpad, s.maxlen, s.dil, s.pmflag, cfg, base + s.off_map, s.n_runs, st))

def _rconv(L, voc, s, B, st, base):
    name, tail = conv_entry(s.bf, s.ck)
    enqueue(getattr(L, name), (base + s.off, s.ng, 1, s.cpad, s.maxlen, s.tcfg, *tail, st))

def _rconvt(L, voc, s, B, st, base):
    enqueue(L.fh_conv_transpose_fused_f32, (base + s.off, s.ng, 1, s.cpad, s.maxlen, s.tcfg, s.phases, st))

def _ramp(L, voc, s, B, st, base):
    name, tail = narrow_entry(s.flags, s.cmax)
    enqueue(getattr(L, name), (base + s.off, s.ng, base + s.off_tiles, s.n_tiles, s.c, s.dil, *tail, st))

def _ract(L, voc, s, B, st, base):
    enqueue(L.fh_act1d_ragged_f32, (base + s.off, s.ng, s.c, s.din, s.dout, s.tiles, s.mult4, st))

def _rsum(L, voc, s, B, st, base):
    enqueue(L.fh_sum_multi_f32, (base + s.off, s.n_jobs, s.max_n, st))


LAUNCH = dict(conv=_conv, convt=_convt, wino=_wino, amp=_amp, act=_act, mean=_mean, sum=_sum, post=_post,
              rwino=_rwino, rconv=_rconv, rconvt=_rconvt, ramp=_ramp, ract=_ract, rsum=_rsum)


def launch_step(voc, s, B, st, base=0):          # (one step, for callers outside; run_steps does the same lookup in its loop)
    LAUNCH[s.kind](hip.lib(), voc, s, B, st, base)


def run_steps(voc, steps, B, st, base=0):
    L = hip.lib()
    for s in steps:
        LAUNCH[s.kind](L, voc, s, B, st, base)


def run_ragged_steps(voc, rp):
    run_steps(voc, rp["steps"], 1, hip.stream(), rp["desc"].data_ptr())
