"""The sampler's ODE solve as launches: ode.run_step over ode.step_plan(method) (fixed-grid explicit Runge-Kutta, torchdiffeq
semantics) on token-major rows [rows, n_mels], with the HIP library behind its two callables.  An evaluation is out = base + h v(x, t)
(eval_fused; a raw k is the same with h = 1 and no base: eval); under classifier-free guidance, v = null + s (cond - null), it is
two chained ones: h (1 - s) on the null condition, then h s onto that.  Uniform form: one time and step size for all rows, the
update is the epilogue of the field's last GEMM, both backbones.  Grouped form (net.grouped_field): the segments of a ragged sequence take
different step counts, those of one count are a group of rows, each group at its own time and step size (ode.mixed_schedule); the
field is written raw and updated by fh_axpy_groups_f32, the bits of that epilogue, so a segment's rows are the bits of the uniform
form on it alone.  The library and the stream are fetched where an entry is called: euler and midpoint call none here."""
import ctypes
import itertools

import torch

from . import hip, ode


def _combine(entry, y, ks, wa, out_a, wb, out_b, h, *size):
    """One launch of a combine entry: the host arrays of ks, wa and wb, h (a float, or one per group) and the entry's sizes."""
    floats = ctypes.c_float * len(ks)
    hip.check(getattr(hip.lib(), entry)(y.data_ptr(), (ctypes.c_void_p * len(ks))(*[k.data_ptr() for k in ks]), len(ks), h, floats(*wa),
                                        out_a.data_ptr(), None if wb is None else floats(*wb), hip.ptr(out_b), *size, hip.stream()), entry)
    return out_a, out_b


def solve(net, method, y0, cond_mel, batch, n, steps, cond_scale=1., ragged=None):
    """y(1) from y(0) = y0 under the field of `net` conditioned on cond_mel; y0, cond_mel [rows, n_mels] on the device.  steps: one
    count (batch clips of n rows, or the segments of `ragged`), or the count of every segment of `ragged`, sorted descending."""
    plan = ode.step_plan(method)          # (NotImplementedError for a name outside ODE_METHODS)
    mixed = isinstance(steps, (list, tuple))
    if mixed:
        groups, passes = ode.mixed_schedule(steps)
        batch, n = len(ragged["frames"]), ragged["max_n"]
        seg_end = list(itertools.accumulate(n_segs for _, n_segs in groups))          # per group: segments and rows up to its end
        row_end = [sum(ragged["frames"][:e]) for e in seg_end]
    else:
        t = torch.linspace(0, 1, steps + 1)
        passes = [((t[i], t[i + 1] - t[i]),) for i in range(steps)]
    net.set_cond(cond_mel, batch, n, ragged=ragged)
    result = torch.empty_like(y0) if mixed else None
    # the results of even and odd passes, 'x', the guidance scratch, (grouped) the raw field
    bufs = [torch.empty_like(y0) for _ in range(5 if mixed else 4)]
    stage = {"x": bufs[2], **{name: torch.empty_like(y0) for name in ode.stage_names(plan)}}

    def uniform(x, times, hs, base, out, null):          # the update is the epilogue of the field's last GEMM
        net.forward(x, times[0], out, batch, n, alpha=hs[0], res=base, null_cond=null, ragged=ragged)

    def grouped(x, times, hs, base, out, null):          # the field raw, then the update over the pass's groups (ends, grp)
        kw = dict(null_cond=null, ragged=ragged, groups=(ends, times), n_seg=seg_end[len(ends) - 1])
        if base is None and not null and all(h == 1. for h in hs):          # (a raw k without guidance)
            return net.forward(x, None, out, 0, 0, **kw)
        net.forward(x, None, bufs[4], 0, 0, **kw)
        hip.check(hip.lib().fh_axpy_groups_f32(bufs[4].data_ptr(), hip.group_floats(hs), hip.ptr(base), out.data_ptr(), ends[-1],
                                               out.shape[-1], ctypes.byref(grp), hip.stream()), "fh_axpy_groups_f32")
    evaluate = grouped if mixed else uniform

    def field(x, c, base, weight, out):          # out = base + h v(x, t0 + c h), every group at its own t0 and h
        times = [ode.stage_time(t0, dt, c) for t0, dt in active]          # float32, from the linspace grid
        hs = [1. if weight is None else ode.fused_weight(weight, dt) for _, dt in active]
        if cond_scale == 1.:
            evaluate(x, times, hs, base, out, False)
        else:
            evaluate(x, times, [h * (1. - cond_scale) for h in hs], base, bufs[3], True)
            evaluate(x, times, [h * cond_scale for h in hs], bufs[3], out, False)
        return out

    def combine(y, *record):
        if mixed:
            return _combine("fh_rk_combine_groups_f32", y, *record, hip.group_floats([float(dt) for _, dt in active]), ends[-1],
                            y.shape[-1], ctypes.byref(grp))
        return _combine("fh_rk_combine_f32", y, *record, float(active[0][1]), y.numel())

    y = y0
    for p, active in enumerate(passes):
        if mixed:
            ends = row_end[:len(active)]
            grp = hip.row_groups(ends)
        stage["y"], stage["out"] = y, bufs[p % 2]
        y = ode.run_step(plan, stage, field, combine)
        # (grouped) the groups whose last step this was (one count: one contiguous range of rows): one device copy
        done = [g for g, (s, _) in enumerate(groups[:len(active)]) if s == p + 1] if mixed else []
        if done:
            r0 = row_end[done[0] - 1] if done[0] else 0
            result[r0:row_end[done[-1]]].copy_(y[r0:row_end[done[-1]]])
    return result if mixed else y
