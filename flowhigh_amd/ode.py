"""Fixed-grid ODE methods of the sampler: explicit Butcher tableaus and the launch plan of one time step.

The reference hands `torchdiffeq_ode_method` to torchdiffeq.odeint (cfm_superresolution.py:115-119,243); the fixed-grid solvers of
that library are restated here as tableaus (c, A, b):  k_j = v(y + h sum_i a_ji k_i, t0 + c_j h),  y' = y + h sum_j b_j k_j.
`step_plan` turns a tableau into named records, in the style of the vocoder's launch records; `run_step` is the one loop over them,
over two callables: integrate.py hands it the launches, the CPU tests their models.  No GPU import: the plans are plain data and the
loop is checked on the CPU (tests/test_ode_cpu.py).

    eval(src, c, dst)                      dst = v(src, t0 + c h)                    the field written raw (alpha = 1, res = None)
    eval_fused(src, c, base, weight, dst)  dst = base + (weight h) v(src, t0 + c h)  the update in the last GEMM's epilogue
    combine(ks, wa, dst_a, wb, dst_b)      dst_a = y + h sum_j wa_j ks_j  (and dst_b with wb, or wb = dst_b = None): one launch
                                           of fh_rk_combine_f32 (csrc/ode.hip)

Buffer names: 'y' the step's input, 'out' its result, 'x' the input of the next stage, 'base' the last stage's base
y + h sum_{i<s} b_i k_i, 'k1', 'k2', ... the stages' fields.
"""
from collections import namedtuple
from fractions import Fraction as Fr
from numbers import Integral

ODE_METHODS = ("euler", "midpoint", "heun2", "heun3", "rk4")

# (c, A, b): A's row j holds a_j1 .. a_j,j-1 (strictly lower triangular).  rk4 is torchdiffeq's fixed-grid 'rk4': the 3/8 rule.
_TABLEAUS = {
    "euler": ((0,), ((),), (1,)),
    "midpoint": ((0, Fr(1, 2)), ((), (Fr(1, 2),)), (0, 1)),
    "heun2": ((0, 1), ((), (1,)), (Fr(1, 2), Fr(1, 2))),
    "heun3": ((0, Fr(1, 3), Fr(2, 3)), ((), (Fr(1, 3),), (0, Fr(2, 3))), (Fr(1, 4), 0, Fr(3, 4))),
    "rk4": ((0, Fr(1, 3), Fr(2, 3), 1), ((), (Fr(1, 3),), (Fr(-1, 3), 1), (1, -1, 1)),
            (Fr(1, 8), Fr(3, 8), Fr(3, 8), Fr(1, 8))),
}

Eval = namedtuple("eval", "src c dst")
EvalFused = namedtuple("eval_fused", "src c base weight dst")
Combine = namedtuple("combine", "ks wa dst_a wb dst_b")
MAX_COMBINE_TERMS = 4          # n_k of fh_rk_combine_f32


def _check(method):
    if method not in ODE_METHODS:
        raise NotImplementedError(f"ode method {method!r}: the fixed-grid methods {', '.join(ODE_METHODS)} are built; "
                                  "adaptive methods (dopri5, dopri8, bosh3, fehlberg2, adaptive_heun) and the multistep ones are not")


def tableau(method):
    """(c, A, b) in floats: c and b of s entries, A of s rows, row j of its j leading entries."""
    _check(method)
    c, A, b = _TABLEAUS[method]
    return tuple(float(v) for v in c), tuple(tuple(float(v) for v in row) for row in A), tuple(float(v) for v in b)


def stages(method):
    _check(method)
    return len(_TABLEAUS[method][0])


def evaluations(method, time_steps, cond_scale=1.):
    """Passes of the vector field in one call: stages x steps, twice that under classifier-free guidance."""
    return stages(method) * int(time_steps) * (1 if float(cond_scale) == 1. else 2)


MAX_STEP_GROUPS = 8            # FH_MAX_GROUPS of include/flowhigh_hip.h: the groups of one launch of csrc/steps.hip

# groups: ((step count, number of segments), ...) in the segments' order, counts strictly descending.
# passes[p]: ((t0_g, dt_g), ...) of the groups still active in pass p (those of count > p: a prefix of `groups`), as 0-d float32
# tensors taken from torch.linspace(0, 1, count + 1)
MixedSchedule = namedtuple("mixed_schedule", "groups passes")


def check_steps(steps, n_clips, what="timestep"):
    """A step count argument -> an int (one count for every clip; a list of equal counts is that int) or a list of one int per
    clip.  Anything else is a ValueError: a bool, a float, a count below 1, a list of another length than n_clips."""
    def one(s):
        if isinstance(s, bool) or not isinstance(s, Integral) or int(s) < 1:
            raise ValueError(f"{what}: a step count is an int >= 1, got {s!r}")
        return int(s)
    if isinstance(steps, (list, tuple)):
        if len(steps) != n_clips:
            raise ValueError(f"{what}: {len(steps)} step counts for {n_clips} clips")
        steps = [one(s) for s in steps]
        return steps[0] if len(set(steps)) == 1 else steps
    return one(steps)


def order_by_steps(steps):
    """The positions 0 .. len(steps) - 1 sorted by step count, descending and stable (equal counts keep their order)."""
    return sorted(range(len(steps)), key=lambda i: -steps[i])


def split_by_steps(order, steps, max_groups=MAX_STEP_GROUPS):
    """`order` (order_by_steps) cut into consecutive sequences of at most max_groups distinct counts each."""
    out, cur, seen = [], [], []
    for i in order:
        if steps[i] not in seen:
            if len(seen) == max_groups:
                out.append(cur)
                cur, seen = [], []
            seen.append(steps[i])
        cur.append(i)
    if cur:
        out.append(cur)
    return out


def step_sequences(idx, counts, max_groups=MAX_STEP_GROUPS):
    """The clips idx, of step counts `counts`, as the ragged sequences they run in: [(clips, their counts), ...], sorted by count
    (descending, stable), cut at max_groups distinct counts; counts that are all one count are that int."""
    parts = split_by_steps(order_by_steps(counts), counts, max_groups)
    steps = [[counts[k] for k in part] for part in parts]
    return [([idx[k] for k in part], s[0] if len(set(s)) == 1 else s) for part, s in zip(parts, steps)]


def mixed_schedule(steps):
    """The time grid of one ragged sequence whose segments take different step counts: steps = the count of every segment,
    sorted descending (order_by_steps).  Segments of one count are a group (at most MAX_STEP_GROUPS); pass p = 0 .. max(steps) - 1
    runs the groups whose count is above p -- after the sort always a prefix of the segments -- and group g takes
    t0_g = linspace(0, 1, s_g + 1)[p] and dt_g = linspace[p + 1] - linspace[p] in float32, the expressions
    integrate.solve uses for a sequence of one count.  stage_time and fused_weight are its uniform form's too."""
    import torch
    steps = [int(s) for s in steps]
    if not steps or min(steps) < 1 or any(a < b for a, b in zip(steps, steps[1:])):
        raise ValueError(f"mixed_schedule: step counts >= 1 sorted descending, got {steps}")
    groups = []
    for s in steps:
        if groups and groups[-1][0] == s:
            groups[-1][1] += 1
        else:
            groups.append([s, 1])
    if len(groups) > MAX_STEP_GROUPS:
        raise ValueError(f"mixed_schedule: {len(groups)} distinct step counts, at most {MAX_STEP_GROUPS} in one sequence (split_by_steps)")
    grids = [torch.linspace(0, 1, s + 1) for s, _ in groups]
    passes = tuple(tuple((t[p], t[p + 1] - t[p]) for (s, _), t in zip(groups, grids) if s > p) for p in range(steps[0]))
    return MixedSchedule(tuple((s, n) for s, n in groups), passes)


def stage_time(t0, dt, c):
    """The time of a stage at c of a step from t0 of size dt (float32 tensors from the linspace grid) as the float the kernels take."""
    return float(t0) if c == 0. else float(t0 + c * dt)


def fused_weight(weight, dt):
    """weight * h of an eval_fused record, rounded as the float32 product it is."""
    return float(weight * dt)


def step_plan(method):
    """The records of one time step.  A stage's k is materialised only where something later reads it beside the next stage's
    input alone (then the stage is an eval_fused onto y: midpoint's first); the last stage is always an eval_fused onto
    base = y + h sum_{i<s} b_i k_i (y itself when those b_i are zero); the last stage's input and that base come out of one
    two-output combine."""
    c, A, b = tableau(method)
    s = len(c)
    plan, src, have = [], "y", []          # have: indices of the stages whose k is in a buffer
    for i in range(s - 1):
        j = i + 1                          # the stage whose input is made now
        last = j == s - 1
        later = [r for r in range(j + 1, s) if A[r][i] != 0.] + (["base"] if b[i] != 0. else [])
        alone = all(A[j][m] == 0. for m in range(i))
        wb = [b[m] for m in have] if last else []
        if not later and alone and not any(wb):
            if A[j][i] == 0.:              # nothing reads this stage at all: the input of the next one is y
                src = "y"
                continue
            plan.append(EvalFused(src, c[i], "y", A[j][i], "x"))
            src = "x"
            continue
        plan.append(Eval(src, c[i], f"k{i + 1}"))
        have.append(i)
        wa = [A[j][m] for m in have]
        wb = [b[m] for m in have] if last and any(b[m] != 0. for m in have) else None
        keep = [n for n in range(len(have)) if wa[n] != 0. or (wb is not None and wb[n] != 0.)]
        ks = tuple(f"k{have[n] + 1}" for n in keep)
        wa = tuple(wa[n] for n in keep)
        wb = None if wb is None else tuple(wb[n] for n in keep)
        assert len(ks) <= MAX_COMBINE_TERMS
        if not ks:                         # the next stage reads no k yet: it starts from y
            src = "y"
        elif not any(wa):                  # it starts from y, and the base is combined alone
            plan.append(Combine(ks, wb, "base", None, None))
            src = "y"
        else:
            plan.append(Combine(ks, wa, "x", wb, "base" if wb is not None else None))
            src = "x"
    base = "base" if any(isinstance(r, Combine) and "base" in (r.dst_a, r.dst_b) for r in plan) else "y"
    plan.append(EvalFused(src, c[s - 1], base, b[s - 1], "out"))
    return plan


def stage_names(plan):
    """The buffers a plan writes besides 'out' and 'x' (and 'y', which it only reads), sorted: 'base', 'k1', ..."""
    return sorted({d for r in plan for d in (r[-1], getattr(r, "dst_a", None)) if d not in (None, "out", "x")})


def run_step(plan, stage, field, combine):
    """One time step, the only loop over the records: `stage` maps names to buffers ('y' and 'out' set by the caller), the backend
    owns t0, h, guidance and rounding.  Its two callables return what they made and are handed the buffer of that name to write
    into (None where `stage` has none: then they return fresh values): field(src, c, base, weight, dst) -> base + (weight h)
    v(src, t0 + c h), or v raw with weight = base = None; combine(y, ks, wa, dst_a, wb, dst_b) -> the record's pair."""
    for r in plan:
        if isinstance(r, Combine):
            stage[r.dst_a], b = combine(stage["y"], [stage[k] for k in r.ks], r.wa, stage.get(r.dst_a), r.wb, stage.get(r.dst_b))
            if r.dst_b is not None:
                stage[r.dst_b] = b
        elif isinstance(r, Eval):
            stage[r.dst] = field(stage[r.src], r.c, None, None, stage.get(r.dst))
        else:
            stage[r.dst] = field(stage[r.src], r.c, stage[r.base], r.weight, stage.get(r.dst))
    return stage["out"]
