"""Fixed-grid ODE methods of the sampler: explicit Butcher tableaus and the launch plan of one time step.

The reference hands `torchdiffeq_ode_method` to torchdiffeq.odeint (cfm_superresolution.py:115-119,243); the fixed-grid solvers of
that library are restated here as tableaus (c, A, b):  k_j = v(y + h sum_i a_ji k_i, t0 + c_j h),  y' = y + h sum_j b_j k_j.
`step_plan` turns a tableau into named records, in the style of the vocoder's launch records; FlowHighSR._integrate runs them.
No GPU import: the plans are plain data and are checked on the CPU (tests/test_ode_cpu.py).

    eval(src, c, dst)                      dst = v(src, t0 + c h)                    the field written raw (alpha = 1, res = None)
    eval_fused(src, c, base, weight, dst)  dst = base + (weight h) v(src, t0 + c h)  the update in the last GEMM's epilogue
    combine(ks, wa, dst_a, wb, dst_b)      dst_a = y + h sum_j wa_j ks_j  (and dst_b with wb, or wb = dst_b = None): one launch
                                           of fh_rk_combine_f32 (csrc/ode.hip)

Buffer names: 'y' the step's input, 'out' its result, 'x' the input of the next stage, 'base' the last stage's base
y + h sum_{i<s} b_i k_i, 'k1', 'k2', ... the stages' fields.
"""
from collections import namedtuple
from fractions import Fraction as Fr

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
