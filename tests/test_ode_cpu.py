"""CPU: the ODE methods' host side -- the tableaus of flowhigh_amd/ode.py (consistency, order of accuracy), step_plan against the
textbook stepper (tests/ref_odeint.py) through ode.run_step, the loop the product runs, the product's uniform driver
(integrate.solve) on a recording net, evaluations(), the C ABI's new entry and its argument checks, the unknown-method error."""
import ctypes
import math
import re
from pathlib import Path

import pytest
import torch

import ref_odeint
from flowhigh_amd import hip, integrate, ode
from oracle import ref_cpu

ROOT = Path(__file__).resolve().parents[1]
NEW = ("heun2", "heun3", "rk4")
ORDER = dict(euler=1, midpoint=2, heun2=2, heun3=3, rk4=4)


def test_methods_and_tableaus_are_consistent():
    assert ode.ODE_METHODS == ("euler", "midpoint", "heun2", "heun3", "rk4")
    for method in ode.ODE_METHODS:
        c, A, b = ode.tableau(method)
        s = len(c)
        assert len(A) == len(b) == s == ode.stages(method)
        assert abs(sum(b) - 1.) <= 1e-15
        for j, row in enumerate(A):
            assert len(row) == j                                        # strictly lower triangular: row j has a_j1 .. a_j,j-1
            assert abs(sum(row) - c[j]) <= 1e-15, (method, j)
        rc_, rA, rb = ref_odeint.TABLEAUS[method]                       # the same numbers as the tests' own table
        assert list(c) == rc_ and [list(r) for r in A] == rA and list(b) == rb
    assert [ode.stages(m) for m in ode.ODE_METHODS] == [1, 2, 2, 3, 4]
    # the written-out coefficients of the three new methods
    assert ode.tableau("heun2") == ((0., 1.), ((), (1.,)), (.5, .5))
    assert ode.tableau("heun3") == ((0., 1 / 3, 2 / 3), ((), (1 / 3,), (0., 2 / 3)), (.25, 0., .75))
    assert ode.tableau("rk4") == ((0., 1 / 3, 2 / 3, 1.), ((), (1 / 3,), (-1 / 3, 1.), (1., -1., 1.)), (1 / 8, 3 / 8, 3 / 8, 1 / 8))


def _linear_problem_error(method, steps, stepper):
    """y' = -y + sin t, y(0) = 1 up to t = 1 in float64: |y_n - y(1)|; y(t) = 1.5 exp(-t) + (sin t - cos t) / 2."""
    t = torch.linspace(0, 1, steps + 1, dtype=torch.float64)
    y = stepper(lambda tt, yy: -yy + torch.sin(tt), torch.ones(1, dtype=torch.float64), t, method)
    return abs(y.item() - (1.5 * math.exp(-1.) + 0.5 * (math.sin(1.) - math.cos(1.))))


def run_plan(f, y0, t, method):
    """step_plan(method) on CPU tensors: ode.run_step, the loop integrate.solve runs with launches, over fresh tensors."""
    plan = ode.step_plan(method)
    y = y0
    for i in range(len(t) - 1):
        t0, h = t[i], t[i + 1] - t[i]

        def field(src, c, base, weight, dst):
            v = f(t0 + c * h, src)
            return v if weight is None else base + (weight * h) * v

        def combine(y_, ks, wa, dst_a, wb, dst_b):
            assert 1 <= len(ks) == len(wa) <= ode.MAX_COMBINE_TERMS and any(wa) and (wb is None or (any(wb) and len(wb) == len(ks)))
            return tuple(None if w is None else y_ + h * ref_odeint.weighted(ks, w) for w in (wa, wb))

        y = ode.run_step(plan, {"y": y}, field, combine)
    return y


@pytest.mark.parametrize("method", NEW)
def test_order_of_accuracy(method):
    for stepper in (ref_odeint.odeint, run_plan):
        e8, e16, e32 = (_linear_problem_error(method, n, stepper) for n in (8, 16, 32))
        p1, p2 = math.log2(e8 / e16), math.log2(e16 / e32)
        print(f"{method} ({stepper.__name__}): errors {e8:.3e} {e16:.3e} {e32:.3e}, observed order {p1:.2f} / {p2:.2f}")
        assert abs(p1 - ORDER[method]) <= 0.25 and abs(p2 - ORDER[method]) <= 0.25


@pytest.mark.parametrize("method", ode.ODE_METHODS)
def test_step_plan_reproduces_the_textbook_stepper(method):
    g = torch.Generator().manual_seed(11)
    M = torch.randn(6, 6, generator=g, dtype=torch.float64) * 0.7
    y0 = torch.randn(5, 6, generator=g, dtype=torch.float64)
    f = lambda tt, y: torch.tanh(y @ M) * (1. + tt) - 0.3 * y * torch.cos(3. * tt)          # non-linear, time-dependent
    for steps in (1, 3):
        t = torch.linspace(0, 1, steps + 1, dtype=torch.float64)
        ref, got = ref_odeint.odeint(f, y0, t, method), run_plan(f, y0, t, method)
        assert ((got - ref).abs() / ref.abs().clamp_min(1.)).max().item() <= 1e-13
    other = "rk4" if method != "rk4" else "heun3"
    t = torch.linspace(0, 1, 2, dtype=torch.float64)
    assert (ref_odeint.odeint(f, y0, t, method) - ref_odeint.odeint(f, y0, t, other)).abs().max().item() > 1e-4      # different samplers


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_textbook_stepper_is_the_oracles_on_its_two_methods(method):
    g = torch.Generator().manual_seed(12)
    M, y0 = torch.randn(6, 6, generator=g) * 0.7, torch.randn(5, 6, generator=g)
    f = lambda tt, y: torch.tanh(y @ M) * (1. + tt)
    t = torch.linspace(0, 1, 4)
    assert torch.equal(ref_odeint.odeint(f, y0, t, method), ref_cpu.odeint_fixed(f, y0, t, method))


def test_plans_launches_per_step():
    kinds = lambda m: [type(r).__name__ for r in ode.step_plan(m)]
    # euler and midpoint: the launches they always were -- fused evaluations onto y and nothing else
    assert ode.step_plan("euler") == [ode.EvalFused("y", 0., "y", 1., "out")]
    assert ode.step_plan("midpoint") == [ode.EvalFused("y", 0., "y", .5, "x"), ode.EvalFused("x", .5, "y", 1., "out")]
    for m in ("euler", "midpoint"):
        assert "combine" not in kinds(m) and "eval" not in kinds(m)
    assert kinds("heun2") == ["eval", "combine", "eval_fused"]
    assert kinds("heun3") == ["eval", "combine", "eval", "combine", "eval_fused"]
    assert kinds("rk4") == ["eval", "combine", "eval", "combine", "eval", "combine", "eval_fused"]
    for m in ode.ODE_METHODS:
        plan = ode.step_plan(m)
        assert sum(not isinstance(r, ode.Combine) for r in plan) == ode.stages(m)
        assert isinstance(plan[-1], ode.EvalFused) and plan[-1].dst == "out" and plan[-1].weight == ode.tableau(m)[2][-1]
        assert sum(r.wb is not None for r in plan if isinstance(r, ode.Combine)) == (m in NEW)      # one two-output combine
        for r in plan:
            if isinstance(r, ode.Combine):
                assert 1 <= len(r.ks) == len(r.wa) <= ode.MAX_COMBINE_TERMS
                assert (r.wb is None) == (r.dst_b is None) and any(r.wa) and (r.wb is None or (any(r.wb) and len(r.wb) == len(r.ks)))
    # the buffers a stepper allocates besides 'y', 'out' and 'x'
    assert [ode.stage_names(ode.step_plan(m)) for m in ode.ODE_METHODS] == \
        [[], [], ["base", "k1"], ["base", "k1", "k2"], ["base", "k1", "k2", "k3"]]
    last = ode.step_plan("rk4")[-2]
    assert last == ode.Combine(("k1", "k2", "k3"), (1., -1., 1.), "x", (1 / 8, 3 / 8, 3 / 8), "base")
    assert ode.step_plan("heun3")[3] == ode.Combine(("k1", "k2"), (0., 2 / 3), "x", (.25, 0.), "base")


def test_evaluations():
    assert ode.evaluations("euler", 1) == 1 and ode.evaluations("midpoint", 4) == 8
    assert ode.evaluations("heun2", 3) == 6 and ode.evaluations("heun3", 2) == 6 and ode.evaluations("rk4", 2) == 8
    assert ode.evaluations("rk4", 2, cond_scale=1.3) == 16 and ode.evaluations("rk4", 1, 1.) == 4


def test_unknown_and_adaptive_methods_name_the_supported_set():
    for name in ("dopri5", "rk45", "adaptive_heun", None):
        for call in (lambda: ode.step_plan(name), lambda: ode.evaluations(name, 1), lambda: ode.tableau(name)):
            with pytest.raises(NotImplementedError, match=r"euler, midpoint, heun2, heun3, rk4.*adaptive") as e:
                call()
            assert repr(name) in str(e.value)

    class Net:                                                # integrate.solve asks for the plan before it touches the net
        def set_cond(self, *a, **k):
            raise AssertionError("the method was not checked first")
    with pytest.raises(NotImplementedError, match=r"heun3.*adaptive"):
        integrate.solve(Net(), "dopri5", torch.zeros(4, 4), torch.zeros(4, 4), 1, 4, 1)


class _RecordingNet:
    """The two methods integrate.solve calls on a net, recorded; nothing is computed."""
    def __init__(self):
        self.calls = []

    def set_cond(self, cond, batch, n, ragged=None):
        self.calls.append(("set_cond", cond, batch, n, ragged))

    def forward(self, x, t, out, batch, n, alpha=1., res=None, null_cond=False, ragged=None):
        self.calls.append(("forward", x, t, out, batch, n, alpha, res, null_cond, ragged))


@pytest.mark.parametrize("cond_scale", [1.0, 1.3])
@pytest.mark.parametrize("steps", [1, 2, 4])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_uniform_backend_sequences_forward_calls(method, steps, cond_scale):
    """The product's uniform driver on CPU tensors (euler and midpoint launch no library entry of their own): every record is
    one net.forward at the record's time and weight from the linspace grid, onto the record's base, or under guidance two
    chained calls through one scratch buffer; set_cond comes once, first; the steps' results alternate between two buffers."""
    net, y0, cond = _RecordingNet(), torch.zeros(6, 4), torch.ones(6, 4)
    got = integrate.solve(net, method, y0, cond, 2, 3, steps, cond_scale)
    assert net.calls[0][0] == "set_cond" and net.calls[0][1] is cond and net.calls[0][2:] == (2, 3, None)
    calls = net.calls[1:]
    assert all(c[0] == "forward" and c[4:6] == (2, 3) and c[9] is None for c in calls)
    plan, t = ode.step_plan(method), torch.linspace(0, 1, steps + 1)
    assert len(calls) == len(plan) * steps * (1 if cond_scale == 1. else 2)
    calls, y, outs, scratch = iter(calls), y0, [], None
    for i in range(steps):
        t0, dt = t[i], t[i + 1] - t[i]
        named = {"y": y}
        for r in plan:                                        # (eval_fused records only: test_plans_launches_per_step)
            tt, h = ode.stage_time(t0, dt, r.c), ode.fused_weight(r.weight, dt)
            _, x, t_a, out, _, _, alpha, res, null, _ = next(calls)
            if cond_scale != 1.:
                assert (t_a, alpha, null) == (tt, h * (1. - 1.3), True) and x is named[r.src] and res is named[r.base]
                scratch = out if scratch is None else scratch
                assert out is scratch
                _, x, t_a, out, _, _, alpha, res, null, _ = next(calls)
                assert (t_a, alpha, null) == (tt, h * 1.3, False) and x is named[r.src] and res is scratch
            else:
                assert (t_a, alpha, null) == (tt, h, False) and x is named[r.src] and res is named[r.base]
            assert all(out is not b for b in (scratch, y0, cond, *named.values()))
            named[r.dst] = out
        y = named["out"]
        outs.append(y)
    assert got is y and next(calls, None) is None
    assert all(a is not b for a, b in zip(outs, outs[1:])) and all(a is b for a, b in zip(outs, outs[2:]))


def test_header_exports_and_abi_are_consistent():
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    name = "fh_rk_combine_f32"
    m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/flowhigh_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert name in hip.EXPORTS and len(hip._SIGS[name]) == len(params) == 10
    for p, ctype in zip(params, hip._SIGS[name]):          # pointer / int / float / long long, in the header's order
        kind = hip._P if "*" in p else hip._F if p.startswith("float") else hip.C.c_longlong if p.startswith("long long") else hip._I
        assert ctype is kind, (name, p)
    assert "ode.hip" in __import__("flowhigh_amd.build", fromlist=["SOURCES"]).SOURCES


def test_library_exports_the_entry_and_checks_its_arguments():
    """The argument checks run on the host before anything is launched, so they can be called without a GPU: the device
    pointers are fake aligned addresses, never dereferenced; ks / wa / wb are the host arrays the entry reads."""
    from flowhigh_amd import build
    build.build(verbose=False)
    L = hip.lib()
    Y, OA, OB = 256, 512, 768
    ks = (ctypes.c_void_p * 4)(1024, 1280, 1536, 1792)
    w = (ctypes.c_float * 4)(1., -1., .5, .25)
    zero = (ctypes.c_float * 4)(0., 0., 0., 0.)

    def bad(*args, say):
        assert L.fh_rk_combine_f32(*args, 0) == -1
        msg = L.fh_last_error()
        assert b"fh_rk_combine_f32" in msg and say in msg, msg

    bad(Y, ks, 0, .5, w, OA, None, 0, 1024, say=b"n_k 0")
    bad(Y, ks, 5, .5, w, OA, None, 0, 1024, say=b"n_k 5")
    bad(Y, ks, 3, .5, w, OA, None, 0, 6, say=b"n 6")
    bad(Y, ks, 3, .5, w, OA, None, 0, 0, say=b"n 0")
    bad(Y + 4, ks, 3, .5, w, OA, None, 0, 1024, say=b"aligned")
    bad(Y, ks, 3, .5, w, OA + 8, None, 0, 1024, say=b"aligned")
    bad(Y, ks, 3, .5, w, OA, w, OB + 4, 1024, say=b"aligned")
    bad(Y, (ctypes.c_void_p * 4)(1024, 1284, 1536, 1792), 3, .5, w, OA, None, 0, 1024, say=b"stage field 1")
    bad(Y, (ctypes.c_void_p * 4)(1024, None, 1536, 1792), 2, .5, w, OA, None, 0, 1024, say=b"stage field 1")
    bad(Y, ks, 3, .5, w, OA, w, 0, 1024, say=b"wb and out_b")
    bad(Y, ks, 3, .5, w, OA, None, OB, 1024, say=b"wb and out_b")
    bad(Y, ks, 3, .5, zero, OA, None, 0, 1024, say=b"all zero")
    bad(Y, ks, 3, .5, w, OA, zero, OB, 1024, say=b"all zero")
    bad(Y, ks, 3, .5, w, OA, w, OA, 1024, say=b"same buffer")
    bad(0, ks, 3, .5, w, OA, None, 0, 1024, say=b"must be given")
    bad(Y, None, 3, .5, w, OA, None, 0, 1024, say=b"must be given")
    bad(Y, ks, 3, .5, None, OA, None, 0, 1024, say=b"must be given")
    bad(Y, ks, 3, .5, w, 0, None, 0, 1024, say=b"must be given")
