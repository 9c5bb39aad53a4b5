"""CPU: one step count per clip -- the schedule of a ragged sequence whose segments take different counts (ode.mixed_schedule),
the argument checks, the reordering and splitting of a list of counts, and BatchingServer(mix_steps=).  No GPU, no library."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ref_odeint                                                          # noqa: E402
from flowhigh_amd import grouping, ode                                     # noqa: E402
from flowhigh_amd import serve                                             # noqa: E402

CASES = [[4, 4, 2, 1], [3, 1], [1], [9, 8, 7, 7, 6, 5, 4, 3, 2]]          # (the last: 8 distinct counts)


# ------------------------------------------------------------------------------------------
# the schedule
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", CASES)
def test_schedule_is_the_linspace_grid_of_every_count(steps):
    sched = ode.mixed_schedule(steps)
    counts = [s for s, _ in sched.groups]
    assert counts == sorted(set(steps), reverse=True) and len(counts) <= ode.MAX_STEP_GROUPS
    assert [n for _, n in sched.groups] == [steps.count(s) for s in counts]
    assert len(sched.passes) == max(steps)
    seen = {s: [] for s in counts}
    for p, active in enumerate(sched.passes):
        # the active groups: those with a step p, a prefix of the groups
        assert len(active) == sum(1 for s in counts if s > p) >= 1
        for s, (t0, dt) in zip(counts, active):
            assert s > p and t0.dtype == dt.dtype == torch.float32
            seen[s].append((t0, dt))
    for s in counts:
        t = torch.linspace(0, 1, s + 1)                      # what integrate.solve takes for a sequence of that count alone
        assert len(seen[s]) == s
        for i, (t0, dt) in enumerate(seen[s]):
            assert torch.equal(t0, t[i]) and torch.equal(dt, t[i + 1] - t[i])

            def field(src, c, base, weight, dst):            # every evaluation of a step: its time and its weight
                assert ode.stage_time(t0, dt, c) == (float(t[i]) if c == 0. else float(t[i] + c * (t[i + 1] - t[i])))
                if weight is not None:
                    assert ode.fused_weight(weight, dt) == float(weight * (t[i + 1] - t[i]))
            for method in ode.ODE_METHODS:
                ode.run_step(ode.step_plan(method), {"y": None}, field, lambda *args: (None, None))


def test_schedule_refuses_what_is_not_sorted_or_too_many_counts():
    for bad in ([], [1, 2], [2, 0], [3, 2, 3]):
        with pytest.raises(ValueError):
            ode.mixed_schedule(bad)
    with pytest.raises(ValueError, match="9 distinct"):
        ode.mixed_schedule(list(range(9, 0, -1)))


# ------------------------------------------------------------------------------------------
# integration over the schedule, all groups in lock-step, against the textbook stepper per clip
# ------------------------------------------------------------------------------------------
def coeff_a(t):
    return np.cos(3.0 * t) - 0.5


def coeff_b(t):
    return np.sin(2.0 * t) + 0.25


def integrate_lockstep(method, steps, y0):
    """The records of step_plan(method) over mixed_schedule(steps) in numpy float64, as integrate.solve sequences its grouped
    form: pass p is ode.run_step over the rows of the active prefix, every row at its group's time and step, a group's rows
    copied out after its last step.  y0 [len(steps), d]; dy/dt = a(t) y + b(t)."""
    sched, plan = ode.mixed_schedule(steps), ode.step_plan(method)
    seg_end = np.cumsum([n for _, n in sched.groups])
    y, result = y0.copy(), np.full_like(y0, np.nan)
    for p, active in enumerate(sched.passes):
        G = len(active)
        rows = int(seg_end[G - 1])
        per_row = np.repeat(np.arange(G), [n for _, n in sched.groups[:G]])
        t0 = np.array([float(a[0]) for a in active])[per_row][:, None]
        dt = np.array([float(a[1]) for a in active])[per_row][:, None]

        def field(src, c, base, weight, dst):
            tt = t0 + c * dt
            v = coeff_a(tt) * src + coeff_b(tt)
            return v if weight is None else base + (weight * dt) * v

        def combine(y_, ks, wa, dst_a, wb, dst_b):
            return tuple(None if w is None else y_ + dt * sum(wj * k for wj, k in zip(w, ks) if wj != 0.) for w in (wa, wb))

        out = ode.run_step(plan, {"y": y[:rows]}, field, combine)
        y = y.copy()
        y[:rows] = out
        for g, (s, _) in enumerate(sched.groups[:G]):
            if s == p + 1:
                r0 = int(seg_end[g - 1]) if g else 0
                result[r0:seg_end[g]] = y[r0:seg_end[g]]
    return result


@pytest.mark.parametrize("method", ode.ODE_METHODS)
@pytest.mark.parametrize("steps", CASES)
def test_lockstep_integration_equals_the_textbook_stepper_per_clip(method, steps):
    y0 = np.random.default_rng(len(steps)).standard_normal((len(steps), 5))
    got = integrate_lockstep(method, steps, y0)
    assert np.isfinite(got).all()
    for i, s in enumerate(steps):
        t = torch.linspace(0, 1, s + 1).double()
        f = lambda tt, y: torch.cos(3.0 * tt) * y - 0.5 * y + torch.sin(2.0 * tt) + 0.25          # noqa: E731
        want = ref_odeint.odeint(f, torch.from_numpy(y0[i]), t, method).numpy()
        assert np.abs(got[i] - want).max() <= 1e-12, (method, steps, i)


# ------------------------------------------------------------------------------------------
# arguments, reordering, splitting
# ------------------------------------------------------------------------------------------
def test_check_steps_takes_an_int_or_one_int_per_clip():
    assert ode.check_steps(4, 3) == 4
    assert ode.check_steps([2, 2, 2], 3) == 2                      # a list of equal counts is the int
    assert ode.check_steps((1, 4, 2), 3) == [1, 4, 2]
    assert ode.check_steps([np.int64(3), 1], 2) == [3, 1]
    for bad in ([1, 2], [1, 2, 3, 4]):
        with pytest.raises(ValueError, match=f"{len(bad)} step counts for 3 clips"):
            ode.check_steps(bad, 3)
    for bad in ([1, 0, 2], [1, True, 2], [1, 2.0, 2], [1, -1, 2], [1, None, 2], 0, True, 1.0, "2"):
        with pytest.raises(ValueError):
            ode.check_steps(bad, 3)


def test_reordering_is_stable_and_inverted_exactly():
    steps = [1, 4, 2, 4, 1, 2, 4]
    order = ode.order_by_steps(steps)
    assert order == [1, 3, 6, 2, 5, 0, 4]                          # descending, equal counts in list order
    assert [steps[i] for i in order] == sorted(steps, reverse=True)
    results = [f"clip{i}" for i in order]                          # what a run over the sorted clips returns
    back = [None] * len(steps)
    for i, y in zip(order, results):
        back[i] = y
    assert back == [f"clip{i}" for i in range(len(steps))]
    assert ode.order_by_steps([3, 3, 3]) == [0, 1, 2]


def test_nine_distinct_counts_split_into_two_sequences():
    steps = [5, 1, 9, 3, 3, 7, 2, 8, 6, 4, 9]
    order = ode.order_by_steps(steps)
    parts = ode.split_by_steps(order, steps)
    assert len(parts) == 2 and [i for part in parts for i in part] == order
    assert sorted({steps[i] for i in parts[0]}, reverse=True) == [9, 8, 7, 6, 5, 4, 3, 2] and {steps[i] for i in parts[1]} == {1}
    for part in parts:
        ode.mixed_schedule([steps[i] for i in part])               # (each is a schedule of at most 8 groups)
    assert ode.split_by_steps(ode.order_by_steps([2, 1, 2]), [2, 1, 2]) == [[0, 2, 1]]
    assert ode.split_by_steps(ode.order_by_steps([2, 1, 2]), [2, 1, 2], 1) == [[0, 2], [1]]


def test_step_sequences_sort_cut_and_collapse_one_count_to_an_int():
    """The clips of a group -> (clips, an int or a descending list of counts) per ragged sequence, the clips by their own ids."""
    idx = [10, 11, 12, 13, 14, 15, 16]
    assert ode.step_sequences(idx, [1, 4, 2, 4, 1, 2, 4]) == [([11, 13, 16, 12, 15, 10, 14], [4, 4, 4, 2, 2, 1, 1])]
    assert ode.step_sequences(idx[:3], [3, 3, 3]) == [([10, 11, 12], 3)]                  # one count: the int, the order kept
    assert ode.step_sequences(idx[:1], [5]) == [([10], 5)] and ode.step_sequences([], []) == []
    # one distinct count per sequence (a backbone without the grouped field): every sequence an int
    assert ode.step_sequences(idx[:4], [2, 1, 2, 3], 1) == [([13], 3), ([10, 12], 2), ([11], 1)]
    # nine distinct counts: eight in the first sequence, the last count alone and therefore an int
    steps = [5, 1, 9, 3, 3, 7, 2, 8, 6, 4, 9, 1]
    seqs = ode.step_sequences(list(range(100, 112)), steps)
    assert [c for c, _ in seqs] == [[102, 110, 107, 105, 108, 100, 109, 103, 104, 106], [101, 111]]
    assert [s for _, s in seqs] == [[9, 9, 8, 7, 6, 5, 4, 3, 3, 2], 1]
    for clips, counts in seqs:                                                           # (what split_by_steps gives, by ids)
        assert isinstance(counts, int) or counts == [steps[i - 100] for i in clips]
    order = ode.order_by_steps(steps)
    assert [[100 + k for k in part] for part in ode.split_by_steps(order, steps)] == [c for c, _ in seqs]


def test_buckets_take_the_step_count_into_their_key():
    lengths, rates, shapes = [100, 100, 100, 200], [12000] * 4, [(1, 4, 8)] * 3 + [(1, 8, 8)]
    assert [p[2] for p in grouping.plan_buckets(lengths, rates, shapes, 1, 64)[1]] == [[0, 1, 2], [3]]
    assert [p[2] for p in grouping.plan_buckets(lengths, rates, shapes, 1, 64, steps=[1, 2, 1, 1])[1]] == [[0, 2], [1], [3]]


# ------------------------------------------------------------------------------------------
# BatchingServer(mix_steps=)
# ------------------------------------------------------------------------------------------
def test_resolve_mix_steps(monkeypatch):
    monkeypatch.delenv("FH_SERVE_MIX_STEPS", raising=False)
    assert serve.MIX_STEPS_DEFAULT is False and serve.resolve_mix_steps() is False
    assert serve.resolve_mix_steps(True) is True and serve.resolve_mix_steps(False) is False
    for env, want in (("1", True), ("0", False), ("", False)):
        monkeypatch.setenv("FH_SERVE_MIX_STEPS", env)
        assert serve.resolve_mix_steps() is want
        assert serve.resolve_mix_steps(not want) is (not want)         # the keyword wins
    monkeypatch.setenv("FH_SERVE_MIX_STEPS", "yes")
    with pytest.raises(ValueError, match="FH_SERVE_MIX_STEPS"):
        serve.resolve_mix_steps()


class _StubModel:
    def __init__(self):
        self.calls = []

    def _draw_noise(self, batch, n_frames, generator):
        return torch.randn(batch, n_frames, 4, generator=generator)

    def generate_many(self, clips, sr, target, steps, noise=None, max_batch=64):
        self.calls.append((len(clips), sr, steps))
        return [torch.from_numpy(np.asarray(c, dtype=np.float32))[None] * (s if isinstance(steps, list) else steps)
                for c, s in zip(clips, steps if isinstance(steps, list) else [steps] * len(clips))]


def _serve(monkeypatch, requests, **kw):
    monkeypatch.delenv("FH_SERVE_MIX_STEPS", raising=False)
    monkeypatch.delenv("FH_SERVE_MIX_RATES", raising=False)
    monkeypatch.delenv("FH_RAGGED_ENDS", raising=False)
    m = _StubModel()
    srv = serve.BatchingServer(m, max_batch=len(requests), max_wait_ms=2000, **kw)
    clips = [np.full(100 + 10 * i, 1.0 + i, dtype=np.float32) for i in range(len(requests))]
    futs = [srv.submit(c, 12000, timestep=s) for c, s in zip(clips, requests)]
    outs = [f.result(timeout=30) for f in futs]
    srv.close()
    for c, s, o in zip(clips, requests, outs):                     # every caller gets its clip, run at its count
        assert np.array_equal(o, c * s)
    return srv, m.calls


def test_server_with_mix_steps_hands_one_list_to_one_call(monkeypatch):
    srv, calls = _serve(monkeypatch, [1, 2, 4], mix_steps=True)
    assert srv.mix_steps is True
    assert calls == [(3, 12000, [1, 2, 4])]
    # a window of one count: the int, as always
    _, calls = _serve(monkeypatch, [2, 2], mix_steps=True)
    assert calls == [(2, 12000, 2)]


def test_default_server_hands_one_int_per_call(monkeypatch):
    srv, calls = _serve(monkeypatch, [1, 2, 4, 2])
    assert srv.mix_steps is False
    assert sorted(calls) == [(1, 12000, 1), (1, 12000, 4), (2, 12000, 2)]
    monkeypatch.setenv("FH_SERVE_MIX_STEPS", "1")
    by_env = serve.BatchingServer(_StubModel(), max_wait_ms=1)
    assert by_env.mix_steps is True
    by_env.close()
