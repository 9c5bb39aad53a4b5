"""A plain-torch fixed-grid stepper over an explicit Butcher tableau: the reference the ODE tests compare against.

torchdiffeq's fixed-grid solvers (`odeint(fn, y0, t, method=...)[-1]`, the reference's call at cfm_superresolution.py:243) in the
textbook form, with tableaus written out here and NOT imported from flowhigh_amd.ode, so that a wrong coefficient there shows.
Dtype-generic: everything runs in the dtype of y0 and t.  f(t, y) is oracle.ref_cpu.vector_field or
tests/ref_convnext.convnext_forward wrapped by the caller."""
import torch

# method: (c, rows of A, b)
TABLEAUS = {
    "euler": ([0.], [[]], [1.]),
    "midpoint": ([0., 1 / 2], [[], [1 / 2]], [0., 1.]),
    "heun2": ([0., 1.], [[], [1.]], [1 / 2, 1 / 2]),
    "heun3": ([0., 1 / 3, 2 / 3], [[], [1 / 3], [0., 2 / 3]], [1 / 4, 0., 3 / 4]),
    "rk4": ([0., 1 / 3, 2 / 3, 1.], [[], [1 / 3], [-1 / 3, 1.], [1., -1., 1.]], [1 / 8, 3 / 8, 3 / 8, 1 / 8]),      # the 3/8 rule
}


def weighted(ks, ws):
    """sum_j ws[j] ks[j] over the non-zero weights, or None where there is none."""
    acc = None
    for k, w in zip(ks, ws):
        if w != 0.:
            acc = w * k if acc is None else acc + w * k
    return acc


def rk_step(f, y, t0, dt, method):
    c, A, b = TABLEAUS[method]
    ks = []
    for cj, row in zip(c, A):
        inc = weighted(ks, row)
        ks.append(f(t0 + cj * dt, y if inc is None else y + dt * inc))
    return y + dt * weighted(ks, b)


def odeint(f, y0, t, method):
    """y(t[-1]) from y(t[0]) = y0 over the grid t (a 1-D tensor), one step of `method` per interval."""
    y = y0
    for i in range(len(t) - 1):
        y = rk_step(f, y, t[i], t[i + 1] - t[i], method)
    return y


@torch.no_grad()
def sample_mel(field, cond_mel, noise, time_steps, method):
    """The sampler behind the log-mel (basic_cfm): field(y, cond_mel, t) integrated from the noise over linspace(0, 1)."""
    t = torch.linspace(0, 1, time_steps + 1, dtype=cond_mel.dtype)
    return odeint(lambda tt, y: field(y, cond_mel, tt), noise.to(cond_mel.dtype), t, method)
