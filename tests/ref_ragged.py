"""Float64 references for the kernel-level tests of the ragged vocoder launches (test_hip_ragged_launches.py,
test_ragged_launches_cpu.py): plain restatements of the definitions, no tiling, no layout."""
import torch
import torch.nn.functional as F


def activation1d_f64(x, alpha, inv_beta, up, down):
    """The closed form in the header of csrc/act1d.hip, in float64.  x [C, L]; alpha, inv_beta [C]; up, down: 12 taps each.
        z[2i]   = snake(2 sum_{q=-3..2} x[i+q] f_up[5-2q])       z[2i+1] = snake(2 sum_{q=-2..3} x[i+q] f_up[6-2q])
        y[i]    = sum_{k=0..11} z[2i+k-5] f_dn[k]                snake(v) = v + inv_beta sin^2(alpha v)
    with the x index clamped to [0, L-1] and the z index to [0, 2L-1]."""
    x = x.double()
    C, L = x.shape
    fu, fd = torch.as_tensor(up, dtype=torch.float64), torch.as_tensor(down, dtype=torch.float64)
    a, ib = alpha.double().view(C, 1), inv_beta.double().view(C, 1)
    i = torch.arange(L)
    xat = lambda j: x[:, j.clamp(0, L - 1)]
    even = 2 * sum(xat(i + q) * fu[5 - 2 * q] for q in range(-3, 3))
    odd = 2 * sum(xat(i + q) * fu[6 - 2 * q] for q in range(-2, 4))
    v = torch.stack([even, odd], dim=-1).reshape(C, 2 * L)
    z = v + ib * torch.sin(a * v) ** 2
    return sum(z[:, (2 * i + k - 5).clamp(0, 2 * L - 1)] * fd[k] for k in range(12))


def conv1d_f64(xs, ws, bias, res, scale, dilation):
    """(sum over segments of Conv1d(x, w), "same" padding (k - 1) // 2 * dilation, + bias + residuals) * scale in float64.
    xs [C_in, L], ws [C_out, C_in, k] (k odd), bias [C_out] or None, res: list of [C_out, L]."""
    y = sum(F.conv1d(x.double()[None], w.double(), None, dilation=dilation, padding=(w.shape[-1] - 1) // 2 * dilation)[0]
            for x, w in zip(xs, ws))
    if bias is not None:
        y = y + bias.double()[:, None]
    return (y + sum(r.double() for r in res)) * scale


def conv1d_abs_f64(xs, ws, bias, res, scale, dilation):
    """A of the fp32 bound (K + 3) u A: the same expression over absolute values."""
    return conv1d_f64([x.abs() for x in xs], [w.abs() for w in ws], None if bias is None else bias.abs(), [r.abs() for r in res],
                      abs(scale), dilation)
