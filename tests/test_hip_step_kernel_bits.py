"""GPU: the bits of the sampler's small kernels, pinned: the time embedding, the GEMV, the adaptive RMS norm, the RK combine and
the grouped field update, each through its one-time and its grouped entry, at the smallest shapes at which the kernel can go
wrong.  tests/golden/step_kernel_bits.json holds a SHA-256 of every output buffer (the NaN guard behind it included), recorded
before the one-time and the grouped kernel of an operator became one body: a change of these kernels must not move a bit.

Inputs are a closed formula of the element index and a seed (integer arithmetic mapped to float32, no library generator), so
the fixture does not depend on a numpy or torch version.
`python tests/test_hip_step_kernel_bits.py --record` rewrites the fixture from the library that is loaded."""
import ctypes
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowhigh_amd import hip             # noqa: E402

FIXTURE = Path(__file__).resolve().parent / "golden" / "step_kernel_bits.json"
GUARD = 64
ENDS = [(1, 5, 9), (9,), (1, 2, 3, 5, 6, 8, 9, 11)]
SCALARS = [0.25, 1 / 3, -0.7, 1.0, 0.125, 1e-3, 2 / 3, 0.9]          # a time / step size / alpha per group (rounded to float32 by ctypes)
M32 = np.uint64(0xFFFFFFFF)


def fill(shape, seed, scale=1.0):
    """Element i of buffer `seed`: a 32-bit integer mix of (i, seed), its top 24 bits as a float32 in [-1, 1), times scale."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    v = (np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9)) & M32
    for _ in range(2):
        v = ((v ^ (v >> np.uint64(16))) * np.uint64(0x45D9F3B)) & M32
    v = (v ^ (v >> np.uint64(16))) >> np.uint64(8)
    f = (v.astype(np.int64) - 2 ** 23).astype(np.float32) * np.float32(2.0 ** -23) * np.float32(scale)
    return torch.from_numpy(f.reshape(shape)).cuda()


def nan(n):
    return torch.full((n + GUARD,), float("nan"), device="cuda")


def sha(*bufs):
    torch.cuda.synchronize()
    return [hashlib.sha256(b.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for b in bufs]


def call(name, *args):
    hip.check(getattr(hip.lib(), name)(*args, hip.stream()), name)


def p(t):
    return hip.ptr(t)


def time_fourier():
    out = {}
    for half in (5, 512):
        w = fill(half, 1)
        o = nan(2 * half)
        call("fh_time_fourier_f32", p(w), 0.3, p(o), half)
        out[f"one half={half}"] = sha(o)
        for G in (3, 8):
            o = nan(G * 2 * half)
            call("fh_time_fourier_groups_f32", p(w), hip.group_floats(SCALARS[:G]), p(o), half, G)
            out[f"groups half={half} G={G}"] = sha(o)
    return out


def gemv():
    out = {}
    for N, K in ((6, 256), (1027, 1024), (8, 260)):
        ldx, ldy = K + 8, N + 3
        W, X, b = fill((N, K), 2, 2.0 ** -4), fill((8, ldx), 3), fill(N, 4)
        for act in (0, 1):
            for bias in (b, None):
                tag = f"N={N} K={K} act={act} bias={int(bias is not None)}"
                y = nan(N)
                call("fh_gemv_f32", p(W), p(X), p(bias), p(y), N, K, act)
                out["one " + tag] = sha(y)
                for T in (1, 3, 8):
                    Y = nan(T * ldy)
                    call("fh_gemv_rows_f32", p(W), p(X), ldx, p(bias), p(Y), ldy, N, K, T, act)
                    out[f"rows T={T} " + tag] = sha(Y)
    return out


def rmsnorm():
    out = {}
    for dim in (256, 4096):
        x, gamma, beta = fill((5, dim), 5, 4.0), fill(dim, 6), fill(dim, 7)
        for rows in (1, 5):
            for bt in (beta, None):
                y = nan(rows * dim)
                call("fh_rmsnorm_f32", p(x), p(gamma), p(bt), p(y), rows, dim)
                out[f"one dim={dim} rows={rows} beta={int(bt is not None)}"] = sha(y)
    for dim in (256, 1024):
        stride = 3 * dim + 4
        x, gb = fill((11, dim), 8, 4.0), fill((8, stride), 9)            # group g: gamma at gb[g, :dim], beta at gb[g, dim:2 dim]
        for ends in ENDS:
            rows, grp = ends[-1], ctypes.byref(hip.row_groups(ends))
            for tag, beta0, st_ in (("beta", p(gb[0, dim:]), stride), ("stride0", 0, 0)):
                y = nan(rows * dim)
                call("fh_rmsnorm_groups_f32", p(x), p(gb), beta0, st_, p(y), rows, dim, grp)
                out[f"groups dim={dim} ends={ends} {tag}"] = sha(y)
    return out


RK_ROWS = {"one": ((0.5, -1.0, 0.25), None), "two": ((0.5, -1.0, 0.25), (1 / 6, 2 / 3, 1 / 6)), "zero_mid": ((0.5, 0.0, 0.25), (0.0, 0.0, 1.0))}


def rk_call(entry, y, ks, h, wa, wb, out_a, out_b, shape):
    kp = (ctypes.c_void_p * len(ks))(*[k.data_ptr() for k in ks])
    fa = (ctypes.c_float * len(ks))(*wa)
    fb = None if wb is None else (ctypes.c_float * len(ks))(*wb)
    call(entry, p(y), kp, len(ks), h, fa, p(out_a), fb, p(out_b), *shape)


def rk_combine():
    out = {}
    for n in (4, 1028):
        for tag, (wa, wb) in RK_ROWS.items():
            y, ks = fill(n, 10), [fill(n, 11 + j) for j in range(3)]
            oa, ob = nan(n), (None if wb is None else nan(n))
            rk_call("fh_rk_combine_f32", y, ks, 0.3, wa, wb, oa, ob, (n,))
            out[f"one n={n} {tag}"] = sha(*([oa] if ob is None else [oa, ob]))
        # out_a onto y, out_b onto a k
        y, ks = fill(n, 10), [fill(n, 11 + j) for j in range(3)]
        wa, wb = RK_ROWS["two"]
        rk_call("fh_rk_combine_f32", y, ks, 0.3, wa, wb, y, ks[1], (n,))
        out[f"one n={n} aliased"] = sha(y, *ks)
    for dim in (256, 260):
        for ends in ENDS:
            rows, grp = ends[-1], ctypes.byref(hip.row_groups(ends))
            y, ks = fill(rows * dim, 14), [fill(rows * dim, 15 + j) for j in range(3)]
            for tag in ("one", "two"):
                wa, wb = RK_ROWS[tag]
                oa, ob = nan(rows * dim), (None if wb is None else nan(rows * dim))
                rk_call("fh_rk_combine_groups_f32", y, ks, hip.group_floats(SCALARS[:len(ends)]), wa, wb, oa, ob, (rows, dim, grp))
                out[f"groups dim={dim} ends={ends} {tag}"] = sha(*([oa] if ob is None else [oa, ob]))
    return out


def axpy_groups():
    out = {}
    ends, dim = ENDS[0], 260
    rows, grp = ends[-1], ctypes.byref(hip.row_groups(ends))
    v, res = fill(rows * dim, 18), fill(rows * dim, 19)
    for r in (res, None):
        o = nan(rows * dim)
        call("fh_axpy_groups_f32", p(v), hip.group_floats(SCALARS[:len(ends)]), p(r), p(o), rows, dim, grp)
        out[f"dim={dim} ends={ends} res={int(r is not None)}"] = sha(o)
    return out


OPERATORS = {"time_fourier": time_fourier, "gemv": gemv, "rmsnorm": rmsnorm, "rk_combine": rk_combine, "axpy_groups": axpy_groups}


def test_the_input_formula_is_what_the_fixture_was_recorded_with():
    """(the formula's own bits: a change of it would move every hash for a reason that is not the kernels')"""
    got = fill(4, 1).cpu().numpy().view(np.uint32).tolist() + fill(2, 9, 4.0).cpu().numpy().view(np.uint32).tolist()
    assert got == json.loads(FIXTURE.read_text())["input_formula"]


@pytest.mark.parametrize("operator", sorted(OPERATORS))
def test_every_output_buffer_has_the_recorded_bits(operator):
    want, got = json.loads(FIXTURE.read_text())[operator], OPERATORS[operator]()
    assert sorted(got) == sorted(want)
    moved = [case for case in got if got[case] != want[case]]
    assert not moved, f"{len(moved)} of {len(got)} cases moved: {moved[:4]}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_hip_step_kernel_bits.py --record   (writes tests/golden/step_kernel_bits.json)")
    rec = {name: fn() for name, fn in OPERATORS.items()}
    rec["input_formula"] = fill(4, 1).cpu().numpy().view(np.uint32).tolist() + fill(2, 9, 4.0).cpu().numpy().view(np.uint32).tolist()
    FIXTURE.write_text(json.dumps(rec, indent=0, sort_keys=True) + "\n")
    print({k: len(v) for k, v in rec.items()})
