"""sha256 of every output of a fixed, seeded list of Winograd conv launches: run once per library (FH_LIB_PATH) in a fresh
process and compare the two listings -- a refactor of conv_wino.hip / conv_wino54_kernel.h must not move a bit.
    python tools/wino_hash.py [out_file]            one line per launch: <name> <sha256>
Every case is c = 384 (a multiple of every block height: 32 / 48 / 64 / 96 / 128), B = 2 (the transposed-conv cases: 192 -> 384
channels).  The list reaches all 32 instantiations: F(4,3) tiles 0 1 4 5 6 and F(5,4) tiles 0 1 2 3 in the fp32 form, F(4,3)
0 1 4 5 6 and F(5,4) 1 2 in the bf16 x 6 form, each with the 16-byte and the 4-byte loader.  Per (kernel, tile, form):
  rows    plain d = 1 L = 1000 and phase-major d = 3 L = 999 (16-byte loader); plain d = 1 L = 1001 and d = 3 L = 778 (4-byte)
  nres    0 .. 3 residuals at L = 1000 (the row ends inside a block: 16-byte stores and the 4-byte tail in one launch)
  seg3    three segments k = 11 / 7 / 3, three residuals, scale 1/3
  ragged  both ragged entries' shapes: clips of 3000 / 1200 / 332 samples (16-byte) and 3000 / 1200 / 333 (4-byte), run_map
  xcd     F(4,3) only: FH_WINO_XCD_RANGES
  convt   F(4,3) only: a transposed conv's phase groups (out_stride > 1; k - u even, and odd: xlen / out_len set)"""
import hashlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowhigh_amd import hip, vocoder as V      # noqa: E402

DEV = torch.device("cuda:0")
C, B = 384, 2
LINES = []
_packed = {}


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def emit(name, out):
    torch.cuda.synchronize()
    LINES.append(f"{name} {hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}")


def weight(f54, bf, k, seed, cin=C, cout=C):
    key = (f54, bf, k, seed, cin, cout)
    if key not in _packed:
        w = rnd(cout, cin, k, seed=seed, scale=1.0 / (cin * k) ** 0.5)
        _packed[key] = (V.pack_wino54_weight_any if f54 else V.pack_wino_weight_any)(w, cout, bf).to(DEV)
    return _packed[key]


def conv(name, f54, tile, bf, ks, L, d=1, pm=False, nres=0, scale=1.0, flags=0):
    lay = (lambda t: V.to_phase_major(t, d)) if pm else (lambda t: t)
    xs = [lay(rnd(B, C, L, seed=10 + i)).to(DEV) for i in range(len(ks))]
    res = [lay(rnd(B, C, L, seed=20 + i)).to(DEV) for i in range(nres)]
    us = [weight(f54, bf, k, 30 + i) for i, k in enumerate(ks)]
    bias = rnd(C, seed=40).to(DEV)
    out = torch.full_like(xs[0], float("nan"))
    g = V.make_wino_group([V.make_wino_seg(x, u, C, k, taps=4 if f54 else 3) for x, u, k in zip(xs, us, ks)], bias, res, out, C, C, L,
                          scale=scale)
    keep = V.conv_wino([g], B, C, L, d, DEV, (V.WINO_F54 if f54 else 0) | tile | (V.WINO_BF16X6 if bf else 0) | flags, phase_major=pm)
    emit(name, out)
    del keep


def ragged(name, f54, tile, bf, lens):
    lib, k = hip.lib(), 7
    u, bias = weight(f54, bf, k, 30), rnd(C, seed=40).to(DEV)
    xs = [rnd(1, C, L, seed=50 + i).to(DEV) for i, L in enumerate(lens)]
    res = [rnd(1, C, L, seed=60 + i).to(DEV) for i, L in enumerate(lens)]
    outs = [torch.full_like(x, float("nan")) for x in xs]
    groups = [V.make_wino_group([V.make_wino_seg(x, u, C, k, taps=4 if f54 else 3)], bias, [r], o, C, C, L)
              for x, r, o, L in zip(xs, res, outs, lens)]
    cfg = tile | (V.WINO_BF16X6 if bf else 0)
    bm = lib.fh_wino54_tile_m(cfg) if f54 else lib.fh_wino_tile_m(cfg)
    bt = lib.fh_wino54_tile_n() if f54 else lib.fh_wino_tile_n(cfg)
    n_tiles = -(-max(lens) // bt)
    run_len = (lib.fh_wino54_run_len if f54 else lib.fh_wino_run_len)(n_tiles)
    rpp, cot = -(-n_tiles // run_len), C // bm
    # the runs that hold real tiles, groups in launch order (planner._merge_wino)
    runs = [(gi * cot + ct) * rpp + r for gi, L in enumerate(lens) for ct in range(cot) for r in range((-(-L // bt) - 1) // run_len + 1)]
    rm = torch.tensor(runs, dtype=torch.int32).to(DEV)
    d = hip.to_device_struct_array(groups, DEV)
    entry = "fh_conv_wino54_ragged_f32" if f54 else "fh_conv_wino_ragged_f32"
    novl = 0 if all(L % 4 == 0 for L in lens) else 2
    hip.check(getattr(lib, entry)(d.data_ptr(), len(groups), C, max(lens), 1, novl, cfg, rm.data_ptr(), rm.numel(), hip.stream()), entry)
    for i, o in enumerate(outs):
        emit(f"{name}.clip{i}", o)


def convt(name, tile, bf, u, k, cin=192, L=157):
    x, wt, b = rnd(B, cin, L, seed=70), rnd(cin, C, k, seed=71, scale=0.2), rnd(C, seed=72).to(DEV)
    extra = V.transposed_conv_extra(k, u)
    lout, npos = u * L + extra, L + extra
    xd, out = x.to(DEV), torch.full((B, C, lout), float("nan"), device=DEV)
    groups, keep = [], []
    for r, taps in enumerate(V.transposed_conv_phases(k, u)):
        w, center = V.wino_phase_weight(wt, taps)
        ud = V.pack_wino_weight_any(w, C, bf).to(DEV)
        keep.append(ud)
        groups.append(V.make_wino_group([V.make_wino_seg(xd, ud, cin, w.shape[-1], center, xlen=L if extra else 0)], b, [], out, C, C,
                                        npos, stride=u, phase=r, out_len=lout if extra else 0))
    keep.append(V.conv_wino(groups, B, C, npos, 1, DEV, tile | (V.WINO_BF16X6 if bf else 0) | (V.WINO_NOVL if extra else 0)))
    emit(name, out)


def main():
    combos = [(False, t, bf) for bf in (False, True) for t in (0, 1, 4, 5, 6)] + [(True, t, False) for t in (0, 1, 2, 3)] + \
             [(True, t, True) for t in (1, 2)]
    for f54, tile, bf in combos:
        n = f"{'f54' if f54 else 'f43'}.t{tile}.{'bf16x6' if bf else 'fp32'}"
        conv(f"{n}.rows.d1.L1000", f54, tile, bf, [7], 1000)
        conv(f"{n}.rows.pm.d3.L999", f54, tile, bf, [7], 999, d=3, pm=True)
        conv(f"{n}.rows.d1.L1001", f54, tile, bf, [7], 1001)
        conv(f"{n}.rows.d3.L778", f54, tile, bf, [7], 778, d=3)
        for nres in range(4):
            conv(f"{n}.nres{nres}", f54, tile, bf, [11], 1000, nres=nres, scale=0.5)
        conv(f"{n}.seg3", f54, tile, bf, [11, 7, 3], 1000, nres=3, scale=1.0 / 3)
        ragged(f"{n}.ragged.vl", f54, tile, bf, [3000, 1200, 332])
        ragged(f"{n}.ragged.b32", f54, tile, bf, [3000, 1200, 333])
        if not f54:
            conv(f"{n}.xcd.d1.L3000", f54, tile, bf, [7], 3000, nres=1, flags=V.WINO_XCD_RANGES)
            conv(f"{n}.xcd.pm.d3.L999", f54, tile, bf, [7], 999, d=3, pm=True, flags=V.WINO_XCD_RANGES)
            convt(f"{n}.convt.u4k8", tile, bf, 4, 8)
            convt(f"{n}.convt.u5k10", tile, bf, 5, 10)
    text = "\n".join(LINES) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text)
    print(text + f"{len(LINES)} outputs, all: {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
