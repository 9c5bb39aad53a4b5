"""GPU: the ragged vocoder launches (what merge_ragged enqueues for generate_many and the batching server), kernel by kernel:
fh_act1d_ragged_f32, fh_conv_wino_ragged_f32, fh_conv_wino54_ragged_f32, and the direct / transposed-fused conv entries called with
batch 1 and groups of different length.  One launch carries one group per clip; the grid is sized for the longest.

In every test each group's input, residual and output tensor is its own exact-size view inside a larger buffer, 16-byte aligned,
with >= 64 floats of guard on either side: NaN around (and in the phase-major pad elements of) the inputs, a sentinel NaN bit
pattern in the outputs and around them.  After the launch the output guards keep their bits, no real output element keeps the
sentinel, every one is finite; each group's result equals, bit for bit, the batched entry run on that group alone (merge_ragged's
promise) and meets a float64 evaluation of the definition at the bar of the kernel's fuzz tool.  (Pad elements of phase-major
OUTPUT rows are no outputs: no kernel here defines them, the consumers select them away, and the tests fill them with NaN on the
input side for that reason.)

Each test prints its worst error over bar (pytest -s)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from flowhigh_amd import hip, synth                                     # noqa: E402
from flowhigh_amd import vocoder as V                                   # noqa: E402
from ref_ragged import activation1d_f64, conv1d_abs_f64, conv1d_f64     # noqa: E402

DEV = "cuda"
GUARD = 64                  # floats of guard on either side of every view
SENT32 = 0x7fc12345         # output sentinel: a NaN no kernel produces
NAN32 = 0x7fc00000
F54 = V.WINO_F54
U32 = 2.0 ** -24            # unit roundoff of fp32


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


class Arena:
    """Exact-size float32 views inside one device buffer, each on a 16-byte boundary with >= GUARD floats of `fill` bits on
    either side.  add() before upload(); view() after."""

    def __init__(self, fill):
        self.fill, self.spans, self.data, self.n = fill, [], [], GUARD

    def add(self, t=None, numel=None):
        """A view holding tensor t's values (or `numel` floats of fill) -> its index."""
        n = t.numel() if t is not None else numel
        self.spans.append((self.n, n))
        self.data.append(None if t is None else t.reshape(-1).float().contiguous())
        self.n = (self.n + n + GUARD + 3) & ~3
        return len(self.spans) - 1

    def upload(self):
        host = torch.full((self.n,), self.fill, dtype=torch.int32)
        for (off, n), t in zip(self.spans, self.data):
            if t is not None:
                host[off:off + n] = t.view(torch.int32)
        self.host = host.clone()
        self.dev = host.to(DEV).view(torch.float32)
        assert self.dev.data_ptr() % 16 == 0 and all(off % 4 == 0 for off, _ in self.spans)
        return self

    def view(self, i, *shape):
        off, n = self.spans[i]
        return self.dev[off:off + n].view(*shape)

    def guards_intact(self):
        """Every element outside the views still holds the bits it was uploaded with."""
        now = self.dev.view(torch.int32).cpu()
        outside = torch.ones(self.n, dtype=torch.bool)
        for off, n in self.spans:
            outside[off:off + n] = False
        return torch.equal(now[outside], self.host[outside])


def nan_pads(xp, d, length):
    """Phase-major rows [C, d * lp] (to_phase_major) with their pad elements -- behind each phase's real samples -- set to NaN."""
    C = xp.shape[0]
    v = xp.view(C, d, -1).clone()
    for p in range(d):
        v[:, p, len(range(p, length, d)):] = float("nan")
    return v.reshape(C, -1)


def lay_in(x, d):
    """[C, L] -> the device layout of an input row set: plain, or phase-major with NaN pads."""
    return nan_pads(V.to_phase_major(x[None], d)[0], d, x.shape[-1]) if d > 1 else x


def pitch(length, d):
    return d * V.phase_len(length, d) if d > 1 else length


def real_part(y, d, length):
    """[C, pitch] device rows -> the [C, length] real elements on the host."""
    y = y.detach().cpu()
    return V.from_phase_major(y[None], d, length)[0] if d > 1 else y


def check_outputs(arena, outs, what):
    """The common post-launch assertions -> nothing; outs: [C, L] real elements per group."""
    assert arena.guards_intact(), f"{what}: a store outside the output tensors"
    for gi, o in enumerate(outs):
        assert not bool((o.view(torch.int32) == SENT32).any()), f"{what}: group {gi} has outputs nobody wrote"
        assert bool(torch.isfinite(o).all()), f"{what}: group {gi} has non-finite outputs"


# ================================================================================================================================
# Activation
# ================================================================================================================================
ACT_LAYOUTS = [(1, 1), (3, 1), (1, 3), (5, 1), (1, 5), (3, 5), (2, 1), (1, 16), (16, 1)]


def act_mix(name):
    tt = hip.lib().fh_act_tile_len()
    return {"any": (3, [2 * tt + 5, 2 * tt, tt + 1, tt, tt - 1, 9, 3, 1]),               # mult4 = 0: scalar loads
            "mult4": (3, [4 * tt + 4, 2 * tt, tt + 4, tt, 8, 4]),                          # mult4 = 1: vector loads
            "g70c1": (1, [1 + 7 * i % 23 for i in range(70)]),                             # second pass of the prefix search
            "g70c2": (2, [1 + 7 * i % 23 for i in range(70)]),
            "batched2": (2, [5, 5, 5]), "batched3": (3, [5, 5, 5])}[name]


@functools.lru_cache(maxsize=None)
def act_case(name):
    """(C, lengths, per group: x [C, L], parameter dict, float64 reference [C, L]).  Input statistics of tests/tools/act_fuzz.py
    (x ~ 1.5 N(0,1), log-scale alpha / beta ~ 0.4 N(0,1)); every group has its own alpha / inv_beta and its own taps: the Kaiser
    filter times a factor in [0.75, 1] per side, different for neighbouring groups (a neighbour's taps move an output by >= 3 %; factors
    <= 1 keep outputs and rounding at or under the fuzz tool's, so its bar holds)."""
    C, lengths = act_mix(name)
    filt = synth.kaiser_sinc_filter().flatten()
    groups = []
    for gi, L in enumerate(lengths):
        x = rnd(C, L, seed=1000 + gi, scale=1.5)
        alpha = torch.exp(rnd(C, seed=2000 + gi, scale=0.4))
        inv_beta = 1.0 / (torch.exp(rnd(C, seed=3000 + gi, scale=0.4)) + 1e-9)
        up = (filt * (1.0 - 0.25 * ((5 * gi) % 8) / 8)).tolist()
        down = (filt * (1.0 - 0.25 * ((3 * gi + 1) % 8) / 8)).tolist()
        p = dict(alpha=alpha, inv_beta=inv_beta, up=up, down=down)
        # (the reference takes the taps as the descriptor holds them: fp32)
        ref = activation1d_f64(x, alpha, inv_beta, torch.tensor(up).float().double(), torch.tensor(down).float().double())
        groups.append((x, p, ref))
    return C, lengths, groups


def act_setup(name, din, dout):
    C, lengths, groups = act_case(name)
    xin, yout = Arena(NAN32), Arena(SENT32)
    for (x, _, _), L in zip(groups, lengths):
        xin.add(lay_in(x, din))
        yout.add(numel=C * pitch(L, dout))
    xin.upload(), yout.upload()
    params = [dict(alpha=p["alpha"].to(DEV), inv_beta=p["inv_beta"].to(DEV), up=p["up"], down=p["down"]) for _, p, _ in groups]
    xs = [xin.view(i, C, pitch(L, din)) for i, L in enumerate(lengths)]
    ys = [yout.view(i, C, pitch(L, dout)) for i, L in enumerate(lengths)]
    return C, lengths, groups, xin, yout, params, xs, ys


def act_alone(x, p, C, L, din, dout):
    """The batched entry on one group, batch 1 -> real elements."""
    y = torch.full((1, C, pitch(L, dout)), float("nan"), device=DEV)
    keep = V.act1d_grouped([V.make_act_group(x, y, p)], 1, C, L, DEV, din, dout)
    torch.cuda.synchronize()
    del keep
    return real_part(y[0], dout, L)


def run_act_ragged(name, din, dout):
    C, lengths, groups, xin, yout, params, xs, ys = act_setup(name, din, dout)
    descs = [V.make_act_group(x, y, p) for x, y, p in zip(xs, ys, params)]
    keep = V.act1d_ragged(descs, lengths, C, DEV, din, dout)
    torch.cuda.synchronize()
    del keep
    what = f"fh_act1d_ragged_f32 {name} din {din} dout {dout}"
    outs = [real_part(y, dout, L) for y, L in zip(ys, lengths)]
    check_outputs(yout, outs, what)
    worst = 0.0
    for gi, (o, L) in enumerate(zip(outs, lengths)):
        assert torch.equal(o, act_alone(xs[gi], params[gi], C, L, din, dout)), f"{what}: group {gi} (len {L}) is not its own launch's bits"
        worst = max(worst, (o.double() - groups[gi][2]).abs().max().item())
    print(f"{what}: {len(lengths)} groups, worst error {worst:.3e} = {worst / 4e-6:.3f} of the bar")
    assert worst <= 4e-6, what                      # tests/tools/act_fuzz.py's bar, its input statistics
    return lengths, C


@pytest.mark.parametrize("din,dout", ACT_LAYOUTS)
@pytest.mark.parametrize("mix", ["any", "mult4"])
def test_act1d_ragged_mixes_in_every_layout(mix, din, dout):
    """Lengths either side of one and two tiles, a few samples, one sample; with and without the vector loads."""
    lengths, _ = run_act_ragged(mix, din, dout)
    assert all(n % 4 == 0 for n in lengths) == (mix == "mult4")


@pytest.mark.parametrize("din,dout", [(1, 1), (3, 5)])
@pytest.mark.parametrize("mix", ["g70c1", "g70c2"])
def test_act1d_ragged_seventy_groups(mix, din, dout):
    """More than 64 groups: the ballot loop of the tile_base search takes its second pass; with C = 1 every tile of a block is
    another group's (its own taps, alpha, length), and the launch's tile count is no multiple of a block's 4."""
    lengths, C = run_act_ragged(mix, din, dout)
    assert len(lengths) == 70 and (C * len(lengths)) % 4 == (2 if C == 1 else 0)


@pytest.mark.parametrize("din,dout", [(1, 1), (3, 1), (1, 5)])
@pytest.mark.parametrize("mix", ["batched2", "batched3"])
def test_act1d_batched_groups_with_their_own_taps(mix, din, dout):
    """fh_act1d_grouped_pm_f32, 3 groups x B = 2 x C channels x L = 5, every group its own taps and parameters.  C = 2: every block's
    4 tiles are one group's and the NEXT block starts with another group's taps; C = 3: a block walks from one group into the next."""
    C, lengths, groups = act_case(mix)
    B, L = 2, 5
    xin, yout = Arena(NAN32), Arena(SENT32)
    x2 = [torch.stack([x, rnd(C, L, seed=4000 + gi, scale=1.5)]) for gi, (x, _, _) in enumerate(groups)]          # [B, C, L]
    for x in x2:
        xin.add(torch.stack([lay_in(x[b], din) for b in range(B)]))
        yout.add(numel=B * C * pitch(L, dout))
    xin.upload(), yout.upload()
    params = [dict(alpha=p["alpha"].to(DEV), inv_beta=p["inv_beta"].to(DEV), up=p["up"], down=p["down"]) for _, p, _ in groups]
    xs = [xin.view(i, B, C, pitch(L, din)) for i in range(3)]
    ys = [yout.view(i, B, C, pitch(L, dout)) for i in range(3)]
    keep = V.act1d_grouped([V.make_act_group(x, y, p) for x, y, p in zip(xs, ys, params)], B, C, L, DEV, din, dout)
    torch.cuda.synchronize()
    del keep
    what = f"fh_act1d_grouped_pm_f32 C {C} din {din} dout {dout}"
    outs = [torch.cat([real_part(y[b], dout, L) for b in range(B)]) for y in ys]                                 # [B C, L]
    check_outputs(yout, outs, what)
    worst = 0.0
    for gi, o in enumerate(outs):
        _, p, _ = groups[gi]
        ref = torch.cat([activation1d_f64(x2[gi][b], p["alpha"], p["inv_beta"], torch.tensor(p["up"]).float().double(),
                                          torch.tensor(p["down"]).float().double()) for b in range(B)])
        worst = max(worst, (o.double() - ref).abs().max().item())
        for b in range(B):
            assert torch.equal(o[b * C:(b + 1) * C], act_alone(xs[gi][b], params[gi], C, L, din, dout)), f"{what}: group {gi} item {b}"
    print(f"{what}: worst error {worst:.3e} = {worst / 4e-6:.3f} of the bar")
    assert worst <= 4e-6, what


# ================================================================================================================================
# Winograd
# ================================================================================================================================
WINO_LAYOUTS = [(1, 0), (3, 0), (3, 1), (5, 0), (5, 1)]                 # (dilation, phase-major)
# (plan tile id, channels, bf16 x 6 form)
F43_FORMS = [(t, c, bf) for bf in (0, 1) for t, c in ((0, 64), (4, 64), (5, 64), (1, 96), (6, 128))]
F54_FORMS = [(F54 | 0, 128, 0), (F54 | 1, 96, 0), (F54 | 2, 64, 0), (F54 | 3, 48, 0), (F54 | 1, 96, 1), (F54 | 2, 64, 1)]


def wino_lengths(bt, aligned, kind="mix"):
    """The longest gives two runs per panel, the short groups own only the first; aligned: every length rounded up to a multiple of
    4 (the vector loader, layout bit 1 clear)."""
    lens = {"mix": [9 * bt + 1, 2 * bt + 3, bt + 1, bt, bt - 1, 5, 1], "equal": [2 * bt + 3, bt + 1, bt + 1, 5],
            "rich": [9 * bt + 1, bt + 1, bt - 1, 5]}[kind]
    return [(n + 3) & ~3 for n in lens] if aligned else lens


def wino_cases(forms):
    """(tile id, c, bf, dilation, pm, aligned, k): every form x layout x {mix, aligned twin}; k = 3 and 7 in turn, 11 in one case per form."""
    out = []
    for t, (cfg, c, bf) in enumerate(forms):
        for li, (dil, pm) in enumerate(WINO_LAYOUTS):
            for aligned in (0, 1):
                k = 11 if (li == t % 5 and aligned == t // 5 % 2) else (3, 7)[(t + li + aligned) % 2]
                out.append((cfg, c, bf, dil, pm, aligned, k))
    return out


def wino_id(case):
    cfg, c, bf, dil, pm, aligned, k = case
    return f"{'f54' if cfg & F54 else 'f43'}t{cfg & 15}-c{c}-{'bf' if bf else 'fp32'}-d{dil}{'pm' if pm else ''}-{'al' if aligned else 'mix'}-k{k}"


@functools.lru_cache(maxsize=64)
def wino_data(c, ks, dil, lengths, nres, scale):
    """Inputs and float64 references of one launch, shared by the tile shapes and forms that run it: per group (xs per segment,
    residuals, reference); two weight / bias sets, group gi takes set gi % 2 (a neighbour's weights would show).  Statistics of
    tests/tools/wino_fuzz.py: x, residuals, bias ~ N(0,1), w ~ N(0,1) / sqrt(c k)."""
    sets = [([rnd(c, c, k, seed=500 + 10 * s + i) / (c * k) ** 0.5 for i, k in enumerate(ks)], rnd(c, seed=540 + s)) for s in (0, 1)]
    groups = []
    for gi, L in enumerate(lengths):
        ws, bias = sets[gi % 2]
        xs = [rnd(c, L, seed=600 + 10 * gi + i) for i in range(len(ks))]
        res = [rnd(c, L, seed=700 + 10 * gi + i) for i in range(nres)]
        groups.append((xs, res, conv1d_f64(xs, ws, bias, res, scale, dil)))
    return sets, groups


def run_wino_ragged(cfg, c, bf, dil, pm, lengths, ks, nres=1, scale=1.0):
    f54 = bool(cfg & F54)
    taps = 4 if f54 else 3
    d_lay = dil if pm else 1
    sets, groups = wino_data(c, tuple(ks), dil, tuple(lengths), nres, scale)
    pack = V.pack_wino54_weight_any if f54 else V.pack_wino_weight_any
    dev_sets = [([pack(w, c, bool(bf)).to(DEV) for w in ws], bias.to(DEV)) for ws, bias in sets]
    xin, yout = Arena(NAN32), Arena(SENT32)
    ix, ir = [], []
    for (xs, res, _), L in zip(groups, lengths):
        ix.append([xin.add(lay_in(x, d_lay)) for x in xs])
        ir.append([xin.add(lay_in(r, d_lay)) for r in res])
        yout.add(numel=c * pitch(L, d_lay))
    xin.upload(), yout.upload()

    def group(gi, out):
        L = lengths[gi]
        us, bias = dev_sets[gi % 2]
        segs = [V.make_wino_seg(xin.view(i, c, pitch(L, d_lay)), us[j], c, ks[j], taps=taps) for j, i in enumerate(ix[gi])]
        return V.make_wino_group(segs, bias, [xin.view(i, c, pitch(L, d_lay)) for i in ir[gi]], out, c, c, L, scale=scale)
    ys = [yout.view(gi, c, pitch(L, d_lay)) for gi, L in enumerate(lengths)]
    flag = V.WINO_BF16X6 if bf else 0
    keep = V.conv_wino_ragged([group(gi, ys[gi]) for gi in range(len(lengths))], lengths, c, dil, DEV, cfg | flag, phase_major=bool(pm))
    torch.cuda.synchronize()
    del keep
    what = f"{'fh_conv_wino54_ragged_f32' if f54 else 'fh_conv_wino_ragged_f32'} tile {cfg & 15} c {c} {'bf16x6' if bf else 'fp32'} " \
           f"d {dil} pm {pm} k {list(ks)} lengths {list(lengths)}"
    outs = [real_part(y, d_lay, L) for y, L in zip(ys, lengths)]
    check_outputs(yout, outs, what)
    # the same loader as the ragged launch took: the F(4,3) entry can be told to leave the vector loader alone (WINO_NOVL); the
    # F(5,4) entry decides from the group's own length, which is what a clip gets in its own plan
    novl = V.WINO_NOVL if (not f54 and not pm and any(n % 4 for n in lengths)) else 0
    bar = (4e-5 if f54 else 3e-5) * len(ks)         # tests/tools/wino_fuzz.py, c <= 192
    worst = 0.0
    for gi, L in enumerate(lengths):
        alone = torch.full((1, c, pitch(L, d_lay)), float("nan"), device=DEV)
        keep = V.conv_wino([group(gi, alone)], 1, c, L, dil, DEV, cfg | flag | novl, phase_major=bool(pm))
        torch.cuda.synchronize()
        del keep
        assert torch.equal(outs[gi], real_part(alone[0], d_lay, L)), f"{what}: group {gi} (len {L}) is not its own launch's bits"
        worst = max(worst, (outs[gi].double() - groups[gi][2]).abs().max().item())
    print(f"{what}: worst error {worst:.3e} = {worst / bar:.3f} of the bar {bar:.0e}")
    assert worst <= bar, what


@pytest.mark.parametrize("case", wino_cases(F43_FORMS), ids=wino_id)
def test_conv_wino_ragged(case):
    cfg, c, bf, dil, pm, aligned, k = case
    run_wino_ragged(cfg, c, bf, dil, pm, wino_lengths(V._WINO_TILES[cfg][1], aligned), [k])


@pytest.mark.parametrize("case", wino_cases(F54_FORMS), ids=wino_id)
def test_conv_wino54_ragged(case):
    cfg, c, bf, dil, pm, aligned, k = case
    run_wino_ragged(cfg, c, bf, dil, pm, wino_lengths(V._WINO_TILES[cfg][1], aligned), [k])


@pytest.mark.parametrize("cfg,c,bf", [(4, 64, 0), (1, 96, 1), (F54 | 2, 64, 0), (F54 | 1, 96, 1)])
def test_conv_wino_ragged_three_segments_two_residuals_scale(cfg, c, bf):
    """The closing conv of a stage: three K segments (k = 11, 7, 3) into one accumulator, two residuals, scale 1/3."""
    run_wino_ragged(cfg, c, bf, 1, 0, wino_lengths(V._WINO_TILES[cfg][1], 0, "rich"), [11, 7, 3], nres=2, scale=1.0 / 3)


@pytest.mark.parametrize("cfg,c,dil,pm", [(0, 64, 1, 0), (5, 64, 3, 1), (F54 | 3, 48, 1, 0), (F54 | 0, 128, 5, 1)])
def test_conv_wino_ragged_two_groups_of_equal_length(cfg, c, dil, pm):
    run_wino_ragged(cfg, c, 0, dil, pm, wino_lengths(V._WINO_TILES[cfg][1], 0, "equal"), [7])


# ================================================================================================================================
# Direct and transposed-fused conv: batch 1, per-group lengths, n_len argument = the longest
# ================================================================================================================================
COUT = 24                   # no multiple of any tile height


def direct_shape(tile):
    """(cin, k, dilation) of the direct-conv launch at a tile id."""
    return [(32, 3, 1), (16, 7, 3), (32, 11, 5), (16, 3, 1), (32, 7, 3), (16, 11, 5), (32, 7, 1)][tile]


def direct_lengths(tile):
    bn = hip.lib().fh_conv_tile_n(tile)
    return [8 * bn + 1, bn + 1, bn, bn - 1, 3, 1]                       # one run of 8 tiles + one tile; around one tile; a few samples


@functools.lru_cache(maxsize=None)
def direct_data(tile):
    """Per group (x, residual, float64 reference, A of the fp32 bound); weights 0.2 N(0,1) as in test_hip_direct_bf.py, one
    residual, scale 0.5; two weight / bias sets, group gi takes set gi % 2."""
    cin, k, dil = direct_shape(tile)
    sets = [(rnd(COUT, cin, k, seed=800 + s, scale=0.2), rnd(COUT, seed=810 + s)) for s in (0, 1)]
    groups = []
    for gi, L in enumerate(direct_lengths(tile)):
        w, b = sets[gi % 2]
        x, r = rnd(cin, L, seed=820 + gi), rnd(COUT, L, seed=840 + gi)
        groups.append((x, r, conv1d_f64([x], [w], b, [r], 0.5, dil), conv1d_abs_f64([x], [w], b, [r], 0.5, dil)))
    return sets, groups


@functools.lru_cache(maxsize=None)
def run_direct_ragged(tile, bf, ck):
    """One ragged launch of fh_conv_grouped_f32 (channel chunk ck) / fh_conv_grouped_bf16x6_f32 with the common assertions and the
    comparison with each group's own launch -> the groups' outputs."""
    cin, k, dil = direct_shape(tile)
    lengths = direct_lengths(tile)
    sets, groups = direct_data(tile)
    bm = hip.lib().fh_conv_tile_m(tile)
    cpad = -(-COUT // bm) * bm
    dev_sets = [((V.pack_conv_bf_weight(w, cpad) if bf else V.pack_conv_weight(w, cpad, ck)).to(DEV), b.to(DEV)) for w, b in sets]
    offs = [(t - (k - 1) // 2) * dil for t in range(k)]
    xin, yout = Arena(NAN32), Arena(SENT32)
    for (x, r, _, _), L in zip(groups, lengths):
        xin.add(x), xin.add(r), yout.add(numel=COUT * L)
    xin.upload(), yout.upload()

    def group(gi, out):
        L = lengths[gi]
        wp, b = dev_sets[gi % 2]
        return V.make_conv_group([V.make_conv_seg(xin.view(2 * gi, cin, L), wp, cin, offs)], b, [xin.view(2 * gi + 1, COUT, L)], out,
                                 COUT, cpad, L, L, L, scale=0.5)
    ys = [yout.view(gi, COUT, L) for gi, L in enumerate(lengths)]
    keep = V.conv_grouped([group(gi, ys[gi]) for gi in range(len(lengths))], 1, cpad, max(lengths), tile, DEV, ck, bf=bool(bf))
    torch.cuda.synchronize()
    del keep
    what = f"{'fh_conv_grouped_bf16x6_f32' if bf else 'fh_conv_grouped_f32'} tile {tile} ck {ck} cin {cin} k {k} d {dil}"
    outs = [y.cpu() for y in ys]
    check_outputs(yout, outs, what)
    for gi, L in enumerate(lengths):
        alone = torch.full((1, COUT, L), float("nan"), device=DEV)
        keep = V.conv_grouped([group(gi, alone)], 1, cpad, L, tile, DEV, ck, bf=bool(bf))
        torch.cuda.synchronize()
        del keep
        assert torch.equal(outs[gi], alone[0].cpu()), f"{what}: group {gi} (len {L}) is not its own launch's bits"
    return outs


def worst_ratio(outs, groups, K):
    """max over the elements of |got - ref| / ((K + 3) u A): <= 1 for ANY order of fp32 accumulation of K products, bias,
    residual and scale (each operation rounds once, relative error u, against the sum of absolute values A)."""
    return max(((o.double() - ref).abs() / ((K + 3) * U32 * A)).max().item() for o, (_, _, ref, A) in zip(outs, groups))


@pytest.mark.parametrize("ck", [16, 8])
@pytest.mark.parametrize("tile", range(7))
def test_conv_grouped_ragged_lengths(tile, ck):
    cin, k, _ = direct_shape(tile)
    outs = run_direct_ragged(tile, 0, ck)
    ratio = worst_ratio(outs, direct_data(tile)[1], cin * k)
    print(f"fh_conv_grouped_f32 tile {tile} ck {ck}: worst |got - ref| / ((K + 3) u A) = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("tile", range(7))
def test_conv_grouped_bf16x6_ragged_lengths(tile):
    """tests/test_hip_direct_bf.py's bar for this kernel (assert_fp32_grade): inside the fp32 test's 5e-5 for such shapes (K <= 2200
    products of ~0.2) and inside twice the fp32 kernel's own error + 1e-7 on the same inputs."""
    groups = direct_data(tile)[1]
    err = lambda outs: max((o.double() - ref).abs().max().item() for o, (_, _, ref, _) in zip(outs, groups))
    e_bf, e32 = err(run_direct_ragged(tile, 1, 16)), err(run_direct_ragged(tile, 0, 16))
    print(f"fh_conv_grouped_bf16x6_f32 tile {tile}: bf16 x 6 {e_bf:.3e}, fp32 MFMA {e32:.3e} against float64: "
          f"{max(e_bf / 5e-5, e_bf / (2.0 * e32 + 1e-7)):.3f} of the bar")
    assert e_bf <= 5e-5
    assert e_bf <= 2.0 * e32 + 1e-7


@pytest.mark.parametrize("tile", [3, 4, 6])
def test_conv_transpose_fused_ragged_lengths(tile):
    """fh_conv_transpose_fused_f32, u = 2, k = 4 (the tile shapes that have the phase-fused form): groups of different input
    length, each writing its own [cout, 2 L] tensor."""
    cin, u, k = 32, 2, 4
    bn, bm = hip.lib().fh_conv_tile_n(tile), hip.lib().fh_conv_tile_m(tile)
    lengths = [8 * bn + 1, bn + 1, bn, bn - 1, 3, 1]
    cpad = -(-COUT // bm) * bm
    sets = [(rnd(cin, COUT, k, seed=900 + s, scale=0.2), rnd(COUT, seed=910 + s)) for s in (0, 1)]
    phases = V.transposed_conv_phases(k, u)
    dev_sets = [([V.pack_conv_weight(torch.stack([wt[:, :, j] for j, _ in taps], dim=-1).permute(1, 0, 2), cpad, 16).to(DEV) for taps in phases],
                 b.to(DEV)) for wt, b in sets]
    xs = [rnd(cin, L, seed=920 + gi) for gi, L in enumerate(lengths)]
    xin, yout = Arena(NAN32), Arena(SENT32)
    for x, L in zip(xs, lengths):
        xin.add(x), yout.add(numel=COUT * u * L)
    xin.upload(), yout.upload()

    def group(gi, out):
        L = lengths[gi]
        wps, b = dev_sets[gi % 2]
        segs = [V.make_conv_seg(xin.view(gi, cin, L), wps[r], cin, [o for _, o in taps]) for r, taps in enumerate(phases)]
        return V.make_conv_group(segs, b, [], out, COUT, cpad, L, u * L, L, stride=u, phase=0)

    def launch(descs, n_len):
        d = hip.to_device_struct_array(descs, DEV)
        hip.check(hip.lib().fh_conv_transpose_fused_f32(d.data_ptr(), len(descs), 1, cpad, n_len, tile, u, hip.stream()), "fh_conv_transpose_fused_f32")
        torch.cuda.synchronize()
    ys = [yout.view(gi, COUT, u * L) for gi, L in enumerate(lengths)]
    launch([group(gi, ys[gi]) for gi in range(len(lengths))], max(lengths))
    what = f"fh_conv_transpose_fused_f32 tile {tile}"
    outs = [y.cpu() for y in ys]
    check_outputs(yout, outs, what)
    ratio = 0.0
    for gi, L in enumerate(lengths):
        alone = torch.full((1, COUT, u * L), float("nan"), device=DEV)
        launch([group(gi, alone)], L)
        assert torch.equal(outs[gi], alone[0].cpu()), f"{what}: group {gi} (len {L}) is not its own launch's bits"
        wt, b = sets[gi % 2]
        ct = lambda x, w, bb: F.conv_transpose1d(x.double()[None], w.double(), bb.double(), stride=u, padding=(k - u) // 2)[0]
        ref, A = ct(xs[gi], wt, b), ct(xs[gi].abs(), wt.abs(), b.abs())
        assert ref.shape == outs[gi].shape
        ratio = max(ratio, ((outs[gi].double() - ref).abs() / ((cin * k // u + 3) * U32 * A)).max().item())
    print(f"{what}: worst |got - ref| / ((K + 3) u A) = {ratio:.3f}")
    assert ratio <= 1.0
