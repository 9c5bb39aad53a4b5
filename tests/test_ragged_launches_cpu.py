"""CPU: host side of the ragged vocoder launches -- the run list of a ragged Winograd launch (planner.wino_run_map) and the group
table of a ragged activation launch (planner.act_ragged_groups) by brute force, and the float64 activation reference of the GPU
tests (ref_ragged.activation1d_f64) against the oracle.

The run list is decoded the way conv_wino_common.h's wino_block_work decodes it (panel = run / runs per panel, tiles
(run % runs per panel) * run_len + 0 .. run_len - 1, cut at n_tiles) and held against "real tile" as the KERNELS decide it, restated
here from their early exits -- not from the planner's t_last formula."""
import numpy as np
import pytest
import torch

from flowhigh_amd import hip, synth
from flowhigh_amd import planner as P
from oracle import ref_cpu
from ref_ragged import activation1d_f64

F54 = P.WINO_F54


def tile_slots54(length, dil):
    """v_tile_slots of conv_wino54_kernel.h."""
    return (((length + dil - 1) // dil + 4) // 5 + 3 + 3) & ~3


def real_tile(cfg, tile, length, dil, pm):
    """Does the block of tile index `tile` (numpy array) of a group of `length` samples get past its kernel's early exit?
      conv_wino.hip:          tb = tile / dil, ph = tile % dil;  return if tb * (4 W_BT) * dil + ph >= len
      conv_wino54_kernel.h:   plain: the same with V_OUT = 320;  phase-major ("cat"): tb = tile, ps = 5 v_tile_slots(len, dil);
                              return if tb * V_OUT >= dil * ps"""
    bt = P._WINO_TILES[cfg][1]
    if cfg & F54 and pm:
        return tile * 320 < dil * 5 * tile_slots54(length, dil)
    tb, ph = tile // dil, tile % dil
    return ph + dil * bt * tb < length


def launch_tiles(cfg, maxlen, dil, pm):
    """n_tiles as the kernels' launchers compute it (launch_wino_vl; wino54_n_tiles)."""
    bt = P._WINO_TILES[cfg][1]
    if cfg & F54 and pm:
        return -(-dil * tile_slots54(maxlen, dil) // 64)
    return -(-(-(-maxlen // dil)) // bt) * dil


@pytest.mark.parametrize("pm", [0, 1])
@pytest.mark.parametrize("dil", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("cfg", sorted(P._WINO_TILES))
def test_wino_run_map_lists_every_real_tile_once_and_no_empty_run(cfg, dil, pm):
    bm, bt = P._WINO_TILES[cfg]
    lengths = [9 * bt + 1] + list(range(3 * bt + 2, 0, -1))           # the longest clip, then every length 3 bt + 2 .. 1
    n_tiles = launch_tiles(cfg, lengths[0], dil, pm)
    assert n_tiles == P.wino_n_tiles(cfg, lengths[0], dil, pm)
    run_len = -(-n_tiles // -(-n_tiles // 8))                          # wino_run_len of conv_wino_common.h, WINO_RUN = 8
    rpp = -(-n_tiles // run_len)
    assert rpp > 1                                                     # more than one run per panel
    lens = np.array(lengths)
    real = np.stack([real_tile(cfg, np.arange(n_tiles), n, dil, pm) for n in lengths])       # [group, tile]
    assert real[:, 0].all() and real[0, run_len:].any() and not real[-1, 1:].any()          # (every group has work; the longest in a later run too)
    for cot in (1, 2, 3):
        runs = np.array(P.wino_run_map(lengths, cfg, cot * bm, dil, bool(pm)))
        assert runs.min() >= 0 and runs.max() < len(lengths) * cot * rpp and len(set(runs.tolist())) == len(runs)
        panel, r = runs // rpp, runs % rpp
        gi, ct = panel // cot, panel % cot
        tiles = r[:, None] * run_len + np.arange(run_len)[None, :]     # [run, tile in run]
        inside = tiles < n_tiles
        is_real = inside & real[gi[:, None], np.minimum(tiles, n_tiles - 1)]
        assert is_real.any(axis=1).all(), "a listed run holds no real tile"
        cover = np.zeros((len(lengths), cot, n_tiles), dtype=np.int64)
        np.add.at(cover, (np.broadcast_to(gi[:, None], tiles.shape)[inside], np.broadcast_to(ct[:, None], tiles.shape)[inside],
                          tiles[inside]), 1)
        assert cover.max() == 1
        missing = real[:, None, :] & (cover == 0)
        assert not missing.any(), f"real tiles without a block: (group, co tile, tile) {np.argwhere(missing)[:4].tolist()}, lengths {lens[np.argwhere(missing)[:4, 0]]}"


def test_wino_run_map_does_not_depend_on_the_order_of_the_groups():
    """Launch order is by weight (K steps) first: a short group may stand in front of the longest one."""
    cfg, dil = 4, 3
    bm, bt = P._WINO_TILES[cfg]
    lengths = [5, 9 * bt + 1, bt + 1, 1, 2 * bt + 3]
    n_tiles = launch_tiles(cfg, max(lengths), dil, 0)
    run_len = -(-n_tiles // -(-n_tiles // 8))
    rpp = -(-n_tiles // run_len)
    runs = P.wino_run_map(lengths, cfg, 2 * bm, dil, False)
    got = {}
    for run in runs:
        got.setdefault(run // rpp // 2, set()).add((run // rpp % 2, run % rpp))
    for gi, n in enumerate(lengths):
        last = max(t for t in range(n_tiles) if real_tile(cfg, np.array(t), n, dil, 0))
        assert got[gi] == {(ct, r) for ct in range(2) for r in range(last // run_len + 1)}


@pytest.mark.parametrize("channels", [1, 2, 3, 48])
def test_act_ragged_groups_prefix_total_and_mult4(channels):
    tt = hip.lib().fh_act_tile_len()
    mixes = [[2 * tt + 5, 2 * tt, tt + 1, tt, tt - 1, 9, 3, 1], [4 * tt + 4, 2 * tt, tt + 4, tt, 8, 4], [1 + 7 * i % 23 for i in range(70)],
             [4], [tt + 1], [8, 4, 3]]
    for lengths in mixes:
        src = []
        for i in range(len(lengths)):
            g = hip.ActGroup()
            g.x, g.y, g.alpha, g.inv_beta = 16 * (4 * i + 1), 16 * (4 * i + 2), 16 * (4 * i + 3), 16 * (4 * i + 4)
            for j in range(12):
                g.up_taps[j], g.down_taps[j] = i + j / 16.0, -i - j / 16.0
            src.append(g)
        out, total, mult4 = P.act_ragged_groups(src, lengths, channels)
        assert len(out) == len(lengths)
        base = 0
        for g, g0, n in zip(out, src, lengths):
            assert g is not g0 and (g0.len, g0.tile_base) == (0, 0)                  # copies: the per-clip descriptors stay as they are
            assert (g.len, g.tile_base) == (n, base)
            assert (g.x, g.y, g.alpha, g.inv_beta) == (g0.x, g0.y, g0.alpha, g0.inv_beta)
            assert list(g.up_taps) == list(g0.up_taps) and list(g.down_taps) == list(g0.down_taps)
            base += channels * -(-n // tt)                                           # tiles of the group: channels x ceil(len / tile length)
        assert total == base
        assert mult4 == int(all(n % 4 == 0 for n in lengths))


@pytest.mark.parametrize("kind", ["snakebeta_log", "snake_lin"])
@pytest.mark.parametrize("L", [1, 2, 5, 6, 13, 300])
def test_activation_closed_form_is_the_oracle_s_activation1d(kind, L):
    """ref_ragged.activation1d_f64 (the closed form of act1d.hip's header, float64) against the oracle's UpSample1d -> Snake ->
    DownSample1d in float64, with a filter per side that is NOT symmetric (a flipped or shifted tap index would show)."""
    g = torch.Generator().manual_seed(L)
    C = 3
    x = (torch.randn(1, C, L, generator=g) * 1.5).double()
    al, be = (torch.randn(C, generator=g) * 0.4).double(), (torch.randn(C, generator=g) * 0.4).double()
    filt = synth.kaiser_sinc_filter().double()
    up = filt * (1.0 + 0.05 * torch.arange(12).double()).view(1, 1, 12)
    down = filt * (1.0 - 0.03 * torch.arange(12).double()).view(1, 1, 12)
    if kind == "snakebeta_log":
        h = {"activation": "snakebeta", "snake_logscale": True}
        sd = {"a.act.alpha": al, "a.act.beta": be}
        alpha, beta = torch.exp(al), torch.exp(be)
    else:
        h = {"activation": "snake", "snake_logscale": False}
        al = al.abs() + 0.5
        sd = {"a.act.alpha": al}
        alpha, beta = al, al
    sd["a.upsample.filter"], sd["a.downsample.lowpass.filter"] = up, down
    ref = ref_cpu.activation1d(sd, "a.", x, h)[0]
    got = activation1d_f64(x[0], alpha, 1.0 / (beta + 1e-9), up.flatten().tolist(), down.flatten().tolist())
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-13                   # float64 rounding of ~25 terms of size <= 3


def test_conv_wino_ragged_refuses_lengths_that_are_not_the_groups_own():
    """The one-off launcher makes the run map from `lengths` and the kernel exits by the descriptors' len: they must agree.
    Refused before anything touches a device."""
    from flowhigh_amd import vocoder as V
    groups = []
    for n in (700, 5):
        g = hip.WinoGroup()
        g.len, g.nseg = n, 1
        groups.append(g)
    with pytest.raises(ValueError, match="lengths"):
        V.conv_wino_ragged(groups, [700, 6], 64, 1, "cpu", 4)
    with pytest.raises(ValueError, match="lengths"):
        V.conv_wino_ragged(groups, [700], 64, 1, "cpu", 4)
