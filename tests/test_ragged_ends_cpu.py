"""CPU: host side of generate_many(ends='ragged') -- how `ends` is resolved, the clip tables of a ragged call (offsets, lengths,
frame counts, the refusal of clips too short for the mel front end) and the layout of the fh_clip descriptor."""
import ctypes

import numpy as np
import pytest

from flowhigh_amd import flowhighsr as M
from flowhigh_amd import frontend, hip, tables
from flowhigh_amd.serve import BatchingServer

LENS = [600, 1500, 2401, 2401, 3000]


def test_ends_keyword_wins_over_environment_over_default(monkeypatch):
    monkeypatch.delenv("FH_RAGGED_ENDS", raising=False)
    assert M.resolve_ends() == "per_clip" and M.resolve_ends(None) == "per_clip"
    assert M.resolve_ends("ragged") == "ragged"
    monkeypatch.setenv("FH_RAGGED_ENDS", "ragged")
    assert M.resolve_ends() == "ragged"
    assert M.resolve_ends("per_clip") == "per_clip"          # the keyword wins
    monkeypatch.setenv("FH_RAGGED_ENDS", "")
    assert M.resolve_ends() == "per_clip"                    # (set but empty: the default)


@pytest.mark.parametrize("bad", ["Ragged", "per-clip", "", 1, True])
def test_wrong_ends_value_is_a_value_error(monkeypatch, bad):
    monkeypatch.delenv("FH_RAGGED_ENDS", raising=False)
    with pytest.raises(ValueError, match="ends must be one of"):
        M.resolve_ends(bad)
    with pytest.raises(ValueError, match="ends must be one of"):
        BatchingServer(None, ends=bad)                       # refused before the worker thread starts
    if isinstance(bad, str) and bad:
        monkeypatch.setenv("FH_RAGGED_ENDS", bad)
        with pytest.raises(ValueError, match="ends must be one of"):
            M.resolve_ends()


def test_generate_many_refuses_a_wrong_ends_before_touching_anything():
    """generate_many resolves ends= first: no model state, no device needed to be told about a wrong value."""
    with pytest.raises(ValueError, match="ends must be one of"):
        M.FlowHighSR.generate_many.__wrapped__.__wrapped__(object(), [np.zeros(600)], 12000, ends="both")


@pytest.mark.parametrize("sr", [12000, 16000, 22050])
def test_clip_tables_are_back_to_back_with_the_per_clip_lengths(sr):
    t = frontend.ragged_clip_tables(LENS, sr)
    n = len(LENS)
    assert t["len_in"] == LENS
    for lens, offs in (("len_in", "in_off"), ("len_out", "out_off"), ("mel_rows", "mel_row0"), ("pp_rows", "pp_row0")):
        assert t[offs][0] == 0
        assert all(t[offs][i + 1] == t[offs][i] + t[lens][i] for i in range(n - 1)), (lens, t[offs])
    assert t["len_out"] == [tables.resample_out_len(v, 48000, sr) for v in LENS]
    assert t["mel_rows"] == [T // 480 for T in t["len_out"]]
    assert t["pp_rows"] == [1 + T // 480 for T in t["len_out"]]
    assert t["pred_len"] == [480 * N for N in t["mel_rows"]]
    if sr == 12000:
        assert t["len_out"] == [2400, 6000, 9604, 9604, 12000] and t["mel_rows"][0] == 5 and t["len_out"][2] % 480
    if sr == 22050:                                          # down > 1: lengths round up
        assert tables.resample_poly_plan(48000, sr)[3] > 1
        assert t["len_out"][0] == -(-600 * 320 // 147)


def test_clip_tables_follow_a_longer_vocoder_output():
    """A vocoder with an odd k - u returns more than 480 N samples: F = min(1 + Tp // 480, 1 + T // 480)."""
    t0 = frontend.ragged_clip_tables(LENS, 12000)
    t = frontend.ragged_clip_tables(LENS, 12000, pred_lens=[480 * N + 98 for N in t0["mel_rows"]])
    assert t["pp_rows"] == t0["pp_rows"] and t["pred_len"] == [480 * N + 98 for N in t0["mel_rows"]]
    short = frontend.ragged_clip_tables(LENS, 12000, pred_lens=[480 * N - 1 for N in t0["mel_rows"]])
    assert short["pp_rows"] == [N for N in t0["mel_rows"]]
    with pytest.raises(ValueError):
        frontend.ragged_clip_tables(LENS, 12000, pred_lens=[480])


def test_clip_tables_at_48k_and_the_refusal_of_short_clips():
    t = frontend.ragged_clip_tables(LENS[1:], 48000)
    assert t["len_out"] == LENS[1:] and t["out_off"] == t["in_off"] == [0, 1500, 3901, 6302]
    assert t["mel_rows"] == [3, 5, 5, 6] and t["pp_rows"] == [4, 6, 6, 7]
    # the per-clip path's refusal (LogMel.__call__), word for word
    for T in (600, 784, 479):
        with pytest.raises(ValueError, match=f"clip of {T} samples is too short for the mel front end"):
            frontend.ragged_clip_tables([1500, T, 3000], 48000)
    assert frontend.ragged_clip_tables([785], 48000)["mel_rows"] == [1]
    with pytest.raises(ValueError, match="clip of 600 samples is too short"):
        frontend.ragged_clip_tables(LENS, 48000)
    assert frontend.ragged_clip_tables(LENS, 48000, check_mel=False)["len_out"] == LENS       # (the resampler alone takes them)
    with pytest.raises(ValueError):
        frontend.ragged_clip_tables([], 12000)


def test_clip_descriptor_mirror_has_the_library_layout():
    assert ctypes.sizeof(hip.Clip) == hip.lib().fh_sizeof_clip() == 32
    arr = frontend.clip_array(src=[16, 32], len_in=[5, 7], row0=[0, 3], rows=[3, 4])
    assert len(arr) == 2 and (arr[1].src, arr[1].dst, arr[1].len_in, arr[1].len_out, arr[1].row0, arr[1].rows) == (32, None, 7, 0, 3, 4)
    seg = frontend.seg_table([0, 3], [3, 4])
    assert seg.dtype == np.int32 and seg.tolist() == [[0, 3], [3, 4]]
    # one buffer for every table of a call, parts 16-byte aligned, contents as given
    buf, addrs = frontend.upload_tables([arr, seg, frontend.clip_array(dst=[8], rows=[1])], "cpu")
    base = buf.data_ptr()
    assert [a - base for a in addrs] == [0, 64, 80] and buf.numel() == 112
    raw = bytes(buf.numpy())
    assert raw[:64] == bytes(arr) and raw[64:80] == seg.tobytes()
