"""CPU: the host side of generate_many with one input rate per clip -- resolve_rates, the clip and rate tables of
fh_resample_poly_rates_seg_f32, the ABI surface of the new entry and the BatchingServer's grouping (stub model)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from flowhigh_amd import frontend as FE
from flowhigh_amd import hip, tables
from flowhigh_amd.flowhighsr import resolve_rates
from flowhigh_amd.serve import BatchingServer

ROOT = Path(__file__).resolve().parents[1]
LENS = [600, 1500, 2401, 2401, 3000]
RATES = [12000, 22050, 48000, 8000, 44100]
ENTRY = "fh_resample_poly_rates_seg_f32"


# ---- resolve_rates ---------------------------------------------------------------------------
def test_resolve_rates_repeats_an_int_and_passes_a_list_through():
    assert resolve_rates(12000, 3) == [12000, 12000, 12000]
    assert resolve_rates(np.int64(8000), 2) == [8000, 8000]
    got = resolve_rates((8000, np.int32(22050), 48000), 3)
    assert got == [8000, 22050, 48000] and all(type(r) is int for r in got)
    assert resolve_rates([], 0) == []


@pytest.mark.parametrize("sr,n", [([8000, 12000], 3), ([8000, 12000, 16000, 24000], 3), ([8000, 0, 12000], 3), ([8000, -12000], 2),
                                  ([8000, 11025.5], 2), ([8000, "12000"], 2), ([8000, None], 2), (0, 2), (-8000, 1), (8000.5, 1),
                                  (None, 1), ([8000, float("nan")], 2)])
def test_resolve_rates_refuses_what_is_not_one_positive_int_per_clip(sr, n):
    with pytest.raises(ValueError):
        resolve_rates(sr, n)


def test_resolve_rates_names_both_counts():
    with pytest.raises(ValueError, match=r"2 rates for 3 clips"):
        resolve_rates([8000, 12000], 3)


# ---- clip tables -----------------------------------------------------------------------------
def test_ragged_clip_tables_with_a_rate_per_clip():
    tab = FE.ragged_clip_tables(LENS, RATES, check_mel=False)
    assert tab["len_out"] == [2400, 3266, 2401, 14406, 3266]
    assert tab["len_out"] == [tables.resample_out_len(n, 48000, r) for n, r in zip(LENS, RATES)]
    assert tab["len_in"] == LENS and tab["in_off"] == [0, 600, 2100, 4501, 6902]
    assert tab["out_off"] == [0, 2400, 5666, 8067, 22473]
    with pytest.raises(ValueError):
        FE.ragged_clip_tables(LENS, RATES[:4], check_mel=False)


@pytest.mark.parametrize("sr", [12000, 22050, 48000])
def test_ragged_clip_tables_int_rate_is_the_repeated_list(sr):
    assert FE.ragged_clip_tables(LENS, sr, check_mel=False) == FE.ragged_clip_tables(LENS, [sr] * 5, check_mel=False)
    assert FE.ragged_clip_tables(LENS, 12000) == FE.ragged_clip_tables(LENS, [12000] * 5)


# ---- rate tables -----------------------------------------------------------------------------
def test_rate_tables_rows_bank_and_rate_of():
    rates = RATES + [22050]
    bank, rows, rate_of = FE.rate_tables(rates)
    assert isinstance(bank, np.ndarray) and bank.dtype == np.float32 and bank.ndim == 1
    assert isinstance(rows, ctypes.Array) and rows._type_ is hip.Rate and len(rows) == 5
    assert rate_of.dtype == np.int32 and rate_of.tolist() == [0, 1, 2, 3, 4, 1]
    spans = []
    for row, sr in zip(rows, RATES):                                   # first-appearance order
        plan = tables.resample_poly_plan(48000, sr)
        if sr == 48000:
            assert plan is None and row.n_taps == 0 and (row.up, row.down, row.n_pre_remove) == (1, 1, 0)
            assert 0 <= row.taps_off <= bank.size
            continue
        taps, pre, up, down = plan
        assert (row.up, row.down, row.n_pre_remove) == (up, down, pre) and row.n_taps == taps.numel() > 0
        assert row.taps_off >= 0 and row.taps_off + row.n_taps <= bank.size
        assert np.array_equal(bank[row.taps_off:row.taps_off + row.n_taps].view(np.uint32), taps.numpy().view(np.uint32))
        spans.append((row.taps_off, row.taps_off + row.n_taps))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "bank slices overlap"
    assert sum(b - a for a, b in spans) == bank.size
    assert [(r.up, r.down) for r in rows] == [(4, 1), (320, 147), (1, 1), (6, 1), (160, 147)]
    # equal rates only: an empty bank and one copy row
    bank, rows, rate_of = FE.rate_tables([48000, 48000])
    assert bank.size == 0 and len(rows) == 1 and rows[0].n_taps == 0 and rate_of.tolist() == [0, 0]


# ---- ABI surface -----------------------------------------------------------------------------
def test_the_new_names_are_exported_and_declared():
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    declared = set(re.findall(r"\b(fh_[a-z0-9_]+)\s*\(", header))
    for name in (ENTRY, "fh_sizeof_rate"):
        assert name in hip.EXPORTS and name in declared
    assert "fh_resample_poly_seg_f32" in hip.EXPORTS                 # (the one-rate entry stays)
    assert re.search(r"\}\s*fh_rate\s*;", header)
    assert ctypes.sizeof(hip.Rate) == 20
    assert [f[0] for f in hip.Rate._fields_] == ["taps_off", "n_taps", "up", "down", "n_pre_remove"]
    assert hip.ABI_VERSION == 6 and re.search(r"#define FH_ABI_VERSION 6\b", header)


def test_the_library_lays_the_rate_row_out_as_hip_py_does():
    from flowhigh_amd import build
    build.build(verbose=False)
    L = hip.lib()
    assert L.fh_sizeof_rate() == 20 == ctypes.sizeof(hip.Rate)
    assert L.fh_abi_version() == 6


def test_argument_errors_of_the_entry_launch_nothing():
    """Fake non-null pointers: every case is refused by the host checks, before a launch."""
    from flowhigh_amd import build
    build.build(verbose=False)
    L = hip.lib()
    P = 16
    good = dict(clips=P, rate_of=P, n_clips=5, max_len_out=100, rates=P, n_rates=2, tap_bank=P, bank_len=64)
    bad = [dict(clips=0), dict(n_clips=0), dict(n_clips=65536), dict(rate_of=0), dict(rates=0), dict(n_rates=0), dict(n_rates=-1),
           dict(max_len_out=0), dict(max_len_out=-5), dict(bank_len=-1), dict(tap_bank=0, bank_len=8)]
    for change in bad:
        a = dict(good, **change)
        rc = L.fh_resample_poly_rates_seg_f32(a["clips"], a["rate_of"], a["n_clips"], a["max_len_out"], a["rates"], a["n_rates"],
                                              a["tap_bank"], a["bank_len"], 0)
        assert rc == -1, change
        assert ENTRY.encode() in L.fh_last_error(), change


# ---- BatchingServer grouping (stub model: no GPU) ------------------------------------------
class StubModel:
    def __init__(self):
        self.calls = []

    def generate_many(self, clips, sr, target, steps, **kw):
        self.calls.append(dict(n=len(clips), sr=sr, steps=steps, lens=[len(c) for c in clips]))
        return [torch.zeros(1, 4) for _ in clips]


def serve(requests, **kw):
    m = StubModel()
    srv = BatchingServer(m, max_batch=len(requests), max_wait_ms=2000, **kw)
    futs = [srv.submit(np.zeros(100 + i, np.float32), sr, steps) for i, (sr, steps) in enumerate(requests)]
    outs = [f.result(timeout=60) for f in futs]
    srv.close()
    assert all(o.shape == (4,) for o in outs)
    return m.calls


def test_server_sends_one_call_for_a_window_of_three_rates(monkeypatch):
    monkeypatch.delenv("FH_SERVE_MIX_RATES", raising=False)
    calls = serve([(8000, 1), (12000, 1), (16000, 1)], mix_rates=True)
    assert len(calls) == 1
    assert calls[0]["sr"] == [8000, 12000, 16000] and calls[0]["lens"] == [100, 101, 102] and calls[0]["steps"] == 1


def test_server_mix_rates_off_is_one_call_per_rate(monkeypatch):
    monkeypatch.delenv("FH_SERVE_MIX_RATES", raising=False)
    calls = serve([(8000, 1), (12000, 1), (16000, 1)], mix_rates=False)
    assert [c["sr"] for c in calls] == [8000, 12000, 16000] and all(type(c["sr"]) is int and c["n"] == 1 for c in calls)


def test_server_never_mixes_step_counts(monkeypatch):
    monkeypatch.delenv("FH_SERVE_MIX_RATES", raising=False)
    for mix in (True, False):
        calls = serve([(8000, 1), (8000, 2)], mix_rates=mix)
        assert sorted(c["steps"] for c in calls) == [1, 2] and all(c["n"] == 1 for c in calls)
    calls = serve([(8000, 1), (12000, 2), (16000, 1)], mix_rates=True)
    assert sorted((c["steps"], c["n"]) for c in calls) == [(1, 2), (2, 1)]
    assert next(c for c in calls if c["steps"] == 1)["sr"] == [8000, 16000]


def test_server_mix_rates_resolves_from_the_environment(monkeypatch):
    from flowhigh_amd import serve as S
    m = StubModel()
    for env, want in (("1", True), ("0", False)):
        monkeypatch.setenv("FH_SERVE_MIX_RATES", env)
        srv = BatchingServer(m)
        assert srv.mix_rates is want
        srv.close()
        srv = BatchingServer(m, mix_rates=not want)                  # the keyword wins
        assert srv.mix_rates is (not want)
        srv.close()
    monkeypatch.delenv("FH_SERVE_MIX_RATES")
    srv = BatchingServer(m)
    assert srv.mix_rates is S.MIX_RATES_DEFAULT
    srv.close()
    monkeypatch.setenv("FH_SERVE_MIX_RATES", "yes")
    with pytest.raises(ValueError):
        BatchingServer(m)
