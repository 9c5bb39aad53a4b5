"""The host side of tests/test_hip_attention_edges.py (tests/tools/attn_edges.py): the builders' own claims in float64, the fp32
restatement of the kernels' frame passing every assertion the GPU test makes, and every one of its ten mutants failing a named
one -- which is what shows that those assertions can fail.  The table with the sizes of the misses: profiles/attention_edges.md."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import attn_edges as AE                                  # noqa: E402

GOOD = AE.EmulatedRunner()
BATCH_N = (1, 65, 129)                                   # where the host also runs the SPLIT = 1 shape (heads = 16: 32 or 16 clips)


def shapes_for(n, heads):
    return ("alone", "batch") if heads == 16 and n in BATCH_N else ("alone",)


# ---- the builders' claims ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", AE.N_EDGES)
def test_uniform_builder(n):
    for c in AE.UNIFORM_C:
        case = AE.uniform(n, 2, 3, c)
        lg = AE.logits2_f64(case)
        assert torch.equal(lg, torch.full_like(lg, c * case.scale * AE.LOG2E)) and lg.abs().max().item() <= AE.MAX_LOGIT2
        ref = AE.attention_f64(case.qkv, 2, n, 3, case.scale).view(2, n, 3 * AE.DH)
        for b in range(2):
            # one number per clip, the mean of its V (to float64 rounding: a sum of <= 257 terms, each within 2^-53)
            assert ref[b].max().item() - ref[b].min().item() <= 1e-12 * ref[b].max().item()
            assert abs(ref[b, 0, 0].item() - ((n + 1) / 2 + 1000 * b)) <= 1e-9 * (1000 * b + n)
            assert abs(float(case.extra["expected"][b]) - ref[b, 0, 0].item()) <= 1e-6 * ref[b, 0, 0].item()


@pytest.mark.parametrize("heads", AE.HEADS)
def test_gather_builder(heads):
    for n in AE.N_EDGES:
        case = AE.gather(n, 1, heads, 2000 + 11 * n + heads)                            # (the builder asserts the gap and the contract)
        assert case.extra["gap2"] >= AE.GATHER_GAP2
        pi = case.extra["pi"]
        for h in range(heads):
            assert sorted(pi[0, h].tolist()) == list(range(n))                         # every key -- every tile, every register -- is hit
        ref = AE.attention_f64(case.qkv, 1, n, heads, case.scale)
        assert torch.equal(ref.float(), case.extra["expected"])                        # float64 softmax: the other weights < 2^-200
        assert np.exp2(-AE.GATHER_GAP2) < 2.0 ** -149 / 2                              # below half the smallest fp32 denormal


@pytest.mark.parametrize("name", AE.F64_BUILDERS)
def test_float64_builders_stay_inside_the_contract(name):
    for n in AE.N_F64:
        case = AE.build(name, n, 1, 16, 5)
        lg = AE.logits2_f64(case)
        assert torch.isfinite(case.qkv).all() and lg.abs().max().item() <= AE.MAX_LOGIT2
        if name == "ramp" and n >= 64:
            q0 = AE.split_heads(case.qkv, 1, n, 16)[0][0, :, :, 0]
            for t in range(0, n - 31, 32):                                              # both signs in every 32-query tile
                assert bool((q0[:, t:t + 32] > 0).any(-1).all()) and bool((q0[:, t:t + 32] < 0).any(-1).all())
            tile_max = torch.stack([lg[0, :, :, t:t + 32].max(-1).values for t in range(0, n, 32)], -1)        # [heads, n, tiles]
            up, down = q0 > 0, q0 < 0
            assert bool((tile_max.diff(dim=-1)[up] > 0.5).all()), "b > 0: every tile raises the running maximum"
            assert bool((tile_max.diff(dim=-1)[down] < -0.5).all()), "b < 0: the first tile holds the maximum"
        if name.startswith("offset"):
            nat = lg / AE.LOG2E
            assert 550 <= nat.abs().min().item() and nat.abs().max().item() <= 650
            assert (nat.max(-1).values - nat.min(-1).values).max().item() <= 30        # the spread: a few nats


# ---- the unmutated restatement passes every assertion of the GPU test ---------------------------------------------------------------
@pytest.mark.parametrize("n", AE.N_EDGES)
def test_emulation_uniform_rows(n):
    for heads in AE.HEADS:
        for c in AE.UNIFORM_C:
            AE.check_uniform(GOOD, n, heads, c, shapes_for(n, heads))


@pytest.mark.parametrize("n", AE.N_EDGES)
def test_emulation_gather_is_exact(n):
    for heads in AE.HEADS:
        AE.check_gather(GOOD, n, heads, shapes_for(n, heads))


@pytest.mark.parametrize("name", AE.F64_BUILDERS)
def test_emulation_against_float64(name):
    for n in AE.N_F64:
        AE.check_float64(GOOD, name, n, 16, shapes_for(n, 16), "emulation")
        if name == "soft":
            AE.check_float64(GOOD, name, n, 3, ("alone",), "emulation")


@pytest.mark.parametrize("repeat", [1, 2])
def test_emulation_segment_form(repeat):
    AE.check_segment(GOOD, 16, repeat)


def test_emulation_is_the_plain_attention():
    """attention_emulated against float64 away from every construction: general data, several clips, heads = 3."""
    case = AE.soft(97, 3, 3, 9)
    err = (AE.attention_emulated(case.qkv, 3, 97, 3, case.scale).double() - AE.attention_f64(case.qkv, 3, 97, 3, case.scale)).abs().max().item()
    assert err <= 5e-6


# ---- every mutant fails a named assertion ------------------------------------------------------------------------------------------
CAUGHT_BY = {                                                                           # mutant -> the check that fails, and where
    "key_order": lambda r: AE.check_gather(r, 33, 16, ("alone",)),
    "mask_le": lambda r: AE.check_uniform(r, 33, 16, 0, ("alone",)),
    "whole_off_by_one": lambda r: AE.check_uniform(r, 63, 16, 0, ("alone",)),
    "skip_last_odd_tile": lambda r: AE.check_uniform(r, 63, 16, 0, ("alone",)),
    "drop_stream1": lambda r: AE.check_uniform(r, 64, 16, 0, ("alone",)),
    "no_corr": lambda r: AE.check_float64(r, "ramp", 129, 16, ("alone",), "no_corr"),
    "corr_skip_any": lambda r: AE.check_float64(r, "ramp", 129, 16, ("alone",), "corr_skip_any"),
    "store_past_n": lambda r: AE.check_uniform(r, 65, 16, 0, ("alone",)),
    "head_pitch": lambda r: AE.check_gather(r, 33, 3, ("alone",)),
    "seg_reads_neighbour": lambda r: AE.check_segment(r, 16, 1),
}


def test_every_mutant_has_a_catcher():
    assert set(CAUGHT_BY) == set(AE.MUTANTS) and len(AE.MUTANTS) == 10


@pytest.mark.parametrize("mutant", AE.MUTANTS)
def test_mutant_fails_its_check(mutant):
    CAUGHT_BY[mutant](GOOD)                                                             # the same call passes unmutated ...
    with pytest.raises(AssertionError) as e:
        CAUGHT_BY[mutant](AE.EmulatedRunner(mutant))                                    # ... and fails mutated
    print(f"{mutant}: {str(e.value)[:300]}")


@pytest.mark.parametrize("mutant,check", [
    ("mask_le", lambda r: AE.check_uniform(r, 33, 16, -64, ("alone",))),                # the extra key (logit 0) takes the whole row
    ("no_corr", lambda r: AE.check_gather(r, 129, 16, ("alone",))),                     # an earlier maximum's V row is not wiped
    ("corr_skip_any", lambda r: AE.check_gather(r, 129, 16, ("alone",))),
    ("store_past_n", lambda r: AE.check_gather(r, 129, 16, ("alone", "batch"))),        # SPLIT = 1: 128-query blocks
    ("head_pitch", lambda r: AE.check_float64(r, "soft", 33, 3, ("alone",), "head_pitch")),
    ("key_order", lambda r: AE.check_float64(r, "soft", 33, 16, ("alone",), "key_order")),
    ("drop_stream1", lambda r: AE.check_float64(r, "model_like", 64, 16, ("alone",), "drop_stream1")),
])
def test_mutant_is_caught_a_second_way(mutant, check):
    check(GOOD)
    with pytest.raises(AssertionError):
        check(AE.EmulatedRunner(mutant))
