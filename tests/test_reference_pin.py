"""CPU: the oracle against the reference on cases that are not among the other golden vectors.  The reference's
outputs are stored in tests/golden/pin.npz (oracle/make_golden.py ran the reference under the shims of
oracle/ref_shim.py: `python -m oracle.make_golden pin`)."""
import json

import numpy as np
import pytest
import torch

from flowhigh_amd import synth
from oracle import ref_cpu
from oracle.make_golden import pin_key
from conftest import GOLDEN


def load_pin():
    with np.load(GOLDEN / "pin.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("cfgname,sr_in,method,steps", [("ALT_CFG", 12000, "euler", 2), ("TINY_CFG", 24000, "midpoint", 1),
                                                        # upsamplers with k - u odd (the vocoder returns 480 N + 98 samples), five kernel sizes
                                                        ("ODD_CFG", 16000, "midpoint", 1), ("NK5_AMP2_CFG", 8000, "euler", 1)])
def test_oracle_equals_live_reference(cfgname, sr_in, method, steps):
    """The reference's generate() on weights seed 11, clip seed 11 and its own prior draw (torch.manual_seed(4242))."""
    cfg = getattr(synth, cfgname)
    sd = synth.make_state_dict(cfg, 11)
    ref = load_pin()[pin_key(cfgname, sr_in, method, steps)]
    audio = synth.lowres_clip(11, 0.23, sr_in)
    n = ref.shape[-1] // 480
    g = torch.Generator().manual_seed(4242)
    from flowhigh_amd.flowhighsr import reference_prior_draw
    noise = reference_prior_draw(n, 256, g)
    out = ref_cpu.generate(sd, cfg, audio, sr_in, noise, steps, method)
    assert out.shape == ref.shape
    assert np.abs(out.numpy() - ref).max() <= 2e-6


def test_reference_state_dict_contract():
    """The synthetic checkpoint loads into the reference with strict=True: key names and shapes of
    flowhigh_amd.synth are exactly the reference's (flowhighsr.py:131-135)."""
    sd = synth.make_state_dict(synth.TINY_CFG, 0)
    ref_shapes = json.loads(str(load_pin()["tiny_state_dict_shapes"]))
    assert set(ref_shapes) == set(sd)
    for k, shape in ref_shapes.items():
        assert tuple(shape) == tuple(sd[k].shape), k
