"""CPU: the VAE encoder's host side -- key layout against the reference module (G13), the complete-set load rule, the facade's
refusals without encoder weights, and the torch restatement the GPU fuzz is judged against (tests/vae_encoder_ref.py) against G13."""
import os

import numpy as np
import pytest
import torch

import diff_foley_amd as P
from diff_foley_amd import synth
from helpers import GOLD, tiny_state_dict
import vae_encoder_ref as R

TINY_SEED, FULL_SEED, SAMPLE_SEED = 131, 132, 5      # tests/golden/make_golden_vae_encoder.py


def g13():
    path = os.path.join(GOLD, "g13_vae_encoder.npz")
    assert os.path.exists(path), "tests/golden/g13_vae_encoder.npz is a committed fixture"
    return dict(np.load(path))


def tiny_encoder_state_dict():
    spec = synth.state_dict_spec(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY, with_encoder=True)
    return synth.make_state_dict(spec, 0)


def close(a, b, tol=2e-5):
    b = torch.as_tensor(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a.double() - b.double()).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), err


@pytest.mark.parametrize("name, cfg, n", [("tiny", synth.VAE_TINY, 64), ("full", synth.VAE_FULL, 108)])
def test_encoder_spec_is_the_reference_modules_key_layout(name, cfg, n):
    g = g13()
    want = {str(k): tuple(int(d) for d in s if d >= 0) for k, s in zip(g[name + "_keys"], g[name + "_shapes"])}
    got = synth.vae_encoder_spec(cfg, "")
    assert len(want) == n
    assert {k: tuple(v) for k, v in got.items()} == want


def test_state_dict_spec_without_the_flag_is_unchanged():
    base = synth.state_dict_spec(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY)
    assert not [k for k in base if ".encoder." in k or ".quant_conv." in k]
    assert list(base) == list(synth.state_dict_spec(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY, with_encoder=False))
    full = synth.state_dict_spec(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY, with_encoder=True)
    enc = synth.vae_encoder_spec(synth.VAE_TINY, "first_stage_model.")
    assert {k: v for k, v in full.items() if k not in enc} == dict(base) and all(full[k] == enc[k] for k in enc)


def _model():
    return P.LatentDiffusion(**P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))


def test_the_encoder_is_taken_only_as_a_complete_key_set():
    sd = tiny_encoder_state_dict()
    enc = synth.vae_encoder_spec(synth.VAE_TINY, "first_stage_model.")
    m = _model()
    missing, unexpected = m.load_state_dict(sd)
    assert missing == [] and unexpected == [] and m._has_encoder
    assert all(k in m._state for k in enc)
    # one key short: the rest is ignored and reported, exactly as before the encoder existed
    part = {k: v for k, v in sd.items() if k != "first_stage_model.quant_conv.bias"}
    m = _model()
    missing, unexpected = m.load_state_dict(part)
    assert not m._has_encoder and not [k for k in m._state if k in enc]
    assert sorted(unexpected) == sorted(k for k in enc if k in part)
    # a lone, wrongly shaped encoder tensor is not a size mismatch (tests/test_boundary_cpu.py loads one)
    m = _model()
    m.load_state_dict(dict(tiny_state_dict(), **{"first_stage_model.encoder.conv_in.weight": torch.zeros(3)}))
    assert not m._has_encoder
    # the complete set with a wrong shape is the usual error
    k = "first_stage_model.encoder.down.0.downsample.conv.weight"
    with pytest.raises(RuntimeError, match="size mismatch for " + k.replace(".", r"\.")):
        _model().load_state_dict(dict(sd, **{k: sd[k][:, :-1]}))


def test_encode_without_encoder_weights_raises_before_anything_else():
    m = _model()
    m.load_state_dict(tiny_state_dict())
    x = torch.zeros(2, 3, 32, 64)
    for call in (m.first_stage_model.encode, m.encode_first_stage):
        with pytest.raises(NotImplementedError, match="encoder"):
            call(x)
        with pytest.raises(NotImplementedError):
            call("not even a tensor")
    with pytest.raises(NotImplementedError, match="not yet implemented"):
        m.get_first_stage_encoding([1, 2])


def test_reference_restatement_meets_g13():
    """tests/vae_encoder_ref.py against the reference's own outputs: moments, the hooked stages and the seeded sample (tiny), the
    full-size moments -- to fp32 round-off, like tests/test_oracle_golden.py."""
    g = g13()
    sd = R.sub_state_dict(tiny_encoder_state_dict())
    hooks = {}
    mom = R.vae_encode(sd, synth.VAE_TINY, R.mel_like((2, 3, 32, 64), TINY_SEED), hooks)
    close(mom, g["tiny_moments"])
    close(hooks["conv_in"][1:2, :, ::2, ::2], g["tiny_conv_in"])
    for k in ("down0", "down1", "mid"):
        close(hooks[k][1:2], g["tiny_" + k])
    torch.manual_seed(SAMPLE_SEED)
    close(R.posterior_sample(mom, torch.randn(2, 4, 8, 16)), g["tiny_sample"])


def test_reference_restatement_meets_g13_full_size():
    g = g13()
    spec = synth.vae_encoder_spec(synth.VAE_FULL, "")
    sd = synth.make_state_dict({"first_stage_model." + k: s for k, s in spec.items()}, 0)
    mom = R.vae_encode(R.sub_state_dict(sd), synth.VAE_FULL, R.mel_like((1, 3, 128, 512), FULL_SEED))
    close(mom, g["full_moments"], 1e-4)
