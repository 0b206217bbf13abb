"""CPU: the CAVP spectrogram tower's host side.  The float64 restatement (tests/cavp_spec_ref.py) is pinned to the reference's own Cnn14
by golden G15 (tests/golden/make_golden_cavp_spec.py); the synthetic key layout, the facade's signatures, its load_state_dict
bookkeeping, the ABI table and the output-row arithmetic are checked without a GPU."""
import inspect
import json
import os
import re

import pytest
import torch

import diff_foley_amd as P
from diff_foley_amd import engine as E, synth
import cavp_spec_ref as R
from helpers import GOLD, gold, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_64, SEED_72, SEED_256 = 151, 152, 153          # make_golden_cavp_spec.py


@pytest.fixture(scope="module")
def full_sd():
    return synth.make_state_dict(synth.cavp_audio_spec(synth.CAVP_AUDIO_FULL))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "g15_cavp_spec.json")) as f:
        return json.load(f)


def test_restatement_reproduces_the_reference(full_sd):
    """Every G15 record to fp32 round-off: the reference ran in fp32, the restatement in float64."""
    g = gold("g15_cavp_spec.npz")
    taps = {}
    mel = synth.synthetic_mel(2, 64, 128, SEED_64)
    got = {"f64_raw": R.encode_spec(full_sd, mel, normalize=False, pool=False, taps=taps),
           "f64_norm": R.encode_spec(full_sd, mel, normalize=True, pool=False),
           "f64_block1": taps["conv_block1"][1, :, ::2, ::2], "f64_block4": taps["conv_block4"][1],
           "f64_block6": taps["conv_block6"][1, ::2],
           "f72_raw": R.encode_spec(full_sd, synth.synthetic_mel(1, 72, 128, SEED_72), normalize=False, pool=False)}
    mel = synth.synthetic_mel(2, 256, 128, SEED_256)
    got["f256_pool"] = R.encode_spec(full_sd, mel, normalize=False, pool=True)
    got["f256_pool_norm"] = R.encode_spec(full_sd, mel, normalize=True, pool=True)
    assert set(got) == set(g)
    for k in sorted(g):
        assert got[k].shape == g[k].shape, k
        err = rel_l2(got[k], g[k])
        print(f"g15 {k}: rel-L2 {err:.2e}, |ref| {float(g[k].abs().mean()):.3e}")
        assert err < 1e-5, (k, err)
    assert g["f72_raw"].shape == (1, 4, 512) and g["f256_pool"].shape == (2, 512)
    # the records are no degenerate case: the two clips, and the rows of a clip, differ
    assert rel_l2(g["f64_raw"][0], g["f64_raw"][1]) > 1e-2 and rel_l2(g["f64_raw"][0, 0], g["f64_raw"][0, 2]) > 1e-3


def test_synthetic_keys_are_the_reference_state_dict(meta):
    spec = synth.cavp_audio_spec(synth.CAVP_AUDIO_FULL)
    assert {k: list(v) for k, v in spec.items()} == meta["keys"]
    assert sum(int(torch.Size(s).numel()) for s in spec.values()) > 80_000_000
    tiny = synth.cavp_audio_spec(synth.CAVP_AUDIO_TINY)
    assert list(tiny) == list(spec) and tiny["spec_encoder.conv_block6.conv2.weight"] == (256, 256, 3, 3)


def test_facade_signatures_are_the_reference_ones(meta):
    assert str(inspect.signature(P.CAVPInference.encode_spec)) == meta["signatures"]["encode_spec"]
    assert str(inspect.signature(P.CAVPInference.forward)) == meta["signatures"]["forward"]


def _tiny_model():
    a = synth.CAVP_AUDIO_TINY
    return P.CAVPInference(embed_dim=a["embed_dim"], stage_blocks=synth.CAVP_TINY["stage_blocks"], spec_channels=a["channels"],
                           spec_fc_dim=a["fc_dim"], spec_n_mels=a["n_mels"])


def test_load_state_dict_bookkeeping():
    video = synth.make_state_dict(synth.cavp_spec(synth.CAVP_TINY))
    audio = synth.make_state_dict(synth.cavp_audio_spec(synth.CAVP_AUDIO_TINY))
    # complete key set: the tower is kept, nothing is unexpected
    m = _tiny_model()
    missing, unexpected = m.load_state_dict({**video, **audio})
    assert missing == [] and unexpected == []
    assert m._spec_state is not None and set(m._spec_state) == set(audio) - {"logit_scale"}
    assert float(m.logit_scale) == float(audio["logit_scale"])
    # one key missing: the tower is dropped and its keys are reported, as every spec_encoder.* key was before
    part = {**video, **audio}
    del part["spec_encoder.conv_block3.bn2.running_var"]
    m = _tiny_model()
    missing, unexpected = m.load_state_dict(part)
    assert missing == [] and sorted(unexpected) == sorted(set(audio) - {"spec_encoder.conv_block3.bn2.running_var"})
    assert m._spec_state is None and m.logit_scale is None
    assert m._spec_missing == ["spec_encoder.conv_block3.bn2.running_var"]
    # video only: as before
    m = _tiny_model()
    assert m.load_state_dict(video) == ([], [])
    assert m._spec_state is None
    # a tower of another width is a size mismatch, as in torch
    wide = synth.make_state_dict(synth.cavp_audio_spec({**synth.CAVP_AUDIO_TINY, "channels": [64, 64, 128, 128, 256, 512], "fc_dim": 512}))
    with pytest.raises(RuntimeError, match="size mismatch"):
        _tiny_model().load_state_dict({**video, **wide})
    with pytest.raises(NotImplementedError):
        P.CAVPInference(spec_encode="cnn10")


def test_without_gpu_encode_spec_fails_loudly():
    m = _tiny_model()
    with pytest.raises(RuntimeError):
        m.encode_spec(torch.zeros(1, 64, 16))


def _header_params(name):
    hdr = open(os.path.join(ROOT, "include", "df_engine.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["df_config_cavp_spec", "df_cavp_spec_encode", "df_cavp_similarity", "df_test_spec_conv_in",
                                  "df_test_avgpool_nhwc", "df_test_spec_head_pool", "df_test_cavp_spec_tap"])
def test_abi_header_and_ctypes_table_agree(name):
    import ctypes as C
    params, sig = _header_params(name), E._SIGS[name]
    assert len(params) == len(sig), (params, sig)
    for p, t in zip(params, sig):
        if "*" in p:
            assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p, t)
        elif p.startswith("float"):
            assert t is C.c_float, (name, p, t)
        else:
            assert p.startswith("int ") and t is C.c_int, (name, p, t)
    assert name in E.exported_symbols()
    fields = dict(E.CavpSpecConfig._fields_)
    assert list(fields) == ["n_mels", "channels", "fc_dim", "embed_dim"] and C.sizeof(E.CavpSpecConfig) == 9 * 4


@pytest.mark.parametrize("frames, rows", [(16, 1), (17, 1), (31, 1), (72, 4), (512, 32), (15, 0)])
def test_output_rows(frames, rows):
    assert E.Engine.cavp_spec_rows(frames) == rows == R.out_rows(frames)
