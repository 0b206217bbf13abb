"""CPU: the host side of the Align-Acc metric model (diff_foley_amd.AlignmentClassifierMetric) against what the reference itself says --
G16 (tests/golden/make_golden_align_metric.py): the key / shape lists of the reference module and the parameter lists of its
constructor and evaluation-path methods -- then the rounding rule and the count in a pure-Python restatement, the dataset rules of
evaluation/dataset.py, and the options that select code this package does not build."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

import diff_foley_amd as P
from diff_foley_amd import ldm, synth
from helpers import GOLD
import align_metric_cases as K
from test_signatures_cpu import _described, compare

REF_TARGET = "diff_foley.modules.double_guidance.alignment_classifier_metric.Alignment_Classifier_metric"


def g16():
    return dict(np.load(os.path.join(GOLD, "g16_align_metric.npz")))


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_spec_is_the_reference_modules_key_and_shape_list(which):
    g = g16()
    ref = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(g[which + "_keys"], g[which + "_shapes"])}
    spec = {k: tuple(s) for k, s in synth.align_metric_spec(*K.CFG[which]).items()}
    assert spec == ref, (sorted(set(spec) ^ set(ref))[:5], [k for k in spec if k in ref and spec[k] != ref[k]][:5])
    if which == "full":
        assert len(spec) == 257


with open(os.path.join(GOLD, "g16_signatures.json")) as _f:
    SIGNATURES = json.load(_f)

# parameters this package adds behind the reference's, each with a default
EXTRAS = {}


def _counterpart(name):
    M = P.AlignmentClassifierMetric
    if name == "model":
        return ldm._MetricBackboneFacade.__call__
    if name == "cond_model":
        return ldm._MetricCondFacade.__call__
    return getattr(M, name)


@pytest.mark.parametrize("point", sorted(SIGNATURES))
def test_facade_takes_what_the_reference_takes(point):
    compare(SIGNATURES[point], _described(_counterpart(point.split(".")[1])), (), EXTRAS.get(point))


def test_fixture_names_the_evaluation_path():
    want = {"__init__", "init_first_from_ckpt", "encode_first_stage", "get_first_stage_encoding", "encode_spec_z", "encode_cond", "forward",
            "model", "cond_model"}
    assert {k.split(".")[1] for k in SIGNATURES} == want
    # what this package adds: the keyword names of the issue's interface
    import inspect
    assert list(inspect.signature(P.AlignmentClassifierMetric.probabilities).parameters) == ["self", "spec", "video_feat", "noise"]
    assert list(inspect.signature(P.AlignmentClassifierMetric.align_acc).parameters)[:5] == ["self", "specs", "video_feats", "labels",
                                                                                              "batch_size"]
    assert inspect.signature(P.AlignmentClassifierMetric.align_acc).parameters["batch_size"].default == 64


def test_round_half_to_even_and_the_count():
    one = np.float32(1.0)
    half = np.float32(0.5)
    below, above = np.nextafter(half, np.float32(0)), np.nextafter(half, one)
    cases = [(0.0, 0.0), (1.0, 1.0), (half, 0.0), (below, 0.0), (above, 1.0), (np.float32(0.25), 0.0), (np.float32(0.75), 1.0),
             (np.nextafter(one, np.float32(0)), 1.0), (np.float32(1.5), 2.0), (np.float32(2.5), 2.0), (np.float32(1e-30), 0.0)]
    for p, want in cases:
        assert K.round_half_even(p) == want, (p, want)
        assert float(torch.round(torch.tensor(float(p), dtype=torch.float32))) == want, p       # torch.round is the rule restated
    assert math.isnan(K.round_half_even(float("nan")))
    probs = [c[0] for c in cases]
    pred, correct, total = K.verdict(probs)
    assert pred == [c[1] for c in cases] and total == len(cases)
    assert correct == sum(1 for c in cases if c[1] == 1.0) == 4          # labels default to ones: 1.5 -> 2 and 2.5 -> 2 match nothing
    labels = [0, 1, 0, 1, 1, 0, 0, 1, 2, 0, 1]
    assert K.verdict(probs, labels)[1] == sum(1 for c, l in zip(cases, labels) if c[1] == l) == 7
    assert K.verdict([float("nan")], [1.0])[1] == 0 and K.verdict([], None) == ([], 0, 0)


def test_dataset_rules():
    # evaluation/dataset.py:36: the last two '_' fields go; the rest keeps its own underscores
    assert ldm.align_acc_clip_name("abc_000123_0_mel.npy") == "abc_000123"
    assert ldm.align_acc_clip_name("-a_b_c_000030_sample_0.npy") == "-a_b_c_000030"
    assert ldm.align_acc_clip_name("x_y.npy") == ""
    # :95-96 with eval_classifier.yaml's fps / truncate / sr, and the int() floor of another setting
    assert ldm.align_acc_frames() == ldm.align_acc_frames(4, 131072, 16000) == 32
    assert ldm.align_acc_frames(21.5, 220000, 22050) == 214
    # :99-107: one-channel mels are cut to 512 columns and repeated to 3 channels; 4-D images pass through untouched
    mel = torch.arange(2 * 4 * 600, dtype=torch.float32).reshape(2, 4, 600)
    x = ldm.align_acc_specs(mel)
    assert tuple(x.shape) == (2, 3, 4, 512)
    for c in range(3):
        assert torch.equal(x[:, c], mel[:, :, :512])
    short = ldm.align_acc_specs(mel[:, :, :100])
    assert tuple(short.shape) == (2, 3, 4, 100)
    img = torch.zeros(2, 3, 8, 16)
    assert ldm.align_acc_specs(img) is img
    with pytest.raises(RuntimeError, match="specs must be"):
        ldm.align_acc_specs(torch.zeros(4, 4))


def test_reference_target_builds_this_class_and_unbuilt_options_raise():
    params = P.align_metric_config(synth.CLS_TINY, synth.VAE_TINY, synth.COND_METRIC_TINY)
    m = P.instantiate_from_config(dict(target=REF_TARGET, params=params))
    assert isinstance(m, P.AlignmentClassifierMetric) and m.scale_factor == 0.18215 and m.num_timesteps == 1000
    assert isinstance(P.instantiate_from_config(dict(target="diff_foley_amd.ldm.AlignmentClassifierMetric", params=params)),
                      P.AlignmentClassifierMetric)
    assert P.AlignmentClassifierMetric(**P.align_metric_config()).cls_cfg == synth.CLS_FULL

    def bad(path, value, **top):
        p = copy.deepcopy(params)
        node = p
        for k in path[:-1]:
            node = node[k]
        if path:
            node[path[-1]] = value
        p.update(top)
        return p
    for p in (bad(("classifier_config", "params", "use_scale_shift_norm"), True), bad(("classifier_config", "params", "transformer_depth"), 2),
              bad(("classifier_config", "params", "num_head_channels"), 32),
              bad(("first_stage_config", "params", "ddconfig", "attn_resolutions"), [16]),
              bad(("first_stage_config", "params", "ddconfig", "tanh_out"), True),
              bad(("first_stage_config", "params", "ddconfig", "double_z"), False),
              bad(("first_stage_config", "params", "ddconfig", "in_channels"), 5),
              bad((), None, beta_schedule="cosine"), bad((), None, given_betas=[0.1, 0.2]), bad((), None, parameterization="mu")):
        with pytest.raises(NotImplementedError):
            P.AlignmentClassifierMetric(**p)
    with pytest.raises(ValueError, match="context_dim"):
        P.AlignmentClassifierMetric(**bad(("cond_stage_config", "params", "embed_dim"), 128))
    with pytest.raises(TypeError):
        P.AlignmentClassifierMetric(classifier_config=params["classifier_config"])        # first_stage_config ... monitor are required


def test_load_state_dict_on_the_host(tmp_path):
    params = P.align_metric_config(synth.CLS_TINY, synth.VAE_TINY, synth.COND_METRIC_TINY)
    sd = K.state_dict("tiny")
    m = P.AlignmentClassifierMetric(**params)
    # the checkpoint's buffers and a decoder, when it has them, are neither missing nor kept; anything else is reported
    extra = dict(sd, scale_factor=torch.tensor(0.25), betas=torch.zeros(1000), stray=torch.zeros(1))
    extra.update(synth.make_state_dict(synth.vae_decoder_spec(synth.VAE_TINY, "first_stage_model."), 0))
    missing, unexpected = m.load_state_dict(extra)
    assert missing == [] and "stray" in unexpected and m.scale_factor == 0.25
    assert all(k == "stray" or k.startswith(("first_stage_model.decoder.", "first_stage_model.post_quant_conv.")) for k in unexpected)
    assert set(m._state) == set(sd)
    # no classifier keys: raises and names them
    with pytest.raises(RuntimeError, match=r"Missing key\(s\).*model\.time_embed\.0\.weight"):
        P.AlignmentClassifierMetric(**params).load_state_dict({k: v for k, v in sd.items() if not k.startswith("model.")})
    # another architecture's tensor is a size mismatch, not a different network
    with pytest.raises(RuntimeError, match="size mismatch for model.classifier.weight"):
        P.AlignmentClassifierMetric(**params).load_state_dict(dict(sd, **{"model.classifier.weight": torch.zeros(1, 7)}))
    # first_stage_ckpt: torch.load, 'state_dict' unwrapped, 'module.' stripped; the rest then comes from load_state_dict
    fs = {"module." + k[len("first_stage_model."):]: v for k, v in sd.items() if k.startswith("first_stage_model.")}
    path = os.path.join(tmp_path, "first_stage.ckpt")
    torch.save({"state_dict": fs}, path)
    m2 = P.AlignmentClassifierMetric(first_stage_ckpt=path, **params)
    assert m2.load_state_dict({k: v for k, v in sd.items() if not k.startswith("first_stage_model.")}) == ([], [])
    assert set(m2._state) == set(sd) and all(torch.equal(m2._state[k], sd[k]) for k in sd)
    # nothing runs without a GPU, and says so
    with pytest.raises(RuntimeError, match="load_state_dict|ROCm|GPU"):
        m2.probabilities(torch.zeros(1, 3, 32, 64), torch.zeros(1, 8, 64))
