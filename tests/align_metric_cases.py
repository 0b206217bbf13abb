"""Shared by the Align-Acc tests and tests/golden/make_golden_align_metric.py: the seeded weights and inputs of G16's draws, and a
pure-Python restatement of the verdict (torch.round + count, evaluation/align_acc.py:85-86)."""
import torch

from diff_foley_amd import synth
from vae_encoder_ref import mel_like

SAMPLE_SEED = 5                  # torch.manual_seed before the posterior draws
TINY_FRAMES = (8, 32)
N_DRAWS = 32
CFG = {"tiny": (synth.CLS_TINY, synth.VAE_TINY, synth.COND_METRIC_TINY), "full": (synth.CLS_FULL, synth.VAE_FULL, synth.COND_METRIC)}

_sd = {}


def state_dict(which, bias=None):
    """Procedural weights (seed 0) under the metric model's prefixes; ``bias`` replaces model.classifier.bias (G16's moved threshold)."""
    if which not in _sd:
        _sd[which] = synth.make_state_dict(synth.align_metric_spec(*CFG[which]), 0)
    sd = dict(_sd[which])
    if bias is not None:
        sd["model.classifier.bias"] = torch.as_tensor(bias, dtype=torch.float32).reshape(sd["model.classifier.bias"].shape).clone()
    return sd


def inputs(which, frames):
    """(images, CAVP-like features, posterior noise) of the N_DRAWS draws of a configuration: row i is draw i."""
    g = torch.Generator().manual_seed(SAMPLE_SEED)
    if which == "tiny":
        x = mel_like((N_DRAWS, 1, 32, 64), 160 + frames).repeat(1, 3, 1, 1)      # as the dataset yields them: one mel, three times
        feats = synth.synthetic_cavp(N_DRAWS, frames, 64, seed=1234 + frames)
        return x, feats, torch.randn(N_DRAWS, 4, 8, 16, generator=g)
    x = synth.synthetic_mel(N_DRAWS, 512, 128, seed=99)[:, None].repeat(1, 3, 1, 1)
    feats = synth.synthetic_cavp(N_DRAWS, frames, 512, seed=1234)
    return x, feats, torch.randn(N_DRAWS, 4, 16, 64, generator=g)


def round_half_even(p):
    """torch.round of one probability, in Python: the nearest integer, a tie to the even one (0.5 -> 0, 1.5 -> 2, 2.5 -> 2)."""
    p = float(p)
    if p != p:
        return p
    lo = float(int(p // 1))
    d = p - lo
    if d > 0.5 or (d == 0.5 and lo % 2 == 1):
        return lo + 1.0
    return lo


def verdict(probs, labels=None):
    """(pred list, correct, total) of one batch: labels default to ones (align_acc.py:76)."""
    probs = [float(v) for v in probs]
    labels = [1.0] * len(probs) if labels is None else [float(v) for v in labels]
    pred = [round_half_even(p) for p in probs]
    return pred, sum(1 for a, b in zip(pred, labels) if a == b), len(probs)
