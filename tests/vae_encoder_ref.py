"""Torch-fp32 restatement of the reference's VAE encoder for the tests (the oracle package is frozen; its ResnetBlock / AttnBlock
restatements are reused).  Test infrastructure only.

  * AutoencoderKL.encode                  diff_foley/models/autoencoder.py:324-328
  * Encoder.forward                       diff_foley/modules/stage1_autoencoder/model.py:529-554
  * Downsample.forward                    model.py:167-171 (F.pad (0,1,0,1), then a stride-2 conv with padding 0)
  * DiagonalGaussianDistribution          model.py:34-47
"""
import torch
import torch.nn.functional as F

from helpers import rnd
from oracle.vae import _conv, _gn, _swish, attn_block, resnet_block


def mel_like(shape, seed):
    """Seeded image in the normalised log-mel's range [-1, 1] (N(0, 0.5), clipped)."""
    return (0.5 * rnd(shape, seed)).clamp_(-1.0, 1.0)


def sub_state_dict(sd, prefix="first_stage_model."):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


@torch.no_grad()
def vae_encode(sd, cfg, x, hooks=None):
    """quant_conv(encoder(x)): the posterior's ``parameters``.  ``sd`` keys relative to ``first_stage_model.``; ``hooks`` (a dict)
    receives 'conv_in', 'down<l>' (each Downsample's output) and 'mid' (mid.block_2's output)."""
    nres = len(cfg["ch_mult"])
    h = _conv(x, sd, "encoder.conv_in")
    if hooks is not None:
        hooks["conv_in"] = h
    for lvl in range(nres):
        for ib in range(cfg["num_res_blocks"]):
            h = resnet_block(sd, f"encoder.down.{lvl}.block.{ib}", h)
        if lvl != nres - 1:
            p = f"encoder.down.{lvl}.downsample.conv"
            h = F.conv2d(F.pad(h, (0, 1, 0, 1)), sd[p + ".weight"], sd[p + ".bias"], stride=2)
            if hooks is not None:
                hooks[f"down{lvl}"] = h
    h = resnet_block(sd, "encoder.mid.block_1", h)
    h = attn_block(sd, "encoder.mid.attn_1", h)
    h = resnet_block(sd, "encoder.mid.block_2", h)
    if hooks is not None:
        hooks["mid"] = h
    h = _conv(_swish(_gn(h, sd, "encoder.norm_out")), sd, "encoder.conv_out")
    return _conv(h, sd, "quant_conv", 0)


def posterior_sample(moments, noise):
    mean, logvar = torch.chunk(moments, 2, dim=1)
    return mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise
