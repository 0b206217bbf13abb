#!/usr/bin/env python
"""Generate G13, the golden vectors of the VAE encoder (first_stage_model.encode).

Runs ONLY in the build container, like make_golden.py: it imports the reference implementation (oracle/ref_import.py stubs) on the
CPU, loads procedurally generated weights (diff_foley_amd/synth.py, with the encoder's keys) and stores the reference's OUTPUTS.
Inputs are regenerated from their seeds by the tests; no reference source is copied.

    python tests/golden/make_golden_vae_encoder.py        # a few seconds

g13_vae_encoder.npz:
  tiny_keys / tiny_shapes, full_keys / full_shapes   the reference module's encoder.* / quant_conv.* parameters (name, shape padded
                                                     with -1 to 4 dims)
  tiny_moments                 AutoencoderKL.encode(x).parameters, x = mel_like((2, 3, 32, 64), 131), VAE_TINY
  tiny_conv_in / tiny_down<l> / tiny_mid             hooked module outputs of SAMPLE 1 (conv_in: every second pixel in both axes)
  tiny_sample                  posterior.sample() under torch.manual_seed(5)
  full_moments                 the same for VAE_FULL, x = mel_like((1, 3, 128, 512), 132)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diff_foley_amd  # noqa: E402,F401
from diff_foley_amd import synth  # noqa: E402
from oracle import ref_import  # noqa: E402
from vae_encoder_ref import mel_like  # noqa: E402

TINY_SEED, FULL_SEED, SAMPLE_SEED = 131, 132, 5


def reference_vae(unet, vae, cond):
    spec = synth.state_dict_spec(unet, vae, cond, with_encoder=True)
    sd = synth.make_state_dict(spec, 0)
    cfg = ref_import.load_ldm_config(unet=unet, vae=vae, cond=cond)
    model, _ = ref_import.build_reference_ldm(cfg, sd)
    fs = model.first_stage_model
    missing = [k for k in fs.state_dict() if k.startswith(("encoder.", "quant_conv.")) and "first_stage_model." + k not in sd]
    assert not missing, missing[:5]
    return fs


def key_map(fs):
    items = [(k, tuple(v.shape)) for k, v in fs.state_dict().items() if k.startswith(("encoder.", "quant_conv."))]
    names = np.array([k for k, _ in items])
    shapes = np.array([list(s) + [-1] * (4 - len(s)) for _, s in items], dtype=np.int64)
    return names, shapes


@torch.no_grad()
def main():
    out = {}
    fs = reference_vae(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY)
    out["tiny_keys"], out["tiny_shapes"] = key_map(fs)
    hooks = {}
    hs = [fs.encoder.conv_in.register_forward_hook(lambda m, i, o: hooks.__setitem__("conv_in", o)),
          fs.encoder.mid.block_2.register_forward_hook(lambda m, i, o: hooks.__setitem__("mid", o))]
    for lvl, d in enumerate(fs.encoder.down):
        if hasattr(d, "downsample"):
            hs.append(d.downsample.register_forward_hook(lambda m, i, o, lvl=lvl: hooks.__setitem__(f"down{lvl}", o)))
    post = fs.encode(mel_like((2, 3, 32, 64), TINY_SEED))
    for h in hs:
        h.remove()
    out["tiny_moments"] = post.parameters
    out["tiny_conv_in"] = hooks.pop("conv_in")[1:2, :, ::2, ::2]
    for k, v in hooks.items():
        out["tiny_" + k] = v[1:2]
    torch.manual_seed(SAMPLE_SEED)
    out["tiny_sample"] = post.sample()

    fs = reference_vae(synth.UNET_TINY, synth.VAE_FULL, synth.COND_TINY)      # the UNet is not run: the tiny one keeps this quick
    out["full_keys"], out["full_shapes"] = key_map(fs)
    out["full_moments"] = fs.encode(mel_like((1, 3, 128, 512), FULL_SEED)).parameters

    path = os.path.join(HERE, "g13_vae_encoder.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print(f"wrote g13_vae_encoder.npz: {os.path.getsize(path) / 1024:.1f} KiB;", {k: tuple(np.shape(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()
