#!/usr/bin/env python
"""Generate G15, the golden vectors of the CAVP spectrogram tower (CAVP_Inference.encode_spec, the reference's own Cnn14).

Runs ONLY in the build container, like make_golden.py: it imports the reference implementation (oracle/ref_import.py) on the CPU,
loads procedurally generated weights (diff_foley_amd/synth.py: cavp_audio_spec(CAVP_AUDIO_FULL)) and stores the reference's OUTPUTS.
Inputs are regenerated from their seeds by the tests (synth.synthetic_mel); no reference source is copied.

    python tests/golden/make_golden_cavp_spec.py        # a few seconds

g15_cavp_spec.npz:
  f64_raw / f64_norm           encode_spec(mel, pool=False), normalize False / True, mel = synthetic_mel(2, 64, 128, SEED_64)
  f64_block1 / _block4 / _block6   forward-hook outputs of conv_block1 / 4 / 6 for CLIP 1 of that call (block1: every second pixel
                               in both axes, block6: every second channel)
  f72_raw                      encode_spec(pool=False) of synthetic_mel(1, 72, 128, SEED_72): 72 -> 36 -> 18 -> 9 -> 4, the fourth pool floors
  f256_pool / f256_pool_norm   encode_spec(pool=True), normalize False / True, synthetic_mel(2, 256, 128, SEED_256): one 16-row window
g15_cavp_spec.json:
  keys        the reference state dict's spec_encoder.* / logit_scale entries, key -> shape (num_batches_tracked left out)
  signatures  str(inspect.signature) of CAVP_Inference.encode_spec and .forward
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import diff_foley_amd  # noqa: E402,F401
from diff_foley_amd import synth  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED_64, SEED_72, SEED_256 = 151, 152, 153


@torch.no_grad()
def main():
    CAVP = ref_import.import_reference_cavp()
    torch.manual_seed(0)
    model = CAVP(video_encode="Slowonly_pool", spec_encode="cnn14_pool", embed_dim=512)
    sd = synth.make_state_dict(synth.cavp_audio_spec(synth.CAVP_AUDIO_FULL))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    bad = [k for k in list(missing) + list(unexpected) if k.startswith("spec_encoder.") or k == "logit_scale"]
    assert not bad, bad[:5]
    model.eval()

    out = {}
    hooks = {}
    enc = model.spec_encoder
    hs = [getattr(enc, f"conv_block{i}").register_forward_hook(lambda m, a, o, i=i: hooks.__setitem__(i, o)) for i in (1, 4, 6)]
    mel = synth.synthetic_mel(2, 64, 128, SEED_64)
    out["f64_raw"] = model.encode_spec(mel, normalize=False, pool=False)
    for h in hs:
        h.remove()
    out["f64_block1"] = hooks[1][1, :, ::2, ::2]
    out["f64_block4"] = hooks[4][1]
    out["f64_block6"] = hooks[6][1, ::2]
    out["f64_norm"] = model.encode_spec(mel, normalize=True, pool=False)
    out["f72_raw"] = model.encode_spec(synth.synthetic_mel(1, 72, 128, SEED_72), normalize=False, pool=False)
    mel = synth.synthetic_mel(2, 256, 128, SEED_256)
    out["f256_pool"] = model.encode_spec(mel, normalize=False, pool=True)
    out["f256_pool_norm"] = model.encode_spec(mel, normalize=True, pool=True)

    path = os.path.join(HERE, "g15_cavp_spec.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    keys = {k: list(v.shape) for k, v in model.state_dict().items()
            if (k.startswith("spec_encoder.") or k == "logit_scale") and not k.endswith("num_batches_tracked")}
    meta = {"keys": keys, "signatures": {"encode_spec": str(inspect.signature(CAVP.encode_spec)),
                                         "forward": str(inspect.signature(CAVP.forward))}}
    with open(os.path.join(HERE, "g15_cavp_spec.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote g15_cavp_spec.npz: {os.path.getsize(path) / 1024:.1f} KiB;", {k: tuple(v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
