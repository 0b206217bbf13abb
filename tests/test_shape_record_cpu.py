"""CPU: the record an Engine keeps of what its config_* calls were given (engine.Configured) -- the numbers every forward call checks its
tensors against before a raw pointer goes to the C ABI -- and a source check that nothing reads or writes them another way."""
import glob
import os
import re

import pytest

from diff_foley_amd.engine import Configured

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff_foley_amd")


def test_record_raises_until_configured_and_returns_what_it_was_given():
    rec = Configured()
    for family, call in (("unet", "config_unet"), ("cls", "config_classifier"), ("vae", "config_vae"), ("vae_encoder", "config_vae_encoder"),
                         ("cond", "config_cond"), ("cavp", "config_cavp"), ("cavp_spec", "config_cavp_spec")):
        with pytest.raises(RuntimeError, match=rf"{family} is not configured.*{call}\b") as ex:
            rec.of(family)
        assert not isinstance(ex.value, AttributeError)
    rec.record("unet", in_channels=4, out_channels=8, context_dim=768.0)
    rec.record("vae", z_channels=4, embed_dim=4, out_ch=3, n_mult=3)
    rec.record("vae_encoder", in_channels=3)
    rec.record("cavp_spec", n_mels=128, channels=[64, 128], embed_dim=512)
    u = rec.of("unet")
    assert (u.in_channels, u.out_channels, u.context_dim) == (4, 8, 768) and all(type(v) is int for v in vars(u).values())
    assert rec.of("unet") is u                                  # the stored object: the per-step path copies nothing
    assert vars(rec.of("vae")) == dict(z_channels=4, embed_dim=4, out_ch=3, n_mult=3)
    assert rec.of("cavp_spec").channels == (64, 128) and rec.of("vae_encoder").in_channels == 3
    with pytest.raises(RuntimeError, match="cls is not configured"):
        rec.of("cls")
    rec.drop("vae_encoder")
    rec.drop("vae_encoder")                                     # dropping what is not there is not an error
    with pytest.raises(RuntimeError, match=r"vae_encoder is not configured.*config_vae_encoder"):
        rec.of("vae_encoder")
    assert rec.of("vae").n_mult == 3 and rec.of("unet") is u    # that family only
    rec.record("unet", in_channels=5, out_channels=5, context_dim=5)
    assert rec.of("unet").in_channels == 5                      # a second config_* call replaces the record


def test_no_shape_bookkeeping_outside_the_record():
    families = "(unet|vae|cond|cls|cavp)"
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        src = open(path).read()
        name = os.path.basename(path)
        assert not re.findall(rf'getattr\(\s*self,\s*"{families}_\w+",\s*None\s*\)', src), name
        assert not re.findall(rf"\b(eng|engine|old)\.{families}_\w+\s*=[^=]", src), name      # no module writes them onto an engine
        if name == "engine.py":
            assert not re.findall(rf"\bself\.{families}_\w+\s*=[^=]", src), name              # nor does Engine beside the record
