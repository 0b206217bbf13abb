"""Randomised differential test of the plan builder over UNet CONFIGURATIONS: the reference's UNetModel is a constructor over
(in_channels, out_channels, model_channels, channel_mult, num_res_blocks, attention_resolutions, num_heads, context_dim)
(openai_unetmodel.py:451-692), and a
user of the reference may bring another YAML than Stage2_LDM.yaml.  Seeded draws of those arguments (inside what GroupNorm32 and the
attention kernel's head dimensions admit), procedurally generated weights for each, one ``apply_model`` through the facade
(libdfengine_f16.so) against the oracle's fp32 forward (oracle/unet.py) at a random latent size / context length / batch, and one
classifier-free-guidance call against the oracle's two-pass combination.  The goldens pin two configurations (tiny, full) and the
classifier's; this walks the builder's other branches (levels without attention, one / three ResBlocks per level, odd multipliers,
a single level pair, head dimensions 32 .. 160).

Tolerance: rel-L2 < 5e-3 for one forward on the fp16-operand build (the tiny configuration's forward sits at 1e-3 .. 1.5e-3)."""
import os

import pytest
import torch

import fuzz_cases
from helpers import fuzz_record_for_run, fuzz_seeds, record_rel_l2, rel_l2

pytestmark = pytest.mark.gpu

TOL = 5e-3
N_CASES = fuzz_cases.N_CASES["unet"]


PREC = os.environ.get("DF_FUZZ_PREC", "fp16")          # exploratory: the bf16-operand build (8 x the rounding unit)
PREC_SCALE = 8.0 if PREC == "bf16" else 1.0
TUNE = os.environ.get("DF_FUZZ_TUNE", "0") != "0"
WIDE = os.environ.get("DF_FUZZ_WIDE", "0") != "0"      # exploratory sweeps: wider maps, batches, contexts and widths than the suite draws


@pytest.mark.parametrize("seed", fuzz_seeds(N_CASES))
def test_unet_configuration_product_vs_oracle(seed):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from oracle import unet as ou
    k = fuzz_cases.unet_case(seed, WIDE)
    cfg, o, cond, sd = k["cfg"], k["o"], k["cond"], k["sd"]
    m = P.LatentDiffusion(precision=PREC, **P.stage2_config(cfg, synth.VAE_TINY, cond))
    m.load_state_dict(sd)
    m.cuda()
    if TUNE:                      # exploratory: the in-plan autotuner walks its top candidates per GEMM (tiles the cost model does not pick)
        m.autotune(True)
    usd = ou.sub_state_dict(sd, "model.diffusion_model.")
    B = o["B"]
    x, c, t, uc, tt = k["x"], k["c"], k["t"], k["uc"], k["tt"]
    ref = ou.unet_forward(usd, cfg, x, t, c)
    y = m.apply_model(x.cuda(), t.cuda(), c.cuda()).cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all(), (cfg, o)
    err = rel_l2(y, ref)
    # classifier-free guidance through the fused entry point (one 2B-row plan, combine in the last GEMM's reduce / epilogue)
    e2 = ou.unet_forward(usd, cfg, torch.cat([x, x]), torch.cat([tt, tt]), torch.cat([uc, c]))
    ref_cfg = e2[:B] + fuzz_cases.UNET_CFG_SCALE * (e2[B:] - e2[:B])
    m.engine.set_context(torch.cat([uc, c]).cuda())
    y_cfg = m.engine.unet_forward_cfg(x.cuda(), tt.float().cuda(), fuzz_cases.UNET_CFG_SCALE).cpu()
    err_cfg = rel_l2(y_cfg, ref_cfg)
    print(f"case {seed}: {cfg} {o} -> rel-L2 {err:.2e}, CFG {err_cfg:.2e}")
    assert err < TOL * PREC_SCALE, (cfg, o, err)
    assert err_cfg < 3 * TOL * PREC_SCALE, (cfg, o, err_cfg)          # guidance amplifies the (e_c - e_u) rounding by the scale
    # ... and against the reference's own result on this case, by the same metric and bounds
    rec = fuzz_record_for_run("unet", seed, dict(cfg=cfg, o=o), WIDE)
    if rec is not None:
        err_r, err_cfg_r = record_rel_l2(rec["y"], y), record_rel_l2(rec["y_cfg"], y_cfg)
        print(f"case {seed}: against the reference's record -> rel-L2 {err_r:.2e}, CFG {err_cfg_r:.2e}")
        assert err_r < TOL * PREC_SCALE, (cfg, o, err_r)
        assert err_cfg_r < 3 * TOL * PREC_SCALE, (cfg, o, err_cfg_r)


@pytest.mark.parametrize("mc,mult,H,W", [(256, [1, 2, 2, 4], 8, 16), (256, [1, 2, 2, 4], 8, 24), (192, [1, 2], 8, 8)])
def test_transformer_blocks_on_two_and_three_token_maps_of_other_widths(mc, mult, H, W):
    """Attention at the deepest level of a small latent: 1 x 2, 1 x 3 and 4 x 4 token maps with 1024- / 384-wide rows take the stand-alone
    LayerNorm kernel, which knew the Stage-2 row lengths only (found by the DF_FUZZ_WIDE sweep of the test above, round 6)."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from oracle import unet as ou
    att = [2 ** (len(mult) - 1)]
    cfg = dict(in_channels=4, out_channels=4, model_channels=mc, attention_resolutions=att, num_res_blocks=1, channel_mult=mult,
               num_heads=8 if mc == 256 else 6, context_dim=64)
    cond = dict(origin_dim=64, embed_dim=64, seq_len=40)
    sd = synth.make_state_dict(synth.state_dict_spec(cfg, synth.VAE_TINY, cond), 77)
    m = P.LatentDiffusion(precision="fp16", **P.stage2_config(cfg, synth.VAE_TINY, cond))
    m.load_state_dict(sd)
    m.cuda()
    g = torch.Generator().manual_seed(78)
    x, c, t = torch.randn(2, 4, H, W, generator=g), torch.randn(2, 9, 64, generator=g), torch.tensor([900, 17])
    ref = ou.unet_forward(ou.sub_state_dict(sd, "model.diffusion_model."), cfg, x, t, c)
    y = m.apply_model(x.cuda(), t.cuda(), c.cuda()).cpu()
    err = rel_l2(y, ref)
    print(f"mc {mc} mult {mult} on {H} x {W}: rel-L2 {err:.2e}")
    assert torch.isfinite(y).all() and err < TOL, err


@pytest.mark.parametrize("mc,mult,heads", [(192, [1, 2], 4), (192, [1, 1], 12), (64, [1, 3, 7], 8), (192, [1, 3], 8)])
def test_other_head_dims(mc, mult, heads):
    """Head dims beside 32 / 40 / 64 / 80 / 128 / 160: 192 channels over 4 heads (48 and 96), over 12 (16), 64 x 1 / 3 / 7 over 8 heads
    (8 is refused; 24 and 56), 192 x 1 / 3 over 8 (24 and 72) -- drawn by the DF_FUZZ_WIDE sweeps since the attention kernel is
    instantiated for them (round 6, closing session)."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from oracle import unet as ou
    att = [2 ** i for i in range(len(mult)) if mc * mult[i] // heads >= 16]
    cfg = dict(in_channels=4, out_channels=4, model_channels=mc, attention_resolutions=att, num_res_blocks=1, channel_mult=mult,
               num_heads=heads, context_dim=64)
    cond = dict(origin_dim=64, embed_dim=64, seq_len=40)
    sd = synth.make_state_dict(synth.state_dict_spec(cfg, synth.VAE_TINY, cond), 81)
    m = P.LatentDiffusion(precision="fp16", **P.stage2_config(cfg, synth.VAE_TINY, cond))
    m.load_state_dict(sd)
    m.cuda()
    g = torch.Generator().manual_seed(82)
    x, c, t = torch.randn(2, 4, 16, 32, generator=g), torch.randn(2, 17, 64, generator=g), torch.tensor([700, 3])
    ref = ou.unet_forward(ou.sub_state_dict(sd, "model.diffusion_model."), cfg, x, t, c)
    y = m.apply_model(x.cuda(), t.cuda(), c.cuda()).cpu()
    err = rel_l2(y, ref)
    print(f"mc {mc} mult {mult} heads {heads} (head dims {sorted({mc * k // heads for k in mult})}): rel-L2 {err:.2e}")
    assert torch.isfinite(y).all() and err < TOL, err


@pytest.mark.parametrize("W", [24, 32, 128])
def test_full_model_on_other_latent_widths(W):
    """``size_len`` other than 64 at FULL size (3 s / 4 s / 16 s of audio): the shipped plan table holds the 16 x 64 shapes, so every GEMM
    takes the entry of its nearest row count (or the cost model's tile) and every halo conv a patch geometry of another map -- one
    forward, the cond half of the CFG plan and the VAE decode against the oracle's fp32 results on the same inputs."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from helpers import full_state_dict
    from oracle import unet as ou, vae as ov
    sd = full_state_dict()
    m = P.LatentDiffusion(**P.stage2_config())          # the facade's default operand type (fp16)
    m.load_state_dict(sd)
    m.cuda()
    usd = ou.sub_state_dict(sd, "model.diffusion_model.")
    vsd = ou.sub_state_dict(sd, "first_stage_model.")
    g = torch.Generator().manual_seed(W)
    x, c, t = torch.randn(1, 4, 16, W, generator=g), torch.randn(1, 32, 768, generator=g) * 0.05, torch.tensor([481])
    ref = ou.unet_forward(usd, synth.UNET_FULL, x, t, c)
    y = m.apply_model(x.cuda(), t.cuda(), c.cuda()).cpu()
    m.engine.set_context(torch.cat([torch.zeros_like(c), c]).cuda())
    ycfg = m.engine.unet_forward_cfg(x.cuda(), t.float().cuda(), 1.0).cpu()           # scale 1 = the cond half of the 2-row plan
    z = torch.randn(1, 4, 16, W, generator=g)
    d = m.decode_first_stage(z.cuda()).cpu()
    dref = ov.decode_first_stage(vsd, synth.VAE_FULL, z)
    errs = rel_l2(y, ref), rel_l2(ycfg, ref), rel_l2(d, dref)
    print(f"full model, 16 x {W} latent: unet {errs[0]:.2e}, CFG plan {errs[1]:.2e}, vae {errs[2]:.2e}")
    assert errs[0] < 3e-3 and errs[1] < 3e-3 and errs[2] < 3e-3, (W, errs)           # the 16 x 64 goldens' bounds on this build
