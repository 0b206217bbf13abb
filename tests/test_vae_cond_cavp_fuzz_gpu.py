"""Randomised differential tests of the three modules either side of the UNet, over the configurations and shapes the reference's
constructors and call sites admit, each through the facade (fp16-operand library) against the CPU oracle on the same seeded inputs:

  * ``decode_first_stage`` (ddpm.py:739-797 -> stage1_autoencoder/model.py:557-663): decoder ddconfig draws (ch, ch_mult,
    num_res_blocks, out_ch), latent sizes from 4 x 8 to 16 x 64, batches 1 .. 5 -- oracle/vae.py;
  * ``get_learned_conditioning`` (ddpm.py:568-579 -> video_feat_encoder.py:12-18): origin_dim / embed_dim / seq_len draws and
    sequence lengths up to seq_len -- oracle/vae.py:cond_stage;
  * ``CAVP_Inference.encode_video`` (cavp_model.py:47-65): stage_blocks draws of the SlowOnly backbone, clips of 1 .. 9 frames,
    frame sizes 64 .. 160 (multiples of 32), 1 .. 3 clips -- oracle/cavp.py.
The goldens pin one tiny and the full configuration of each; the plan builders have loops over levels / blocks / stages that only
other configurations walk."""
import os

import numpy as np
import pytest
import torch

import fuzz_cases
from helpers import fuzz_record_for_run, fuzz_seeds, record_rel_l2, rel_l2

pytestmark = pytest.mark.gpu


PREC = os.environ.get("DF_FUZZ_PREC", "fp16")          # exploratory: the bf16-operand build (8 x the rounding unit), in-plan autotuner
PREC_SCALE = 8.0 if PREC == "bf16" else 1.0
TUNE = os.environ.get("DF_FUZZ_TUNE", "0") != "0"
WIDE = os.environ.get("DF_FUZZ_WIDE", "0") != "0"      # exploratory sweeps: wider spaces than the suite draws


@pytest.mark.parametrize("seed", fuzz_seeds(fuzz_cases.N_CASES["vae"]))
def test_vae_decoder_configuration_product_vs_oracle(seed):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from oracle import unet as ou, vae as ov
    k = fuzz_cases.vae_case(seed, WIDE)
    cfg, o, sd, z = k["cfg"], k["o"], k["sd"], k["z"]
    m = P.LatentDiffusion(precision=PREC, **P.stage2_config(synth.UNET_TINY, cfg, synth.COND_TINY))
    m.load_state_dict(sd)
    m.cuda()
    if TUNE:
        m.autotune(True)
    vsd = ou.sub_state_dict(sd, "first_stage_model.")
    ref = ov.decode_first_stage(vsd, cfg, z)
    y = m.decode_first_stage(z.cuda()).cpu()
    up = 2 ** (len(cfg["ch_mult"]) - 1)
    assert y.shape == ref.shape == (o["B"], cfg["out_ch"], o["H"] * up, o["W"] * up) and torch.isfinite(y).all(), (cfg, o)
    err = rel_l2(y, ref)
    print(f"vae case {seed}: {cfg} {o} -> rel-L2 {err:.2e}")
    assert err < 3e-3 * PREC_SCALE, (cfg, o, err)              # the full decoder measures 9.2e-4 on this build
    rec = fuzz_record_for_run("vae", seed, dict(cfg=cfg, o=o), WIDE)          # ... and against the reference's own result on this case
    if rec is not None:
        err_r = record_rel_l2(rec["y"], y)
        print(f"vae case {seed}: against the reference's record -> rel-L2 {err_r:.2e}")
        assert err_r < 3e-3 * PREC_SCALE, (cfg, o, err_r)


@pytest.mark.parametrize("seed", fuzz_seeds(fuzz_cases.N_CASES["cond"]))
def test_cond_stage_configuration_product_vs_oracle(seed):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from oracle import unet as ou, vae as ov
    k = fuzz_cases.cond_case(seed, WIDE)
    cond, ucfg, sd = k["cond"], k["ucfg"], k["sd"]
    rec = fuzz_record_for_run("cond", seed, dict(cond=cond, calls=k["calls"]), WIDE)
    m = P.LatentDiffusion(precision="fp16", **P.stage2_config(ucfg, synth.VAE_TINY, cond))
    m.load_state_dict(sd)
    m.cuda()
    csd = ou.sub_state_dict(sd, "cond_stage_model.")
    for i, (call, f) in enumerate(zip(k["calls"], k["feats"])):
        B, T = call["B"], call["T"]
        ref = ov.cond_stage(csd, f)
        c = m.get_learned_conditioning(f.cuda()).cpu()
        assert c.shape == ref.shape == (B, T, cond["embed_dim"])
        err = rel_l2(c, ref)
        print(f"cond case {seed}: {cond} B={B} T={T} -> rel-L2 {err:.2e}")
        assert err < 2e-3, (cond, B, T, err)
        if rec is not None:                       # ... and against the reference's own result on this call
            err_r = record_rel_l2(rec[f"c{i}"], c)
            print(f"cond case {seed}: B={B} T={T} against the reference's record -> rel-L2 {err_r:.2e}")
            assert err_r < 2e-3, (cond, B, T, err_r)
    # longer than the positional table: the reference's embedding lookup fails (IndexError on the CPU, a device-side assert --
    # RuntimeError -- on a GPU); the product's exception is both
    with pytest.raises(RuntimeError) as ei:
        m.get_learned_conditioning(torch.randn(1, cond["seq_len"] + 1, cond["origin_dim"]).cuda())
    if rec is not None:
        assert rec["too_long_raises"] in [b.__name__ for b in type(ei.value).__mro__], (rec["too_long_raises"], type(ei.value).__mro__)


@pytest.mark.parametrize("seed", fuzz_seeds(fuzz_cases.N_CASES["cavp"]))
def test_cavp_configuration_product_vs_oracle(seed):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from oracle import cavp as ocavp
    k = fuzz_cases.cavp_case(seed, WIDE)
    cfg, sd, v = k["cfg"], k["sd"], k["video"]
    n, T, S = k["o"]["n"], k["o"]["T"], k["o"]["S"]
    rec = fuzz_record_for_run("cavp", seed, dict(cfg=cfg, o=k["o"]), WIDE)
    m = P.CAVPInference(embed_dim=cfg["embed_dim"], stage_blocks=cfg["stage_blocks"], precision=PREC)
    missing, unexpected = m.load_state_dict(sd)
    assert not missing and not unexpected
    m.cuda()
    for normalize in (True, False):
        ref = ocavp.encode_video(sd, v, normalize=normalize, stage_blocks=tuple(cfg["stage_blocks"]))
        f = m.encode_video(v.cuda(), normalize=normalize, pool=False).cpu()
        assert f.shape == ref.shape == (n, T, cfg["embed_dim"]) and torch.isfinite(f).all()
        err = rel_l2(f, ref)
        cos = torch.nn.functional.cosine_similarity(f, ref, dim=-1).min().item()
        print(f"cavp case {seed}: {cfg} clips={n} frames={T} size={S} normalize={normalize} -> rel-L2 {err:.2e}, min cos {cos:.6f}")
        assert err < 2e-3 * PREC_SCALE and cos > 1 - 1e-5 * PREC_SCALE ** 2, (cfg, n, T, S, err, cos)
        if rec is not None:                       # ... and against the reference's own features on this case
            stored = rec["feats" if normalize else "feats_raw"]
            f_rec = torch.from_numpy(stored["full"])
            err_r = record_rel_l2(stored, f)
            cos_r = torch.nn.functional.cosine_similarity(f, f_rec, dim=-1).min().item()
            print(f"cavp case {seed}: normalize={normalize} against the reference's record -> rel-L2 {err_r:.2e}, min cos {cos_r:.6f}")
            assert err_r < 2e-3 * PREC_SCALE and cos_r > 1 - 1e-5 * PREC_SCALE ** 2, (cfg, n, T, S, err_r, cos_r)


@pytest.mark.parametrize("H,W", [(2, 8), (4, 8), (4, 24), (8, 20)])
def test_vae_decode_latents_whose_token_count_is_not_a_multiple_of_64(H, W):
    """The decoder's mid attention (model.py:273-297) contracts P V over the H * W tokens; the GEMM kernels walk the contraction in
    whole 64-element steps, so 16 / 32 / 96 / 160 tokens need the padded form (zero probabilities against zeroed V^T columns).
    Found by the draws above: before round 6 the tail (all of it below 64 tokens) was dropped silently -- rel-L2 8e-2 .. 1.2e-1."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from helpers import tiny_state_dict
    from oracle import unet as ou, vae as ov
    sd = tiny_state_dict()
    vsd = ou.sub_state_dict(sd, "first_stage_model.")
    for prec, tol in (("fp16", 3e-3), ("bf16", 2e-2)):
        m = P.LatentDiffusion(precision=prec, **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
        m.load_state_dict(sd)
        m.cuda()
        z = torch.randn(3, 4, H, W, generator=torch.Generator().manual_seed(H * 100 + W))
        ref = ov.decode_first_stage(vsd, synth.VAE_TINY, z)
        y = m.decode_first_stage(z.cuda()).cpu()
        err = rel_l2(y, ref)
        print(f"vae {H}x{W} ({H * W} tokens) [{prec}]: rel-L2 {err:.2e}")
        assert y.shape == ref.shape and err < tol, (H, W, prec, err)


def test_a_contraction_length_the_kernels_cannot_walk_fails_loudly():
    """context_dim = 96 is a legal UNetModel argument; the GEMM kernels' K loop takes whole 64-element steps, so the engine refuses
    the plan (RuntimeError naming the GEMM) instead of dropping the last 32 context channels."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    ucfg = dict(synth.UNET_TINY, context_dim=96)
    cond = dict(origin_dim=64, embed_dim=96, seq_len=40)
    sd = synth.make_state_dict(synth.state_dict_spec(ucfg, synth.VAE_TINY, cond), 3)
    m = P.LatentDiffusion(precision="bf16", **P.stage2_config(ucfg, synth.VAE_TINY, cond))
    m.load_state_dict(sd)
    m.cuda()
    with pytest.raises(RuntimeError, match="multiple of 64"):
        c = m.get_learned_conditioning(torch.randn(1, 8, 64).cuda())
        m.apply_model(torch.randn(1, 4, 16, 64).cuda(), torch.tensor([10]).cuda(), c)


def test_cavp_edge_inputs():
    import diff_foley_amd as P
    from diff_foley_amd import synth
    m = P.CAVPInference(embed_dim=synth.CAVP_TINY["embed_dim"], stage_blocks=synth.CAVP_TINY["stage_blocks"], precision="fp16")
    m.load_state_dict(synth.make_state_dict(synth.cavp_spec(synth.CAVP_TINY)))
    m.cuda()
    E = synth.CAVP_TINY["embed_dim"]
    assert m.encode_video(torch.zeros(0, 4, 3, 64, 64).cuda(), normalize=True, pool=False).shape == (0, 4, E)
    assert m.encode_video(torch.zeros(2, 0, 3, 64, 64).cuda(), normalize=True, pool=False).shape == (2, 0, E)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        m.encode_video(torch.zeros(1, 2, 3, 72, 64).cuda(), normalize=True, pool=False)
    with pytest.raises(RuntimeError, match=r"\(B,T,3,H,W\)"):
        m.encode_video(torch.zeros(2, 3, 64, 64).cuda(), normalize=True, pool=False)
    with pytest.raises(RuntimeError, match=r"\(B,T,3,H,W\)"):
        m.encode_video(torch.zeros(1, 2, 4, 64, 64).cuda(), normalize=True, pool=False)
    ex = P.ExtractCAVPFeatures(fps=4, batch_size=4, video_shape=(64, 64), stage1_model=m)
    f = np.random.default_rng(0).integers(0, 256, (9, 40, 56, 3), dtype=np.uint8)
    a = ex.forward_frames(f)                          # 4 + 4 + 1 frames
    assert a.shape == (9, E)
    b = ex.forward_frames(f[:4])                      # exactly one batch
    assert np.array_equal(a[:4], b)
    with pytest.raises(ValueError):
        ex.forward_frames(f[:0])
