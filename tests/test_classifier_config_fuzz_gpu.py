"""Randomised differential test of the hand-written classifier backward pass (csrc/backward.hip, engine_cls_grad.hip:build_classifier_grad)
over classifier CONFIGURATIONS: seeded draws of the Classifier_Backbone's constructor arguments (alignment_backbone.py:420-640:
model_channels, channel_mult, num_res_blocks, attention_resolutions, num_heads, context_dim), procedurally generated weights, and
``d sum(log p) / d x`` (cal_classifier_loglikelihood_grad, ddim.py:333-341) from ``df_classifier_grad`` against torch autograd through
the oracle's fp32 forward (oracle/unet.py:classifier_forward) at a random latent size, batch and number of video frames.  The golden
G6 pins the tiny and the full configuration; the tape builder has a branch per block kind and per channel change, which this walks.

Tolerance (fp16-operand build): probability within 5e-3, gradient rel-L2 < 1.5e-2 (the full-size configuration measures 3.7e-3)."""
import os

import pytest
import torch

import fuzz_cases
from helpers import fuzz_record_for_run, fuzz_seeds, record_rel_l2, rel_l2, tiny_state_dict

pytestmark = pytest.mark.gpu

N_CASES = fuzz_cases.N_CASES["classifier"]
REGRESSION_SEEDS = fuzz_cases.REGRESSION_SEEDS["classifier"]


PREC = os.environ.get("DF_FUZZ_PREC", "fp16")          # exploratory: the bf16-operand build (8 x the rounding unit), in-plan autotuner
PREC_SCALE = 8.0 if PREC == "bf16" else 1.0
TUNE = os.environ.get("DF_FUZZ_TUNE", "0") != "0"
WIDE = os.environ.get("DF_FUZZ_WIDE", "0") != "0"      # exploratory sweeps: wider maps, batches and widths than the suite draws


@pytest.mark.parametrize("seed", sorted(set(fuzz_seeds(N_CASES)) | set(REGRESSION_SEEDS)))
def test_classifier_gradient_product_vs_autograd(seed):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from oracle import unet as ou, samplers as osamp
    k = fuzz_cases.classifier_case(seed, WIDE)
    cfg, o, sd = k["cfg"], k["o"], k["sd"]
    host = P.LatentDiffusion(precision=PREC, **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    host.load_state_dict(tiny_state_dict())
    host.cuda()
    if TUNE:
        host.autotune(True)
    cls = P.AlignmentClassifier(classifier_config=dict(params=dict(cfg)))
    cls.load_state_dict(sd)
    cls.attach(host)
    csd = ou.sub_state_dict(sd, "model.")
    x, vf, t = k["x"], k["vf"], k["t"]
    p_ref = ou.classifier_forward(csd, cfg, x, t, vf).detach()
    g_ref = osamp.classifier_grad(lambda xx, tt, cc: ou.classifier_forward(csd, cfg, xx, tt, cc), x, t, vf)
    p = cls(x.cuda(), t=t.cuda(), video_feat=vf.cuda()).cpu()
    grad, prob = host.engine.classifier_grad(x.cuda(), t.cuda(), vf.cuda(), want_prob=True)
    assert grad.shape == x.shape and torch.isfinite(grad).all(), (cfg, o)
    err = rel_l2(grad.cpu(), g_ref)
    per = _per_sample(grad.cpu(), g_ref)
    print(f"case {seed}: {cfg} {o} -> p {p.flatten().tolist()} (ref {p_ref.flatten().tolist()}), grad rel-L2 {err:.2e}, "
          f"per sample {[f'{e:.1e}' for e in per]}")
    assert torch.allclose(p, p_ref, atol=5e-3 * PREC_SCALE) and torch.allclose(prob.cpu(), p_ref, atol=5e-3 * PREC_SCALE), (cfg, o)
    assert err < 1.5e-2 * PREC_SCALE, (cfg, o, err)
    assert max(per) < 1.5e-2 * PREC_SCALE, (cfg, o, per)
    # ... and against the reference's own probability and gradient on this case, by the same metrics and bounds
    rec = fuzz_record_for_run("classifier", seed, dict(cfg=cfg, o=o), WIDE)
    if rec is not None:
        p_rec, g_rec = torch.from_numpy(rec["p"]["full"]), torch.from_numpy(rec["grad"]["full"])
        err_r, per_r = record_rel_l2(rec["grad"], grad), _per_sample(grad.cpu(), g_rec)
        print(f"case {seed}: against the reference's record -> grad rel-L2 {err_r:.2e}, per sample {[f'{e:.1e}' for e in per_r]}")
        assert torch.allclose(p, p_rec, atol=5e-3 * PREC_SCALE) and torch.allclose(prob.cpu(), p_rec, atol=5e-3 * PREC_SCALE), (cfg, o)
        assert err_r < 1.5e-2 * PREC_SCALE, (cfg, o, err_r)
        assert max(per_r) < 1.5e-2 * PREC_SCALE, (cfg, o, per_r)


@pytest.mark.parametrize("name,S", [("DDIM", 4), ("DPM_Solver", 4)])
def test_double_guidance_on_a_wide_latent(name, S):
    """``size_len`` = 128 (a 16 s latent, ddpm.py:1327-1356 takes any length): the classifier's first attention level then works on
    8 x 64 = 512 tokens, more than the LDS-resident backward kernels hold -- the tiled pair (csrc/backward.hip) runs inside the
    sampler.  Product (facade) against the oracle's double-guidance loop (ddim.py:344-396 / dpm_solver.py:1377-1393) with autograd
    through the oracle's classifier."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from helpers import tiny_classifier_sd
    from oracle import unet as ou, vae as ov, samplers as osamp, schedule as osch
    sd = tiny_state_dict()
    host = P.LatentDiffusion(precision="fp16", **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    host.load_state_dict(sd)
    host.cuda()
    cls = P.AlignmentClassifier(classifier_config=dict(params=dict(synth.CLS_TINY)))
    cls.load_state_dict(tiny_classifier_sd())
    cls.attach(host)
    usd = ou.sub_state_dict(sd, "model.diffusion_model.")
    csd = ou.sub_state_dict(sd, "cond_stage_model.")
    ksd = ou.sub_state_dict(tiny_classifier_sd(), "model.")
    B, W = 1, 128
    g = torch.Generator().manual_seed(31)
    xT = torch.randn(B, 4, 16, W, generator=g)
    vf = synth.synthetic_cavp(B, 33, 64, seed=4321)
    c_ref = ov.cond_stage(csd, vf[:, :32])
    uc_ref = torch.zeros_like(c_ref)
    apply_model = lambda x, t, c: ou.unet_forward(usd, synth.UNET_TINY, x, t, c)
    classifier = lambda x, t, c: ou.classifier_forward(ksd, synth.CLS_TINY, x, t, c)
    fn = osamp.ddim_sample if name == "DDIM" else osamp.dpm_solver_sample
    z_ref, _ = fn(apply_model, osch.ddpm_schedule()["alphas_cumprod"], S, xT, c_ref, 4.5, uc_ref, classifier=classifier,
                  origin_cond=vf, classifier_scale=50.0)
    c = host.get_learned_conditioning(vf[:, :32].cuda())
    z, _ = host.sample_log_with_classifier_diff_sampler(
        c, origin_cond=vf.cuda(), batch_size=B, sampler_name=name, ddim_steps=S, size_len=W, unconditional_guidance_scale=4.5,
        unconditional_conditioning=torch.zeros_like(c), classifier=cls, classifier_guide_scale=50.0, x_T=xT.clone())
    err = rel_l2(z.cpu(), z_ref)
    print(f"double guidance on a 16 x {W} latent, {name}-{S}: rel-L2 {err:.2e}")
    assert z.shape == (B, 4, 16, W) and err < 1e-2


@pytest.mark.parametrize("W", [32, 64, 128, 192])
def test_full_classifier_gradient_on_other_latent_widths(W):
    """The FULL alignment classifier (Classifier_Backbone as configured in the reference's double-guidance YAML) on 16 x W latents:
    W = 128 / 192 put 512 / 768 tokens into its first attention level -- the tiled backward pair -- W = 32 / 64 stay on the
    LDS-resident MFMA kernel.  Gradient and probability against autograd through the oracle."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from helpers import full_classifier_sd
    from oracle import unet as ou, samplers as osamp
    host = P.LatentDiffusion(precision="fp16", **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    host.load_state_dict(tiny_state_dict())
    host.cuda()
    sd = full_classifier_sd()
    cls = P.AlignmentClassifier(classifier_config=dict(params=dict(synth.CLS_FULL)))
    cls.load_state_dict(sd)
    cls.attach(host)
    ksd = ou.sub_state_dict(sd, "model.")
    g = torch.Generator().manual_seed(W)
    B = 2
    x = torch.randn(B, 4, 16, W, generator=g)
    vf = synth.synthetic_cavp(B, 33, 512, seed=W)
    t = torch.tensor([640.0, 12.0])
    p_ref = ou.classifier_forward(ksd, synth.CLS_FULL, x, t, vf).detach()
    g_ref = osamp.classifier_grad(lambda xx, tt, cc: ou.classifier_forward(ksd, synth.CLS_FULL, xx, tt, cc), x, t, vf)
    grad, prob = host.engine.classifier_grad(x.cuda(), t.cuda(), vf.cuda(), want_prob=True)
    err = rel_l2(grad.cpu(), g_ref)
    per = _per_sample(grad.cpu(), g_ref)
    print(f"full classifier, 16 x {W} latent: p {prob.flatten().tolist()} (ref {p_ref.flatten().tolist()}), grad rel-L2 {err:.2e}, "
          f"per sample {[f'{e:.1e}' for e in per]}")
    assert torch.allclose(prob.cpu(), p_ref, atol=5e-3) and err < 1e-2, (W, err)
    assert max(per) < 1e-2, (W, per)


def _per_sample(grad, ref):
    """rel-L2 of every sample on its own: the gradient of sample n is (1 - p_n) dz_n / dx, so a sample the classifier is confident
    about is orders of magnitude smaller than the others and invisible in a batch-wide norm."""
    return [rel_l2(grad[i], ref[i]) for i in range(ref.shape[0])]


def _confident_batch(sd, cfg, seed):
    """A batch of three samples whose probabilities are 0.5, ~0.99 and 1 - 1e-4: of 16 candidate samples the two with the lowest and
    the highest head logit w . pooled, and the one nearest logit(0.99) in between; the head Linear is rescaled and its bias moved so
    that z = alpha w . pooled + b puts the first at p = 0.5 and the last at p = 1 - 1e-4 exactly."""
    from diff_foley_amd import synth
    from oracle import unet as ou
    g = torch.Generator().manual_seed(seed)
    n = 16
    x = torch.randn(n, 4, 16, 64, generator=g)
    vf = synth.synthetic_cavp(n, 33, cfg["context_dim"], seed=seed + 1)
    t = torch.randint(0, 1000, (n,), generator=g).float()
    sd = dict(sd)
    sd["model.classifier.bias"] = torch.zeros_like(sd["model.classifier.bias"])
    p0 = ou.classifier_forward(ou.sub_state_dict(sd, "model."), cfg, x, t, vf).detach().double().flatten()
    s0 = torch.log(p0) - torch.log1p(-p0)
    lo, hi = int(s0.argmin()), int(s0.argmax())
    L_hi = float(torch.logit(torch.tensor(1 - 1e-4, dtype=torch.float64)))
    alpha = L_hi / float(s0[hi] - s0[lo])
    b = -alpha * float(s0[lo])
    mid = int((alpha * s0 + b - float(torch.logit(torch.tensor(0.99, dtype=torch.float64)))).abs().argmin())
    sd["model.classifier.weight"] = (sd["model.classifier.weight"].double() * alpha).float()
    sd["model.classifier.bias"] = torch.full_like(sd["model.classifier.bias"], b)
    idx = [lo, mid, hi]
    return sd, x[idx], t[idx], vf[idx]


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_classifier_gradient_per_sample_when_confident(which, prec):
    """One batch holding samples at p = 0.5, ~0.99 and 1 - 1e-4: the confident samples' gradients are (1 - p) times smaller than the
    first one's, and each must still match autograd through the oracle on its own.  The gradient plan's operand-type stores must not
    saturate on the way (df_debug_saturations)."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from helpers import full_classifier_sd, tiny_classifier_sd
    from oracle import unet as ou, samplers as osamp
    cfg = synth.CLS_TINY if which == "tiny" else synth.CLS_FULL
    sd, x, t, vf = _confident_batch(tiny_classifier_sd() if which == "tiny" else full_classifier_sd(), cfg, 77)
    host = P.LatentDiffusion(precision=prec, **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    host.load_state_dict(tiny_state_dict())
    host.cuda()
    cls = P.AlignmentClassifier(classifier_config=dict(params=dict(cfg)))
    cls.load_state_dict(sd)
    cls.attach(host)
    ksd = ou.sub_state_dict(sd, "model.")
    p_ref = ou.classifier_forward(ksd, cfg, x, t, vf).detach()
    g_ref = osamp.classifier_grad(lambda xx, tt, cc: ou.classifier_forward(ksd, cfg, xx, tt, cc), x, t, vf)
    eng = host.engine
    eng.debug_saturations(True)
    try:
        grad, prob = eng.classifier_grad(x.cuda(), t.cuda(), vf.cuda(), want_prob=True)
        torch.cuda.synchronize()
        sats = eng.debug_saturations_read()
    finally:
        eng.debug_saturations(False)
    # the gradient is (1 - p_n) dz_n / dx: compared as dz / dx, so that the forward's probability error, which the head's rescaling
    # multiplies by alpha and which the atol above judges, is not counted a second time through 1 - p (8 % at p = 0.99 on bf16)
    per = _per_sample(grad.cpu() / (1 - prob.cpu().double()).reshape(-1, 1, 1, 1), g_ref / (1 - p_ref.double()).reshape(-1, 1, 1, 1))
    print(f"{which} classifier [{prec}], p {prob.flatten().tolist()} (ref {p_ref.flatten().tolist()}): per-sample dz/dx rel-L2 "
          f"{[f'{e:.2e}' for e in per]}, gradient norms {[f'{float(g_ref[i].norm()):.2e}' for i in range(3)]}")
    assert abs(float(p_ref[0]) - 0.5) < 1e-3 and float(p_ref[2]) > 1 - 2e-4
    assert torch.allclose(prob.cpu(), p_ref, atol=5e-3 * (8 if prec == "bf16" else 1))
    assert sats and all(n == 0 for _, n in sats), [s_ for s_ in sats if s_[1]][:5]
    assert max(per) < 1e-2 * (8 if prec == "bf16" else 1), per


@pytest.mark.parametrize("which,H,W", [("full", 16, 68), ("tiny", 16, 68), ("full", 10, 64), ("full", 16, 66), ("tiny", 6, 32)])
def test_classifier_maps_the_downsampling_does_not_divide(which, H, W):
    """The engine sizes a Downsample output as floor(H / 2) where torch's stride-2 conv gives the ceiling: a latent whose sides are
    not multiples of 2^(levels - 1) (4 for both configurations) is refused by the forward and the gradient entry, like the UNet's;
    16 x 68 (68 = 4 x 17: 68 -> 34 -> 17) divides and matches the oracle."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from helpers import full_classifier_sd, tiny_classifier_sd
    from oracle import unet as ou, samplers as osamp
    cfg = synth.CLS_TINY if which == "tiny" else synth.CLS_FULL
    sd = tiny_classifier_sd() if which == "tiny" else full_classifier_sd()
    host = P.LatentDiffusion(precision="fp16", **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    host.load_state_dict(tiny_state_dict())
    host.cuda()
    cls = P.AlignmentClassifier(classifier_config=dict(params=dict(cfg)))
    cls.load_state_dict(sd)
    cls.attach(host)
    g = torch.Generator().manual_seed(H * 1000 + W)
    B = 2
    x = torch.randn(B, 4, H, W, generator=g)
    vf = synth.synthetic_cavp(B, 8, cfg["context_dim"], seed=W)
    t = torch.tensor([100.0, 700.0])
    q = 2 ** (len(cfg["channel_mult"]) - 1)
    if H % q or W % q:
        with pytest.raises(RuntimeError, match="not divisible"):
            cls(x.cuda(), t=t.cuda(), video_feat=vf.cuda())
        with pytest.raises(RuntimeError, match="not divisible"):
            host.engine.classifier_grad(x.cuda(), t.cuda(), vf.cuda(), want_prob=True)
        return
    ksd = ou.sub_state_dict(sd, "model.")
    p_ref = ou.classifier_forward(ksd, cfg, x, t, vf).detach()
    g_ref = osamp.classifier_grad(lambda xx, tt, cc: ou.classifier_forward(ksd, cfg, xx, tt, cc), x, t, vf)
    p = cls(x.cuda(), t=t.cuda(), video_feat=vf.cuda()).cpu()
    grad, prob = host.engine.classifier_grad(x.cuda(), t.cuda(), vf.cuda(), want_prob=True)
    per = _per_sample(grad.cpu(), g_ref)
    print(f"{which} classifier on {H} x {W}: p {prob.flatten().tolist()} (ref {p_ref.flatten().tolist()}), per-sample grad rel-L2 {per}")
    assert torch.allclose(p, p_ref, atol=5e-3) and torch.allclose(prob.cpu(), p_ref, atol=5e-3)
    assert max(per) < 1e-2, per
