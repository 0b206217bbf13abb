"""Randomised differential test of the sampler front end: seeded draws over the OPTIONS the reference API admits -- sampler (DDIM /
PLMS / DPM-Solver++ / the ancestral ``sample()``), step count, batch, latent width (``size_len``), context length, guidance scale with a
zero / random / absent unconditional conditioning, eta with temperature and noise_dropout, log_every_t, mask / x0 inpainting -- each run
through the product (``LatentDiffusion`` facade -> libdfengine_f16.so) AND through the CPU oracle's restatement of the reference's loop
(oracle/samplers.py: ddim.py:179-273, plms.py:113-236, dpm_solver.py:1071-1105, ddpm.py:1201-1250) with the oracle's fp32 UNet and
cond stage, on the same x_T, features and noise.  The goldens pin a handful of option combinations; this walks the product of them.

Tolerance: rel-L2 of the final latent < 1e-2 on the fp16-operand build of the tiny configuration (measured 3e-5 .. 2e-3 over the 20
cases; a wrong coefficient, table index, noise order or blend is an O(0.1 .. 1) difference)."""
import os

import pytest
import torch

import fuzz_cases
from helpers import fuzz_record_for_run, fuzz_seeds, record_rel_l2, rel_l2, tiny_state_dict

pytestmark = pytest.mark.gpu

TOL = 1e-2
N_CASES = fuzz_cases.N_CASES["samplers"]
WIDE = os.environ.get("DF_FUZZ_WIDE", "0") != "0"


@pytest.fixture(scope="module")
def tiny16():
    import diff_foley_amd as P
    from diff_foley_amd import synth
    m = P.LatentDiffusion(precision="fp16", **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    m.load_state_dict(tiny_state_dict())
    m.cuda()
    return m


@pytest.fixture(scope="module")
def oracle_tiny():
    from diff_foley_amd import synth
    from oracle import unet as ou, vae as ov, schedule as osch
    sd = tiny_state_dict()
    usd = ou.sub_state_dict(sd, "model.diffusion_model.")
    csd = ou.sub_state_dict(sd, "cond_stage_model.")
    sched = osch.ddpm_schedule()
    apply_model = lambda x, t, c: ou.unet_forward(usd, synth.UNET_TINY, x, t, c)
    cond = lambda feats: ov.cond_stage(csd, feats)
    return apply_model, cond, sched


@pytest.mark.parametrize("seed", fuzz_seeds(N_CASES))
def test_sampler_options_product_vs_oracle(tiny16, oracle_tiny, seed):
    from oracle import samplers as osamp
    apply_model, cond_fn, sched = oracle_tiny
    acp = sched["alphas_cumprod"]
    k = fuzz_cases.sampler_case(seed, WIDE)
    o = k["o"]
    rec = fuzz_record_for_run("samplers", seed, o, WIDE)          # the reference's own run of this case
    B, W, S, name = o["B"], o["W"], o["S"], o["name"]
    feats, xT, uc_ref, x0, mask = k["feats"], k["xT"], k["uc"], k["x0"], k["mask"]
    c_ref = cond_fn(feats)
    c = tiny16.get_learned_conditioning(feats.cuda())
    assert rel_l2(c.cpu(), c_ref) < 5e-3
    uc = None if uc_ref is None else uc_ref.cuda()
    gq = torch.Generator()
    qn = lambda shape: torch.randn(tuple(shape), generator=gq)
    noise = lambda s: torch.randn(tuple(s))                  # the global CPU generator, like the reference (and F.dropout's mask)

    def seed_all():
        gq.manual_seed(k["q_seed"])
        torch.manual_seed(k["noise_seed"])

    # ---- a step count whose uniform grid runs past the schedule (S = 9: 999 + 1; util.py:48-57) fails in the reference with an
    # IndexError when the tables are gathered; the product fails the same way, before any launch
    if fuzz_cases.sampler_grid_overruns(o):
        with pytest.raises(IndexError):
            osamp.ddim_sample(apply_model, acp, S, xT, c_ref) if name == "DDIM" else osamp.plms_sample(apply_model, acp, S, xT, c_ref)
        with pytest.raises(IndexError) as ei:
            tiny16.sample_log_diff_sampler(c, B, name, S, size_len=W, x_T=xT.clone())
        if rec is not None:
            assert rec.get("raises") == type(ei.value).__name__, (rec.get("raises"), ei.value)
        return
    assert rec is None or "raises" not in rec, rec.get("raises")
    # ---- oracle
    seed_all()
    if name == "DDIM":
        z_ref, inter_ref = osamp.ddim_sample(apply_model, acp, S, xT, c_ref, o["scale"], uc_ref, eta=o["eta"],
                                             log_every_t=o["log_every_t"], noise_fn=noise, mask=mask, x0=x0, q_noise_fn=qn,
                                             temperature=o["temperature"], noise_dropout=o["noise_dropout"])
    elif name == "PLMS":
        z_ref, inter_ref = osamp.plms_sample(apply_model, acp, S, xT, c_ref, o["scale"], uc_ref, log_every_t=o["log_every_t"],
                                             mask=mask, x0=x0, q_noise_fn=qn)
    elif name == "DPM_Solver":
        z_ref, inter_ref = osamp.dpm_solver_sample(apply_model, acp, S, xT, c_ref, o["scale"], uc_ref)
    else:
        z_ref, inter_ref = osamp.ddpm_sample(apply_model, sched, xT, c_ref, timesteps=S, noise_fn=noise,
                                             log_every_t=o["log_every_t"], mask=mask, x0=x0, q_noise_fn=qn)
    # ---- product
    seed_all()
    kw = dict(x_T=xT.clone())
    if o["inpaint"]:
        kw.update(mask=mask, x0=x0, q_noise_fn=qn)
    if name == "DDPM":
        # sample() hands p_sample_loop none of its **kwargs (ddpm.py:1253-1268), so the option is the model's log_every_t attribute
        # (the oracle restates p_sample_loop, which takes it as a parameter)
        keep = tiny16.log_every_t
        tiny16.log_every_t = o["log_every_t"]
        try:
            z, inter = tiny16.sample(c, batch_size=B, return_intermediates=True, timesteps=S, shape=(B, 4, 16, W), noise_fn=noise, **kw)
        finally:
            tiny16.log_every_t = keep
        assert len(inter) == len(inter_ref), o
        if rec is not None:
            assert len(inter) == rec["n_inter"], (o, len(inter), rec["n_inter"])
    else:
        if name == "DDIM":
            kw.update(eta=o["eta"], temperature=o["temperature"], noise_dropout=o["noise_dropout"], noise_fn=noise)
        if name != "DPM_Solver":
            kw.update(log_every_t=o["log_every_t"])
        z, inter = tiny16.sample_log_diff_sampler(c, B, name, S, size_len=W, unconditional_guidance_scale=o["scale"],
                                                  unconditional_conditioning=uc, **kw)
        if name == "DPM_Solver":
            assert inter is None
            assert rec is None or not any(f.startswith("n_") for f in rec), rec.keys()
        else:
            assert len(inter["x_inter"]) == len(inter_ref["x_inter"]) and len(inter["pred_x0"]) == len(inter_ref["pred_x0"]), o
            assert rel_l2(inter["pred_x0"][-1].cpu(), inter_ref["pred_x0"][-1]) < TOL, o
            if rec is not None:
                assert (len(inter["x_inter"]), len(inter["pred_x0"])) == (rec["n_x_inter"], rec["n_pred_x0"]), o
                assert record_rel_l2(rec["pred_x0_last"], inter["pred_x0"][-1]) < TOL, o
    assert z.shape == z_ref.shape and z.dtype == torch.float32 and torch.isfinite(z).all(), o
    err = rel_l2(z.cpu(), z_ref)
    print(f"case {seed}: {o} -> rel-L2 {err:.2e}")
    assert err < TOL, (o, err)
    if rec is not None:
        err_r = record_rel_l2(rec["z"], z)
        print(f"case {seed}: against the reference's record -> rel-L2 {err_r:.2e}")
        assert err_r < TOL, (o, err_r)


def test_sample_ignores_a_log_every_t_argument_like_the_reference(tiny16):
    """LatentDiffusion.sample() of the reference forwards none of its **kwargs to p_sample_loop (ddpm.py:1253-1268): log_every_t (and
    callback / img_callback) given to sample() change nothing, the intermediates follow model.log_every_t.  The reference's own pair
    of runs is on record (n_inter_kwarg_1 == n_inter, equal latents); here sample(log_every_t=1) returns what sample() returns."""
    seed = next(s for s in fuzz_cases.suite_seeds("samplers") if fuzz_cases.sampler_draw(s)["name"] == "DDPM"
                and fuzz_cases.sampler_draw(s)["log_every_t"] != 1)
    k = fuzz_cases.sampler_case(seed)
    o = k["o"]
    rec = fuzz_record_for_run("samplers", seed, o)
    assert rec is not None and rec["n_inter_kwarg_1"] == rec["n_inter"] and rec["kwarg_latents_equal"] is True
    B, W, S = o["B"], o["W"], o["S"]
    c = tiny16.get_learned_conditioning(k["feats"].cuda())
    gq = torch.Generator()
    kw = dict(x_T=k["xT"].clone(), noise_fn=lambda s: torch.randn(tuple(s)))
    if o["inpaint"]:
        kw.update(mask=k["mask"], x0=k["x0"], q_noise_fn=lambda shape: torch.randn(tuple(shape), generator=gq))
    calls = []
    out = []
    for extra in (dict(), dict(log_every_t=1, callback=calls.append, img_callback=lambda img, i: calls.append(i))):
        gq.manual_seed(k["q_seed"])
        torch.manual_seed(k["noise_seed"])
        out.append(tiny16.sample(c, batch_size=B, return_intermediates=True, timesteps=S, shape=(B, 4, 16, W), **kw, **extra))
    (z0, inter0), (z1, inter1) = out
    assert torch.equal(z0, z1) and len(inter0) == len(inter1) and not calls
    # the count is model.log_every_t's: x_T, the first step's image (i == S - 1) and those of the steps it divides
    assert len(inter0) == 1 + len([i for i in range(S) if i % tiny16.log_every_t == 0 or i == S - 1])
    assert record_rel_l2(rec["z"], z0) < TOL


@pytest.mark.parametrize("seed", fuzz_seeds(fuzz_cases.N_CASES["double_guidance"]))
def test_double_guidance_options_product_vs_oracle(tiny16, oracle_tiny, seed):
    """The classifier-guided samplers (ddim.py:276-396, dpm_solver/sampler.py:90-156 -> dpm_solver.py:1377-1393) over their options:
    sampler, steps, batch, latent width, CFG scale, classifier scale (0 = the gradient is formed and multiplied away), video frames
    33 (the notebook's) / 32 / 8, eta for DDIM.  Oracle: the same loops with autograd through the oracle's classifier."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from helpers import tiny_classifier_sd
    from oracle import unet as ou, samplers as osamp
    apply_model, cond_fn, sched = oracle_tiny
    k = fuzz_cases.double_guidance_case(seed, WIDE)
    o = k["o"]
    name, B, W, S, scale, cscale, F, eta = (o[f] for f in ("name", "B", "W", "S", "scale", "cscale", "F", "eta"))
    cls = P.AlignmentClassifier(classifier_config=dict(params=dict(synth.CLS_TINY)))
    cls.load_state_dict(tiny_classifier_sd())
    cls.attach(tiny16)
    ksd = ou.sub_state_dict(tiny_classifier_sd(), "model.")
    classifier = lambda x, t, c: ou.classifier_forward(ksd, synth.CLS_TINY, x, t, c)
    vf, xT = k["vf"], k["xT"]
    c_ref = cond_fn(vf[:, :32])
    c = tiny16.get_learned_conditioning(vf[:, :32].cuda())
    noise = lambda s: torch.randn(tuple(s))
    torch.manual_seed(k["noise_seed"])
    if name == "DDIM":
        z_ref, _ = osamp.ddim_sample(apply_model, sched["alphas_cumprod"], S, xT, c_ref, scale, torch.zeros_like(c_ref), eta=eta,
                                     classifier=classifier, origin_cond=vf, classifier_scale=cscale, noise_fn=noise)
    else:
        z_ref, _ = osamp.dpm_solver_sample(apply_model, sched["alphas_cumprod"], S, xT, c_ref, scale, torch.zeros_like(c_ref),
                                           classifier=classifier, origin_cond=vf, classifier_scale=cscale)
    torch.manual_seed(k["noise_seed"])
    kw = dict(eta=eta, noise_fn=noise) if name == "DDIM" else {}
    z, _ = tiny16.sample_log_with_classifier_diff_sampler(
        c, origin_cond=vf.cuda(), batch_size=B, sampler_name=name, ddim_steps=S, size_len=W, unconditional_guidance_scale=scale,
        unconditional_conditioning=torch.zeros_like(c), classifier=cls, classifier_guide_scale=cscale, x_T=xT.clone(), **kw)
    err = rel_l2(z.cpu(), z_ref)
    print(f"double guidance case {seed}: {name}-{S} B={B} W={W} scale={scale} classifier scale={cscale} frames={F} eta={eta} -> rel-L2 {err:.2e}")
    assert z.shape == z_ref.shape and err < TOL, (name, S, B, W, scale, cscale, F, eta, err)
    rec = fuzz_record_for_run("double_guidance", seed, o, WIDE)          # ... and against the reference's own run of this case
    if rec is not None:
        err_r = record_rel_l2(rec["z"], z)
        print(f"double guidance case {seed}: against the reference's record -> rel-L2 {err_r:.2e}")
        assert err_r < TOL, (o, err_r)
