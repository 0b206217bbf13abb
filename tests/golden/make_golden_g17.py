"""G17: what the reference's LatentDiffusion and DDIMSampler do with a latent x0 -- q_sample / stochastic_encode, p_losses and
decode -- on the tiny model of the other goldens (build container only; needs the reference checkout, see oracle/ref_import.py).

    python tests/golden/make_golden_g17.py          # seconds

Writes g17_q_sample.npz, g17_p_losses.npz, g17_decode.npz and g17_signatures.json beside this file.  The models, seeded weights and
helpers are make_golden.py's, imported, not restated.  Inputs that a test can regenerate from a seed (helpers.rnd, synth.synthetic_*)
are not stored; the seeds are the constants below and tests/test_start_from_sound_gpu.py repeats them.

One line of the reference needs help to run at all: p_sample_ddim reads ``self.model.ddim_sigmas_for_original_num_steps``
(ddim.py:256), a table that make_schedule registers on the SAMPLER (ddim.py:56), so decode(use_original_steps=True) raises
AttributeError as shipped.  The use_original_steps case below hands the model the sampler's table before the call -- the evident
intent -- and changes nothing else."""
import inspect
import json
import os

import numpy as np
import torch

import make_golden as MG
from make_golden import HERE, ref_import, rnd, save, synth

SEED_X0, SEED_NOISE, SEED_LATENT, SEED_FEATS, SEED_ETA = 1700, 1701, 1710, 1234, 77
SHAPE = (4, 16, 64)
T_MODEL = [0, 999, 37]          # q_sample / p_losses: first, last and an interior DDPM timestep
T_DDIM = [0, 7, 3]              # stochastic_encode on the S = 8 table: first, last, interior
S = 8


def tiny_model(**extra):
    spec = synth.state_dict_spec(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY)
    sd = synth.make_state_dict(spec, 0)
    cfg = ref_import.load_ldm_config(unet=synth.UNET_TINY, vae=synth.VAE_TINY, cond=synth.COND_TINY)
    cfg.update(extra)
    return ref_import.build_reference_ldm(cfg, sd)


def g17_q_sample():
    model, ns = tiny_model()
    x0, noise = rnd((3,) + SHAPE, SEED_X0), rnd((3,) + SHAPE, SEED_NOISE)
    out = {"t_model": np.asarray(T_MODEL), "t_ddim": np.asarray(T_DDIM)}
    with torch.no_grad():
        out["q_sample"] = model.q_sample(x0, torch.tensor(T_MODEL), noise)
        smp = ns.DDIMSampler(model)
        smp.make_schedule(S, ddim_eta=0.0, verbose=False)
        out["encode_ddim"] = smp.stochastic_encode(x0, torch.tensor(T_DDIM), noise=noise)
        out["encode_original"] = smp.stochastic_encode(x0, torch.tensor(T_MODEL), use_original_steps=True, noise=noise)
    # the tables each of the three read (ddpm.py:281-282; ddim.py:404-408)
    out["model_sqrt_alphas_cumprod"] = model.sqrt_alphas_cumprod
    out["model_sqrt_one_minus_alphas_cumprod"] = model.sqrt_one_minus_alphas_cumprod
    out["ddim_sqrt_alphas"] = torch.sqrt(torch.as_tensor(smp.ddim_alphas))
    out["ddim_sqrt_one_minus_alphas"] = torch.as_tensor(smp.ddim_sqrt_one_minus_alphas)
    out["original_sqrt_alphas_cumprod"] = torch.as_tensor(smp.sqrt_alphas_cumprod)
    out["original_sqrt_one_minus_alphas_cumprod"] = torch.as_tensor(smp.sqrt_one_minus_alphas_cumprod)
    save("g17_q_sample.npz", **out)


P_LOSSES_CASES = {          # tag -> constructor arguments beyond Stage2_LDM.yaml's
    "l2": dict(loss_type="l2"),
    "l1": dict(loss_type="l1"),
    "elbo": dict(loss_type="l2", original_elbo_weight=0.5, logvar_init=-0.3),
    "learn": dict(loss_type="l2", learn_logvar=True, l_simple_weight=0.7, original_elbo_weight=0.25),
}


def g17_p_losses():
    x0, noise = rnd((3,) + SHAPE, SEED_X0), rnd((3,) + SHAPE, SEED_NOISE)
    feats = synth.synthetic_cavp(3, 32, 64, seed=SEED_FEATS)
    t = torch.tensor(T_MODEL)
    out = {"t": np.asarray(T_MODEL)}
    for tag, extra in P_LOSSES_CASES.items():
        model, ns = tiny_model(**extra)
        if extra.get("learn_logvar"):      # a trained logvar is not constant: a ramp, stored for the test's load_state_dict
            with torch.no_grad():
                model.logvar.copy_(torch.linspace(-0.5, 0.3, model.num_timesteps))
        cap = {}
        h = model.model.register_forward_hook(lambda mod, inp, y: cap.update(x_noisy=inp[0].detach().clone(), y=y.detach().clone()))
        with torch.no_grad():
            cond = model.get_learned_conditioning(feats)
            loss, ld = model.p_losses(x0, cond, t, noise=noise)
            loss_simple = model.get_loss(cap["y"], noise, mean=False).mean([1, 2, 3])
        h.remove()
        assert not model.training
        if "x_noisy" in out:                # the same weights, inputs and timesteps: one x_noisy and one model_output for all cases
            assert torch.equal(cap["x_noisy"], out["x_noisy"]) and torch.equal(cap["y"], out["model_output"])
        else:
            out["x_noisy"], out["model_output"] = cap["x_noisy"], cap["y"]
        out[f"{tag}__loss_simple"] = loss_simple
        out[f"{tag}__loss"] = loss
        out[f"{tag}__logvar"] = model.logvar.detach()
        out[f"{tag}__keys"] = np.frombuffer(json.dumps(list(ld.keys())).encode(), dtype=np.uint8)      # the key order, as JSON bytes
        for k, v in ld.items():
            out[f"{tag}__dict__{k.replace('/', '.')}"] = np.float64(v)
        print(tag, {k: f"{v:.6g}" for k, v in ld.items()})
    out["lvlb_weights"] = model.lvlb_weights
    eta = 0.5
    smp = ns.DDIMSampler(model)
    smp.make_schedule(S, ddim_eta=eta, verbose=False)
    out["original_eta"] = np.float64(eta)
    out["original_alphas_cumprod"] = model.alphas_cumprod                                 # ddim.py:253
    out["original_alphas_cumprod_prev"] = model.alphas_cumprod_prev                       # :254
    out["original_sqrt_one_minus_alphas_cumprod"] = model.sqrt_one_minus_alphas_cumprod   # :255
    out["original_ddim_sigmas_for_original_num_steps"] = smp.ddim_sigmas_for_original_num_steps      # :256 (see the module docstring)
    save("g17_p_losses.npz", **out)


def g17_decode():
    import diff_foley.models.diffusion.ddim as ref_ddim
    model, ns = tiny_model()
    B = 2
    x = rnd((B,) + SHAPE, SEED_LATENT)
    feats = synth.synthetic_cavp(B, 32, 64, seed=SEED_FEATS)
    out = {}
    with torch.no_grad():
        c = model.get_learned_conditioning(feats)
        uc = torch.zeros_like(c)
        smp = ns.DDIMSampler(model)
        smp.make_schedule(S, ddim_eta=0.0, verbose=False)
        for t_start in (0, 1, 5, 8):
            out[f"scale1_t{t_start}"] = smp.decode(x.clone(), c, t_start)
        for t_start in (5, 8):
            out[f"scale3_t{t_start}"] = smp.decode(x.clone(), c, t_start, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
        model.ddim_sigmas_for_original_num_steps = smp.ddim_sigmas_for_original_num_steps      # see the module docstring
        out["original_t3"] = smp.decode(x.clone(), c, 3, use_original_steps=True)
        # eta = 0.5: every step draws noise (ddim.py:269); the draws are recorded in the order the reference makes them
        smp = ns.DDIMSampler(model)
        smp.make_schedule(S, ddim_eta=0.5, verbose=False)
        rec, plain = [], ref_ddim.noise_like
        ref_ddim.noise_like = lambda shape, device, repeat=False: rec.append(plain(shape, device, repeat)) or rec[-1]
        try:
            torch.manual_seed(SEED_ETA)
            out["eta05_scale3_t5"] = smp.decode(x.clone(), c, 5, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
        finally:
            ref_ddim.noise_like = plain
        assert len(rec) == 5
        out["eta05_noise"] = torch.stack(rec)
        out["eta05_sigmas"] = np.asarray(smp.ddim_sigmas, dtype=np.float64)
    save("g17_decode.npz", **out)


def g17_signatures():
    ns = ref_import.import_reference()
    LD, DS = ns.LatentDiffusion, ns.DDIMSampler
    points = {"LatentDiffusion.q_sample": LD.q_sample, "LatentDiffusion.get_loss": LD.get_loss, "LatentDiffusion.p_losses": LD.p_losses,
              "LatentDiffusion.forward": LD.forward, "DDIMSampler.stochastic_encode": DS.stochastic_encode, "DDIMSampler.decode": DS.decode}
    out = {name: [dict(name=p.name, kind=p.kind.name, default=None if p.default is inspect.Parameter.empty else repr(p.default))
                  for p in inspect.signature(fn).parameters.values()] for name, fn in points.items()}
    path = os.path.join(HERE, "g17_signatures.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote g17_signatures.json: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    assert MG.HERE == os.path.dirname(os.path.abspath(__file__))
    g17_q_sample()
    g17_p_losses()
    g17_decode()
    g17_signatures()
