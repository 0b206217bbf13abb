"""GPU: q_sample, p_losses / forward and DDIMSampler.stochastic_encode / decode of the facade on the tiny model, both builds, against the
reference's own output (golden G17, tests/golden/make_golden_g17.py) -- and one full-size p_losses.

Tolerances.  The UNet runs on bf16 / fp16 MFMA operands, so everything behind it inherits the bounds the existing golden tests
apply to that build: a single forward rel-L2 2e-2 (bf16: FWD_TOL, tests/test_path_gpu.py:18) / 3e-3 (fp16:
tests/test_path_fp16_gpu.py:139), a DDIM trajectory rel-L2 5e-2 (bf16: TRAJ_TOL, tests/test_path_gpu.py:19) / 1e-2 (fp16:
tests/test_path_fp16_gpu.py:152).  decode runs a suffix of that very loop and is held to the trajectory bound; what p_losses adds to
the UNet is fp32 and is held to 1e-5 against the float64 restatement (tests/diffusion_ref.py) of the device's own apply_model output.

The loss against the golden: with r the forward bound above and, per sample, rho = r |eps_ref| / |eps_ref - target| from the
golden's tensors, a UNet error delta with |delta| <= r |eps_ref| moves the l2 loss |eps - target|^2 / n by at most
(2 |eps_ref - target| |delta| + |delta|^2) / n, i.e. relatively by 2 rho + rho^2.  For l1 the change is at most |delta|_1 <=
sqrt(n) |delta|_2 against |eps_ref - target|_1, i.e. relatively kappa rho with kappa = sqrt(n) |.|_2 / |.|_1 of the residual
(1.25 for a Gaussian residual; asserted <= 2 on the golden), so 2 rho + rho^2 covers it too.

The single-host-copy assertion the full-size test was meant to carry is not made: the suite has no hook that counts device-to-host
copies (the lifecycle tests synchronise streams, they do not count copies), and none is added here."""
import json

import numpy as np
import pytest
import torch

import diffusion_ref as R
from helpers import full_state_dict, gold, rel_l2, rnd, tiny_state_dict
from test_path_gpu import FWD_TOL, TRAJ_TOL

pytestmark = pytest.mark.gpu

FWD = {"bf16": FWD_TOL, "fp16": 3e-3}            # tests/test_path_gpu.py:18, tests/test_path_fp16_gpu.py:139
TRAJ = {"bf16": TRAJ_TOL, "fp16": 1e-2}          # tests/test_path_gpu.py:19, tests/test_path_fp16_gpu.py:152
SEED_X0, SEED_NOISE, SEED_LATENT, SEED_FEATS, SEED_ETA = 1700, 1701, 1710, 1234, 77      # tests/golden/make_golden_g17.py
SHAPE = (4, 16, 64)
CASES = {"l2": dict(loss_type="l2"), "l1": dict(loss_type="l1"),
         "elbo": dict(loss_type="l2", original_elbo_weight=0.5, logvar_init=-0.3),
         "learn": dict(loss_type="l2", learn_logvar=True, l_simple_weight=0.7, original_elbo_weight=0.25)}
KEYS = {False: ["val/loss_simple", "val/loss_vlb", "val/loss"],
        True: ["val/loss_simple", "val/loss_gamma", "logvar", "val/loss_vlb", "val/loss"]}      # ddpm.py:1062-1079, eval mode
_models = {}


def _tiny(prec, tag="l2"):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    if (prec, tag) not in _models:
        g = gold("g17_p_losses.npz")
        m = P.LatentDiffusion(precision=prec, **dict(P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY), **CASES[tag]))
        sd = dict(tiny_state_dict())
        if CASES[tag].get("learn_logvar"):
            sd["logvar"] = g["learn__logvar"]              # a trained logvar arrives through the state dict
        m.load_state_dict(sd)
        m.cuda()
        assert torch.equal(m.logvar.cpu(), g[f"{tag}__logvar"]) and m.logvar.is_cuda and m.lvlb_weights.is_cuda
        _models[(prec, tag)] = m
    return _models[(prec, tag)]


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def prec(request):
    yield request.param
    for k in [k for k in _models if k[0] == request.param]:
        del _models[k]


def _inputs(m, B=3):
    from diff_foley_amd import synth
    x0, noise = rnd((B,) + SHAPE, SEED_X0), rnd((B,) + SHAPE, SEED_NOISE)
    cond = m.get_learned_conditioning(synth.synthetic_cavp(B, 32, 64, seed=SEED_FEATS).cuda())
    return x0, noise, cond


def _own_parts(m, x0, noise, t, cond):
    """loss_dict of the float64 restatement applied to the device's EXISTING apply_model output at the q_sample the facade returns."""
    x_noisy = m.q_sample(x0.cuda(), t.cuda(), noise.cuda())
    eps = m.apply_model(x_noisy, t.cuda(), cond)
    ls, sc = R.diffusion_loss_ref(eps, noise, t, m.logvar, m.lvlb_weights, m.loss_type, m.l_simple_weight, m.original_elbo_weight)
    return R.loss_dict_ref(sc, m.learn_logvar), eps, ls


def _assert_dict(got, want, rel, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        assert isinstance(got[k], float)
        assert abs(got[k] - want[k]) <= rel * abs(want[k]), (what, k, got[k], want[k])


def test_q_sample_and_stochastic_encode_against_the_reference(prec):
    from diff_foley_amd import samplers as S
    m = _tiny(prec)
    g = gold("g17_q_sample.npz")
    x0, noise = rnd((3,) + SHAPE, SEED_X0), rnd((3,) + SHAPE, SEED_NOISE)
    smp = S.DDIMSampler(m)
    smp.make_schedule(8, ddim_eta=0.0, verbose=False)
    runs = (("q_sample", lambda t: m.q_sample(x0.cuda(), t, noise.cuda()), "t_model", "model_sqrt_alphas_cumprod",
             "model_sqrt_one_minus_alphas_cumprod"),
            ("encode_ddim", lambda t: smp.stochastic_encode(x0.cuda(), t, noise=noise.cuda()), "t_ddim", "ddim_sqrt_alphas",
             "ddim_sqrt_one_minus_alphas"),
            ("encode_original", lambda t: smp.stochastic_encode(x0.cuda(), t, use_original_steps=True, noise=noise.cuda()), "t_model",
             "original_sqrt_alphas_cumprod", "original_sqrt_one_minus_alphas_cumprod"))
    for name, fn, tk, A, Sg in runs:
        ref, bound = R.q_sample_ref(x0, noise, g[tk], g[A], g[Sg])
        for t in (g[tk].cuda(), g[tk]):                   # a device t (not read on the host) and a host t
            out = fn(t)
            assert out.shape == x0.shape and out.dtype == torch.float32 and out.is_cuda
            got = out.cpu().double().numpy()
            assert (np.abs(got - ref) <= bound).all(), name                                       # the kernel's own rounding
            assert (np.abs(got - g[name].double().numpy()) <= 2 * bound).all(), name               # two fp32 evaluations of one value
    with pytest.raises(IndexError):
        m.q_sample(x0.cuda(), torch.tensor([0, 1000, 5]), noise.cuda())
    with pytest.raises(IndexError):
        smp.stochastic_encode(x0.cuda(), torch.tensor([0, 8, 5]), noise=noise.cuda())
    with pytest.raises(ValueError, match=r"expected \(3, 4, 16, 64\)"):
        m.q_sample(x0.cuda(), torch.tensor([0, 1, 5]), noise[:2].cuda())
    torch.manual_seed(5)
    a = m.q_sample(x0.cuda(), g["t_model"].cuda())
    torch.manual_seed(5)
    b = m.q_sample(x0.cuda(), g["t_model"].cuda(), torch.randn_like(x0.cuda()))
    assert torch.equal(a, b)                              # noise=None draws randn_like(x_start), as ddpm.py:280


@pytest.mark.parametrize("tag", list(CASES))
def test_p_losses_against_its_own_parts_and_the_reference(prec, tag):
    m = _tiny(prec, tag)
    g = gold("g17_p_losses.npz")
    x0, noise, cond = _inputs(m)
    t = g["t"]
    loss, ld = m.p_losses(x0.cuda(), cond, t.cuda(), noise=noise.cuda())
    assert loss.ndim == 0 and loss.is_cuda and loss.dtype == torch.float32
    assert list(ld) == KEYS[m.learn_logvar] == json.loads(bytes(g[f"{tag}__keys"].numpy()).decode())
    assert float(loss) == ld["val/loss"]
    # (a) the fused chain adds nothing of its own
    from diff_foley_amd import engine as E
    want, eps, ls_own = _own_parts(m, x0, noise, t, cond)
    _assert_dict(ld, want, 1e-5, (prec, tag, "own parts"))
    ls_dev = E.diffusion_loss(eps, noise.cuda(), t.cuda(), m.logvar, m.lvlb_weights, m.loss_type)[0].cpu().double().numpy()
    assert (np.abs(ls_dev - ls_own) <= 1e-5 * ls_own).all()
    # (b) the reference: per-sample loss_simple within what a UNet error of relative size r allows
    eps_ref, target = g["model_output"].double(), noise.double()
    ls_ref = g[f"{tag}__loss_simple"].double().numpy()
    n = eps_ref[0].numel()
    for b in range(3):
        res = (eps_ref[b] - target[b]).flatten()
        rho = FWD[prec] * float(eps_ref[b].norm()) / float(res.norm())
        if m.loss_type == "l1":
            assert np.sqrt(n) * float(res.norm()) / float(res.abs().sum()) <= 2.0
        bound = 2 * rho + rho * rho
        ratio = abs(ls_dev[b] - ls_ref[b]) / ls_ref[b]
        print(f"p_losses {prec} {tag} sample {b} (t = {int(t[b])}): |d loss_simple| / loss_ref = {ratio:.3e}, "
              f"bound 2 rho + rho^2 = {bound:.3e} (rho = {rho:.3e}), observed / bound = {ratio / bound:.3f}")
        assert ratio <= bound, (prec, tag, b, ratio, bound)
    for k in KEYS[m.learn_logvar]:
        print(f"p_losses {prec} {tag} {k}: {ld[k]:.6f} (reference {float(g[f'{tag}__dict__' + k.replace('/', '.')]):.6f})")
    # what the UNet does not touch equals the reference to fp32 rounding
    if m.learn_logvar:
        assert abs(ld["logvar"] - float(g["learn__dict__logvar"])) <= 1e-5 * abs(float(g["learn__dict__logvar"]))
    # a host t gives the same bits; wrong shapes are ValueErrors that name the expected shape
    loss2, ld2 = m.p_losses(x0.cuda(), cond, t, noise=noise.cuda())
    assert ld2 == ld and torch.equal(loss, loss2)
    with pytest.raises(ValueError, match=r"expected \(3, 4, 16, 64\)"):
        m.p_losses(x0.cuda(), cond, t.cuda(), noise=noise[:, :, :8].cuda())
    with pytest.raises(ValueError, match=r"expected \(3,\)"):
        m.p_losses(x0.cuda(), cond, t[:2].cuda(), noise=noise.cuda())
    with pytest.raises(IndexError):
        m.p_losses(x0.cuda(), cond, torch.tensor([0, 1000, 5]), noise=noise.cuda())


def test_get_loss_matches_the_restatement(prec):
    m1, m2 = _tiny(prec, "l1"), _tiny(prec, "l2")
    a, b = rnd((3,) + SHAPE, 1), rnd((3,) + SHAPE, 2)
    for m, kind in ((m1, "l1"), (m2, "l2")):
        ref = R.loss_simple_ref(a, b, kind)
        got = m.get_loss(a.cuda(), b.cuda())
        assert got.ndim == 0 and abs(float(got) - ref.mean()) <= (1e-5 + 3 * R.U) * ref.mean()
        full = m.get_loss(a.cuda(), b.cuda(), mean=False)
        assert full.shape == a.shape
        assert np.allclose(full.reshape(3, -1).mean(1).cpu().double().numpy(), ref, rtol=1e-5, atol=0)


@pytest.mark.parametrize("tag", ["l2", "learn"])
def test_forward_draws_t_and_noise_on_the_device_then_is_p_losses(prec, tag):
    from diff_foley_amd import synth
    m = _tiny(prec, tag)
    x0 = rnd((3,) + SHAPE, SEED_X0).cuda()
    feats = synth.synthetic_cavp(3, 32, 64, seed=SEED_FEATS).cuda()
    torch.manual_seed(123)
    loss, ld = m(x0, feats)
    torch.manual_seed(123)
    t = torch.randint(0, m.num_timesteps, (3,), device=m.device).long()
    noise = torch.randn_like(x0)
    loss2, ld2 = m.p_losses(x0, m.get_learned_conditioning(feats), t, noise=noise)
    assert list(ld) == KEYS[m.learn_logvar] and ld == ld2 and torch.equal(loss, loss2)
    assert all(np.isfinite(v) for v in ld.values())
    torch.manual_seed(124)
    assert m.forward(x0, feats)[1] != ld                  # another seed, another t and noise


def _decode_inputs(m):
    from diff_foley_amd import synth
    x = rnd((2,) + SHAPE, SEED_LATENT)
    c = m.get_learned_conditioning(synth.synthetic_cavp(2, 32, 64, seed=SEED_FEATS).cuda())
    return x, c, torch.zeros_like(c)


def test_decode_against_the_reference(prec, capsys):
    from diff_foley_amd import samplers as S
    m = _tiny(prec)
    g = gold("g17_decode.npz")
    x, c, uc = _decode_inputs(m)
    smp = S.DDIMSampler(m)
    with pytest.raises(AttributeError):
        smp.decode(x.cuda(), c, 5)                        # no schedule yet, as in the reference
    smp.make_schedule(8, ddim_eta=0.0, verbose=False)
    xd = x.cuda()
    capsys.readouterr()
    assert smp.decode(xd, c, 0) is xd and torch.equal(xd.cpu(), g["scale1_t0"]) and torch.equal(xd.cpu(), x)
    assert "Running DDIM Sampling with 0 timesteps" in capsys.readouterr().out
    runs = [(f"scale1_t{k}", dict(t_start=k)) for k in (1, 5, 8)]
    runs += [(f"scale3_t{k}", dict(t_start=k, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)) for k in (5, 8)]
    runs += [("original_t3", dict(t_start=3, use_original_steps=True))]
    for name, kw in runs:
        z = smp.decode(x.cuda(), c, **kw)
        assert f"Running DDIM Sampling with {kw['t_start']} timesteps" in capsys.readouterr().out
        err = rel_l2(z.cpu(), g[name])
        print(f"decode {prec} {name}: rel-L2 {err:.3e} (bound {TRAJ[prec]:.0e})")
        assert z.shape == x.shape and err < TRAJ[prec], (name, err)
    # eta = 0.5: sigma is the table's, noise is drawn at every step; the reference's draws replayed through the sampler's noise hook
    smp = S.DDIMSampler(m)
    smp.make_schedule(8, ddim_eta=0.5, verbose=False)
    assert np.allclose(smp.ddim_sigmas.astype(np.float64), g["eta05_sigmas"].numpy(), rtol=2e-6, atol=0) and (smp.ddim_sigmas != 0).all()
    draws = iter(g["eta05_noise"])
    smp.noise_fn = lambda size: next(draws)
    z = smp.decode(x.cuda(), c, 5, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    assert next(draws, None) is None                      # five steps, five draws
    err = rel_l2(z.cpu(), g["eta05_scale3_t5"])
    print(f"decode {prec} eta05_scale3_t5: rel-L2 {err:.3e} (bound {TRAJ[prec]:.0e})")
    assert err < TRAJ[prec]
    assert rel_l2(z.cpu(), g["scale3_t5"]) > 0.05         # ... and the noise was applied


def test_decode_and_sample_do_not_disturb_each_other(prec):
    """Context and hoisted-timestep-table ownership: decode after sample() on the same model, and sample() after decode, return what
    each returns in isolation -- bit for bit."""
    from diff_foley_amd import samplers as S, synth
    m = _tiny(prec)
    x, c, uc = _decode_inputs(m)
    xT = synth.synthetic_xT(2, seed=21)
    smp = S.DDIMSampler(m)
    smp.make_schedule(8, ddim_eta=0.0, verbose=False)
    kw = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    z0 = smp.decode(x.cuda(), c, 5, **kw)
    s0, _ = m.sample_log_diff_sampler(c, 2, "DDIM", 4, unconditional_guidance_scale=4.5, unconditional_conditioning=uc, x_T=xT.clone())
    z1 = smp.decode(x.cuda(), c, 5, **kw)
    s1, _ = m.sample_log_diff_sampler(c, 2, "DDIM", 4, unconditional_guidance_scale=4.5, unconditional_conditioning=uc, x_T=xT.clone())
    e0 = m.apply_model(x.cuda(), torch.tensor([500, 37]).cuda(), c)      # apply_model's own context cache in between
    z2 = smp.decode(x.cuda(), c, 5, **kw)
    e1 = m.apply_model(x.cuda(), torch.tensor([500, 37]).cuda(), c)
    assert torch.equal(z0, z1) and torch.equal(z0, z2) and torch.equal(s0, s1) and torch.equal(e0, e1)
    # the chain a caller would run: noise a latent to step 5 of 8, denoise it from there
    t = torch.full((2,), 4, dtype=torch.long, device="cuda")
    z = smp.decode(smp.stochastic_encode(x.cuda(), t, noise=rnd((2,) + SHAPE, 3).cuda()), c, 5, **kw)
    assert z.shape == x.shape and torch.isfinite(z).all()


def test_full_size_p_losses():
    """B = 2, the Stage-2 UNet, t = (0, 999): finite, and equal to the restatement applied to the device's own apply_model output."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    m = P.LatentDiffusion(precision="fp16", **P.stage2_config())
    m.load_state_dict(full_state_dict())
    m.cuda()
    x0, noise = rnd((2,) + SHAPE, SEED_X0), rnd((2,) + SHAPE, SEED_NOISE)
    cond = m.get_learned_conditioning(synth.synthetic_cavp(2, 32, 512, seed=SEED_FEATS).cuda())
    t = torch.tensor([0, 999])
    loss, ld = m.p_losses(x0.cuda(), cond, t.cuda(), noise=noise.cuda())
    assert list(ld) == KEYS[False] and all(np.isfinite(v) for v in ld.values()) and torch.isfinite(loss)
    want, _, _ = _own_parts(m, x0, noise, t, cond)
    _assert_dict(ld, want, 1e-5, "full size")
    print("full-size p_losses:", {k: round(v, 6) for k, v in ld.items()})
