"""GPU: diff_foley_amd.dpm_solver on the tiny model, both builds, against the reference's own output (golden G18,
tests/golden/make_golden_g18.py).

  (b) final latents of the fixed-step methods on the fast route (LatentDiffusion.dpm_solver), predict_x0 True and False, within the
      trajectory bound TRAJ[prec] of tests/test_start_from_sound_gpu.py -- trajectories of at most 15 evaluations;
  (c) the adaptive solver with a closed-form fp32 model through the generic route: the decision sequence equals the reference's, the
      tried times and the final latent agree to 1e-4 relative (fp32 on both sides; the maker keeps every E at least 0.02 from 1);
  (d) the adaptive solver on the tiny UNet, fast route: it terminates at t_0 and the final latent is within TRAJ[prec] + d_ref, d_ref
      being the reference's own sensitivity to its step sequence.  No assertion on the number of evaluations;
  *   DPMSolverSampler.sample is the fast route with multistep / order 2 / time_uniform / predict_x0: bit-equal latents;
  *   the generic route around ``lambda x, t, c: m.apply_model(x, t, c)`` agrees with the fast route within FWD[prec] per evaluation;
  *   guidance_type='classifier' through AlignmentClassifier.log_prob_grad and the x_start / v conversions equal their expressions."""
import numpy as np
import pytest
import torch

from helpers import gold, rel_l2, rnd, tiny_classifier_sd, tiny_state_dict
from test_start_from_sound_gpu import FWD, TRAJ

pytestmark = pytest.mark.gpu

SEED_LATENT, SEED_FEATS, SEED_VF, SEED_CLOSED = 1810, 1234, 4321, 1800      # tests/golden/make_golden_g18.py
SHAPE = (4, 16, 64)
B = 2
SCALE, CLS_SCALE = 3.0, 50.0
CLOSED_SHAPE = (3, 4, 8, 8)
CLOSED = dict(a=1.6, w=12.0, b=0.4)
FIXED_CASES = {
    "ss3_logsnr": dict(steps=7, order=3, method="singlestep", skip_type="logSNR"),
    "ss3_logsnr_taylor": dict(steps=8, order=3, method="singlestep", skip_type="logSNR", solver_type="taylor"),
    "ms3_nolower": dict(steps=6, order=3, method="multistep", lower_order_final=False),
    "ms3_15": dict(steps=15, order=3, method="multistep"),
    "sf2_logsnr": dict(steps=6, order=2, method="singlestep_fixed", skip_type="logSNR"),
    "sf2_quad_taylor": dict(steps=5, order=2, method="singlestep_fixed", skip_type="time_quadratic", solver_type="taylor"),
    "ss3_uniform": dict(steps=7, order=3, method="singlestep", skip_type="time_uniform"),
}
X0_ONLY_CASES = {
    "ms2_thr_dz": dict(steps=6, order=2, method="multistep", denoise_to_zero=True),
    "ms2_tstart": dict(steps=6, order=2, method="multistep", t_start=0.6),
    "ms2_double": dict(steps=6, order=2, method="multistep"),
}
EVALUATIONS = {"ss3_logsnr": 7, "ss3_logsnr_taylor": 8, "ms3_nolower": 6, "ms3_15": 15, "sf2_logsnr": 6, "sf2_quad_taylor": 4,
               "ss3_uniform": 7, "ms2_thr_dz": 7, "ms2_tstart": 6, "ms2_double": 6}
_models = {}


def _tiny(prec):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    if prec not in _models:
        m = P.LatentDiffusion(precision=prec, **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
        m.load_state_dict(tiny_state_dict())
        m.cuda()
        _models[prec] = m
    return _models[prec]


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def prec(request):
    yield request.param
    _models.pop(request.param, None)


def _inputs(m):
    from diff_foley_amd import synth
    x = rnd((B,) + SHAPE, SEED_LATENT).cuda()
    c = m.get_learned_conditioning(synth.synthetic_cavp(B, 32, 64, seed=SEED_FEATS).cuda())
    return x, c, torch.zeros_like(c)


def _count_evaluations(monkeypatch):
    """Every guided evaluation of the fast route, with whether it found its time in the hoisted table."""
    from diff_foley_amd import dpm_solver as D
    seen = []
    plain = D._FastSession.__call__

    def call(self, x, t):
        seen.append((float(t), self.index.get(float(t)) is not None and self.eps.hoisted))
        return plain(self, x, t)
    monkeypatch.setattr(D._FastSession, "__call__", call)
    return seen


@pytest.mark.parametrize("tag_p", ["x0", "eps"])
def test_fixed_step_latents_against_the_reference(prec, tag_p, monkeypatch):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    m = _tiny(prec)
    g = gold(f"g18_latents_{tag_p}.npz")
    x, c, uc = _inputs(m)
    px = tag_p == "x0"
    seen = _count_evaluations(monkeypatch)
    runs = [(tag, kw, {}) for tag, kw in FIXED_CASES.items()]
    if px:
        cls = P.AlignmentClassifier(classifier_config=dict(params=dict(synth.CLS_TINY)))
        cls.load_state_dict(tiny_classifier_sd())
        vf = synth.synthetic_cavp(B, 33, 64, seed=SEED_VF).cuda()
        runs += [("ms2_thr_dz", X0_ONLY_CASES["ms2_thr_dz"], dict(thresholding=True)), ("ms2_tstart", X0_ONLY_CASES["ms2_tstart"], {}),
                 ("ms2_double", X0_ONLY_CASES["ms2_double"], dict(classifier=cls, origin_cond=vf, classifier_guide_scale=CLS_SCALE))]
    for tag, kw, extra in runs:
        del seen[:]
        sol = m.dpm_solver(c, SCALE, uc, predict_x0=px, **extra)
        assert sol.fast
        z = sol.sample(x.clone(), **kw)
        err = rel_l2(z.cpu(), g[tag])
        print(f"dpm family {prec} {tag_p} {tag}: rel-L2 {err:.3e} (bound {TRAJ[prec]:.0e}), {len(seen)} evaluations")
        assert z.shape == x.shape and z.dtype == torch.float32 and z.is_cuda
        assert len(seen) == EVALUATIONS[tag], (tag, len(seen))
        assert all(hit for _, hit in seen), (tag, "a time was not hoisted", seen)
        assert err < TRAJ[prec], (tag, err)
        if tag == "ms2_thr_dz":
            assert float(z.abs().max()) <= 1.0


def test_fast_route_2m_is_bit_equal_to_the_dpm_solver_sampler(prec):
    """DPMSolverSampler.sample builds the model's DPM_Solver and asks for DPM-Solver++(2M): the latents of that call and of the
    solver asked directly for multistep / order 2 / time_uniform are the same bits, so the sampler selects that configuration
    (lower_order_final included: 6 and 15 steps are its two sides) and adds nothing to it."""
    import diff_foley_amd as P
    m = _tiny(prec)
    x, c, uc = _inputs(m)
    for steps in (6, 15):          # lower_order_final lowers the last step below 15 only
        old, _ = P.DPMSolverSampler(m).sample(steps, B, SHAPE, c, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc,
                                              x_T=x.clone())
        new = m.dpm_solver(c, SCALE, uc).sample(x.clone(), steps=steps, order=2, method="multistep", skip_type="time_uniform")
        assert torch.equal(old, new), (steps, rel_l2(new.cpu(), old.cpu()))
    # ... and without guidance (scale 1: the conditional evaluation alone)
    old, _ = P.DPMSolverSampler(m).sample(6, B, SHAPE, c, x_T=x.clone())
    new = m.dpm_solver(c).sample(x.clone(), steps=6, order=2, method="multistep", skip_type="time_uniform")
    assert torch.equal(old, new)


def test_generic_route_agrees_with_the_fast_route(prec):
    from diff_foley_amd import dpm_solver as D
    m = _tiny(prec)
    x, c, uc = _inputs(m)
    fast = m.dpm_solver(c, SCALE, uc, predict_x0=False)
    ns = fast.noise_schedule
    fn = D.model_wrapper(lambda xx, t, cc: m.apply_model(xx, t, cc), ns, model_type="noise", guidance_type="classifier-free",
                         condition=c, unconditional_condition=uc, guidance_scale=SCALE)
    generic = D.DPM_Solver(fn, ns, predict_x0=False)
    assert fast.fast and not generic.fast
    for t in (1.0, 0.4567, 1e-3):
        a, b = fast.noise_prediction_fn(x, t), generic.noise_prediction_fn(x, torch.full((B,), t, device="cuda"))
        err = rel_l2(b.cpu(), a.cpu())
        print(f"generic vs fast {prec} t = {t}: rel-L2 {err:.3e} (bound {FWD[prec]:.0e})")
        assert err < FWD[prec], (t, err)
    kw = FIXED_CASES["ss3_logsnr"]
    za, zb = fast.sample(x.clone(), **kw), generic.sample(x.clone(), **kw)
    err = rel_l2(zb.cpu(), za.cpu())
    print(f"generic vs fast {prec} ss3_logsnr: rel-L2 {err:.3e} (7 evaluations, bound {TRAJ[prec]:.0e})")
    assert err < TRAJ[prec]
    with pytest.raises(ValueError, match="must be equal"):
        generic.noise_prediction_fn(x, torch.tensor([0.5, 0.4], device="cuda"))


def closed_model(x, t):
    return CLOSED["a"] * x * torch.cos(CLOSED["w"] * t)[:, None, None, None] + CLOSED["b"] * torch.sin(3 * x)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("tag_p", ["x0", "eps"])
def test_adaptive_decisions_with_a_closed_form_model(order, tag_p, capsys):
    """Generic route, no UNet: every accept / reject of the reference, its tried times and its final latent."""
    from diff_foley_amd import dpm_solver as D, schedule
    g = gold("g18_adaptive.npz")
    k = f"closed__{order}__{tag_p}"
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=schedule.register_schedule(0.00085, 0.0120, 1000)["alphas_cumprod"])
    sol = D.DPM_Solver(closed_model, ns, predict_x0=tag_p == "x0")
    capsys.readouterr()
    z = sol.sample(rnd(CLOSED_SHAPE, SEED_CLOSED).cuda(), order=order, method="adaptive")
    assert capsys.readouterr().out == bytes(g[k + "__said"].numpy()).decode()      # the reference's closing line
    t_ref, E_ref, acc_ref = g[k + "__t"].numpy(), g[k + "__E"].numpy(), g[k + "__accepted"].numpy()
    assert np.abs(E_ref - 1).min() >= 0.02 and acc_ref.any() and not acc_ref.all()
    tr = sol.adaptive_trace
    for i, (t, e, a) in enumerate(tr[:len(t_ref)]):
        print(f"adaptive closed order {order} {tag_p} attempt {i}: t {t:.6f} (ref {t_ref[i]:.6f}), E {e:.4f} (ref {E_ref[i]:.4f}), "
              f"{'accepted' if a else 'rejected'}")
    assert [a for _, _, a in tr] == acc_ref.tolist()
    t_err = max(abs(t - r) / r for (t, _, _), r in zip(tr, t_ref))
    z_err = rel_l2(z.cpu(), g[k + "__z"])
    print(f"adaptive closed order {order} {tag_p}: times rel {t_err:.3e}, latent rel-L2 {z_err:.3e} (bound 1e-4)")
    assert t_err <= 1e-4 and z_err <= 1e-4


@pytest.mark.parametrize("order", [2, 3])
def test_adaptive_on_the_tiny_unet(prec, order, capsys, monkeypatch):
    m = _tiny(prec)
    g = gold("g18_adaptive.npz")
    x, c, uc = _inputs(m)
    seen = _count_evaluations(monkeypatch)
    sol = m.dpm_solver(c, SCALE, uc)
    capsys.readouterr()
    z = sol.sample(x.clone(), order=order, method="adaptive")
    tr = sol.adaptive_trace
    assert capsys.readouterr().out == f"adaptive solver nfe {order * len(tr)}\n"
    assert tr and tr[-1][2] and abs(tr[-1][0] - 1e-3) <= 1e-5                # the last attempt was accepted, at t_0
    assert all(tr[i][0] > tr[j][0] for i, j in zip(range(len(tr)), range(1, len(tr))) if tr[i][2])      # accepted steps move down
    assert len(seen) == order * len(tr) and not any(hit for _, hit in seen)  # the in-step embedding: no table
    d_ref = float(g[f"unet__{order}__d_ref"])
    err = rel_l2(z.cpu(), g[f"unet__{order}__z"])
    print(f"adaptive unet {prec} order {order}: {len(tr)} attempts ({int(g[f'unet__{order}__attempts'])} in the reference), "
          f"{sum(not a for _, _, a in tr)} rejected, rel-L2 {err:.3e} (bound {TRAJ[prec]:.0e} + d_ref {d_ref:.3e})")
    assert err < TRAJ[prec] + d_ref


def test_classifier_guidance_and_the_model_type_conversions(prec):
    """guidance_type='classifier' through AlignmentClassifier.log_prob_grad, and the x_start / v conversions of the generic route: each
    against the same expression in torch on the device's own tensors (fp32 arithmetic around given tensors: a few roundings)."""
    import diff_foley_amd as P
    from diff_foley_amd import dpm_solver as D, synth
    m = _tiny(prec)
    x, c, uc = _inputs(m)
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=m.alphas_cumprod)
    cls = P.AlignmentClassifier(classifier_config=dict(params=dict(synth.CLS_TINY)))
    cls.load_state_dict(tiny_classifier_sd())
    cls.attach(m)
    vf = synth.synthetic_cavp(B, 33, 64, seed=SEED_VF).cuda()
    t = 0.4567
    t_in = torch.full((B,), float(ns.tables.model_time(t)), device="cuda")
    sigma, alpha = float(ns.tables.sigma(t)), float(ns.tables.alpha(t))
    fn = D.model_wrapper(lambda xx, tt: m.apply_model(xx, tt, c), ns, guidance_type="classifier", condition=vf, guidance_scale=2.0,
                         classifier_fn=cls)
    got = D.DPM_Solver(fn, ns).noise_prediction_fn(x, t)
    eps, grad = m.apply_model(x, t_in, c), cls.log_prob_grad(x, t_in, vf)
    want = eps.double() - 2.0 * sigma * grad.double()
    scale = eps.double().abs() + 2.0 * sigma * grad.double().abs()
    assert bool(((got.double() - want).abs() <= 4 * 2.0 ** -24 * scale).all()) and float(grad.abs().max()) > 0
    out = rnd((B,) + SHAPE, 7).cuda()
    for model_type, ref in (("x_start", (x.double() - alpha * out.double()) / sigma), ("v", alpha * out.double() + sigma * x.double())):
        fn = D.model_wrapper(lambda xx, tt: out, ns, model_type=model_type)
        got = D.DPM_Solver(fn, ns).noise_prediction_fn(x, torch.tensor(t))
        size = (x.double().abs() + alpha * out.double().abs()) / (sigma if model_type == "x_start" else 1.0) + sigma * x.double().abs()
        assert bool(((got.double() - ref).abs() <= 4 * 2.0 ** -24 * size).all()), model_type
