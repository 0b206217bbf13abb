"""CPU: the host side of diff_foley_amd.dpm_solver against the reference's own output (golden G18, tests/golden/make_golden_g18.py).

  * the five NoiseScheduleVP functions of the three schedules (and the betas route of 'discrete') on the golden's time grid, the
    inverse_lambda round trip, get_time_steps for the three spacings and get_orders_and_timesteps_for_singlestep_solver for
    steps 1-10 x order 1-3;
  * every public entry point takes what the reference's takes (g18_signatures.json, with test_signatures_cpu.compare);
  * the exception classes the reference raises on its arguments, and the two documented deviations;
  * df_dpm_data_prediction and df_dpm_adaptive_error are declared in the header and exported by both builds.

Tolerances (u = 2^-24, one fp32 rounding).  Both sides evaluate the same few fp32 operations, the reference with torch and the product
with numpy on the host, whose exp / log / cos may differ in the last bit; so each value is held to a handful of roundings times the
conditioning of the expression it comes from:
  log(alpha)   8 u |la| + 2 u                          (the absolute part: log(cos x) of the cosine schedule near cos x = 1)
  alpha        alpha (D_la + 2 u)
  sigma        D_s2 / (2 sigma) + 2 u sigma,   D_s2 = alpha^2 (2 D_la + 2 u) + u   the error of 1 - exp(2 la), which cancels
  lambda       D_la + D_s2 / (2 sigma^2) + 4 u |lambda|
  a time that comes back through inverse_lambda      8 u / min |d la / dt| + 16 u t: lambda -> log(alpha) = -0.5 log1p(exp(-2 lambda))
               carries an absolute error of about u whatever the size of log(alpha), and t(log alpha) has slope 1 / (d la / dt).  The
               slope is measured on the golden's own (t, log alpha) pairs.
  time_uniform / time_quadratic grids                 4 u t (the same torch.linspace on both sides)."""
import json
import os

import numpy as np
import pytest
import torch

import diff_foley_amd as P
from diff_foley_amd import dpm_solver as D, engine as E, schedule, synth
from helpers import GOLD, gold
from test_signatures_cpu import _described, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
TAGS = ["discrete", "betas10", "linear", "cosine"]


def _schedule(tag, g):
    if tag == "discrete":
        return D.NoiseScheduleVP("discrete", alphas_cumprod=schedule.register_schedule(0.00085, 0.0120, 1000)["alphas_cumprod"])
    if tag == "betas10":
        return D.NoiseScheduleVP("discrete", betas=g["betas10"])
    return D.NoiseScheduleVP(tag)


def _bounds(g, tag):
    t = g[f"{tag}__t"].double().numpy()
    la = g[f"{tag}__marginal_log_mean_coeff"].double().numpy()
    al, sg, lam = (g[f"{tag}__{k}"].double().numpy() for k in ("marginal_alpha", "marginal_std", "marginal_lambda"))
    d_la = 8 * U * np.abs(la) + 2 * U
    d_s2 = al ** 2 * (2 * d_la + 2 * U) + U
    tu, first = np.unique(t, return_index=True)                                 # the grid may name a time twice
    slope = np.abs(np.diff(la[first]) / np.diff(tu)).min()
    return dict(marginal_log_mean_coeff=d_la, marginal_alpha=al * (d_la + 2 * U), marginal_std=d_s2 / (2 * sg) + 2 * U * sg,
                marginal_lambda=d_la + d_s2 / (2 * sg ** 2) + 4 * U * np.abs(lam)), lambda tt: 8 * U / slope + 16 * U * np.abs(tt)


@pytest.mark.parametrize("tag", TAGS)
def test_schedule_functions_equal_the_reference(tag):
    g = gold("g18_schedule.npz")
    ns = _schedule(tag, g)
    assert ns.schedule == ("discrete" if tag == "betas10" else tag)
    assert float(ns.T) == float(g[f"{tag}__T"]) and int(ns.total_N) == int(g[f"{tag}__total_N"])
    t = g[f"{tag}__t"]
    bounds, t_tol = _bounds(g, tag)
    for name, tol in bounds.items():
        got = getattr(ns, name)(t)
        assert torch.is_tensor(got) and got.dtype == torch.float32 and got.shape == t.shape, name
        ref = g[f"{tag}__{name}"].double().numpy()
        ok = ~np.isnan(ref)          # a grid time in front of the first knot extrapolates to alpha > 1: sigma is NaN there, on both sides
        assert (np.isnan(got.numpy()) == ~ok).all() and ok.sum() >= len(ok) - 1, (tag, name)
        err = np.abs(got.double().numpy() - ref)
        assert (err[ok] <= tol[ok]).all(), (tag, name, float((err[ok] / tol[ok]).max()))
        one = getattr(ns, name)(float(t[3]))                                    # a float in, a host fp32 scalar out
        assert isinstance(one, np.float32) and one == got[3].numpy() and ok[3]
    # the round trip, on the reference's own lambda (inverse_lambda alone) and on the product's
    want = g[f"{tag}__inverse_lambda"].double().numpy()
    for lam in (g[f"{tag}__marginal_lambda"], ns.marginal_lambda(t)):
        back = ns.inverse_lambda(lam).double().numpy()
        ok = ~np.isnan(want)
        assert (np.isnan(back) == ~ok).all()
        assert (np.abs(back - want)[ok] <= t_tol(want)[ok]).all(), (tag, float(np.abs(back - want)[ok].max()))
        assert (np.abs(back - t.double().numpy())[ok] <= 2 * t_tol(want)[ok]).all()
    with pytest.raises(ValueError, match="Unsupported noise schedule"):
        D.NoiseScheduleVP("sigmoid")


@pytest.mark.parametrize("tag", ["discrete", "linear", "cosine"])
def test_time_grids_and_singlestep_orders_equal_the_reference(tag):
    g = gold("g18_schedule.npz")
    ns = _schedule(tag, g)
    sol = D.DPM_Solver(lambda x, t: x, ns)
    _, t_tol = _bounds(g, tag)
    t_0, t_T = 1. / ns.total_N, ns.T
    for skip in ("logSNR", "time_uniform", "time_quadratic"):
        tol = t_tol if skip == "logSNR" else (lambda tt: 4 * U * np.abs(tt))
        got = sol.get_time_steps(skip, t_T, t_0, 10, "cpu")
        want = g[f"{tag}__steps__{skip}"].double().numpy()
        assert got.dtype == torch.float32 and got.shape == (11,)
        assert (np.abs(got.double().numpy() - want) <= tol(want)).all(), (tag, skip)
        for steps in range(1, 11):
            for order in (1, 2, 3):
                outer, orders = sol.get_orders_and_timesteps_for_singlestep_solver(steps, order, skip, t_T, t_0, "cpu")
                assert orders == g[f"{tag}__orders__{skip}__{steps}__{order}"].tolist() and sum(orders) == steps
                want = g[f"{tag}__outer__{skip}__{steps}__{order}"].double().numpy()
                assert tuple(outer.shape) == want.shape      # (order 1 on logSNR: K = 1, two times for `steps` orders, as there)
                assert (np.abs(outer.double().numpy() - want) <= tol(want)).all(), (tag, skip, steps, order)
    with pytest.raises(ValueError, match="Unsupported skip_type"):
        sol.get_time_steps("cosine", t_T, t_0, 10, "cpu")
    with pytest.raises(ValueError, match="'order' must be"):
        sol.get_orders_and_timesteps_for_singlestep_solver(6, 4, "logSNR", t_T, t_0, "cpu")


with open(os.path.join(GOLD, "g18_signatures.json")) as _f:
    SIGNATURES = json.load(_f)


def _counterpart(point):
    obj = D
    for part in point.split("."):
        obj = getattr(obj, part)
    return obj


def test_the_fixture_names_every_public_entry_point():
    assert len(SIGNATURES) == 24
    assert {p.split(".")[0] for p in SIGNATURES} == {"NoiseScheduleVP", "DPM_Solver", "model_wrapper", "model_wrapper_with_classifier"}
    for name in ("NoiseScheduleVP", "DPM_Solver", "model_wrapper", "model_wrapper_with_classifier", "dpm_solver"):
        assert hasattr(P, name)                          # exported beside the samplers
    assert P.DPM_Solver is D.DPM_Solver


@pytest.mark.parametrize("point", sorted(SIGNATURES))
def test_entry_point_takes_what_the_reference_takes(point):
    compare(SIGNATURES[point], _described(_counterpart(point)))      # no deviations, no extras


def test_latent_diffusion_dpm_solver_parameters():
    got = [(p["name"], p["default"]) for p in _described(P.LatentDiffusion.dpm_solver)]
    assert got == [("self", None), ("cond", None), ("unconditional_guidance_scale", "1.0"), ("unconditional_conditioning", "None"),
                   ("classifier", "None"), ("origin_cond", "None"), ("classifier_guide_scale", "0.0"), ("predict_x0", "True"),
                   ("thresholding", "False"), ("max_val", "1.0")]
    m = P.LatentDiffusion(**P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    sol = m.dpm_solver(torch.zeros(1, 32, 8), unconditional_guidance_scale=3.0, unconditional_conditioning=torch.zeros(1, 32, 8))
    assert isinstance(sol, D.DPM_Solver) and sol.fast and sol.predict_x0 and not sol.thresholding
    assert sol.noise_schedule.total_N == 1000 and sol.model.guidance_type == "classifier-free"
    # the fast route is the bound apply_model and nothing else
    wrapped = lambda x, t, c: m.apply_model(x, t, c)
    ns = sol.noise_schedule
    assert not D.DPM_Solver(D.model_wrapper(wrapped, ns, guidance_type="classifier-free", condition=torch.zeros(1, 32, 8)), ns).fast
    assert D.DPM_Solver(D.model_wrapper(m.apply_model, ns, guidance_type="classifier-free", condition=torch.zeros(1, 32, 8)), ns).fast
    assert not D.DPM_Solver(D.model_wrapper(m.apply_model, ns, model_type="v", guidance_type="classifier-free",
                                            condition=torch.zeros(1, 32, 8)), ns).fast


def test_argument_errors_have_the_reference_classes():
    ns = D.NoiseScheduleVP("linear")
    f = lambda x, t: x
    with pytest.raises(AssertionError):
        D.model_wrapper(f, ns, model_type="score")
    with pytest.raises(AssertionError):
        D.model_wrapper(f, ns, guidance_type="double-guide")              # only model_wrapper_with_classifier knows it
    with pytest.raises(AssertionError):
        D.model_wrapper_with_classifier(f, ns, guidance_type="triple")
    D.model_wrapper_with_classifier(f, ns, guidance_type="double-guide")
    with pytest.raises(NotImplementedError, match="autograd"):
        D.model_wrapper(f, ns, guidance_type="classifier", classifier_fn=lambda x, t, c: x)
    with pytest.raises(NotImplementedError, match="autograd"):
        D.model_wrapper_with_classifier(f, ns, guidance_type="double-guide", classifier=lambda x, t, video_feat: x)
    sol = D.DPM_Solver(f, ns)
    x = torch.zeros(2, 4, 4, 4)
    with pytest.raises(AssertionError):
        sol.sample(x, steps=2, order=3, method="multistep")                 # steps >= order
    for steps in (4, 6, 14):
        with pytest.raises(ValueError, match=r"lower_order_final=False or steps >= 15"):
            sol.sample(x, steps=steps, order=3, method="multistep")
    with pytest.raises(ValueError, match="Unsupported skip_type"):
        sol.sample(x, steps=6, order=2, method="multistep", skip_type="uniform")
    with pytest.raises(ValueError, match="Unsupported skip_type"):
        sol.sample(x, steps=6, order=2, method="singlestep", skip_type="uniform")
    with pytest.raises(ValueError, match="'order' must be"):
        sol.sample(x, steps=6, order=4, method="singlestep", skip_type="logSNR")
    with pytest.raises(ValueError, match="order must be 2 or 3"):
        sol.sample(x, order=1, method="adaptive")
    with pytest.raises(ValueError, match="Unsupported method"):
        sol.sample(x, method="euler")
    for call in (lambda: sol.singlestep_dpm_solver_second_update(x, 0.5, 0.4, solver_type="heun"),
                 lambda: sol.singlestep_dpm_solver_third_update(x, 0.5, 0.4, solver_type="heun"),
                 lambda: sol.multistep_dpm_solver_second_update(x, [x, x], [0.6, 0.5], 0.4, solver_type="heun")):
        with pytest.raises(ValueError, match="'solver_type' must be either"):
            call()
    with pytest.raises(ValueError, match="Solver order must be 1 or 2 or 3"):
        sol.singlestep_dpm_solver_update(x, 0.5, 0.4, 4)
    with pytest.raises(ValueError, match="Solver order must be 1 or 2 or 3"):
        sol.multistep_dpm_solver_update(x, [x], [0.5], 0.4, 0)
    with pytest.raises(ValueError, match="history of two"):
        sol.multistep_dpm_solver_second_update(x, [x, x, x], [0.7, 0.6, 0.5], 0.4)
    with pytest.raises(TypeError):
        D.DPM_Solver(f, object())


def test_times_are_host_scalars_and_unequal_entries_are_refused():
    assert D._scalar(0.25) == np.float32(0.25) and isinstance(D._scalar(0.25), np.float32)
    assert D._scalar(torch.tensor(0.3)) == np.float32(0.3)
    assert D._scalar(torch.full((5,), 0.7)) == np.float32(0.7)
    assert D._scalar(np.full((2,), 0.7, dtype=np.float32)) == np.float32(0.7)
    with pytest.raises(ValueError, match="must be equal"):
        D._scalar(torch.tensor([0.5, 0.5, 0.4]))
    with pytest.raises(ValueError, match="empty"):
        D._scalar(torch.zeros(0))
    sol = D.DPM_Solver(lambda x, t: x, D.NoiseScheduleVP("linear"))
    with pytest.raises(ValueError, match="must be equal"):
        sol.dpm_solver_first_update(torch.zeros(2, 3), torch.tensor([0.5, 0.6]), torch.tensor([0.4, 0.4]), model_s=torch.zeros(2, 3))


def test_singlestep_plan_knows_every_time_before_the_loop():
    """The times the fast route hoists: s, s1, s2 of every singlestep step, from the same host arithmetic the updates use."""
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=schedule.register_schedule(0.00085, 0.0120, 1000)["alphas_cumprod"])
    sol = D.DPM_Solver(lambda x, t: x, ns)
    for skip in ("logSNR", "time_uniform", "time_quadratic"):
        plan = sol._singlestep_plan(15, 3, skip, 1.0, 1e-3, fixed=False)
        assert [p[2] for p in plan] == [3, 3, 3, 3, 2, 1]
        times = []
        for s, t, o, r1, r2 in plan:
            inner = [v for v in sol._inner_times(s, t, r1, r2) if v is not None]
            assert len(inner) == o - 1 and all(float(t) < float(v) < float(s) for v in inner)
            times += [s] + inner
        assert len(times) == 15 and times == sorted(times, reverse=True)
        assert float(plan[0][0]) == 1.0 and abs(float(plan[-1][1]) - 1e-3) < 1e-6
    plan = sol._singlestep_plan(7, 3, "logSNR", 1.0, 1e-3, fixed=True)
    assert [p[2] for p in plan] == [3, 3]


def test_new_symbols_are_in_the_header_and_in_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "df_engine.h")).read()
    src = open(os.path.join(ROOT, "diff_foley_amd", "csrc", "sources.txt")).read().split()
    assert "dpm" in src and os.path.exists(os.path.join(ROOT, "diff_foley_amd", "csrc", "dpm.hip"))
    for name in ("df_dpm_data_prediction", "df_dpm_adaptive_error"):
        assert f"int {name}(" in hdr and name in E.exported_symbols()
        for prec in ("bf16", "fp16"):
            assert hasattr(E.lib(prec), name), (name, prec)
