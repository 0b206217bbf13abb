"""G18: the reference's DPM-Solver family (diff_foley/models/diffusion/dpm_solver/dpm_solver.py) -- schedule functions, step grids,
final latents of the fixed-step methods on the tiny model of the other goldens, and the adaptive solver step by step (build container
only; needs the reference checkout, see oracle/ref_import.py).

    python tests/golden/make_golden_g18.py          # about a minute on a CPU

Writes g18_schedule.npz, g18_latents_x0.npz, g18_latents_eps.npz, g18_adaptive.npz and g18_signatures.json beside this file.  The
models, seeded weights and helpers are make_golden.py's and make_golden_g17.py's, imported, not restated.  Inputs that a test can
regenerate from a seed are not stored; the seeds and the case tables are the constants below and the tests repeat them.

One line of the reference needs help to run at all: get_orders_and_timesteps_for_singlestep_solver calls ``torch.cumsum`` without
``dim`` (dpm_solver.py:495), so method='singlestep' raises TypeError on every skip_type but 'logSNR' -- on the docstring's own
recommended call.  The 'time_uniform' / 'time_quadratic' singlestep records below are made with ``torch.cumsum`` given ``dim=0`` for
the duration of the call -- the evident intent -- and nothing else changed.

The adaptive records (c) use a closed-form fp32 model, so that the decision sequence is a property of the solver's arithmetic and not
of a UNet's operand type; every error estimate E, decision and tried time is recorded through the solver's own calls (the lower-order
update is entered once per attempt with the tried time, torch.float_power once per attempt with E).  The maker asserts that no
recorded E lies within 0.02 of 1, the acceptance threshold."""
import contextlib
import inspect
import io
import json
import os

import numpy as np
import torch

import make_golden as MG
from make_golden import HERE, ref_import, rnd, save, synth
from make_golden_g17 import SHAPE, tiny_model

SEED_LATENT, SEED_FEATS, SEED_VF, SEED_CLOSED = 1810, 1234, 4321, 1800
B = 2
SCALE = 3.0
CLS_SCALE = 50.0
CLOSED_SHAPE = (3, 4, 8, 8)
CLOSED = dict(a=1.6, w=12.0, b=0.4)         # model(x, t) = a x cos(w t) + b sin(3 x); chosen on the CPU, see g18_adaptive()

FIXED_CASES = {          # tag -> sample() arguments; each with predict_x0 True ("x0") and False ("eps")
    "ss3_logsnr": dict(steps=7, order=3, method="singlestep", skip_type="logSNR"),
    "ss3_logsnr_taylor": dict(steps=8, order=3, method="singlestep", skip_type="logSNR", solver_type="taylor"),
    "ms3_nolower": dict(steps=6, order=3, method="multistep", lower_order_final=False),
    "ms3_15": dict(steps=15, order=3, method="multistep"),
    "sf2_logsnr": dict(steps=6, order=2, method="singlestep_fixed", skip_type="logSNR"),
    "sf2_quad_taylor": dict(steps=5, order=2, method="singlestep_fixed", skip_type="time_quadratic", solver_type="taylor"),
    "ss3_uniform": dict(steps=7, order=3, method="singlestep", skip_type="time_uniform"),      # the assisted line, see above
}
X0_ONLY_CASES = {        # predict_x0 True only
    "ms2_thr_dz": dict(steps=6, order=2, method="multistep", denoise_to_zero=True),            # thresholding=True
    "ms2_tstart": dict(steps=6, order=2, method="multistep", t_start=0.6),
    "ms2_double": dict(steps=6, order=2, method="multistep"),                                  # guidance_type='double-guide'
}


@contextlib.contextmanager
def cumsum_dim0():
    plain = torch.cumsum
    torch.cumsum = lambda t, *a, **k: plain(t, *a, **k) if (a or "dim" in k) else plain(t, dim=0)
    try:
        yield
    finally:
        torch.cumsum = plain


def ref_dpm():
    ref_import.import_reference()
    import diff_foley.models.diffusion.dpm_solver.dpm_solver as RD
    return RD


def time_grid(N, T):
    knots = [1, 2, 3, 37, 500, N - 1, N]
    t = [k / N for k in knots] + [(k + 0.5) / N for k in (1, 2, 37, 500, N - 2)] + [0.0123456, 0.2, 0.4567, 0.9]
    return torch.tensor(sorted(v for v in t if v <= T), dtype=torch.float32)


def g18_schedule():
    RD = ref_dpm()
    from diff_foley_amd import schedule
    tab = schedule.register_schedule(0.00085, 0.0120, 1000)
    betas10 = torch.linspace(1e-3, 0.3, 10)
    scheds = {"discrete": RD.NoiseScheduleVP("discrete", alphas_cumprod=tab["alphas_cumprod"]),
              "betas10": RD.NoiseScheduleVP("discrete", betas=betas10),
              "linear": RD.NoiseScheduleVP("linear"), "cosine": RD.NoiseScheduleVP("cosine")}
    out = {"betas10": betas10}
    for tag, ns in scheds.items():
        t = time_grid(ns.total_N if tag != "betas10" else 10, ns.T)
        out[f"{tag}__t"] = t
        out[f"{tag}__T"], out[f"{tag}__total_N"] = np.float64(ns.T), np.int64(ns.total_N)
        for name in ("marginal_log_mean_coeff", "marginal_alpha", "marginal_std", "marginal_lambda"):
            out[f"{tag}__{name}"] = getattr(ns, name)(t)
        out[f"{tag}__inverse_lambda"] = ns.inverse_lambda(ns.marginal_lambda(t))      # the round trip
    for tag in ("discrete", "linear", "cosine"):
        ns = scheds[tag]
        sol = RD.DPM_Solver(lambda x, t: x, ns)
        t_0, t_T = 1. / ns.total_N, ns.T
        for skip in ("logSNR", "time_uniform", "time_quadratic"):
            out[f"{tag}__steps__{skip}"] = sol.get_time_steps(skip, t_T, t_0, 10, "cpu")
            for steps in range(1, 11):
                for order in (1, 2, 3):
                    with cumsum_dim0():
                        outer, orders = sol.get_orders_and_timesteps_for_singlestep_solver(steps, order, skip, t_T, t_0, "cpu")
                    out[f"{tag}__outer__{skip}__{steps}__{order}"] = outer
                    out[f"{tag}__orders__{skip}__{steps}__{order}"] = np.asarray(orders)
    save("g18_schedule.npz", **out)


def _inputs(model):
    x = rnd((B,) + SHAPE, SEED_LATENT)
    with torch.no_grad():
        c = model.get_learned_conditioning(synth.synthetic_cavp(B, 32, 64, seed=SEED_FEATS))
    return x, c, torch.zeros_like(c)


def _solver(RD, model, c, uc, predict_x0, thresholding=False, double=None):
    ns = RD.NoiseScheduleVP("discrete", alphas_cumprod=model.alphas_cumprod)
    apply = lambda x, t, cond: model.apply_model(x, t, cond)
    if double is None:
        fn = RD.model_wrapper(apply, ns, model_type="noise", guidance_type="classifier-free", condition=c, unconditional_condition=uc,
                              guidance_scale=SCALE)
    else:
        cls, vf = double
        fn = RD.model_wrapper_with_classifier(apply, ns, model_type="noise", guidance_type="double-guide", condition=c, origin_cond=vf,
                                              unconditional_condition=uc, guidance_scale=SCALE, classifier=cls,
                                              classifier_guide_scale=CLS_SCALE)
    return RD.DPM_Solver(fn, ns, predict_x0=predict_x0, thresholding=thresholding)


def g18_latents():
    RD = ref_dpm()
    model, _ = tiny_model()
    x, c, uc = _inputs(model)
    cls = ref_import.build_reference_classifier(dict(synth.CLS_TINY), synth.make_state_dict(synth.classifier_spec(synth.CLS_TINY), 0))
    wrap = lambda xx, t, video_feat: cls(xx, context=video_feat, timesteps=t)
    vf = synth.synthetic_cavp(B, 33, 64, seed=SEED_VF)
    for tag_p, px in (("x0", True), ("eps", False)):
        out = {}
        for tag, kw in FIXED_CASES.items():
            with cumsum_dim0() if tag == "ss3_uniform" else contextlib.nullcontext(), torch.no_grad():
                z = _solver(RD, model, c, uc, px).sample(x.clone(), **kw)
            assert torch.isfinite(z).all(), tag
            out[tag] = z
        if px:
          with torch.no_grad():
            z = _solver(RD, model, c, uc, True, thresholding=True).sample(x.clone(), **X0_ONLY_CASES["ms2_thr_dz"])
            assert float(z.abs().max()) <= 1.0
            out["ms2_thr_dz"] = z
            out["ms2_tstart"] = _solver(RD, model, c, uc, True).sample(x.clone(), **X0_ONLY_CASES["ms2_tstart"])
            out["ms2_double"] = _solver(RD, model, c, uc, True, double=(wrap, vf)).sample(x.clone(), **X0_ONLY_CASES["ms2_double"])
        save(f"g18_latents_{tag_p}.npz", **out)


def closed_model(x, t):
    return CLOSED["a"] * x * torch.cos(CLOSED["w"] * t)[:, None, None, None] + CLOSED["b"] * torch.sin(3 * x)


def _traced_adaptive(RD, sol, x, order, **kw):
    """dpm_solver_adaptive with every attempt's (t, E) recorded through the solver's own calls."""
    ts, Es = [], []
    name = "dpm_solver_first_update" if order == 2 else "singlestep_dpm_solver_second_update"
    plain_update, plain_pow = getattr(sol, name), torch.float_power

    def update(x_, s, t, *a, **k):
        if k.get("return_intermediate"):          # the lower-order update: entered once per attempt
            ts.append(float(t[0]))
        return plain_update(x_, s, t, *a, **k)
    setattr(sol, name, update)
    torch.float_power = lambda E, p: (Es.append(float(E)), plain_pow(E, p))[1]
    try:
        with contextlib.redirect_stdout(io.StringIO()) as said:
            z = sol.dpm_solver_adaptive(x, order=order, **kw)
    finally:
        torch.float_power = plain_pow
        delattr(sol, name)
    assert len(ts) == len(Es)
    return z, np.asarray(ts, dtype=np.float64), np.asarray(Es, dtype=np.float64), said.getvalue()


def g18_adaptive():
    RD = ref_dpm()
    out = {}
    # (c) the closed-form model on the Stage-2 schedule
    from diff_foley_amd import schedule
    ns = RD.NoiseScheduleVP("discrete", alphas_cumprod=schedule.register_schedule(0.00085, 0.0120, 1000)["alphas_cumprod"])
    x = rnd(CLOSED_SHAPE, SEED_CLOSED)
    for order in (2, 3):
        for tag_p, px in (("x0", True), ("eps", False)):
            sol = RD.DPM_Solver(closed_model, ns, predict_x0=px)
            z, ts, Es, said = _traced_adaptive(RD, sol, x.clone(), order, t_T=1.0, t_0=1e-3)
            acc = Es <= 1.0
            margin = float(np.abs(Es - 1.0).min())
            print(f"closed order {order} {tag_p}: {len(Es)} attempts, {int((~acc).sum())} rejected, max E {Es.max():.3f}, "
                  f"min |E - 1| {margin:.3f}; said {said.strip()!r}")
            assert acc.any() and (~acc).any(), "the reference must both accept and reject steps"
            assert margin >= 0.02, margin
            assert torch.isfinite(z).all()
            k = f"closed__{order}__{tag_p}"
            out[k + "__z"], out[k + "__t"], out[k + "__E"], out[k + "__accepted"] = z, ts, Es, acc
            out[k + "__said"] = np.frombuffer(said.encode(), dtype=np.uint8)
    # (d) the tiny UNet at default tolerances, and the solver's sensitivity to its own step sequence
    model, _ = tiny_model()
    xT, c, uc = _inputs(model)
    for order in (2, 3):
        with torch.no_grad():
            z, ts, Es, _ = _traced_adaptive(RD, _solver(RD, model, c, uc, True), xT.clone(), order, t_T=1.0, t_0=1e-3)
            z4, _, _, _ = _traced_adaptive(RD, _solver(RD, model, c, uc, True), xT.clone(), order, t_T=1.0, t_0=1e-3, h_init=0.04)
        d_ref = float((z4.double() - z.double()).norm() / z.double().norm())
        print(f"unet order {order}: {len(Es)} attempts, {int((Es > 1).sum())} rejected, max E {Es.max():.3f}, d_ref {d_ref:.3e}")
        out[f"unet__{order}__z"], out[f"unet__{order}__d_ref"], out[f"unet__{order}__attempts"] = z, np.float64(d_ref), np.int64(len(Es))
    save("g18_adaptive.npz", **out)


def g18_signatures():
    RD = ref_dpm()
    NS, DS = RD.NoiseScheduleVP, RD.DPM_Solver
    points = {"NoiseScheduleVP.__init__": NS.__init__, "model_wrapper": RD.model_wrapper,
              "model_wrapper_with_classifier": RD.model_wrapper_with_classifier, "DPM_Solver.__init__": DS.__init__}
    for name in ("marginal_log_mean_coeff", "marginal_alpha", "marginal_std", "marginal_lambda", "inverse_lambda"):
        points["NoiseScheduleVP." + name] = getattr(NS, name)
    for name in ("noise_prediction_fn", "data_prediction_fn", "model_fn", "get_time_steps", "get_orders_and_timesteps_for_singlestep_solver",
                 "denoise_to_zero_fn", "dpm_solver_first_update", "singlestep_dpm_solver_second_update",
                 "singlestep_dpm_solver_third_update", "multistep_dpm_solver_second_update", "multistep_dpm_solver_third_update",
                 "singlestep_dpm_solver_update", "multistep_dpm_solver_update", "dpm_solver_adaptive", "sample"):
        points["DPM_Solver." + name] = getattr(DS, name)
    out = {name: [dict(name=p.name, kind=p.kind.name, default=None if p.default is inspect.Parameter.empty else repr(p.default))
                  for p in inspect.signature(fn).parameters.values()] for name, fn in points.items()}
    path = os.path.join(HERE, "g18_signatures.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote g18_signatures.json: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    assert MG.HERE == os.path.dirname(os.path.abspath(__file__))
    g18_schedule()
    g18_latents()
    g18_adaptive()
    g18_signatures()
