"""G19: every update formula of the reference's DPM-Solver (diff_foley/models/diffusion/dpm_solver/dpm_solver.py) at fp32 accuracy, with
G18's closed-form model ``a x cos(w t) + b sin(3 x)`` on the Stage-2 discrete schedule (build container only; needs the reference
checkout, see oracle/ref_import.py).

    python tests/golden/make_golden_g19.py          # about ten seconds on a CPU

Writes g19_traj_{x0,eps}.npz (``sample()``: the base matrix, the option cells and -- x0 only -- the thresholding cells) and
g19_upd_{x0,eps}_{dpm_solver,taylor}.npz (direct calls of each update method) beside this file.

Every cell runs the reference twice: in fp32, and in float64 -- ``alphas_cumprod``, ``x`` and the time vectors given as float64; the
reference keeps that dtype except for its fp32 ``t_array`` and for the time grids ``sample()`` makes itself with ``torch.linspace``.  The
closed model casts the time it is given to the latent's dtype, so that cos(w t) is a float64 value in the float64 run.  A cell records
the float64 result as float64, ``<key>__delta`` = rel-L2 of the fp32 result to it (the reference's own fp32 evaluation noise, the
yardstick of tests/test_dpm_updates_*.py) and, where the two solver types are different formulas, ``<key>__sens`` = rel-L2 of the
'taylor' float64 result to the 'dpm_solver' one (what a test has to be able to tell apart).  Order 1, the third multistep update
and denoise_to_zero_fn have one expansion and no sens.  Neither have the direct calls at (s, t) = (0.5, 0.49): that pair is there
for the cancellation in the coefficients at small h (0.05), where both expansions have the same limit and lie 2e-7 to 1.6e-5 apart,
under the 80 deltas a sens must reach.  The fp32 tensors are not stored.  Inputs are functions of the seeds and tables below, which
the tests repeat.

The direct calls take time vectors of length B, as the reference's loop passes them.  The multistep updates get the irregular history
(s + 0.13, s + 0.05, s) with model values ``model_fn(x + 0.05 rnd(SEED_HIST + j), t_j)`` at the entry j steps back (x itself at s); an
(s, t) whose history would pass t = 1 is dropped.  Each singlestep update is also called with return_intermediate=True -- x_t under
``__inter``, every intermediate under ``__inter_<name>`` -- and again with the model values it returned given back (``__given``).

method='singlestep' on 'time_uniform' / 'time_quadratic' runs under make_golden_g18.cumsum_dim0(), for the reason that file states.
method='singlestep', order=1, skip_type='logSNR' is no latent: K = 1 gives two outer times for ``steps`` orders, and the reference
raises IndexError; the class name is recorded under ``<key>__raises``.

Before it writes, the maker asserts on the reference alone: every delta <= 1e-4, every latent finite, 8 x (largest delta of the cell's
group) <= sens / 10 wherever a sens is recorded, and no (method, order, skip_type, predict_x0, solver_type) of the base matrix empty."""
import contextlib
import os

import numpy as np
import torch

import make_golden as MG
from make_golden import rnd, save
from make_golden_g18 import CLOSED, closed_model, cumsum_dim0, ref_dpm

SEED_X, SEED_HIST = 1900, 1901
SHAPE = (2, 4, 4, 8)
PAIRS = (("x0", True), ("eps", False))
SOLVERS = ("dpm_solver", "taylor")
SKIPS = ("logSNR", "time_uniform", "time_quadratic")
BASE = {          # method -> (orders, steps); all with lower_order_final=False
    "singlestep": ((1, 2, 3), (7, 20)),          # steps 7: the order-3 plan ends 3, 3, 1
    "singlestep_fixed": ((2, 3), (6, 20)),
    "multistep": ((1, 2, 3), (6, 20)),
}
RAISES = ("singlestep", 1, "logSNR")             # IndexError in the reference, for every steps > 1
OPTIONS = {       # tag -> sample() arguments, per (predict_x0, solver_type)
    "ms2_lower": dict(method="multistep", order=2, steps=6),
    "ms3_lower3": dict(method="multistep", order=3, steps=3),
    "ms3_lower16": dict(method="multistep", order=3, steps=16),
    "ms2_dz": dict(method="multistep", order=2, steps=6, denoise_to_zero=True),
    "ss3_window": dict(method="singlestep", order=3, steps=7, t_start=0.6, t_end=0.05),
}
THRESHOLDING = {  # predict_x0=True, thresholding=True
    "ms2_thr": dict(method="multistep", order=2, steps=6),
    "ss3_thr": dict(method="singlestep", order=3, steps=7, skip_type="logSNR"),
}
ST = ((1.0, 0.8), (0.5, 0.35), (0.05, 0.02), (0.5, 0.49), (0.3, 0.001))
SMALL_H = (0.5, 0.49)                             # no sens recorded there, see above
R1_SECOND = (0.5, 0.3)
R_THIRD = ((1. / 3., 2. / 3.), (0.25, 0.8))
HISTORY = (0.13, 0.05, 0.0)                       # t_prev_list = s + these
HIST_EPS = 0.05
DELTA_CAP = 1e-4
FACTOR = 8
SIZE_CAP = 397175                                 # g17_decode.npz, the largest golden before this one


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def model(x, t):
    return closed_model(x, t.to(x.dtype))


def base_key(method, order, steps, skip, solver):
    return f"{method}__{order}__{steps}__{skip}__{solver}"


def sample_ctx(kw):
    assisted = kw["method"] == "singlestep" and kw.get("skip_type", "time_uniform") != "logSNR"
    return cumsum_dim0() if assisted else contextlib.nullcontext()


class Both:
    """The reference's solver in fp32 and in float64 over the same numbers."""

    def __init__(self, RD, predict_x0, thresholding=False):
        from diff_foley_amd import schedule
        ac = schedule.register_schedule(0.00085, 0.0120, 1000)["alphas_cumprod"]
        self.sol = {dt: RD.DPM_Solver(model, RD.NoiseScheduleVP("discrete", alphas_cumprod=ac.to(dt)), predict_x0=predict_x0,
                                      thresholding=thresholding) for dt in (torch.float32, torch.float64)}

    def run(self, fn):
        """fn(solver, dtype) -> tensor or tuple of tensors; returns ([float64 results], [delta per result])."""
        with torch.no_grad():
            lo, hi = fn(self.sol[torch.float32], torch.float32), fn(self.sol[torch.float64], torch.float64)
        lo, hi = (v if isinstance(v, (tuple, list)) else (v,) for v in (lo, hi))
        for a, b in zip(lo, hi):
            assert a.dtype == torch.float32 and b.dtype == torch.float64, (a.dtype, b.dtype)
            assert torch.isfinite(a).all() and torch.isfinite(b).all()
        return list(hi), [rel(a, b) for a, b in zip(lo, hi)]


def traj_group(kw, tag_p):
    return ("traj", kw["method"], kw["order"], tag_p)


def g19_traj(RD, deltas, senses, files):
    x = rnd(SHAPE, SEED_X)
    for tag_p, px in PAIRS:
        out, cells = {}, {}
        runs = []
        for method, (orders, steps_list) in BASE.items():
            for order in orders:
                for steps in steps_list:
                    for skip in SKIPS:
                        runs.append(("{}", dict(method=method, order=order, steps=steps, skip_type=skip, lower_order_final=False), False))
        runs += [(tag + "__{}", kw, False) for tag, kw in OPTIONS.items()]
        if px:
            runs += [(tag + "__{}", kw, True) for tag, kw in THRESHOLDING.items()]
        for pattern, kw, thr in runs:
            both = Both(RD, px, thresholding=thr)
            z = {}
            for solver in SOLVERS:
                key = pattern.format(base_key(kw["method"], kw["order"], kw["steps"], kw["skip_type"], solver)) if pattern == "{}" \
                    else pattern.format(solver)
                call = lambda sol, dt: sol.sample(x.to(dt), solver_type=solver, **kw)
                with sample_ctx(kw):
                    if (kw["method"], kw["order"], kw.get("skip_type")) == RAISES:
                        try:
                            both.run(call)
                            raise AssertionError(f"{key}: the reference was expected to raise")
                        except IndexError as e:
                            out[key + "__raises"] = np.frombuffer(type(e).__name__.encode(), dtype=np.uint8)
                        continue
                    (z[solver],), (d,) = both.run(call)
                out[key], out[key + "__delta"] = z[solver], np.float64(d)
                deltas.setdefault(traj_group(kw, tag_p), []).append(d)
                cells[key] = (kw, solver)
            if z and kw["order"] > 1:
                s = rel(z["taylor"], z["dpm_solver"])
                for solver in SOLVERS:
                    key = pattern.format(base_key(kw["method"], kw["order"], kw["steps"], kw["skip_type"], solver)) if pattern == "{}" \
                        else pattern.format(solver)
                    out[key + "__sens"] = np.float64(s)
                    senses.append((traj_group(kw, tag_p), f"{tag_p} {key}", s))
        for method, (orders, _) in BASE.items():      # no combination of the base matrix is empty
            for order in orders:
                for skip in SKIPS:
                    for solver in SOLVERS:
                        have = [k for k, (kw, sv) in cells.items() if (kw["method"], kw["order"], kw.get("skip_type"), sv) == (method, order, skip, solver)
                                and "lower_order_final" in kw]
                        assert have or (method, order, skip) == RAISES, (method, order, skip, tag_p, solver)
        files[f"g19_traj_{tag_p}.npz"] = out


def vec(v, dt):
    return torch.full((SHAPE[0],), v, dtype=dt)


def history(sol, x, s, dt, n):
    ts = [vec(s + d, dt) for d in HISTORY[-n:]]
    back = range(n - 1, -1, -1)                   # steps back from s: the last entry is x itself at s
    xs = [x.to(dt) + HIST_EPS * rnd(SHAPE, SEED_HIST + j).to(dt) if j else x.to(dt) for j in back]
    return [sol.model_fn(xk, tk) for xk, tk in zip(xs, ts)], ts


def g19_updates(RD, deltas, senses, files):
    x = rnd(SHAPE, SEED_X)
    two_formulas = set()
    results = {}
    for tag_p, px in PAIRS:
        both = Both(RD, px)
        for solver in SOLVERS:
            out = {}

            def put(group, key, names, fn, sens=True):
                zs, ds = both.run(fn)
                assert len(zs) == len(names)
                for name, z, d in zip(names, zs, ds):
                    k = key + ("" if name is None else "__" + name)
                    out[k], out[k + "__delta"] = z, np.float64(d)
                    deltas.setdefault(("upd", group), []).append(d)
                    if sens and name is None and (s, t) != SMALL_H:
                        two_formulas.add((group, k))
            for s, t in ST:
                st = f"{s}__{t}"
                put("dpm_solver_first_update", f"first__{st}", [None],
                    lambda sol, dt: sol.dpm_solver_first_update(x.to(dt), vec(s, dt), vec(t, dt)), sens=False)
                for r1 in R1_SECOND:
                    put("singlestep_dpm_solver_second_update", f"second__{st}__r{r1}", [None],
                        lambda sol, dt: sol.singlestep_dpm_solver_second_update(x.to(dt), vec(s, dt), vec(t, dt), r1=r1, solver_type=solver))
                for k, (r1, r2) in enumerate(R_THIRD):
                    put("singlestep_dpm_solver_third_update", f"third__{st}__r{k}", [None],
                        lambda sol, dt: sol.singlestep_dpm_solver_third_update(x.to(dt), vec(s, dt), vec(t, dt), r1=r1, r2=r2,
                                                                               solver_type=solver))

                def with_intermediates(name, n_inter, **kw):
                    names = ["model_s", "model_s1", "model_s2"][:n_inter]

                    def fn(sol, dt):
                        z, inter = getattr(sol, name)(x.to(dt), vec(s, dt), vec(t, dt), return_intermediate=True, **kw)
                        assert list(inter) == names, (name, list(inter))
                        given = {k: inter[k] for k in names[:max(1, n_inter - 1)]}          # model_s (and model_s1 for the third)
                        z2 = getattr(sol, name)(x.to(dt), vec(s, dt), vec(t, dt), **given, **kw)
                        return (z, z2) + tuple(inter[k] for k in names)
                    return ["inter", "given"] + ["inter_" + k for k in names], fn
                for name, short, n_inter, kw in (("dpm_solver_first_update", "first", 1, {}),
                                                 ("singlestep_dpm_solver_second_update", "second", 2, dict(solver_type=solver)),
                                                 ("singlestep_dpm_solver_third_update", "third", 3, dict(solver_type=solver))):
                    names, fn = with_intermediates(name, n_inter, **kw)
                    put(name, f"{short}__{st}", names, fn, sens=False)
                if s + HISTORY[0] <= 1.0:
                    def ms(n, name):
                        def fn(sol, dt):
                            ms_, ts = history(sol, x, s, dt, n)
                            return getattr(sol, name)(x.to(dt), ms_, ts, vec(t, dt), solver_type=solver)
                        return fn
                    put("multistep_dpm_solver_second_update", f"ms2__{st}", [None], ms(2, "multistep_dpm_solver_second_update"))
                    put("multistep_dpm_solver_third_update", f"ms3__{st}", [None], ms(3, "multistep_dpm_solver_third_update"),
                        sens=False)
                put("denoise_to_zero_fn", f"dz__{s}", [None], lambda sol, dt: sol.denoise_to_zero_fn(x.to(dt), vec(s, dt)), sens=False)
            results[(tag_p, solver)] = out
    for tag_p, _ in PAIRS:
        a, b = results[(tag_p, "dpm_solver")], results[(tag_p, "taylor")]
        for group, k in sorted(two_formulas):
            s = rel(b[k], a[k])
            a[k + "__sens"] = b[k + "__sens"] = np.float64(s)
            senses.append((("upd", group), f"{tag_p} {k}", s))
        for solver in SOLVERS:
            files[f"g19_upd_{tag_p}_{solver}.npz"] = results[(tag_p, solver)]


if __name__ == "__main__":
    assert MG.HERE == os.path.dirname(os.path.abspath(__file__))
    assert CLOSED == dict(a=1.6, w=12.0, b=0.4)
    RD = ref_dpm()
    deltas, senses, files = {}, [], {}
    g19_traj(RD, deltas, senses, files)
    g19_updates(RD, deltas, senses, files)
    worst = {g: max(v) for g, v in deltas.items()}
    for g in sorted(worst, key=str):
        print(f"group {g}: {len(deltas[g])} records, delta {min(deltas[g]):.2e} ... {worst[g]:.2e}")
    bad = []
    for g, name, s in senses:
        ratio = s / (10 * FACTOR * worst[g])
        if ratio < 1:
            bad.append((name, s, worst[g]))
    weakest = min(senses, key=lambda e: e[2] / worst[e[0]])
    print(f"{len(senses)} sens records; weakest {weakest[1]}: sens {weakest[2]:.2e} against group delta {worst[weakest[0]]:.2e}")
    assert max(worst.values()) <= DELTA_CAP, max(worst.values())
    assert not bad, bad
    for name, out in files.items():
        save(name, **out)
    for f in sorted(os.listdir(MG.HERE)):
        if f.startswith("g19_") and f.endswith(".npz"):
            assert os.path.getsize(os.path.join(MG.HERE, f)) <= SIZE_CAP, f
