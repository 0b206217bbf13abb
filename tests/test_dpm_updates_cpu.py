"""CPU: every update formula of diff_foley_amd.dpm_solver against the reference at fp32 accuracy (golden G19,
tests/golden/make_golden_g19.py), and the golden itself.

dpm_solver.py re-derives the reference's updates so that each is one ``df_lincomb`` over host fp32 coefficients.  Here ``engine.lincomb``
is replaced by a plain fp32 torch sum of ``coef * tensor``; with thresholding off nothing else in the solver needs the device, so the
whole host algebra -- times, coefficients, merged terms, histories -- runs on CPU tensors through the generic route with G18's closed
model ``1.6 x cos(12 t) + 0.4 sin(3 x)``.  tests/test_dpm_updates_gpu.py runs the same cells through the kernels.

The bound.  The yardstick is the reference, never the product: each cell records the reference's float64 result and ``delta``, the
rel-L2 of the reference's own fp32 run to it.  A cell passes when the product's rel-L2 to the float64 record is at most
8 x (largest delta of the cell's group); a group is (method, order, predict_x0) for ``sample()`` and the update method for direct
calls.  The group maximum, because one cell's delta is a single draw of fp32 evaluation noise (2e-7 ... 3e-5 across neighbouring
cells); 8 is the factor of tests/test_norm_forms_gpu.py against the same kind of yardstick.

Power.  Wherever the two solver types are different formulas the golden records ``sens``, their rel-L2 distance in float64 (at least
80 group deltas, the maker asserts it); the product run with the OTHER solver type must miss the record by more than the bound."""
import os

import numpy as np
import pytest
import torch

from diff_foley_amd import dpm_solver as D, engine as E, schedule
from helpers import GOLD, gold, rel_l2, rnd

SEED_X, SEED_HIST = 1900, 1901                    # tests/golden/make_golden_g19.py
SHAPE = (2, 4, 4, 8)
CLOSED = dict(a=1.6, w=12.0, b=0.4)
PAIRS = (("x0", True), ("eps", False))
SOLVERS = ("dpm_solver", "taylor")
SKIPS = ("logSNR", "time_uniform", "time_quadratic")
BASE = {
    "singlestep": ((1, 2, 3), (7, 20)),
    "singlestep_fixed": ((2, 3), (6, 20)),
    "multistep": ((1, 2, 3), (6, 20)),
}
RAISES = ("singlestep", 1, "logSNR")
OPTIONS = {
    "ms2_lower": dict(method="multistep", order=2, steps=6),
    "ms3_lower3": dict(method="multistep", order=3, steps=3),
    "ms3_lower16": dict(method="multistep", order=3, steps=16),
    "ms2_dz": dict(method="multistep", order=2, steps=6, denoise_to_zero=True),
    "ss3_window": dict(method="singlestep", order=3, steps=7, t_start=0.6, t_end=0.05),
}
THRESHOLDING = {
    "ms2_thr": dict(method="multistep", order=2, steps=6),
    "ss3_thr": dict(method="singlestep", order=3, steps=7, skip_type="logSNR"),
}
ST = ((1.0, 0.8), (0.5, 0.35), (0.05, 0.02), (0.5, 0.49), (0.3, 0.001))
SMALL_H = (0.5, 0.49)
R1_SECOND = (0.5, 0.3)
R_THIRD = ((1. / 3., 2. / 3.), (0.25, 0.8))
HISTORY = (0.13, 0.05, 0.0)
HIST_EPS = 0.05
DELTA_CAP = 1e-4
FACTOR = 8
SIZE_CAP = 397175
FILES = ["g19_traj_x0.npz", "g19_traj_eps.npz"] + [f"g19_upd_{p}_{s}.npz" for p, _ in PAIRS for s in SOLVERS]
METHOD_ORDERS = [(m, o) for m, (orders, _) in BASE.items() for o in orders]
UPDATE_GROUPS = {"first": "dpm_solver_first_update", "second": "singlestep_dpm_solver_second_update",
                 "third": "singlestep_dpm_solver_third_update", "ms2": "multistep_dpm_solver_second_update",
                 "ms3": "multistep_dpm_solver_third_update", "dz": "denoise_to_zero_fn"}
INTERMEDIATES = {"first": ["model_s"], "second": ["model_s", "model_s1"], "third": ["model_s", "model_s1", "model_s2"]}


def closed_model(x, t):
    return CLOSED["a"] * x * torch.cos(CLOSED["w"] * t)[:, None, None, None] + CLOSED["b"] * torch.sin(3 * x)


def torch_lincomb(terms, out=None):
    """engine.lincomb in plain fp32 torch: the sum of coef * tensor, left to right."""
    acc = None
    for c, t in terms:
        assert t.dtype == torch.float32
        term = float(np.float32(c)) * t
        acc = term if acc is None else acc + term
    if out is not None:
        out.copy_(acc)
        return out
    return acc


def solver(px, thresholding=False):
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=schedule.register_schedule(0.00085, 0.0120, 1000)["alphas_cumprod"])
    return D.DPM_Solver(closed_model, ns, predict_x0=px, thresholding=thresholding)


# ---------------------------------------------------------------------- the case tables, as the maker builds them
def base_key(method, order, steps, skip, solver_type):
    return f"{method}__{order}__{steps}__{skip}__{solver_type}"


def traj_cells(method=None, order=None, thresholding=False):
    """(key, sample() arguments, solver_type, raises) of every trajectory cell of one predict_x0: the base matrix and the option
    cells, or the thresholding cells."""
    for tag, kw in (THRESHOLDING if thresholding else OPTIONS).items():
        if (method, order) in ((None, None), (kw["method"], kw["order"])):
            for s in SOLVERS:
                yield f"{tag}__{s}", kw, s, False
    if thresholding:
        return
    for m, (orders, steps_list) in BASE.items():
        for o in orders:
            if (method, order) not in ((None, None), (m, o)):
                continue
            for steps in steps_list:
                for skip in SKIPS:
                    for s in SOLVERS:
                        yield (base_key(m, o, steps, skip, s), dict(method=m, order=o, steps=steps, skip_type=skip, lower_order_final=False),
                               s, (m, o, skip) == RAISES)


def update_keys():
    """key -> update method of every direct-call record of one (predict_x0, solver_type) file."""
    keys = {}
    for s, t in ST:
        st = f"{s}__{t}"
        keys[f"first__{st}"] = "first"
        for r1 in R1_SECOND:
            keys[f"second__{st}__r{r1}"] = "second"
        for k in range(len(R_THIRD)):
            keys[f"third__{st}__r{k}"] = "third"
        for short, names in INTERMEDIATES.items():
            for name in ["inter", "given"] + ["inter_" + n for n in names]:
                keys[f"{short}__{st}__{name}"] = short
        if s + HISTORY[0] <= 1.0:
            keys[f"ms2__{st}"], keys[f"ms3__{st}"] = "ms2", "ms3"
        keys[f"dz__{s}"] = "dz"
    return keys


def has_sens(key, short):
    return short in ("second", "third", "ms2") and key.split("__")[-1] not in ("inter", "given") and "inter_" not in key \
        and f"{SMALL_H[0]}__{SMALL_H[1]}" not in key


def traj_tolerances(tag_p):
    """(method, order) -> 8 x the largest delta the golden stores for that group of this predict_x0 (thresholding cells included)."""
    g = gold(f"g19_traj_{tag_p}.npz")
    worst = {}
    for thr in (False, True) if tag_p == "x0" else (False,):
        for key, kw, _, raises in traj_cells(thresholding=thr):
            if not raises:
                k = (kw["method"], kw["order"])
                worst[k] = max(worst.get(k, 0.0), float(g[key + "__delta"]))
    return {k: FACTOR * v for k, v in worst.items()}


def update_tolerances():
    """update method -> 8 x the largest delta over the four files."""
    worst = {}
    for tag_p, _ in PAIRS:
        for s in SOLVERS:
            g = gold(f"g19_upd_{tag_p}_{s}.npz")
            for key, short in update_keys().items():
                worst[short] = max(worst.get(short, 0.0), float(g[key + "__delta"]))
    return {k: FACTOR * v for k, v in worst.items()}


# ---------------------------------------------------------------------- running the product
def run_traj(px, kw, solver_type, device, thresholding=False):
    return solver(px, thresholding).sample(rnd(SHAPE, SEED_X).to(device), solver_type=solver_type, **kw)


def vec(v, device):
    return torch.full((SHAPE[0],), v, device=device)


def history(sol, x, s, n):
    back = range(n - 1, -1, -1)
    ts = [vec(s + d, x.device) for d in HISTORY[-n:]]
    xs = [x + HIST_EPS * rnd(SHAPE, SEED_HIST + j).to(x.device) if j else x for j in back]
    return [sol.model_fn(xk, tk) for xk, tk in zip(xs, ts)], ts


def run_updates(px, solver_type, device):
    """key -> the product's tensor for every record of update_keys(), the calls the maker makes of the reference."""
    sol = solver(px)
    x = rnd(SHAPE, SEED_X).to(device)
    out = {}
    for s, t in ST:
        st = f"{s}__{t}"
        vs, vt = vec(s, device), vec(t, device)
        out[f"first__{st}"] = sol.dpm_solver_first_update(x, vs, vt)
        for r1 in R1_SECOND:
            out[f"second__{st}__r{r1}"] = sol.singlestep_dpm_solver_second_update(x, vs, vt, r1=r1, solver_type=solver_type)
        for k, (r1, r2) in enumerate(R_THIRD):
            out[f"third__{st}__r{k}"] = sol.singlestep_dpm_solver_third_update(x, vs, vt, r1=r1, r2=r2, solver_type=solver_type)
        for short, names in INTERMEDIATES.items():
            fn = getattr(sol, UPDATE_GROUPS[short])
            kw = {} if short == "first" else dict(solver_type=solver_type)
            z, inter = fn(x, vs, vt, return_intermediate=True, **kw)
            assert list(inter) == names, (short, list(inter))          # the reference's keys, in its order
            out[f"{short}__{st}__inter"] = z
            out[f"{short}__{st}__given"] = fn(x, vs, vt, **{n: inter[n] for n in names[:max(1, len(names) - 1)]}, **kw)
            for n in names:
                out[f"{short}__{st}__inter_{n}"] = inter[n]
        if s + HISTORY[0] <= 1.0:
            ms, ts = history(sol, x, s, 2)
            out[f"ms2__{st}"] = sol.multistep_dpm_solver_second_update(x, ms, ts, vt, solver_type=solver_type)
            ms, ts = history(sol, x, s, 3)
            out[f"ms3__{st}"] = sol.multistep_dpm_solver_third_update(x, ms, ts, vt, solver_type=solver_type)
        out[f"dz__{s}"] = sol.denoise_to_zero_fn(x, vs)
    return out


def other(solver_type):
    return SOLVERS[1 - SOLVERS.index(solver_type)]


def check_traj_group(method, order, device, where, power=True):
    """Every base and option cell of (method, order), both predictions; returns the largest err / tolerance."""
    ratios = []
    for tag_p, px in PAIRS:
        g, tol = gold(f"g19_traj_{tag_p}.npz"), traj_tolerances(tag_p)[(method, order)]
        worst = 0.0
        for key, kw, solver_type, raises in traj_cells(method, order):
            if raises:
                with pytest.raises(IndexError):
                    run_traj(px, kw, solver_type, device)
                continue
            z = run_traj(px, kw, solver_type, device)
            assert z.dtype == torch.float32 and z.shape == SHAPE
            err = rel_l2(z.cpu(), g[key])
            worst = max(worst, err / tol)
            assert err <= tol, (where, tag_p, key, err, tol)
            if power and key + "__sens" in g:
                miss = rel_l2(run_traj(px, kw, other(solver_type), device).cpu(), g[key])
                assert miss > tol, (where, tag_p, key, "the other solver type passes", miss, tol)
        print(f"dpm updates {where} {method} order {order} {tag_p}: worst err / tolerance {worst:.3f} (tolerance {tol:.2e})")
        ratios.append(worst)
    return max(ratios)


def check_update_files(device, where, power=True):
    tol = update_tolerances()
    worst = {}
    for tag_p, px in PAIRS:
        for solver_type in SOLVERS:
            g = gold(f"g19_upd_{tag_p}_{solver_type}.npz")
            got = run_updates(px, solver_type, device)
            wrong = run_updates(px, other(solver_type), device) if power else None
            keys = update_keys()
            assert sorted(got) == sorted(keys)
            for key, short in keys.items():
                err = rel_l2(got[key].cpu(), g[key])
                worst[short] = max(worst.get(short, 0.0), err / tol[short])
                assert err <= tol[short], (where, tag_p, solver_type, key, err, tol[short])
                if power and key + "__sens" in g:
                    miss = rel_l2(wrong[key].cpu(), g[key])
                    assert miss > tol[short], (where, tag_p, solver_type, key, "the other solver type passes", miss, tol[short])
    for short, w in worst.items():
        print(f"dpm updates {where} {UPDATE_GROUPS[short]}: worst err / tolerance {w:.3f} (tolerance {tol[short]:.2e})")
    return worst


# ---------------------------------------------------------------------- the golden itself
def test_golden_holds_every_cell_and_its_caps():
    for f in FILES:
        assert os.path.getsize(os.path.join(GOLD, f)) <= SIZE_CAP, f
    n_sens = 0
    for tag_p, _ in PAIRS:
        g = gold(f"g19_traj_{tag_p}.npz")
        want, groups = set(), {}
        for thr in (False, True) if tag_p == "x0" else (False,):
            for key, kw, solver_type, raises in traj_cells(thresholding=thr):
                if raises:
                    assert bytes(g[key + "__raises"].numpy()).decode() == "IndexError"
                    want.add(key + "__raises")
                    continue
                z, d = g[key], float(g[key + "__delta"])
                assert z.dtype == torch.float64 and tuple(z.shape) == SHAPE and bool(torch.isfinite(z).all()), key
                assert 0 < d <= DELTA_CAP, (key, d)
                want |= {key, key + "__delta"}
                groups.setdefault((kw["method"], kw["order"]), []).append(key)
                if kw["order"] > 1:              # the two solver types are different formulas from order 2 on
                    sens = float(g[key + "__sens"])
                    stem = key[:-len(solver_type)]          # taylor against dpm_solver, whichever of the two this cell is
                    assert sens == float(g[stem + other(solver_type) + "__sens"])
                    assert abs(sens - rel_l2(g[stem + "taylor"], g[stem + "dpm_solver"])) <= 1e-9 * sens
                    want.add(key + "__sens")
                    n_sens += 1
        assert set(g) == want, sorted(set(g) ^ want)[:8]
        tol = traj_tolerances(tag_p)
        for (m, o), keys in groups.items():
            for key in keys:
                if key + "__sens" in g:
                    assert tol[(m, o)] <= float(g[key + "__sens"]) / 10, (tag_p, key)
        for m, (orders, _) in BASE.items():      # no combination of the base matrix is empty
            for o in orders:
                for skip in SKIPS:
                    for s in SOLVERS:
                        assert (m, o, skip) == RAISES or any(f"{m}__{o}__" in k and f"__{skip}__{s}" in k for k in groups[(m, o)])
    tol = update_tolerances()
    for tag_p, _ in PAIRS:
        for s in SOLVERS:
            g = gold(f"g19_upd_{tag_p}_{s}.npz")
            want = set()
            for key, short in update_keys().items():
                z, d = g[key], float(g[key + "__delta"])
                assert z.dtype == torch.float64 and tuple(z.shape) == SHAPE and bool(torch.isfinite(z).all()), key
                assert 0 < d <= DELTA_CAP, (key, d)
                want |= {key, key + "__delta"}
                if has_sens(key, short):
                    pair = {v: gold(f"g19_upd_{tag_p}_{v}.npz")[key] for v in SOLVERS}
                    sens = float(g[key + "__sens"])
                    assert abs(sens - rel_l2(pair["taylor"], pair["dpm_solver"])) <= 1e-9 * sens and tol[short] <= sens / 10, (tag_p, s, key)
                    want.add(key + "__sens")
                    n_sens += 1
            assert set(g) == want, sorted(set(g) ^ want)[:8]
            for (s_, t_) in ST:                  # the model value given back is the model value computed: the same result, to the bit
                for short in INTERMEDIATES:
                    assert torch.equal(g[f"{short}__{s_}__{t_}__given"], g[f"{short}__{s_}__{t_}__inter"])
    assert len(ST) == 5 and sum(s + HISTORY[0] <= 1.0 for s, _ in ST) == 4 and n_sens == (82 + 86) + 4 * 19


# ---------------------------------------------------------------------- the host algebra
@pytest.fixture
def host_lincomb(monkeypatch):
    monkeypatch.setattr(E, "lincomb", torch_lincomb)


@pytest.mark.parametrize("method,order", METHOD_ORDERS)
def test_every_trajectory_cell_on_the_host(method, order, host_lincomb):
    check_traj_group(method, order, "cpu", "cpu stand-in")


def test_every_update_cell_on_the_host(host_lincomb):
    check_update_files("cpu", "cpu stand-in")


def test_singlestep_order_1_on_logsnr_raises_what_the_reference_raises(host_lincomb):
    g = gold("g19_traj_eps.npz")
    key = base_key("singlestep", 1, 7, "logSNR", "dpm_solver")
    assert bytes(g[key + "__raises"].numpy()).decode() == "IndexError"
    with pytest.raises(IndexError):
        run_traj(False, dict(method="singlestep", order=1, steps=7, skip_type="logSNR"), "dpm_solver", "cpu")
