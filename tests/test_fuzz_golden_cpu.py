"""CPU: the oracle (oracle/*.py) against the REFERENCE on every case the randomised GPU tests draw.

The GPU fuzz tests judge the product by the oracle over the space the reference's constructors and call sites admit; the goldens G1-G13
pin the oracle to the reference at two configurations and a dozen sampler option sets only.  The G14 records
(tests/golden/g14_fuzz_<surface>*.npz, written by ``make_golden.py --fuzz`` from the reference itself) close the triangle: for every
seed of tests/fuzz_cases.py's surfaces the reference's result is on file, and here

  * redrawing the seed gives the stored draw exactly (a changed draw function without regenerated records fails);
  * the oracle on the rebuilt inputs matches the stored values at test_oracle_golden.py's tolerances for the same kind of result
    (2e-5 one forward, 2e-4 sampler latents, 1e-5 / 1e-4 classifier probability / gradient, G7's allclose for CAVP; the last-axis
    sums of a summarised value at the tolerance times the axis length), and its intermediate counts and exceptions are the
    reference's;
  * the seeds on file are range(N_CASES) and the regression seeds of the surface, no more and no fewer.

The judgement is one function, and three mutants show that it bites: a stored element off by 1e-3 of the value's maximum (in both
storage forms), a count off by one, a draw with one field changed."""
import copy
import json

import numpy as np
import pytest
import torch

import fuzz_cases as fc
from helpers import tiny_classifier_sd, tiny_state_dict
from diff_foley_amd import synth
from oracle import cavp as ocavp, samplers as osamp, schedule as osch, unet as ou, vae as ov

TOL_FORWARD = 2e-5
TOL_LATENT = 2e-4
TOL_PROB, TOL_GRAD = 1e-5, 1e-4

# (surface, seed) of the records whose oracle run takes longer than the slowest unmarked test of test_oracle_golden.py in the same run:
# none -- the slowest record (samplers 8) takes 4 s where test_g5_tiny_samplers takes 36 s; the whole file runs in under a minute
SLOW = set()

_oracle_cache = {}


def _tiny_oracle():
    if "tiny" not in _oracle_cache:
        sd = tiny_state_dict()
        usd = ou.sub_state_dict(sd, "model.diffusion_model.")
        csd = ou.sub_state_dict(sd, "cond_stage_model.")
        _oracle_cache["tiny"] = (lambda x, t, c: ou.unet_forward(usd, synth.UNET_TINY, x, t, c), lambda f: ov.cond_stage(csd, f),
                                 osch.ddpm_schedule())
    return _oracle_cache["tiny"]


def _raised(fn):
    try:
        fn()
    except Exception as ex:          # the NAME is what the record holds
        return type(ex).__name__
    return None


def _run_oracle(surface, seed):
    """What the oracle gives on the case: values by name, counts by name, the name of the exception it raises."""
    out = dict(values={}, counts={}, raises=None)
    v = out["values"]
    if surface == "unet":
        k = fc.unet_case(seed)
        usd = ou.sub_state_dict(k["sd"], "model.diffusion_model.")
        B = k["o"]["B"]
        v["y"] = ou.unet_forward(usd, k["cfg"], k["x"], k["t"], k["c"])
        e2 = ou.unet_forward(usd, k["cfg"], torch.cat([k["x"], k["x"]]), torch.cat([k["tt"], k["tt"]]), torch.cat([k["uc"], k["c"]]))
        v["y_cfg"] = e2[:B] + fc.UNET_CFG_SCALE * (e2[B:] - e2[:B])
    elif surface == "vae":
        k = fc.vae_case(seed)
        v["y"] = ov.decode_first_stage(ou.sub_state_dict(k["sd"], "first_stage_model."), k["cfg"], k["z"])
    elif surface == "cond":
        k = fc.cond_case(seed)
        csd = ou.sub_state_dict(k["sd"], "cond_stage_model.")
        for i, f in enumerate(k["feats"]):
            v[f"c{i}"] = ov.cond_stage(csd, f)
        out["too_long_raises"] = _raised(lambda: ov.cond_stage(csd, torch.zeros(1, k["cond"]["seq_len"] + 1, k["cond"]["origin_dim"])))
    elif surface == "classifier":
        k = fc.classifier_case(seed)
        csd = ou.sub_state_dict(k["sd"], "model.")
        cls = lambda x, t, c: ou.classifier_forward(csd, k["cfg"], x, t, c)
        v["p"] = cls(k["x"], k["t"], k["vf"]).detach()
        v["grad"] = osamp.classifier_grad(cls, k["x"], k["t"], k["vf"])
    elif surface == "cavp":
        k = fc.cavp_case(seed)
        for name, normalize in (("feats", True), ("feats_raw", False)):
            v[name] = ocavp.encode_video(k["sd"], k["video"], normalize=normalize, stage_blocks=tuple(k["cfg"]["stage_blocks"]))
    elif surface == "samplers":
        apply_model, cond_fn, sched = _tiny_oracle()
        acp = sched["alphas_cumprod"]
        k = fc.sampler_case(seed)
        o = k["o"]
        gq = torch.Generator()
        qn = lambda shape: torch.randn(tuple(shape), generator=gq)
        noise = lambda s: torch.randn(tuple(s))
        c = cond_fn(k["feats"])

        def run():
            gq.manual_seed(k["q_seed"])
            torch.manual_seed(k["noise_seed"])
            if o["name"] == "DDIM":
                return osamp.ddim_sample(apply_model, acp, o["S"], k["xT"], c, o["scale"], k["uc"], eta=o["eta"], log_every_t=o["log_every_t"],
                                         noise_fn=noise, mask=k["mask"], x0=k["x0"], q_noise_fn=qn, temperature=o["temperature"],
                                         noise_dropout=o["noise_dropout"])
            if o["name"] == "PLMS":
                return osamp.plms_sample(apply_model, acp, o["S"], k["xT"], c, o["scale"], k["uc"], log_every_t=o["log_every_t"],
                                         mask=k["mask"], x0=k["x0"], q_noise_fn=qn)
            if o["name"] == "DPM_Solver":
                return osamp.dpm_solver_sample(apply_model, acp, o["S"], k["xT"], c, o["scale"], k["uc"])
            return osamp.ddpm_sample(apply_model, sched, k["xT"], c, timesteps=o["S"], noise_fn=noise, log_every_t=o["log_every_t"],
                                     mask=k["mask"], x0=k["x0"], q_noise_fn=qn)
        try:
            z, inter = run()
        except IndexError as ex:
            out["raises"] = type(ex).__name__
            return out
        v["z"] = z
        if o["name"] == "DDPM":
            out["counts"]["n_inter"] = len(inter)
        elif inter is not None:
            out["counts"]["n_x_inter"], out["counts"]["n_pred_x0"] = len(inter["x_inter"]), len(inter["pred_x0"])
            v["pred_x0_last"] = inter["pred_x0"][-1]
    elif surface == "double_guidance":
        apply_model, cond_fn, sched = _tiny_oracle()
        ksd = ou.sub_state_dict(tiny_classifier_sd(), "model.")
        classifier = lambda x, t, c: ou.classifier_forward(ksd, synth.CLS_TINY, x, t, c)
        k = fc.double_guidance_case(seed)
        o = k["o"]
        c = cond_fn(k["vf"][:, :32])
        torch.manual_seed(k["noise_seed"])
        if o["name"] == "DDIM":
            z, _ = osamp.ddim_sample(apply_model, sched["alphas_cumprod"], o["S"], k["xT"], c, o["scale"], torch.zeros_like(c), eta=o["eta"],
                                     classifier=classifier, origin_cond=k["vf"], classifier_scale=o["cscale"],
                                     noise_fn=lambda s: torch.randn(tuple(s)))
        else:
            z, _ = osamp.dpm_solver_sample(apply_model, sched["alphas_cumprod"], o["S"], k["xT"], c, o["scale"], torch.zeros_like(c),
                                           classifier=classifier, origin_cond=k["vf"], classifier_scale=o["cscale"])
        v["z"] = z
    return out


def _oracle(surface, seed):
    if (surface, seed) not in _oracle_cache:
        _oracle_cache[(surface, seed)] = _run_oracle(surface, seed)
    return _oracle_cache[(surface, seed)]


_TOL = {("unet", "y"): TOL_FORWARD, ("unet", "y_cfg"): TOL_FORWARD, ("vae", "y"): TOL_FORWARD, ("classifier", "p"): TOL_PROB,
        ("classifier", "grad"): TOL_GRAD, ("samplers", "z"): TOL_LATENT, ("samplers", "pred_x0_last"): TOL_LATENT,
        ("double_guidance", "z"): TOL_LATENT}
_G7 = {"feats": dict(atol=1e-5), "feats_raw": dict(atol=1e-4, rtol=1e-4)}          # test_g7_cavp_oracle_matches_reference_vectors


def judge(surface, seed, rec):
    """Raises AssertionError unless the record is what the oracle and a redraw of the seed give."""
    assert fc.draw_json(surface, seed) == rec["draw"], ("draw", fc.draw_json(surface, seed), rec["draw"])
    o = _oracle(surface, seed)
    assert o["raises"] == rec.get("raises"), ("raises", o["raises"], rec.get("raises"))
    if surface == "cond":
        assert o["too_long_raises"] == rec.get("too_long_raises"), (o["too_long_raises"], rec.get("too_long_raises"))
    stored = {k: v for k, v in rec.items() if isinstance(v, dict)}
    assert sorted(stored) == sorted(o["values"]), (sorted(stored), sorted(o["values"]))
    counts = {k: v for k, v in rec.items() if k.startswith("n_") and k != "n_inter_kwarg_1"}
    assert counts == o["counts"], ("counts", counts, o["counts"])
    for name, t in o["values"].items():
        if surface == "cavp":
            ref, got = fc.value_pair(stored[name], t)
            assert torch.allclose(got, ref, **_G7[name]), (name, float((got - ref).abs().max()))
        else:
            fc.check_value(stored[name], t, TOL_FORWARD if surface == "cond" else _TOL[(surface, name)])
    if "n_inter_kwarg_1" in rec:
        # the reference's sample() drops a log_every_t argument (ddpm.py:1253-1268): same count, same latents as without it
        assert rec["n_inter_kwarg_1"] == rec["n_inter"] and rec["kwarg_latents_equal"] is True, rec


def _params():
    out = []
    for surface in fc.SURFACES:
        for seed in fc.suite_seeds(surface):
            out.append(pytest.param(surface, seed, id=f"{surface}-{seed}", marks=[pytest.mark.slow] if (surface, seed) in SLOW else []))
    return out


@pytest.mark.parametrize("surface,seed", _params())
def test_oracle_matches_the_reference_record(surface, seed):
    rec = fc.load_records(surface).get(seed)
    assert rec is not None, f"no reference record for {surface} seed {seed}: run tests/golden/make_golden.py --fuzz"
    judge(surface, seed, rec)


@pytest.mark.parametrize("surface", fc.SURFACES)
def test_the_records_cover_the_suite_seeds_exactly(surface):
    assert sorted(fc.load_records(surface)) == fc.suite_seeds(surface)
    assert fc.suite_seeds(surface) == sorted(set(range(fc.N_CASES[surface])) | set(fc.REGRESSION_SEEDS[surface]))


def test_sampler_records_hold_each_outcome_kind():
    """The records the mutants and the GPU tests lean on are there: the S = 9 IndexError, intermediates of all three kinds, and the
    ancestral sampler's dropped log_every_t argument with a drawn value that differs from the model's default."""
    recs = fc.load_records("samplers")
    assert recs[0].get("raises") == "IndexError" and "z" not in recs[0]
    assert any("n_x_inter" in r for r in recs.values()) and any("n_inter" in r for r in recs.values())
    assert any("z" in r and not any(k.startswith("n_") for k in r) for r in recs.values())          # DPM-Solver: no intermediates
    assert any(r.get("n_inter_kwarg_1") is not None and json.loads(r["draw"])["log_every_t"] != 1 for r in recs.values())


# ------------------------------------------------------------------------------------------------------------------------------ mutants
def _first_value(form):
    """(surface, seed, name) of the first stored value of the storage form ("full" / "vals") among the single-forward surfaces."""
    for surface in ("unet", "vae"):
        for seed, rec in sorted(fc.load_records(surface).items()):
            for name, v in rec.items():
                if isinstance(v, dict) and form in v:
                    return surface, seed, name
    raise AssertionError(f"no value stored as '{form}'")


@pytest.mark.parametrize("form", ["full", "vals"])
def test_mutant_one_element_off_by_a_thousandth_of_the_maximum_is_caught(form):
    surface, seed, name = _first_value(form)
    rec = fc.load_records(surface)[seed]
    judge(surface, seed, rec)                                    # the record as it is passes
    bad = copy.deepcopy(rec)
    a = bad[name][form].copy()
    a.flat[a.size // 2] += np.float32(1e-3 * float(rec[name]["absmax"]))
    bad[name][form] = a
    with pytest.raises(AssertionError, match="values"):
        judge(surface, seed, bad)


@pytest.mark.parametrize("field", ["n_x_inter", "n_pred_x0", "n_inter"])
def test_mutant_a_count_off_by_one_is_caught(field):
    seed, rec = next((s, r) for s, r in sorted(fc.load_records("samplers").items()) if field in r)
    judge("samplers", seed, rec)
    for d in (-1, 1):
        bad = dict(rec, **{field: rec[field] + d})
        with pytest.raises(AssertionError, match="counts|n_inter"):
            judge("samplers", seed, bad)


@pytest.mark.parametrize("surface", fc.SURFACES)
def test_mutant_a_draw_with_one_field_changed_is_caught(surface):
    seed = fc.suite_seeds(surface)[-1]
    rec = fc.load_records(surface)[seed]
    draw = json.loads(rec["draw"])

    def bump(d):          # the first number found, depth first in key order, moves by one
        for k in sorted(d) if isinstance(d, dict) else range(len(d)):
            if isinstance(d[k], (dict, list)):
                if bump(d[k]):
                    return True
            elif isinstance(d[k], (int, float)) and not isinstance(d[k], bool):
                d[k] += 1
                return True
        return False
    assert bump(draw)
    bad = dict(rec, draw=json.dumps(draw, sort_keys=True, separators=(",", ":")))
    assert bad["draw"] != rec["draw"]
    with pytest.raises(AssertionError, match="draw"):
        judge(surface, seed, bad)
