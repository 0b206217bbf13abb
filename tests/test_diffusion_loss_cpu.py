"""CPU: the host side of q_sample / stochastic_encode / decode / p_losses against the reference's own output (golden G17,
tests/golden/make_golden_g17.py), and the pin of the float64 yardstick the GPU tests of csrc/diffusion.hip are judged by.

  * lvlb_weights and the use_original_steps tables equal the reference's bit for bit (like G1);
  * the six new entry points take what the reference's take (g17_signatures.json, with test_signatures_cpu.compare);
  * tests/diffusion_ref.py reproduces the reference's q_sample, stochastic_encode and loss_dict to 1e-6 relative.  For q_sample,
    whose two terms can cancel, "relative" is per element against |A x0| + |S noise| (the size of what is added, which is what a
    rounding error scales with) and, over the whole tensor, in L2;
  * df_q_sample and df_diffusion_loss are declared in the header and exported by both builds;
  * what the facade decides on the host: the stored loss settings, the logvar key, range and shape errors before any launch."""
import json
import os

import numpy as np
import pytest
import torch

import diff_foley_amd as P
from diff_foley_amd import engine as E, samplers as S, synth
import diffusion_ref as R
from helpers import GOLD, gold, rnd
from test_signatures_cpu import _described, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_X0, SEED_NOISE = 1700, 1701          # tests/golden/make_golden_g17.py
SHAPE = (4, 16, 64)
CASES = {"l2": dict(loss_type="l2"), "l1": dict(loss_type="l1"),
         "elbo": dict(loss_type="l2", original_elbo_weight=0.5, logvar_init=-0.3),
         "learn": dict(loss_type="l2", learn_logvar=True, l_simple_weight=0.7, original_elbo_weight=0.25)}
REL = 1e-6


def _tiny(**extra):
    return P.LatentDiffusion(**dict(P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY), **extra))


def test_lvlb_weights_and_original_step_tables_equal_the_reference_bit_for_bit():
    g = gold("g17_p_losses.npz")
    m = _tiny()
    assert m.lvlb_weights.dtype == torch.float32 and torch.equal(m.lvlb_weights, g["lvlb_weights"])
    assert torch.equal(P.LatentDiffusion(**P.stage2_config()).lvlb_weights, g["lvlb_weights"])      # the schedule is the full model's too
    assert float(m.lvlb_weights[0]) == float(m.lvlb_weights[1]) and torch.isfinite(m.lvlb_weights).all()
    smp = S.DDIMSampler(m)
    smp.make_schedule(8, ddim_eta=float(g["original_eta"]), verbose=False)
    for k in ("alphas_cumprod", "alphas_cumprod_prev", "sqrt_one_minus_alphas_cumprod", "ddim_sigmas_for_original_num_steps"):
        got = smp.original[k]
        assert got.dtype == np.float32 and np.array_equal(got, g["original_" + k].numpy()), k
    assert np.array_equal(smp.ddim_sigmas_for_original_num_steps, g["original_ddim_sigmas_for_original_num_steps"].numpy())
    assert smp.ddim_sigmas_for_original_num_steps[0] == 0.0 and (smp.ddim_sigmas_for_original_num_steps[1:] > 0).all()
    # the tables stochastic_encode reads: the sampler's own fp32 square roots (ddim.py:39-40, 407-408)
    q = gold("g17_q_sample.npz")
    assert np.array_equal(smp.sqrt_alphas_cumprod, q["original_sqrt_alphas_cumprod"].numpy())
    assert np.array_equal(smp.sqrt_one_minus_alphas_cumprod, q["original_sqrt_one_minus_alphas_cumprod"].numpy())
    assert np.array_equal(np.sqrt(smp.ddim_alphas), q["ddim_sqrt_alphas"].numpy())
    assert np.array_equal(smp.ddim_sqrt_one_minus_alphas, q["ddim_sqrt_one_minus_alphas"].numpy())
    assert torch.equal(m.sqrt_alphas_cumprod, q["model_sqrt_alphas_cumprod"])
    # eta = 0: no noise at any original step
    smp.make_schedule(8, ddim_eta=0.0, verbose=False)
    assert not smp.ddim_sigmas_for_original_num_steps.any()


with open(os.path.join(GOLD, "g17_signatures.json")) as _f:
    SIGNATURES = json.load(_f)
COUNTERPART = {"LatentDiffusion": P.LatentDiffusion, "DDIMSampler": S.DDIMSampler}
POINTS = ["LatentDiffusion.q_sample", "LatentDiffusion.get_loss", "LatentDiffusion.p_losses", "LatentDiffusion.forward",
          "DDIMSampler.stochastic_encode", "DDIMSampler.decode"]


def test_the_fixture_names_the_six_entry_points():
    assert sorted(SIGNATURES) == sorted(POINTS)


@pytest.mark.parametrize("point", POINTS)
def test_new_entry_point_takes_what_the_reference_takes(point):
    cls, method = point.split(".")
    compare(SIGNATURES[point], _described(getattr(COUNTERPART[cls], method)))      # no deviations, no extras
    if point == "LatentDiffusion.forward":
        kinds = [p["kind"] for p in _described(P.LatentDiffusion.forward)]
        assert kinds == [p["kind"] for p in SIGNATURES[point]] and "VAR_POSITIONAL" in kinds
        assert P.LatentDiffusion.__call__ is P.LatentDiffusion.forward


def _close(got, ref, what):
    got, ref = float(got), float(ref)
    assert abs(got - ref) <= REL * abs(ref), (what, got, ref)


def test_float64_restatement_reproduces_the_reference_q_sample():
    g = gold("g17_q_sample.npz")
    x0, noise = rnd((3,) + SHAPE, SEED_X0), rnd((3,) + SHAPE, SEED_NOISE)
    for name, t, A, Sg in (("q_sample", "t_model", "model_sqrt_alphas_cumprod", "model_sqrt_one_minus_alphas_cumprod"),
                           ("encode_ddim", "t_ddim", "ddim_sqrt_alphas", "ddim_sqrt_one_minus_alphas"),
                           ("encode_original", "t_model", "original_sqrt_alphas_cumprod", "original_sqrt_one_minus_alphas_cumprod")):
        out, bound = R.q_sample_ref(x0, noise, g[t], g[A], g[Sg])
        ref = g[name].numpy().astype(np.float64)
        terms = bound / (2.0 * R.U)                                   # |A x0| + |S noise|
        assert (np.abs(out - ref) <= REL * terms).all(), name
        assert np.linalg.norm(out - ref) <= REL * np.linalg.norm(ref), name
        assert (np.abs(out - ref) <= bound).all(), name               # ... and the fp32 reference sits inside the derived rounding bound
    # an index outside the table: NaN for that sample only
    out, _ = R.q_sample_ref(x0, noise, [0, 1000, -1], g["model_sqrt_alphas_cumprod"], g["model_sqrt_one_minus_alphas_cumprod"])
    assert np.isfinite(out[0]).all() and np.isnan(out[1]).all() and np.isnan(out[2]).all()


@pytest.mark.parametrize("tag", list(CASES))
def test_float64_restatement_reproduces_the_reference_loss_dict(tag):
    g = gold("g17_p_losses.npz")
    kw = CASES[tag]
    noise = rnd((3,) + SHAPE, SEED_NOISE)
    ls, sc = R.diffusion_loss_ref(g["model_output"], noise, g["t"], g[f"{tag}__logvar"], g["lvlb_weights"], kw["loss_type"],
                                  kw.get("l_simple_weight", 1.0), kw.get("original_elbo_weight", 0.0))
    for b in range(3):
        _close(ls[b], g[f"{tag}__loss_simple"][b], (tag, "loss_simple", b))
    d = R.loss_dict_ref(sc, learn_logvar=kw.get("learn_logvar", False))
    keys = json.loads(bytes(g[f"{tag}__keys"].numpy()).decode())
    assert list(d) == keys
    for k in keys:
        _close(d[k], g[f"{tag}__dict__{k.replace('/', '.')}"], (tag, k))
    _close(sc["loss"], g[f"{tag}__loss"], (tag, "loss"))
    # x_noisy of the golden is the reference's q_sample of the same inputs
    out, bound = R.q_sample_ref(rnd((3,) + SHAPE, SEED_X0), noise, g["t"], _tiny().sqrt_alphas_cumprod, _tiny().sqrt_one_minus_alphas_cumprod)
    assert (np.abs(out - g["x_noisy"].numpy()) <= bound).all()


def test_restatement_propagates_an_out_of_range_timestep_to_that_sample_and_the_means():
    pred, target = rnd((3, 60), 1), rnd((3, 60), 2)
    lv, w = torch.rand(10), torch.rand(10)
    ls, sc = R.diffusion_loss_ref(pred, target, [0, 10, 9], lv, w)
    assert np.isfinite(ls[[0, 2]]).all() and np.isnan(ls[1])
    assert all(np.isnan(sc[k]) for k in ("simple", "gamma", "vlb", "loss")) and np.isfinite(sc["logvar"])
    ls, sc = R.diffusion_loss_ref(pred, pred, [0, 1, 9], lv, w, "l1")
    assert (ls == 0).all() and sc["simple"] == 0 and sc["vlb"] == 0


def test_new_symbols_are_in_the_header_and_in_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "df_engine.h")).read()
    src = open(os.path.join(ROOT, "diff_foley_amd", "csrc", "sources.txt")).read().split()
    assert "diffusion" in src and os.path.exists(os.path.join(ROOT, "diff_foley_amd", "csrc", "diffusion.hip"))
    for name in ("df_q_sample", "df_diffusion_loss"):
        assert f"int {name}(" in hdr and name in E.exported_symbols()
        for prec in ("bf16", "fp16"):
            assert hasattr(E.lib(prec), name), (name, prec)


def test_facade_keeps_the_loss_settings_and_takes_a_logvar():
    m = _tiny()
    assert (m.loss_type, m.l_simple_weight, m.original_elbo_weight, m.learn_logvar) == ("l2", 1.0, 0.0, False)
    assert m.logvar.shape == (1000,) and m.logvar.dtype == torch.float32 and not m.logvar.any() and not m.training
    m = _tiny(**CASES["elbo"])
    assert m.original_elbo_weight == 0.5 and torch.equal(m.logvar, torch.full((1000,), -0.3))
    m = _tiny(**CASES["learn"], timesteps=1000)
    assert m.learn_logvar and m.l_simple_weight == 0.7
    with pytest.raises(NotImplementedError, match="unknown loss type"):
        _tiny(loss_type="huber")
    ramp = torch.linspace(-0.5, 0.3, 1000)
    sd = dict(synth.make_state_dict(synth.state_dict_spec(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY), 0), logvar=ramp)
    missing, unexpected = m.load_state_dict(sd)
    assert torch.equal(m.logvar, ramp) and "logvar" not in unexpected
    with pytest.raises(RuntimeError, match="logvar"):
        m.load_state_dict(dict(sd, logvar=ramp[:10]))


def test_host_side_timestep_and_shape_errors():
    """A host t out of range is an IndexError before anything is uploaded; a t or noise of the wrong shape a ValueError that names
    the expected shape; a float t is refused (an index, not a timestep value)."""
    cpu = torch.device("cpu")
    for bad in ([0, 1000, 5], [0, -1, 5], torch.tensor([3, 4, 1 << 40])):
        with pytest.raises(IndexError, match="out of bounds"):
            E._timestep_indices(bad, 3, 1000, cpu, "q_sample")
    with pytest.raises(ValueError, match=r"expected \(3,\)"):
        E._timestep_indices([0, 1], 3, 1000, cpu, "q_sample")
    with pytest.raises(ValueError, match=r"expected \(3,\)"):
        E._timestep_indices(torch.zeros(3, 1, dtype=torch.long), 3, 1000, cpu, "q_sample")
    with pytest.raises(TypeError):
        E._timestep_indices(torch.tensor([0.0, 1.0, 2.0]), 3, 1000, cpu, "q_sample")
    t = E._timestep_indices(torch.tensor([0, 999, 5], dtype=torch.int32), 3, 1000, cpu, "q_sample")
    assert t.dtype == torch.int64 and t.tolist() == [0, 999, 5]
    x = torch.zeros(3, 4, 8, 8)
    tab = torch.ones(1000)
    with pytest.raises(ValueError, match=r"expected \(3, 4, 8, 8\)"):
        E.q_sample(x, torch.zeros(3, 4, 8, 4), [0, 1, 2], tab, tab)
    with pytest.raises(IndexError):
        E.q_sample(x, x, [0, 1, 1000], tab, tab)
    with pytest.raises(ValueError, match=r"expected \(3, 4, 8, 8\)"):
        E.diffusion_loss(x, torch.zeros(3, 4, 8, 4), [0, 1, 2], tab, tab)
    with pytest.raises(NotImplementedError, match="unknown loss type"):
        E.diffusion_loss(x, x, [0, 1, 2], tab, tab, loss_type="huber")


def test_encode_and_decode_need_a_schedule_like_the_reference():
    smp = S.DDIMSampler(_tiny())
    x = torch.zeros(1, 4, 16, 64)
    for call in (lambda: smp.stochastic_encode(x, torch.tensor([0])), lambda: smp.stochastic_encode(x, torch.tensor([0]), True),
                 lambda: smp.decode(x, None, 2), lambda: smp.decode(x, None, 2, use_original_steps=True)):
        with pytest.raises(AttributeError):
            call()
    with pytest.raises(AttributeError):
        smp.ddim_sigmas_for_original_num_steps
    with pytest.raises(AttributeError):
        smp.no_such_attribute
