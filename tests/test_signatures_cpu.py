"""CPU: the facade's entry points take what the reference's take.  tests/golden/g14_signatures.json (``make_golden.py --signatures``)
holds the parameter names, their order and the repr of their defaults for the reference entry points diff_foley_amd stands in for; each
counterpart here must take the same names in the same order with equal defaults, and may add parameters of its own only behind them,
each with a default -- so that a call written for the reference, positional or by keyword, means the same here.

What a parameter DOES is the business of the differential tests; one case of a name that was taken and handled otherwise than the
reference handles it is test_sampler_fuzz_gpu.py::test_sample_ignores_a_log_every_t_argument_like_the_reference."""
import inspect
import json
import os

import pytest

import diff_foley_amd as P
from diff_foley_amd import samplers as S
from helpers import GOLD

COUNTERPART = {"LatentDiffusion": P.LatentDiffusion, "DDIMSampler": S.DDIMSampler, "PLMSSampler": S.PLMSSampler,
               "DPMSolverSampler": P.DPMSolverSampler, "CAVP_Inference": P.CAVPInference}

# Deviations, each with its reason: {entry point: {parameter: reason}}.  A parameter listed here is exempt from the name / order /
# default comparison.  A parameter the reference uses and the product silently ignores may NOT be listed: that is a wrong result, not
# a deviation.  None today.
DEVIATIONS = {}

# Parameters the product adds behind the reference's, and why.
EXTRAS = {"DDIMSampler.sample": {"classifier", "origin_cond", "classifier_guide_scale"},          # sample_with_classifier is this method
          "DPMSolverSampler.sample": {"classifier", "origin_cond", "classifier_guide_scale"}}

with open(os.path.join(GOLD, "g14_signatures.json")) as _f:
    REFERENCE = json.load(_f)

ENTRY_POINTS = ["LatentDiffusion.sample", "LatentDiffusion.sample_log", "LatentDiffusion.sample_log_diff_sampler",
                "LatentDiffusion.sample_log_with_classifier", "LatentDiffusion.sample_log_with_classifier_diff_sampler",
                "LatentDiffusion.apply_model", "LatentDiffusion.decode_first_stage", "LatentDiffusion.get_learned_conditioning",
                "DDIMSampler.sample", "DDIMSampler.sample_with_classifier", "PLMSSampler.sample", "DPMSolverSampler.sample",
                "DPMSolverSampler.sample_with_classifier", "CAVP_Inference.encode_video"]


def _described(fn):
    return [dict(name=p.name, kind=p.kind.name, default=None if p.default is inspect.Parameter.empty else repr(p.default))
            for p in inspect.signature(fn).parameters.values()]


def compare(ref, got, deviations=(), extras=None):
    """Raises AssertionError unless ``got`` is ``ref``, with parameters of its own (all with defaults, and no others than ``extras``
    where that is given) between the reference's last named parameter and its **kwargs."""
    named = lambda ps: [p for p in ps if p["kind"] != "VAR_KEYWORD"]
    r, g = named(ref), named(got)
    assert len(g) >= len(r), ("missing", [p["name"] for p in r[len(g):]])
    for i, (a, b) in enumerate(zip(r, g)):
        if a["name"] in deviations:
            continue
        assert a == b, ("position", i, a, b)
    added = g[len(r):]
    assert all(p["default"] is not None for p in added), ("extra without a default", added)
    assert {p["name"] for p in added} == set(extras or ()), ("extras", [p["name"] for p in added], extras)
    assert [p["kind"] for p in ref if p["kind"] == "VAR_KEYWORD"] == [p["kind"] for p in got if p["kind"] == "VAR_KEYWORD"], "**kwargs"


def test_the_fixture_names_every_entry_point():
    assert sorted(REFERENCE) == sorted(ENTRY_POINTS)
    assert set(DEVIATIONS) <= set(ENTRY_POINTS) and set(EXTRAS) <= set(ENTRY_POINTS)


def test_the_moved_sampler_keeps_its_earlier_spelling():
    from diff_foley_amd import dpm_solver
    assert S.DPMSolverSampler is P.DPMSolverSampler is dpm_solver.DPMSolverSampler


@pytest.mark.parametrize("point", ENTRY_POINTS)
def test_entry_point_takes_what_the_reference_takes(point):
    cls, method = point.split(".")
    compare(REFERENCE[point], _described(getattr(COUNTERPART[cls], method)), DEVIATIONS.get(point, ()), EXTRAS.get(point))


def test_the_comparison_catches_a_moved_a_renamed_and_a_defaultless_parameter():
    ref = REFERENCE["DDIMSampler.sample"]
    got = _described(S.DDIMSampler.sample)
    compare(ref, got, extras=EXTRAS["DDIMSampler.sample"])
    i = [p["name"] for p in got].index("eta")
    moved = got[:i] + got[i + 1:i + 3] + [got[i]] + got[i + 3:]
    renamed = [dict(p, name="steps") if p["name"] == "S" else p for p in got]
    other_default = [dict(p, default="50") if p["name"] == "log_every_t" else p for p in got]
    bare_extra = [dict(p, default=None) if p["name"] == "classifier" else p for p in got]
    no_kwargs = [p for p in got if p["kind"] != "VAR_KEYWORD"]
    for bad in (moved, renamed, other_default, bare_extra, no_kwargs, got[:-4] + got[-1:]):
        with pytest.raises(AssertionError):
            compare(ref, bad, extras=EXTRAS["DDIMSampler.sample"])
