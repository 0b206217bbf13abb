"""GPU: every GEMM form of the shipped plan tables on every (tile, split-K) pair the autotuner may pick for it.

The cases (shapes, descriptor fields, float64 references, per-element bounds, checks) are built on the CPU by tests/gemm_cases.py;
tests/test_gemm_cases_cpu.py asserts that they reach every (form, tile, split-K) triple of diff_foley_amd/tuned/*.txt.  Here each case
goes through the loop of tests/test_gemm_epilogues_gpu.py (run_on_every_tuner_pair): every pair of tuner_pairs(), both builds, NaN
poison on all outputs, gm 0 and 1, 2, 4, 8, 16 plus a repeated launch bit-identical, the slabs of a deferred reduce finished by the
GroupNorm bit-equal to the GEMM's own reduce, and a printed line with pairs run / refused and the worst error / bound."""
import pytest
import torch

import gemm_cases as G
import test_gemm_epilogues_gpu as EP

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["bf16", "fp16"], autouse=True)
def prec(request):
    EP.PREC = request.param
    yield request.param
    EP.PREC = "bf16"


class DevForm(EP.Case):
    """A gemm_cases.FormCase on the device, with the interface run_on_every_tuner_pair drives."""

    def __init__(self, cs):
        super().__init__(cs.name)
        self.cs = cs.to("cuda")
        self.batch, self.defer, self.M, self.N = cs.batch, cs.defer, cs.Mo, cs.No
        self.f = cs.desc_fields({k: self.dev(t).data_ptr() for k, t in cs.ins.items()})
        self.outs = cs.blank("cuda")
        if cs.defer:
            self.gn_x = torch.empty(cs.Mo, cs.No, device="cuda")
            self.gn_out = torch.empty(cs.Mo, cs.No, dtype=EP.odt(), device="cuda")
            self.gn_g, self.gn_b = self.dev(cs.gn_g), self.dev(cs.gn_b)

    def set_outs(self, d, sk):
        for k, t in self.outs.items():
            setattr(d, k, t.data_ptr())

    def check(self, sk):
        fails, worst, _ = self.cs.check(self.outs, sk)
        return fails, worst


@pytest.mark.parametrize("case", list(G.CASES))
def test_form_on_every_tuner_pair(case):
    """Every (tile, split-K) pair autotune_plan may launch for this form: float64 reference within the per-element bound, untouched
    gaps, slack rows and V^T padding stay NaN, copies bit-equal, gm walk orders and a repeated launch bit-identical, batch slices and
    deferred reduces equal to their single-launch forms."""
    EP.run_on_every_tuner_pair(case, DevForm(G.CASES[case](EP.PREC)))
