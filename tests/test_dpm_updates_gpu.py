"""GPU: every update formula of diff_foley_amd.dpm_solver through ``df_lincomb`` and ``df_dpm_data_prediction``, both builds, against the
reference at fp32 accuracy (golden G19, tests/golden/make_golden_g19.py).

The cells, the runners and the bound are tests/test_dpm_updates_cpu.py's: the generic route with the closed model
``1.6 x cos(12 t) + 0.4 sin(3 x)`` evaluated on device tensors between the stages of an update -- no UNet, no engine plan.  What the
CPU stand-in cannot reach is here: ``df_lincomb`` itself, the model on the device, and thresholding in the loop (data prediction
only: multistep order 2 and singlestep order 3).  ``return_intermediate`` returns the reference's dict keys, each value within the
bound; a model value given back gives the result its computation gave; a repeated trajectory is bit-equal.  The power check (the
product run with the OTHER solver type must miss the record by more than the bound) runs for one cell per method; the CPU file
runs it for every cell.

The bound is 8 x the largest reference fp32-to-float64 rel-L2 of the cell's group, see the CPU file.  Device sin / cos and the fused
multiply-adds of df_lincomb round differently from the CPU's, but not more.

Observed err / tolerance, the largest of each group, x0 / eps (2026-10-20; ``python -m pytest tests/test_dpm_updates_cpu.py -s`` for the
CPU stand-in, ``python -m pytest -m gpu tests/test_dpm_updates_gpu.py -s`` on an MI355X; the bf16 and fp16 builds print the same
figures -- the kernels used here are fp32 in both).  No group needs more than a third of the bound:
  group                                  tolerance x0 / eps      CPU stand-in       device
  singlestep order 1                     4.10e-06 / 1.24e-05     0.133 / 0.129      0.116 / 0.129
  singlestep order 2                     2.53e-04 / 3.52e-05     0.077 / 0.108      0.079 / 0.114
  singlestep order 3                     2.38e-05 / 4.15e-05     0.237 / 0.127      0.228 / 0.132
  singlestep_fixed order 2               7.73e-05 / 2.75e-05     0.100 / 0.125      0.092 / 0.125
  singlestep_fixed order 3               6.12e-05 / 1.94e-05     0.127 / 0.157      0.110 / 0.159
  multistep order 1                      1.72e-05 / 2.48e-05     0.094 / 0.076      0.092 / 0.082
  multistep order 2                      1.77e-04 / 1.89e-05     0.166 / 0.179      0.146 / 0.177
  multistep order 3                      3.75e-05 / 2.12e-05     0.226 / 0.217      0.225 / 0.195
  dpm_solver_first_update                2.87e-06                0.125              0.121
  singlestep_dpm_solver_second_update    1.91e-05                0.125              0.125
  singlestep_dpm_solver_third_update     9.14e-06                0.304              0.304
  multistep_dpm_solver_second_update     3.56e-06                0.207              0.248
  multistep_dpm_solver_third_update      7.02e-06                0.167              0.130
  denoise_to_zero_fn                     1.47e-06                0.173              0.173
  thresholding (device only)             ms2 1.77e-04, ss3 2.38e-05                 0.001, 0.021
The whole file takes under five seconds, both builds."""
import pytest
import torch

from diff_foley_amd import engine as E
from helpers import gold, rel_l2
from test_dpm_updates_cpu import (METHOD_ORDERS, PAIRS, SHAPE, base_key, check_traj_group, check_update_files, other, run_traj,
                                  traj_cells, traj_tolerances)

pytestmark = pytest.mark.gpu

POWER_CELLS = [dict(method="singlestep", order=3, steps=7, skip_type="time_uniform", lower_order_final=False),
               dict(method="singlestep_fixed", order=2, steps=6, skip_type="logSNR", lower_order_final=False),
               dict(method="multistep", order=3, steps=20, skip_type="logSNR", lower_order_final=False)]


@pytest.fixture(params=["bf16", "fp16"])
def prec(request, monkeypatch):
    """The solver's engine calls go to this build of the library."""
    plain = E.lib
    monkeypatch.setattr(E, "lib", lambda precision=None: plain(precision or request.param))
    return request.param


@pytest.mark.parametrize("method,order", METHOD_ORDERS)
def test_every_trajectory_cell_on_the_device(prec, method, order):
    check_traj_group(method, order, "cuda", f"gpu {prec}", power=False)


def test_every_update_cell_on_the_device(prec):
    """Direct calls at five (s, t), non-default r1 / r2, an irregular history, return_intermediate (the reference's keys, asserted in
    run_updates) and model values given back."""
    check_update_files("cuda", f"gpu {prec}", power=False)


def test_thresholding_in_the_loop(prec):
    g, tol = gold("g19_traj_x0.npz"), traj_tolerances("x0")
    for key, kw, solver_type, _ in traj_cells(thresholding=True):
        z = run_traj(True, kw, solver_type, "cuda", thresholding=True)
        err, t = rel_l2(z.cpu(), g[key]), tol[(kw["method"], kw["order"])]
        print(f"dpm updates gpu {prec} thresholding {key}: err / tolerance {err / t:.3f} (tolerance {t:.2e})")
        assert z.is_cuda and z.dtype == torch.float32 and z.shape == SHAPE
        assert err <= t, (key, err, t)
        plain = "ms2_lower__" + solver_type if kw["method"] == "multistep" else base_key("singlestep", 3, 7, "logSNR", solver_type)
        assert rel_l2(g[plain], g[key]) > 1.0                                       # ... and a run that skipped it is far away


@pytest.mark.parametrize("kw", POWER_CELLS, ids=lambda kw: kw["method"])
def test_the_other_solver_type_misses_the_record(prec, kw):
    for tag_p, px in PAIRS:
        g, tol = gold(f"g19_traj_{tag_p}.npz"), traj_tolerances(tag_p)[(kw["method"], kw["order"])]
        for solver_type in ("dpm_solver", "taylor"):
            key = base_key(kw["method"], kw["order"], kw["steps"], kw["skip_type"], solver_type)
            assert tol <= float(g[key + "__sens"]) / 10
            miss = rel_l2(run_traj(px, kw, other(solver_type), "cuda").cpu(), g[key])
            assert miss > tol, (tag_p, key, miss, tol)


def test_a_repeated_trajectory_is_bit_equal(prec):
    kw = dict(method="singlestep", order=3, steps=20, skip_type="time_quadratic")
    assert torch.equal(run_traj(True, kw, "taylor", "cuda"), run_traj(True, kw, "taylor", "cuda"))
    kw = dict(method="multistep", order=2, steps=6)
    assert torch.equal(run_traj(True, kw, "dpm_solver", "cuda", thresholding=True), run_traj(True, kw, "dpm_solver", "cuda", thresholding=True))
