"""CPU: the C-ABI library builds/loads and exports every symbol include/df_engine.h declares; host logic
(schedules, facade construction, error behaviour without a GPU)."""
import os
import re

import numpy as np
import pytest
import torch

import diff_foley_amd as P
from diff_foley_amd import engine as E, schedule as S, synth
from helpers import gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not all(os.path.exists(p) for p in E.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()


def test_header_symbols_exported():
    hdr = open(os.path.join(ROOT, "include", "df_engine.h")).read()
    declared = set(re.findall(r"\b(df_[a-z0-9_]+)\s*\(", hdr))
    for prec, want in (("bf16", b"bf16"), ("fp16", b"f16")):      # both operand-type builds of the same sources
        lib = E.lib(prec)
        for name in sorted(declared):
            assert hasattr(lib, name), f"{name} declared in df_engine.h but not exported by the {prec} build"
        assert lib.df_abi_version() == 1
        assert lib.df_operand_dtype() == want
    assert declared == set(E.exported_symbols()), declared ^ set(E.exported_symbols())


def test_built_libraries_pass_the_layout_checks():
    """Two hand-placed idioms the compiler cannot vouch for are checked on the BUILT code objects (run by __graft_entry__.build() as
    well): every GEMM translation unit's own-code prefetch is bounded by a .bss symbol that really lies behind .text
    (tools/check_code_touch.py), and -- sampled here on one library, the full scan takes 20 s -- no inline-asm 16-byte write-through
    store is followed by a VALU write of its data registers within two wait states (tools/check_store_hazard.py)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_code_touch.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 violation(s)" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_store_hazard.py"), E.LIB_PATHS["fp16"]],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "0 hazard(s)" in r.stdout, r.stdout + r.stderr


def test_gemm_desc_binding_matches_the_build():
    """The ctypes mirror of df_test_gemm_desc has the C struct's size (the entries check `size` and refuse any other value before
    touching the GPU), and the validity query answers on the host: a K = 4096 linear takes split-K 32 on the generic tiles and
    never on a halo tile; the cross-attention score epilogue refuses split-K."""
    import ctypes as C
    for prec in ("bf16", "fp16"):
        L = E.lib(prec)
        d = E.GemmDesc(M=256, N=128, K=4096)
        assert L.df_test_gemm_valid(C.byref(d), 0, 1, 32) == 1
        assert L.df_test_gemm_valid(C.byref(d), 5, 1, 1) == 0
        one = (C.c_float * 4096)()
        xs = E.GemmDesc(M=256, N=128, K=192, out_operand=1, ln_stats=C.addressof(one), ln_slots=3, ln_C=192, ln_cs=C.addressof(one),
                        bias=C.addressof(one), w_rows=128, sm_w=32, sm_valid=17)
        assert L.df_test_gemm_valid(C.byref(xs), 0, 1, 1) == 1
        assert L.df_test_gemm_valid(C.byref(xs), 0, 1, 2) == 0
        bad = E.GemmDesc(M=256, N=128, K=4096)
        bad.size = C.sizeof(bad) - 8
        assert L.df_test_gemm_valid(C.byref(bad), 0, 1, 1) == -1
        assert b"descriptor" in L.df_last_error()
        assert L.df_test_gemm_ex(C.byref(bad), None) != 0
        assert b"descriptor" in L.df_last_error()


def test_no_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = P.LatentDiffusion(**P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    with pytest.raises(RuntimeError):
        m.cuda()
    with pytest.raises(RuntimeError):
        m.decode_first_stage(torch.zeros(1, 4, 16, 64))


def test_product_schedule_matches_reference_golden():
    g = gold("g1_schedules.npz")
    m = P.LatentDiffusion(**P.stage2_config())
    for k in S.BUFFER_NAMES:
        assert torch.equal(getattr(m, k), g[k]), k
    for s in (25, 50):
        t = S.DDIMTables(m.alphas_cumprod, s)
        assert np.array_equal(t.timesteps, g[f"ddim{s}_timesteps"].numpy())
        assert np.array_equal(t.alphas.astype(np.float64), g[f"ddim{s}_alphas"].numpy())
        assert np.array_equal(t.alphas_prev.astype(np.float64), g[f"ddim{s}_alphas_prev"].numpy())
        assert np.array_equal(t.sqrt_one_minus_alphas.astype(np.float64), g[f"ddim{s}_sqrt_one_minus_alphas"].numpy())
        d = S.DPMTables(m.alphas_cumprod)
        ts = d.time_steps(s)
        assert np.array_equal(ts, g[f"dpm{s}_t"].numpy())
        for name, fn in (("lambda", d.lam), ("alpha", d.alpha), ("sigma", d.sigma)):
            got = np.array([fn(t_) for t_ in ts])
            ref = g[f"dpm{s}_{name}"].numpy()
            assert np.allclose(got, ref, rtol=2e-6, atol=2e-6), name
    d = S.DPMTables(m.alphas_cumprod)
    got = np.array([d.log_alpha(t_) for t_ in g["interp_t"].numpy()])
    assert np.allclose(got, g["interp_log_alpha"].numpy(), rtol=2e-6, atol=1e-7)


def test_product_quad_discretisation_matches_reference_golden():
    """DDIMSampler.make_schedule(ddim_discretize="quad"): tables bit-equal to the reference's (sigmas to fp32 rounding)."""
    g = gold("g11_ddim_quad.npz")
    m = P.LatentDiffusion(**P.stage2_config())
    for s in (10, 25, 50):
        for eta in (0, 1):
            smp = P.DDIMSampler(m)
            smp.make_schedule(s, ddim_discretize="quad", ddim_eta=float(eta), verbose=False)
            tag = f"quad{s}_eta{eta}"
            assert np.array_equal(smp.ddim_timesteps, g[f"{tag}_timesteps"].numpy())
            assert np.array_equal(smp.ddim_alphas.astype(np.float64), g[f"{tag}_alphas"].numpy())
            assert np.array_equal(smp.ddim_alphas_prev.astype(np.float64), g[f"{tag}_alphas_prev"].numpy())
            assert np.array_equal(smp.ddim_sqrt_one_minus_alphas.astype(np.float64), g[f"{tag}_sqrt_one_minus_alphas"].numpy())
            assert np.allclose(smp.ddim_sigmas.astype(np.float64), g[f"{tag}_sigmas"].numpy(), rtol=2e-6, atol=0)
    with pytest.raises(NotImplementedError):
        P.DDIMSampler(m).make_schedule(25, ddim_discretize="cosine")


def test_ddim_step_count_quirk():
    m = P.LatentDiffusion(**P.stage2_config())
    with pytest.raises(IndexError):
        S.DDIMTables(m.alphas_cumprod, 3)      # 1000//3 -> timestep 1000 out of range, as in the reference


def test_state_dict_spec_counts():
    spec = synth.state_dict_spec()
    n_unet = sum(int(np.prod(s)) for k, s in spec.items() if k.startswith("model.diffusion_model."))
    assert n_unet == 859_520_964
