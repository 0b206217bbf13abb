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


def test_gemm_desc_operand_fields_answer_on_the_host():
    """One positive and one negative df_test_gemm_valid query per operand-side field of df_test_gemm_desc, and the tune-cache key
    (df_test_gemm_key) of each form."""
    import ctypes as C
    one = (C.c_float * 4096)()
    p = C.addressof(one)
    for prec in ("bf16", "fp16"):
        L = E.lib(prec)
        valid = lambda d, t, sk=1, batch=1: L.df_test_gemm_valid(C.byref(d), t, batch, sk)

        def key(d, batch=1):
            buf = C.create_string_buffer(160)
            assert L.df_test_gemm_key(C.byref(d), batch, buf, 160) == 0, L.df_last_error()
            return buf.value.decode()
        # ups + zstuff: MODE 2, the generic tiles that have it; never a halo or a producer-specialised tile
        z = E.GemmDesc(conv=1, NB=2, H=4, Wd=8, Cin=128, N=64, stride=1, ups=1, zstuff=1, aux=p, ld_aux=64)
        assert valid(z, 4, 8) == 1 and valid(z, 4, 12) == 0 and valid(z, 25) == 0 and valid(z, 26) == 0
        assert key(z) == "256_64_1152_9_1_1_1_0_e8"
        assert valid(E.GemmDesc(conv=1, NB=2, H=4, Wd=8, Cin=128, N=64, stride=1, zstuff=1), 4) == -1      # zstuff without ups
        # conv == 2: the phase-decomposed upsample conv on tiles 3 / 8 / 9 ..., split-K needs N % 4 == 0 and K / 64 >= 2 sk
        u = E.GemmDesc(conv=2, NB=2, H=5, Wd=7, Cin=384, N=68)
        assert valid(u, 3, 12) == 1 and valid(u, 3, 16) == 0 and valid(u, 0) == 0
        assert key(u) == "70_68_1536_4_1_0_1_0_e0"
        assert valid(E.GemmDesc(conv=2, NB=2, H=5, Wd=7, Cin=384, N=66), 3, 2) == 0
        # A2 / lda2 / Cin2, conv: the folded skip runs on the generic tiles and the producer-specialised halo tiles only
        sk_ = E.GemmDesc(conv=1, NB=2, H=6, Wd=16, Cin=128, N=128, stride=1, A2=p, lda2=64, Cin2=64)
        assert valid(sk_, 25) == 1 and valid(sk_, 5) == 0 and valid(sk_, 3) == 1
        assert key(sk_) == "192_128_1216_9_1_0_1_0_e32"
        odd = E.GemmDesc(conv=1, NB=2, H=6, Wd=16, Cin=128, N=128, stride=1, A2=p, lda2=68, Cin2=64)
        assert valid(odd, 25) == 0 and valid(odd, 3) == 1        # halo: lda2 % 8
        assert valid(E.GemmDesc(conv=1, NB=2, H=6, Wd=16, Cin=128, N=128, stride=1, A2=p, lda2=32, Cin2=64), 3) == -1
        # ... linear: K = K + Cin2 over two operand tensors
        ff = E.GemmDesc(M=64, N=64, K=256, A2=p, lda2=64, Cin2=64, res=p, ldr=64, defer_reduce=1)
        assert valid(ff, 3, 2) == 1 and valid(ff, 3, 3) == 0
        assert key(ff) == "64_64_320_1_1_0_1_0_e112"
        # geglu: LayerNorm-folded on the persistent and wide tiles; the 10-slot persistent tiles refuse C = 1280
        ln = dict(ln_stats=p, ln_C=1280, ln_slots=20, ln_cs=p, bias=p, out_operand=1)
        g = E.GemmDesc(M=64, N=2560, K=1280, geglu=1, A=p, W=p, C=p, **ln)
        assert valid(g, 31) == 1 and valid(g, 30) == 0 and valid(g, 33) == 1 and valid(g, 3) == 1 and valid(g, 3, 2) == 0
        assert key(g) == "64_2560_1280_1_1_0_1_1_e1"
        assert valid(E.GemmDesc(M=64, N=2560, K=1280, A=p, W=p, C=p, **ln), 31) == 0          # the same projection without geglu
        assert valid(E.GemmDesc(M=64, N=2688, K=1280, geglu=1, A=p, W=p, C=p, **ln), 33) == 0    # N % 320
        # vt: whole tiles only -- no split-K, vt_col0 a multiple of the tile's BN
        ln = dict(ln_stats=p, ln_C=320, ln_slots=5, ln_cs=p, bias=p, out_operand=1)
        v = E.GemmDesc(M=128, N=960, K=320, vt=p, vt_col0=640, vt_T=64, ldvt=72, ldc=648, **ln)
        assert valid(v, 3) == 1 and valid(v, 3, 2) == 0 and valid(v, 8) == 0
        assert key(v) == "128_960_320_1_1_0_1_0_e5"


# What a GEMM tile id means: the ids are written into the shipped plan tables (diff_foley_amd/tuned/) and into every tune-cache file,
# so they are a file format.  (display name, family, BM, BN) per id, restated here independently of csrc/gemm_tiles.def.
_TILE_TABLE = {
    0: ("128x128", "generic", 128, 128), 1: ("128x64", "generic", 128, 64), 2: ("64x128", "generic", 64, 128),
    3: ("64x64", "generic", 64, 64), 4: ("32x128", "generic", 32, 128),
    5: ("H128x64", "halo", 128, 64), 6: ("H256x64", "halo", 256, 64), 7: ("H128x128", "halo", 128, 128),
    8: ("128x256", "generic", 128, 256), 9: ("256x128", "generic", 256, 128),
    10: ("128x128s", "generic", 128, 128), 11: ("128x64s", "generic", 128, 64), 12: ("64x128s", "generic", 64, 128),
    13: ("64x64s", "generic", 64, 64), 14: ("32x128s", "generic", 32, 128),
    15: ("H128x64d", "halo", 128, 64),
    16: ("H256x64d", "retired", 256, 64),      # no feature map ever fitted its LDS budget (csrc/gemm_tiles.def); the id stays reserved
    17: ("H192x64", "halo", 192, 64),
    18: ("P256x128", "ps", 256, 128), 19: ("P128x128", "ps", 128, 128), 20: ("P2_128x128", "ps", 128, 128),
    21: ("P128", "pgeglu", 128, 128), 22: ("P64", "pgeglu", 64, 128),
    23: ("HP192x64", "halo", 192, 64), 24: ("HP128x64", "halo", 128, 64), 25: ("HP128x128", "halo", 128, 128),
    26: ("P64x64", "ps", 64, 64), 27: ("P2_64x64", "ps", 64, 64), 28: ("P128x64", "ps", 128, 64), 29: ("P64x128", "ps", 64, 128),
    30: ("P128w8", "pgeglu", 128, 128), 31: ("P128w8L", "pgeglu", 128, 128),
    32: ("W256", "wgeglu", 256, 320), 33: ("W128", "wgeglu", 128, 320), 34: ("W64", "wgeglu", 64, 320),
}
_TILE_RETIRED = {16: (512, 8)}      # (DMA threads, weight ring) of a retired halo id that the GPU tests' literal lists still name


def test_gemm_tile_table_is_pinned():
    """df_test_gemm_tile_info answers on the host, on both builds, with the 35 rows written out above, and refuses ids outside the
    table.  The literal tile lists the GPU tests keep (an independent restatement there) equal what the table says: generic +
    producer-specialised ids, halo ids with their (BM, BN, DMA threads, weight ring), the generic ids that take MODE 2, the row
    count.  A retired id stays in the halo lists of the GPU tests (they skip a pair the library refuses); the table must refuse it."""
    import ctypes as C
    import test_backward_kernels_gpu as TB
    import test_gemm_epilogues_gpu as TG
    import test_kernels_gpu as TK
    for prec in ("bf16", "fp16"):
        L = E.lib(prec)
        tiles = E.gemm_tiles(L)
        assert {t: (r["name"], r["family"], r["bm"], r["bn"]) for t, r in tiles.items()} == _TILE_TABLE
        info = E.GemmTile(size=C.sizeof(E.GemmTile))
        for bad in (-1, len(_TILE_TABLE), 1 << 20):
            assert L.df_test_gemm_tile_info(bad, C.byref(info)) != 0
        info.size -= 8
        assert L.df_test_gemm_tile_info(0, C.byref(info)) != 0
        fam = lambda *names: [t for t, r in tiles.items() if r["family"] in names]
        assert TG.TILE_ALL == len(tiles)
        assert TK.TILES == fam("generic", "ps")
        assert TB._TILES_S2 == [t for t in fam("generic") if 2 in tiles[t]["modes"]] == fam("generic")
        halo = {t: (r["bm"], r["bn"], r["dma_threads"], r["ring"]) for t, r in tiles.items() if r["family"] == "halo"}
        for t, geo in _TILE_RETIRED.items():
            assert tiles[t]["family"] == "retired" and tiles[t]["modes"] == ()
            halo[t] = (tiles[t]["bm"], tiles[t]["bn"]) + geo
        assert TK._HALO_GEO == halo and list(TK.HALO) == sorted(halo)
        # a retired id is refused for every problem: the conv every live halo tile accepts, and a plain linear
        conv = E.GemmDesc(conv=1, NB=2, H=16, Wd=64, Cin=64, N=64, stride=1)
        lin = E.GemmDesc(M=256, N=128, K=256)
        for t, r in tiles.items():
            if r["family"] == "halo":
                assert r["modes"] == (1,) and L.df_test_gemm_valid(C.byref(conv), t, 1, 1) == 1
            if r["family"] == "retired":
                assert L.df_test_gemm_valid(C.byref(conv), t, 1, 1) == 0 and L.df_test_gemm_valid(C.byref(lin), t, 1, 1) == 0


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
