"""CPU: the one launch decision of the GEMM stack (csrc/gemm.hip gemm_route) through its host-only query df_test_gemm_why --
0 launchable and inside the tuner's split policy, 1 launchable and outside it, 2 refused with the rule.  launch_gemm asks the same
function first, so what is refused here is never launched (tests/test_gemm_route_gpu.py)."""
import ctypes as C
import os

import pytest

from diff_foley_amd import engine as E

_ONE = (C.c_float * 4096)()
P = C.addressof(_ONE)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not all(os.path.exists(p) for p in E.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()


def why(L, d, tile, sk=1, batch=1):
    buf = C.create_string_buffer(256)
    r = L.df_test_gemm_why(C.byref(d), tile, batch, sk, buf, 256)
    assert r >= 0, L.df_last_error()
    assert (r == 0) == (L.df_test_gemm_valid(C.byref(d), tile, batch, sk) == 1)
    assert (r == 2) == bool(buf.value), (r, buf.value)
    return r, buf.value.decode()


def lin(**kw):
    kw = dict(dict(M=128, N=128, K=192), **kw)
    return E.GemmDesc(A=P, W=P, C=P, **kw)


def conv(**kw):
    return E.GemmDesc(A=P, W=P, C=P, conv=1, NB=2, H=8, Wd=16, Cin=128, N=128, stride=1, **kw)


LN = dict(ln_stats=P, ln_slots=3, ln_C=192, ln_cs=P, bias=P)
VT = dict(M=128, N=384, K=192, vt=P, vt_col0=192, vt_T=64, ldvt=72, ldc=200, out_operand=1, **LN)
XS = dict(M=128, N=128, K=192, out_operand=1, w_rows=64, sm_w=32, sm_valid=17, **LN)
PG = dict(N=2560, K=128, geglu=1, out_operand=1, ln_stats=P, ln_slots=2, ln_C=128, ln_cs=P, bias=P)

# (name, accepted descriptor, refused descriptor, tile, split-K, words of the rule that refuses).  The first group are rules only
# launch_gemm or a launcher under it knew before there was one decision function; the second are descriptors launch_gemm used to
# LAUNCH, with a silently wrong result, unless the caller had asked gemm_tile_valid by hand.
MOVED = [
    # the PROD / LNC / GEGLU / XS epilogues are built for linear GEMMs; a conv's statistics come from the split-K reduce
    ("stats_conv", None, conv(stats=P, stats_slots=2), 3, 1, "MODE 0"),
    ("stats_conv_splitk", conv(stats=P, stats_slots=2), None, 3, 2, ""),
    ("aux_ln", lin(**LN), lin(aux=P, ld_aux=128, **LN), 3, 1, "aux with ln_stats"),
    ("alpha_geglu", lin(geglu=1, out_operand=1), lin(geglu=1, out_operand=1, alpha=0.5), 3, 1, "alpha / relu / silu"),
    ("relu_stats", lin(stats=P, stats_slots=2), lin(stats=P, stats_slots=2, relu=1), 3, 1, "alpha / relu / silu"),
    ("cfg_odd_m", lin(M=8, N=4, K=256, store_nchw=1, hw_out=4, cfg_out=P, cfg_scale=2.0),
     lin(M=9, N=4, K=256, store_nchw=1, hw_out=4, cfg_out=P, cfg_scale=2.0), 3, 2, "cfg_out"),
    ("dup_defer", lin(M=64, K=256, dup_rows=64), lin(M=64, K=256, dup_rows=64, defer_reduce=1), 3, 2, "deferred"),
    ("stats_n96", lin(stats=P, stats_slots=2), lin(N=96, stats=P, stats_slots=2), 3, 1, "N % 64"),
    ("vt_T", lin(**VT), lin(**dict(VT, vt_T=62)), 3, 1, "vt_T"),
    # the persistent GEGLU kernel: 32-bit byte offsets into its output, and the LNS column of its tile's row
    ("pgeglu_2gib", lin(M=1 << 19, **PG), lin(M=1 << 20, **PG), 22, 1, "2 GiB"),
    ("pgeglu_lns", lin(M=64, **dict(PG, K=640, ln_slots=10, ln_C=640)), lin(M=64, **dict(PG, K=1280, ln_slots=20, ln_C=1280)), 30, 1, "LNS"),
]
HOLES = [
    ("vt_splitk", lin(**VT), 3, 2, "vt"),
    ("sm_w_splitk", lin(**XS), 3, 2, "sm_w"),
    ("geglu_ln_splitk", lin(geglu=1, out_operand=1, **LN), 3, 2, "scalar reduce"),
    ("w_rows_bm", lin(M=96, w_rows=48), 3, 1, "w_rows"),
    ("vt_col0_bn", lin(**VT), 0, 1, "vt_col0"),          # 192 is no multiple of the 128 columns of tile 0
    ("dup_geglu", lin(geglu=1, out_operand=1, dup_rows=128), 3, 1, "dup_rows"),
]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_every_moved_rule_answers_with_its_reason(prec):
    """One accepted and one refused query per rule that moved into gemm_route from launch_gemm, launch_cfg or launch_pgeglu; the
    refusal names that rule.  Not expressible through a descriptor, so not here: the MODE 3 shape conditions (the entry's
    gp_conv3_ups4 derives OH, OW, K and w_bs itself), the halo tiles' 2^22-patch bound (a 2 GiB operand comes first)."""
    L = E.lib(prec)
    for name, ok, bad, tile, sk, words in MOVED:
        if ok is not None:
            r, msg = why(L, ok, tile, sk)
            assert r in (0, 1), f"{name}: the accepted form is refused: {msg}"
        if bad is not None:
            r, msg = why(L, bad, tile, sk)
            assert r == 2 and words in msg, f"{name}: {r} {msg!r}"


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_descriptors_launch_gemm_used_to_launch_wrongly_are_refused(prec):
    """Transposed V, the score softmax and LayerNorm-folded GEGLU with split-K (no reduce kernel knows them), per-sample weights
    that are no whole row tiles, a V^T column range that starts inside a tile, duplicated rows with GEGLU: each is refused, by the
    function launch_gemm itself asks.  The halo tiles' lda % 8 rule cannot be expressed through a descriptor: the entry's gp_conv3
    sets lda = Cin, and Cin is a multiple of 64."""
    L = E.lib(prec)
    for name, d, tile, sk, words in HOLES:
        r, msg = why(L, d, tile, sk)
        assert r == 2 and words in msg, f"{name}: {r} {msg!r}"
    # ... and each of them is fine where the rule does not bite
    for d, tile, sk in ((lin(**VT), 3, 1), (lin(**XS), 3, 1), (lin(geglu=1, out_operand=1, **LN), 3, 1), (lin(M=128, w_rows=64), 3, 1)):
        assert why(L, d, tile, sk)[0] == 0


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_split_policy_is_not_a_refusal(prec):
    """72 x 128 x 192 is three K steps: split-K 2 leaves a slab with one, which the tuner does not time (1) -- it still runs."""
    L = E.lib(prec)
    d = lin(M=72, N=128, K=192)
    assert why(L, d, 3, 2) == (1, "")
    assert L.df_test_gemm_valid(C.byref(d), 3, 1, 2) == 0
    assert why(L, d, 3, 1) == (0, "")
    assert why(L, lin(M=72, N=128, K=256), 3, 2) == (0, "")
    # halo tiles: one 64-channel chunk per slab is enough for the tuner, none is outside its policy
    assert why(L, conv(), 5, 2)[0] == 0 and why(L, conv(), 5, 3)[0] == 1
    bad = lin()
    bad.size -= 8
    assert L.df_test_gemm_why(C.byref(bad), 3, 1, 1, None, 0) == -1 and b"descriptor" in L.df_last_error()
