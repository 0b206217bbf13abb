"""GPU: the seven fixed-shape GEMM test entry points (df_test_gemm, _epi, _dual, df_test_conv3x3, _skip, _ups4, df_test_geglu)
are fills of df_test_gemm_desc: each is called once and then df_test_gemm_ex with the equivalent descriptor written out here, on the
same operands and NaN-prefilled outputs.  Same kernel, same tile, deterministic slab reduce: the outputs are equal bit for bit
(torch.equal also fails on an element either launch left at NaN).  Shapes are the smallest that still exercise each field: a ragged
M tile (72 rows on the 64 x 64 tile), split-K slabs, the four-slab phase-decomposed conv, a halo tile.  Every test runs on both
builds."""
import ctypes as C

import pytest
import torch

from helpers import rnd

pytestmark = pytest.mark.gpu

PREC = "bf16"


@pytest.fixture(params=["bf16", "fp16"], autouse=True)
def prec(request):
    global PREC
    PREC = request.param
    yield PREC
    PREC = "bf16"


def _eng():
    from diff_foley_amd import engine as E
    return E


def lib():
    return _eng().lib(PREC)


def op(t):
    return t.to(_eng().OPERAND_DTYPE[PREC]).cuda().contiguous()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def both(shape, operand_out, shim, tile, splitk, **fields):
    """shim(C) through the old entry point, then df_test_gemm_ex with `fields`; both into NaN-prefilled outputs of `shape`."""
    L = lib()
    dt = _eng().OPERAND_DTYPE[PREC] if operand_out else torch.float32
    c_shim = torch.full(shape, float("nan"), dtype=dt, device="cuda")
    c_desc = torch.full(shape, float("nan"), dtype=dt, device="cuda")
    rc = shim(c_shim)
    assert rc == 0, L.df_last_error()
    d = _eng().GemmDesc(C=c_desc.data_ptr(), tile=tile, splitk=splitk, out_operand=1 if operand_out else 0, **fields)
    rc = L.df_test_gemm_ex(C.byref(d), stream())
    assert rc == 0, L.df_last_error()
    torch.cuda.synchronize()
    assert torch.equal(c_shim, c_desc)


M, N, K = 72, 192, 256


@pytest.mark.parametrize("splitk", [1, 2])
def test_gemm(splitk):
    a, w = op(rnd((M, K), 1)), op(rnd((N, K), 2) / K ** 0.5)
    both((M, N), False, lambda c: lib().df_test_gemm(ptr(a), ptr(w), ptr(c), M, N, K, 3, splitk, stream()), 3, splitk,
         A=a.data_ptr(), W=w.data_ptr(), M=M, N=N, K=K)


def test_gemm_epi():
    a, w = op(rnd((M, K), 3)), op(rnd((N, K), 4) / K ** 0.5)
    bias, res = rnd((N,), 5).cuda(), rnd((M, N), 6).cuda()
    both((M, N), True, lambda c: lib().df_test_gemm_epi(ptr(a), ptr(w), ptr(bias), ptr(res), ptr(c), M, N, K, 1, 1, 3, 2, stream()), 3, 2,
         A=a.data_ptr(), W=w.data_ptr(), M=M, N=N, K=K, bias=bias.data_ptr(), res=res.data_ptr(), ldr=N, silu=1)


def test_gemm_dual():
    K1, K2 = 128, 64
    a, a2, w = op(rnd((M, K1), 7)), op(rnd((M, K2), 8)), op(rnd((N, K1 + K2), 9) / (K1 + K2) ** 0.5)
    both((M, N), False, lambda c: lib().df_test_gemm_dual(ptr(a), ptr(a2), ptr(w), ptr(c), M, N, K1, K2, 3, 1, stream()), 3, 1,
         A=a.data_ptr(), W=w.data_ptr(), M=M, N=N, K=K1, A2=a2.data_ptr(), lda2=K2, Cin2=K2)


NB, H, W, CIN, COUT = 1, 4, 16, 64, 64


@pytest.mark.parametrize("tile,stride", [(3, 1), (5, 1), (3, 2)])       # 5: the 128 x 64 halo tile
def test_conv3x3(tile, stride):
    a, w, bias = op(rnd((NB * H * W, CIN), 10)), op(rnd((COUT, 9 * CIN), 11) / (3 * CIN ** 0.5)), rnd((COUT,), 12).cuda()
    rows = NB * (H // stride) * (W // stride)
    both((rows, COUT), False,
         lambda c: lib().df_test_conv3x3(ptr(a), ptr(w), ptr(bias), ptr(c), NB, H, W, CIN, COUT, stride, 0, tile, 1, stream()), tile, 1,
         A=a.data_ptr(), W=w.data_ptr(), conv=1, NB=NB, H=H, Wd=W, Cin=CIN, N=COUT, stride=stride, bias=bias.data_ptr())


def test_conv3x3_skip():
    CIN2 = 64
    a, a2 = op(rnd((NB * H * W, CIN), 13)), op(rnd((NB * H * W, CIN2), 14))
    w, bias = op(rnd((COUT, 9 * CIN + CIN2), 15) / (3 * CIN ** 0.5)), rnd((COUT,), 16).cuda()
    both((NB * H * W, COUT), False,
         lambda c: lib().df_test_conv3x3_skip(ptr(a), ptr(a2), ptr(w), ptr(bias), ptr(c), NB, H, W, CIN, CIN2, COUT, 3, 1, stream()), 3, 1,
         A=a.data_ptr(), W=w.data_ptr(), conv=1, NB=NB, H=H, Wd=W, Cin=CIN, N=COUT, stride=1, A2=a2.data_ptr(), lda2=CIN2, Cin2=CIN2,
         bias=bias.data_ptr())


@pytest.mark.parametrize("splitk", [1, 2])       # the only entry whose split-K leaves four slabs per split
def test_conv3x3_ups4(splitk):
    a, w, bias = op(rnd((NB * H * W, CIN), 17)), (rnd((COUT, CIN, 3, 3), 18) / (3 * CIN ** 0.5)).cuda(), rnd((COUT,), 19).cuda()
    w4 = torch.zeros(16 * COUT * CIN, dtype=_eng().OPERAND_DTYPE[PREC], device="cuda")      # packed by the entry point, read by the descriptor
    both((NB * 4 * H * W, COUT), False,
         lambda c: lib().df_test_conv3x3_ups4(ptr(a), ptr(w), ptr(bias), ptr(c), ptr(w4), NB, H, W, CIN, COUT, 3, splitk, stream()), 3,
         splitk, A=a.data_ptr(), W=w4.data_ptr(), conv=2, NB=NB, H=H, Wd=W, Cin=CIN, N=COUT, bias=bias.data_ptr())


def test_geglu():
    Mg, Kg, N1 = 64, 128, 256
    x, Wf = rnd((Mg, Kg), 20) * 1.5 + 0.3, rnd((N1, Kg), 21) * 0.06
    w = op(Wf)
    cs = w.float().sum(1).contiguous()              # column sums of the operand-rounded rows, as the packer computes them
    bias = (rnd((N1,), 22) * 0.2).cuda()
    xs = x.view(Mg, Kg // 64, 64)
    stats = torch.stack([xs.sum(2), (xs * xs).sum(2)], dim=-1).contiguous().cuda()      # per-row partials over 64-column slots
    a = op(x)
    both((Mg, N1 // 2), True,
         lambda c: lib().df_test_geglu(ptr(a), ptr(w), ptr(stats), ptr(cs), ptr(bias), ptr(c), Mg, Kg, N1, 3, 0, stream()), 3, 1,
         A=a.data_ptr(), W=w.data_ptr(), M=Mg, N=N1, K=Kg, geglu=1, ln_stats=stats.data_ptr(), ln_slots=Kg // 64, ln_C=Kg, ln_eps=1e-5,
         ln_cs=cs.data_ptr(), bias=bias.data_ptr())
