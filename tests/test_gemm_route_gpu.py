"""GPU: launch_gemm obeys gemm_route (csrc/gemm.hip).  A descriptor the rules refuse is refused on the host, with the rule in the
message and nothing launched -- through df_test_gemm_ex, the entry that asks nothing before launch_gemm; a split the tuner's policy
leaves out (df_test_gemm_why == 1) still runs and is right."""
import ctypes as C

import pytest
import torch

from helpers import rnd, rel_l2
from test_gemm_route_cpu import HOLES, lin, why

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["bf16", "fp16"])
def prec(request):
    return request.param


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("name", [h[0] for h in HOLES])
def test_refused_descriptor_is_not_launched(prec, name):
    """The descriptors launch_gemm used to run with a silently wrong result (no reduce kernel knows vt / sm_w / GEGLU's ln_stats,
    ...): an error that names launch_gemm and the rule df_test_gemm_why gives, and C and V^T still all NaN after a synchronise."""
    from diff_foley_amd import engine as E
    L = E.lib(prec)
    _, d, tile, sk, _ = next(h for h in HOLES if h[0] == name)
    r, reason = why(L, d, tile, sk)
    assert r == 2 and reason
    assert d.M <= 128 and d.N <= 384 and d.K <= 256
    ins = torch.zeros(1 << 20, device="cuda")                 # every input pointer: 4 MiB of zeros, more than any operand here
    out = torch.full((2 * d.M + d.dup_rows, 1024), float("nan"), device="cuda")
    vt = torch.full((1 << 18,), float("nan"), device="cuda")
    run = lin()
    C.memmove(C.byref(run), C.byref(d), C.sizeof(d))
    for f, ctype in E.GemmDesc._fields_:
        if ctype is C.c_void_p and getattr(run, f):
            setattr(run, f, ins.data_ptr())
    run.C = out.data_ptr()
    if run.vt:
        run.vt = vt.data_ptr()
    run.tile, run.splitk = tile, sk
    rc = L.df_test_gemm_ex(C.byref(run), _stream())
    msg = L.df_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "launch_gemm refused" in msg and reason in msg, msg
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(vt).all()) and not bool(ins.any())


def test_split_outside_the_tuner_policy_runs(prec):
    """72 x 128 x 192 at split-K 2 on the 64 x 64 tile: three K steps, so one slab gets a single step -- outside the tuner's policy
    (1), inside what the kernels compute.  float64 reference, the fp32-output bound of tests/test_kernels_gpu.py."""
    from diff_foley_amd import engine as E
    L = E.lib(prec)
    M, N, K = 72, 128, 192
    a = rnd((M, K), 1).to(E.OPERAND_DTYPE[prec]).cuda()
    w = rnd((N, K), 2).to(E.OPERAND_DTYPE[prec]).cuda()
    c = torch.full((M, N), float("nan"), device="cuda")
    d = E.GemmDesc(A=a.data_ptr(), W=w.data_ptr(), C=c.data_ptr(), M=M, N=N, K=K, tile=3, splitk=2)
    assert why(L, d, 3, 2) == (1, "")
    assert L.df_test_gemm_ex(C.byref(d), _stream()) == 0, L.df_last_error()
    torch.cuda.synchronize()
    ref = a.double().cpu() @ w.double().cpu().t()
    err = rel_l2(c.cpu().double(), ref)
    print(f"\n72x128x192 split-K 2 [{prec}]: rel_l2 {float(err):.3g}")
    assert torch.isfinite(c).all() and err < 2e-3
