"""GPU: the two kernels of csrc/diffusion.hip through their C ABI, against the float64 restatement tests/diffusion_ref.py (pinned to
the reference's goldens by tests/test_diffusion_loss_cpu.py) applied to the very fp32 inputs the kernel reads.

  df_q_sample        out[b] = A[t[b]] x0[b] + S[t[b]] noise[b]                          ddpm.py:279-282, ddim.py:412-413
  df_diffusion_loss  per-sample mean of (target - pred)^2 | |target - pred| and the five scalars of loss_dict   ddpm.py:1061-1079

Bounds (u = 2^-24, the unit roundoff of fp32; derived, not measured):
  q_sample, per element: 2 u (|A x0| + |S noise|) -- two rounded products and one rounded sum, or one rounded product and one FMA.
  loss_simple, relative: 1e-5.  Every term is non-negative, so the relative error of a sum is at most (additions in the longest
      chain + 1) u: a lane chains at most n / 64 = 64 additions (this kernel: n / 256 = 16), the wavefront tree and the LDS step add
      at most 10 levels, the difference and the square / the division by n two more: (64 + 10 + 2) u = 4.5e-6 < 1e-5.
  the five scalars, relative: 1e-5 + B u -- the per-sample bound plus the chain over the batch.  The tables of these tests are
      non-negative (logvar in [0, 0.5], lvlb_weights in [0, 1], weights >= 0), which is what the bound assumes: a gamma term
      loss / exp(logvar) + logvar of mixed signs would be judged by its cancellation, not by the kernel.

Both builds hold the same fp32 kernels; both are run."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_foley_amd import engine as E
import diffusion_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(params=["bf16", "fp16"])
def L(request):
    return E.lib(request.param)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tables(T, seed):
    g = _gen(seed)
    a = torch.rand(T, generator=g)
    return a.sqrt().cuda(), (1 - a).sqrt().cuda()


def _slice(values, offset, pad=64):
    """``values`` (flat fp32, CPU) as a device view that starts ``offset`` elements into an allocation filled with the sentinel,
    with ``pad`` sentinel elements behind it: (view, whole allocation)."""
    buf = torch.full((offset + values.numel() + pad,), SENTINEL, device="cuda")
    view = buf[offset:offset + values.numel()]
    view.copy_(values)
    return view, buf


def _distinct_t(B, T, seed):
    """B distinct indices that include 0 and T - 1 where B allows."""
    t = [0, T - 1, T // 3][:B] if B <= 3 else [0, T - 1] + list(torch.randperm(T - 2, generator=_gen(seed))[:B - 2] + 1)
    return torch.tensor([int(v) for v in t], dtype=torch.int64)


# (x0, noise, out) offsets in elements from their allocations: aligned; shifted alike (float4 body behind a scalar head); one input
# or the output shifted alone (no common alignment: the scalar path)
OFFSETS = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 0, 3)]


@pytest.mark.parametrize("T", [1000, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_q_sample_element_by_element_against_float64(L, B, T):
    """n = 60, 4096 (float4 only), 4100 (float4 with a partial last pass), 4099 (odd: the head moves from sample to sample), each at
    every alignment of OFFSETS.  One test per (build, B, T) walks them: the cases are milliseconds each."""
    A, S = _tables(T, 7)
    for n in (60, 4096, 4100, 4099):
        g = _gen(1000 * B + n + T)
        x0, noise = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
        t = _distinct_t(B, T, n)
        ref, bound = R.q_sample_ref(x0, noise, t, A, S)
        for offsets in OFFSETS:
            _q_sample_case(L, x0, noise, t, A, S, T, offsets, ref, bound)


def _q_sample_case(L, x0, noise, t, A, S, T, offsets, ref, bound):
    B, n = x0.shape
    xv, _ = _slice(x0.flatten(), offsets[0])
    nv, _ = _slice(noise.flatten(), offsets[1])
    ov, obuf = _slice(torch.full((B * n,), SENTINEL), offsets[2])
    td = t.cuda()      # every device tensor stays referenced until the result is read: a freed block may be handed to the next one
    assert L.df_q_sample(ptr(xv), ptr(nv), ptr(td), ptr(A), ptr(S), ptr(ov), B, n, T, stream()) == 0, L.df_last_error()
    whole = obuf.cpu()
    out = whole[offsets[2]:offsets[2] + B * n].double().numpy().reshape(B, n)
    err = np.abs(out - ref)
    assert (err <= bound).all(), (n, offsets, float((err / np.maximum(bound, 1e-300)).max()), int((err > bound).sum()))
    assert (whole[:offsets[2]] == SENTINEL).all() and (whole[offsets[2] + B * n:] == SENTINEL).all(), (n, offsets)      # nothing outside B n elements


@pytest.mark.parametrize("T", [1000, 8])
@pytest.mark.parametrize("bad", ["T", -1])
def test_q_sample_out_of_range_index_is_nan_for_that_sample_only(L, bad, T):
    B, n = 3, 4100
    g = _gen(5)
    x0, noise = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    x0[1, :7] = 0.0                                   # NaN * 0 must still be NaN
    noise[1, :7] = 0.0
    t = torch.tensor([T - 1, T if bad == "T" else -1, 0], dtype=torch.int64)
    A, S = _tables(T, 9)
    out = torch.full((B * n + 64,), SENTINEL, device="cuda")
    xd, nd, td = x0.cuda(), noise.cuda(), t.cuda()
    assert L.df_q_sample(ptr(xd), ptr(nd), ptr(td), ptr(A), ptr(S), ptr(out), B, n, T, stream()) == 0
    got = out[:B * n].cpu().double().numpy().reshape(B, n)
    ref, bound = R.q_sample_ref(x0, noise, t, A, S)
    assert np.isnan(got[1]).all() and np.isnan(ref[1]).all()
    for b in (0, 2):
        assert (np.abs(got[b] - ref[b]) <= bound[b]).all()
    assert (out[B * n:] == SENTINEL).all()


def test_q_sample_refuses_empty_and_null_arguments(L):
    x = torch.zeros(8, device="cuda")
    t = torch.zeros(2, dtype=torch.int64, device="cuda")
    tab = torch.ones(4, device="cuda")
    for B, n, T in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4)):
        assert L.df_q_sample(ptr(x), ptr(x), ptr(t), ptr(tab), ptr(tab), ptr(x), B, n, T, stream()) != 0
    assert L.df_q_sample(ptr(x), None, ptr(t), ptr(tab), ptr(tab), ptr(x), 2, 4, 4, stream()) != 0
    assert b"null" in L.df_last_error()
    for B, n in ((0, 4), (2, 0)):
        assert L.df_diffusion_loss(ptr(x), ptr(x), ptr(t), ptr(tab), ptr(tab), ptr(x), ptr(x), B, n, 4, 0, 1.0, 0.0, stream()) != 0
    assert L.df_diffusion_loss(ptr(x), ptr(x), ptr(t), ptr(tab), ptr(tab), ptr(x), ptr(x), 2, 4, 4, 2, 1.0, 0.0, stream()) != 0
    assert b"loss_type" in L.df_last_error()


def test_q_sample_wrapper_takes_a_device_t_unread_and_checks_a_host_t():
    B, n, T = 3, 60, 8
    g = _gen(11)
    x0, noise = torch.randn(B, 3, 4, 5, generator=g), torch.randn(B, 3, 4, 5, generator=g)
    A, S = _tables(T, 3)
    t = torch.tensor([0, 7, 3])
    ref, bound = R.q_sample_ref(x0.reshape(B, n), noise.reshape(B, n), t, A, S)
    for tt in (t.cuda(), t, [0, 7, 3], t.int().cuda()):
        out = E.q_sample(x0.cuda(), noise.cuda(), tt, A, S)
        assert out.shape == x0.shape and (np.abs(out.cpu().double().numpy().reshape(B, n) - ref) <= bound).all()
    with pytest.raises(IndexError):
        E.q_sample(x0.cuda(), noise.cuda(), [0, 8, 3], A, S)
    nan = E.q_sample(x0.cuda(), noise.cuda(), torch.tensor([0, 8, 3]).cuda(), A, S)      # a device t is the kernel's to answer
    assert torch.isnan(nan[1]).all() and torch.isfinite(nan[0]).all() and torch.isfinite(nan[2]).all()
    assert E.q_sample(x0[:0].cuda(), noise[:0].cuda(), torch.zeros(0, dtype=torch.long), A, S).shape == (0, 3, 4, 5)


def _loss_inputs(B, n, T, seed):
    g = _gen(seed)
    pred, target = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    logvar, lvlb = 0.5 * torch.rand(T, generator=g), torch.rand(T, generator=g)
    return pred, target, _distinct_t(B, T, seed), logvar, lvlb


def _run_loss(L, pred, target, t, logvar, lvlb, loss_type, w_simple, w_elbo, offset=0):
    B, n = pred.shape
    pv, _ = _slice(pred.flatten(), offset)
    tv, _ = _slice(target.flatten(), offset)
    ls = torch.full((B + 16,), SENTINEL, device="cuda")
    sc = torch.full((5 + 16,), SENTINEL, device="cuda")
    td, lv, lw = t.cuda(), logvar.cuda(), lvlb.cuda()      # referenced until the result is read (see above)
    rc = L.df_diffusion_loss(ptr(pv), ptr(tv), ptr(td), ptr(lv), ptr(lw), ptr(ls), ptr(sc), B, n, logvar.numel(),
                             {"l2": 0, "l1": 1}[loss_type], w_simple, w_elbo, stream())
    assert rc == 0, L.df_last_error()
    ls, sc = ls.cpu(), sc.cpu()
    assert (ls[B:] == SENTINEL).all() and (sc[5:] == SENTINEL).all()
    return ls[:B], sc[:5]


SCALARS = ("simple", "gamma", "vlb", "loss", "logvar")


@pytest.mark.parametrize("B", [1, 3, 5])
def test_diffusion_loss_against_float64(L, B):
    """n = 60 and 4096, l2 and l1, tensors aligned (float4 loads) and shifted by one element (scalar loads): one test per (build, B)
    walks them."""
    for n in (60, 4096):
        for loss_type in ("l2", "l1"):
            for offset in (0, 1):
                _loss_case(L, B, n, loss_type, offset)


def _loss_case(L, B, n, loss_type, offset):
    T = 1000
    pred, target, t, logvar, lvlb = _loss_inputs(B, n, T, 100 * B + n)
    w_simple, w_elbo = 0.7, 0.25
    ls, sc = _run_loss(L, pred, target, t, logvar, lvlb, loss_type, w_simple, w_elbo, offset)
    ls_ref, sc_ref = R.diffusion_loss_ref(pred, target, t, logvar, lvlb, loss_type, w_simple, w_elbo)
    rel = np.abs(ls.double().numpy() - ls_ref) / ls_ref
    assert (rel <= 1e-5).all(), (n, loss_type, offset, rel)
    tol = 1e-5 + B * R.U
    for i, k in enumerate(SCALARS):
        assert abs(float(sc[i]) - sc_ref[k]) <= tol * abs(sc_ref[k]), (n, loss_type, offset, k, float(sc[i]), sc_ref[k])
    ls2, sc2 = _run_loss(L, pred, target, t, logvar, lvlb, loss_type, w_simple, w_elbo, offset)      # equal inputs, equal bits
    assert torch.equal(ls, ls2) and torch.equal(sc, sc2)


def test_diffusion_loss_of_equal_tensors_is_exactly_zero(L):
    pred, _, t, logvar, lvlb = _loss_inputs(3, 4096, 1000, 3)
    for loss_type in ("l2", "l1"):
        ls, sc = _run_loss(L, pred, pred.clone(), t, logvar, lvlb, loss_type, 1.0, 0.0)
        assert (ls == 0).all() and float(sc[0]) == 0.0 and float(sc[2]) == 0.0


@pytest.mark.parametrize("bad", [1000, -1])
def test_diffusion_loss_out_of_range_index_is_nan_for_that_sample_and_the_means(L, bad):
    pred, target, t, logvar, lvlb = _loss_inputs(3, 4096, 1000, 4)
    t = torch.tensor([999, bad, 0], dtype=torch.int64)
    ls, sc = _run_loss(L, pred, target, t, logvar, lvlb, "l2", 1.0, 0.5)
    ref = R.loss_simple_ref(pred, target, "l2")
    assert torch.isnan(ls[1]) and torch.isnan(sc[:4]).all()
    for b in (0, 2):
        assert abs(float(ls[b]) - ref[b]) <= 1e-5 * ref[b]
    assert abs(float(sc[4]) - float(logvar.double().mean())) <= (1e-5 + R.U) * float(logvar.double().mean())      # the table's own mean stands


def test_diffusion_loss_wrapper_and_an_empty_batch():
    pred, target, t, logvar, lvlb = _loss_inputs(3, 60, 8, 6)
    ls, sc = E.diffusion_loss(pred.reshape(3, 3, 4, 5).cuda(), target.reshape(3, 3, 4, 5).cuda(), t.cuda(), logvar, lvlb, "l1", 1.0, 0.5)
    ls_ref, sc_ref = R.diffusion_loss_ref(pred, target, t, logvar, lvlb, "l1", 1.0, 0.5)
    assert ls.shape == (3,) and sc.shape == (5,) and ls.is_cuda and sc.is_cuda
    assert np.allclose(ls.cpu().double().numpy(), ls_ref, rtol=1e-5, atol=0)
    assert np.allclose(sc.cpu().double().numpy(), [sc_ref[k] for k in SCALARS], rtol=1e-5 + 3 * R.U, atol=0)
    ls, sc = E.diffusion_loss(pred[:0].cuda(), target[:0].cuda(), torch.zeros(0, dtype=torch.long), logvar, lvlb)
    assert ls.shape == (0,) and torch.isnan(sc).all()
