"""GPU: the two kernels of csrc/dpm.hip through their C ABI, each alone, against float64 applied to the very fp32 inputs the kernel reads.

  df_dpm_data_prediction  x0 = (x - sigma eps) / alpha; thresholding: s = max(quantile_0.995(|x0|), max_val), clamp(x0, -s, s) / s
                          dpm_solver.py:386-399
  df_dpm_adaptive_error   max_b sqrt(mean(((x_hi - x_lo) / max(atol, rtol max(|x_lo|, |x_prev|)))^2))      dpm_solver.py:952-954

Bounds (u = 2^-24; derived, not measured):
  x0, per element: 2 u (|x| + |sigma eps|) / alpha -- one FMA and one division, each rounded once (the per-term bound of df_q_sample).
  s: within 4 ulp of torch.quantile(|x0|, 0.995) on the kernel's own fp32 x0 (the plain launch returns it: both launches evaluate
      one expression), then max(., max_val).  The selection is exact; rank, weight and the interpolation round three times.
  thresholded output, per element: the x0 bound divided by s, plus 2 u |out| for the division by s (the clamp is exact).
  the error norm, relative: 1e-5, the bound df_diffusion_loss carries -- non-negative terms, at most n / 256 chained additions a lane
      (n <= 4097 here: 17) plus the 10 levels of the trees, the quotient, the square, the mean and the root: under 40 u = 2.4e-6.

Both builds hold the same fp32 kernels; both are run."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_foley_amd import engine as E

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -12345.0
SIZES = [1, 2, 60, 201, 202, 4096, 4097]      # 60 = 4 * 3 * 5; 201: rank 0.995 * 200 = 199 exactly; 4096 / 4097: four passes of the block


@pytest.fixture(params=["bf16", "fp16"])
def L(request):
    return E.lib(request.param)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _padded(shape, pad=64):
    """A device view of ``shape`` inside a sentinel-filled allocation with ``pad`` sentinel elements on both sides."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), SENTINEL, device="cuda")
    return buf[pad:pad + n].view(shape), buf, pad


def _pads_intact(buf, pad):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all())


def _data_prediction(L, x, eps, alpha, sigma, thresholding, max_val):
    B, n = x.shape
    out, obuf, pad = _padded((B, n))
    s, sbuf, spad = _padded((B,))
    rc = L.df_dpm_data_prediction(ptr(x), ptr(eps), ptr(out), ptr(s) if thresholding else None, B, n, alpha, sigma,
                                  1 if thresholding else 0, max_val, stream())
    assert rc == 0, L.df_last_error().decode()
    torch.cuda.synchronize()
    assert _pads_intact(obuf, pad) and _pads_intact(sbuf, spad)
    if not thresholding:
        assert bool((s == SENTINEL).all())          # s_out is not written without thresholding
    return out.cpu(), s.cpu()


# family -> (x, eps, max_val) for a sample size; x0 = (x - sigma eps) / alpha.  eps = 0 keeps ties of x as ties of x0.
def _family(name, B, n, g):
    z = torch.zeros(B, n)
    if name == "normal":
        return 2 * torch.randn(B, n, generator=g), torch.randn(B, n, generator=g), 1.0
    if name == "all_equal":                       # every order statistic is the same value
        return torch.full((B, n), 0.7), z, 0.5
    if name == "ties":                            # five values: the two ranks fall inside a run of ties, or straddle its end
        vals = torch.tensor([0.5, 1.0, 1.5, 2.0, 3.0])
        x = vals[torch.randint(0, 5, (B, n), generator=g)] * (2 * torch.randint(0, 2, (B, n), generator=g) - 1)
        if n >= 201:                              # a run of ties that ENDS at rank k = floor(0.995 (n - 1)): rank k + 1 is the first
            k = int(np.floor(np.float32(0.995) * np.float32(n - 1)))      # element above it (n = 201: rank 199 exactly, no interpolation)
            x[:, :] = 2.0
            x[:, 3:3 + (n - 1 - k)] = -3.0
        return x, z, 0.5
    if name == "zeros":                           # quantile 0: s = max_val
        return z.clone(), z, 1.0
    if name == "below_max_val":
        return 0.1 * torch.randn(B, n, generator=g), 0.1 * torch.randn(B, n, generator=g), 2.0
    if name == "mostly_negative":
        x = -3 * torch.randn(B, n, generator=g).abs()
        x[:, ::7] = 0.25
        return x, 0.1 * torch.randn(B, n, generator=g), 0.5
    raise KeyError(name)


FAMILIES = ["normal", "all_equal", "ties", "zeros", "below_max_val", "mostly_negative"]
ALPHA, SIGMA = 0.8, 0.6


def _check_thresholding(L, x, eps, max_val, what):
    B, n = x.shape
    xd, ed = x.cuda(), eps.cuda()
    x0_k, _ = _data_prediction(L, xd, ed, ALPHA, SIGMA, False, max_val)
    a64, s64 = float(np.float32(ALPHA)), float(np.float32(SIGMA))
    x0_64 = (x.double() - s64 * eps.double()) / a64
    b_x0 = 2 * U * (x.double().abs() + (s64 * eps.double()).abs()) / a64
    clean = ~torch.isnan(x0_64).any(1)
    assert bool(((x0_k.double() - x0_64).abs() <= b_x0)[clean].all()), what
    out, s = _data_prediction(L, xd, ed, ALPHA, SIGMA, True, max_val)
    out2, s2 = _data_prediction(L, xd, ed, ALPHA, SIGMA, True, max_val)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(s.view(torch.int32), s2.view(torch.int32)), what
    q = torch.quantile(x0_k.abs(), 0.995, dim=1)                              # fp32, the 'linear' rule, NaN for a sample with a NaN
    s_ref = torch.maximum(q, torch.full_like(q, max_val))
    assert torch.equal(torch.isnan(s), ~clean) and torch.equal(torch.isnan(s_ref), ~clean), what
    assert bool(torch.isnan(out[~clean]).all()), what                         # the whole sample, as torch.quantile poisons s
    if clean.any():
        sk, sr = s[clean].numpy(), s_ref[clean].numpy()
        assert (np.abs(sk.astype(np.float64) - sr.astype(np.float64)) <= 4 * np.spacing(sr).astype(np.float64)).all(), (what, sk, sr)
        s_k = s[clean].double()[:, None]
        ref = torch.clamp(x0_64[clean], -s_k, s_k) / s_k
        bound = b_x0[clean] / s_k + 2 * U * ref.abs()
        err = (out[clean].double() - ref).abs()
        assert bool((err <= bound).all()), (what, float((err / bound.clamp_min(1e-300)).max()))
        assert float(out[clean].abs().max()) <= 1.0


@pytest.mark.parametrize("B", [1, 3, 5])
def test_thresholded_data_prediction_against_torch_quantile_and_float64(L, B):
    for n in SIZES:
        for k, fam in enumerate(FAMILIES):
            x, eps, max_val = _family(fam, B, n, _gen(100 * n + 10 * B + k))
            _check_thresholding(L, x, eps, max_val, (fam, B, n))
        # one NaN sample among clean ones (B = 1: the only one)
        x, eps, max_val = _family("normal", B, n, _gen(7 * n + B))
        x[B // 2, n // 3] = float("nan")
        _check_thresholding(L, x, eps, max_val, ("nan", B, n))


def test_thresholding_at_the_largest_latent(L):
    """n = 4 * 16 * 1024: 64 elements a lane a pass."""
    g = _gen(65536)
    x, eps = 2 * torch.randn(2, 65536, generator=g), torch.randn(2, 65536, generator=g)
    _check_thresholding(L, x, eps, 1.0, ("normal", 2, 65536))
    _check_thresholding(L, x, eps, 10.0, ("max_val wins", 2, 65536))


def test_plain_data_prediction_and_the_python_wrapper(L):
    g = _gen(5)
    x, eps = torch.randn(3, 4, 5, 7, generator=g), torch.randn(3, 4, 5, 7, generator=g)
    a, s = np.float32(0.31), np.float32(0.95)
    x0 = E.dpm_data_prediction(x.cuda(), eps.cuda(), a, s)
    ref = (x.double() - float(s) * eps.double()) / float(a)
    assert x0.shape == x.shape and bool(((x0.cpu().double() - ref).abs() <= 2 * U * (x.double().abs() + float(s) * eps.double().abs()) / float(a)).all())
    thr, sv = E.dpm_data_prediction(x.cuda(), eps.cuda(), a, s, True, 1.0, return_s=True)
    q = torch.maximum(torch.quantile(x0.cpu().abs().reshape(3, -1), 0.995, dim=1), torch.ones(3))
    assert (np.abs(sv.cpu().numpy().astype(np.float64) - q.numpy()) <= 4 * np.spacing(q.numpy())).all()
    assert float(thr.abs().max()) <= 1.0 and thr.shape == x.shape
    with pytest.raises(ValueError, match=r"expected \(3, 4, 5, 7\)"):
        E.dpm_data_prediction(x.cuda(), eps[:2].cuda(), a, s)
    assert L.df_dpm_data_prediction(None, ptr(x0), ptr(x0), None, 3, 140, 1.0, 0.0, 0, 1.0, stream()) != 0      # a null pointer is an error
    assert L.df_dpm_data_prediction(ptr(x0), ptr(x0), ptr(thr), None, 0, 140, 1.0, 0.0, 1, 1.0, stream()) != 0


def _error_ref(hi, lo, prev, atol, rtol):
    a, r = float(np.float32(atol)), float(np.float32(rtol))
    delta = torch.maximum(torch.full_like(hi.double(), a), r * torch.maximum(lo.double().abs(), prev.double().abs()))
    v = (hi.double() - lo.double()) / delta
    norm = torch.sqrt((v * v).mean(1))
    return norm, norm.max(), delta


def _adaptive_error(L, hi, lo, prev, atol, rtol):
    B, n = hi.shape
    norm, nbuf, npad = _padded((B,))
    out, obuf, opad = _padded((1,))
    rc = L.df_dpm_adaptive_error(ptr(hi), ptr(lo), ptr(prev), ptr(norm), ptr(out), B, n, atol, rtol, stream())
    assert rc == 0, L.df_last_error().decode()
    torch.cuda.synchronize()
    assert _pads_intact(nbuf, npad) and _pads_intact(obuf, opad)
    return norm.cpu(), out.cpu()


@pytest.mark.parametrize("B", [1, 3, 5])
def test_adaptive_error_against_float64(L, B):
    atol, rtol = 0.0078, 0.05
    for n in SIZES:
        g = _gen(31 * n + B)
        lo, prev = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
        d = torch.randn(B, n, generator=g)
        small = torch.where(torch.arange(n) % 2 == 1, 1e-2, 1.0)
        cases = {"atol wins": (1e-3 * lo, 1e-3 * prev, 1e-3 * d),            # rtol max(|lo|, |prev|) ~ 5e-5 < atol everywhere
                 "rtol wins": (3 * lo + 5 * lo.sign(), 3 * prev, 0.2 * d),   # |lo| >= 5: rtol |lo| >= 0.25 > atol everywhere
                 # one sample repeated with a growing difference: the norms grow with b, the maximum sits in the last sample
                 # (every second element a hundred times smaller: there atol wins, elsewhere rtol does)
                 "mixed, max in the last sample": ((lo * small)[:1].repeat(B, 1), (0.1 * prev * small)[:1].repeat(B, 1),
                                                   0.05 * d[:1] * torch.linspace(0.2, 2.0, B)[:, None])}
        for what, (l, p, dd) in cases.items():
            h = l + dd
            ref_norm, ref_max, delta = _error_ref(h, l, p, atol, rtol)
            a32 = float(np.float32(atol))
            if what == "atol wins":
                assert bool((delta == a32).all())
            elif what == "rtol wins":
                assert bool((delta > a32).all())
            else:
                assert int(ref_norm.argmax()) == B - 1
                if n >= 60:      # both branches of the max in one sample
                    assert bool((delta == a32).any()) and bool((delta > a32).any())
            args = (h.cuda(), l.cuda(), p.cuda())
            norm, out = _adaptive_error(L, *args, atol, rtol)
            norm2, out2 = _adaptive_error(L, *args, atol, rtol)
            assert torch.equal(norm.view(torch.int32), norm2.view(torch.int32)) and torch.equal(out.view(torch.int32), out2.view(torch.int32))
            assert bool(((norm.double() - ref_norm).abs() <= 1e-5 * ref_norm).all()), (what, B, n)
            assert abs(float(out[0]) - float(ref_max)) <= 1e-5 * float(ref_max), (what, B, n)
            assert float(out[0]) == float(norm.max())                        # the second launch only selects
            E_dev, norm_dev = E.dpm_adaptive_error(*args, atol, rtol)
            assert torch.equal(E_dev.cpu(), out) and torch.equal(norm_dev.cpu(), norm)


def test_adaptive_error_propagates_nan_and_refuses_bad_arguments(L):
    g = _gen(9)
    lo, prev, hi = (torch.randn(3, 200, generator=g) for _ in range(3))
    hi[1, 17] = float("nan")
    norm, out = _adaptive_error(L, hi.cuda(), lo.cuda(), prev.cuda(), 0.0078, 0.05)
    assert torch.isnan(norm).tolist() == [False, True, False] and bool(torch.isnan(out[0]))
    x = lo.cuda()
    assert L.df_dpm_adaptive_error(ptr(x), ptr(x), None, ptr(x), ptr(x), 3, 200, 0.1, 0.1, stream()) != 0
    assert L.df_dpm_adaptive_error(ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), 3, 0, 0.1, 0.1, stream()) != 0
    with pytest.raises(ValueError, match=r"expected \(3, 200\)"):
        E.dpm_adaptive_error(x, x[:2], x, 0.1, 0.1)
