"""GPU: the packing, casting, pooling, embedding, softmax and sampler kernels that so far ran only inside end-to-end tests (global
rel-L2 1.5e-2), one launcher at a time through the C ABI against plain torch.  Both operand builds.

Three kinds of check, per kernel:
  exact    pure data movement and single roundings: torch.equal on the bits, pad columns exactly zero, guard elements behind
           every output keep their sentinel.
  one ulp  an operand-type result of a short fp32 computation: within one operand-type ulp of the float64 result.
  fp32     every element within K * 2^-24 * sum|terms| of the float64 result on the same fp32 inputs, K = the largest number
           of fp32 roundings one term passes through on its way to the result (a K-term dot product: the product and K - 1
           additions; other formulas: counted in the test's docstring).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import rnd

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
U = 2.0 ** -24                    # unit round-off of fp32


def _eng():
    from diff_foley_amd import engine as E
    return E


PREC = "bf16"


@pytest.fixture(params=["bf16", "fp16"], autouse=True)
def prec(request):
    global PREC
    PREC = request.param
    yield PREC
    PREC = "bf16"


def odt():
    return _eng().OPERAND_DTYPE[PREC]


def op(t):
    return t.to(odt())


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    L = _eng().lib(PREC)
    rc = getattr(L, name)(*args, stream())
    assert rc == 0, L.df_last_error()
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int16)


def op_out(n, guard=64):
    """Operand-type output of n elements followed by `guard` sentinel elements that must survive."""
    return torch.full((n + guard,), SENTINEL, dtype=torch.int16, device="cuda").view(odt())


def f32_out(n, guard=64):
    return torch.full((n + guard,), float("nan"), device="cuda")


def take(buf, n, shape=None):
    """The first n elements on the host; asserts the guard behind them is untouched."""
    h = buf.cpu()
    tail = h[n:]
    if h.dtype == torch.float32:
        assert bool(torch.isnan(tail).all()), "written past the end of the output"
    else:
        assert bool((bits(tail) == SENTINEL).all()), "written past the end of the output"
    return h[:n].reshape(shape) if shape else h[:n]


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == torch.float32:
        return torch.equal(got.view(torch.int32), want.view(torch.int32))
    return torch.equal(bits(got), bits(want))


def ulp_op(y, dt):
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    return torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(2.0 ** emin))) - mant)


def within_f32(got, y64, K, abs_terms, what):
    """|got - y64| <= K 2^-24 sum|terms| for every element."""
    err = (got.double() - y64).abs()
    bound = K * U * abs_terms
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"MARGIN {what} {PREC} err/bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements beyond {K} x 2^-24 x sum|terms| (worst {worst:.2f} x)"


# ---------------------------------------------------------------------------------------------------------- CAVP data movement
@pytest.mark.parametrize("Fr,H,W,KP", [(3, 9, 11, 148), (2, 8, 12, 192), (1, 16, 7, 192), (2, 1, 1, 148)])
def test_stem_im2col(Fr, H, W, KP):
    """(1,7,7) stride-2 pad-3 patches: F.unfold of the zero-padded frame, reordered from unfold's (c, ky, kx) to the kernel's
    (ky, kx, c); columns [147, KP) exactly zero.  Odd and even H / W put the border taps on both sides."""
    x = rnd((Fr, 3, H, W), 70) + 2.0                       # no zeros inside the image: a border tap read as data shows
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    unf = F.unfold(F.pad(x, (3, 3, 3, 3)), kernel_size=7, stride=2)              # [F][3*49][OH*OW]
    assert unf.shape[2] == OH * OW
    ref = torch.zeros(Fr * OH * OW, KP)
    ref[:, :147] = unf.reshape(Fr, 3, 7, 7, OH * OW).permute(0, 4, 2, 3, 1).reshape(Fr * OH * OW, 147)
    xc, out = x.cuda(), op_out(Fr * OH * OW * KP)
    call("df_test_stem_im2col", ptr(xc), ptr(out), Fr, H, W, OH, OW, KP)
    got = take(out, Fr * OH * OW * KP, (Fr * OH * OW, KP))
    assert same_bits(got, op(ref))
    assert bool((bits(got[:, 147:]) == 0).all())


@pytest.mark.parametrize("Fr,H,W,Cc", [(2, 7, 9, 8), (3, 8, 6, 64), (1, 5, 5, 72), (2, 1, 2, 8)])
def test_maxpool3x3s2(Fr, H, W, Cc):
    """All inputs negative: a padding tap taken as 0 (or an accumulator started at 0) would win every border window."""
    x = op(-(rnd((Fr, Cc, H, W), 71).abs() + 0.5))
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ref = F.max_pool2d(x.float(), 3, 2, 1)
    assert ref.shape[2:] == (OH, OW) and bool((ref < 0).all())
    xc, out = x.permute(0, 2, 3, 1).contiguous().cuda(), op_out(Fr * OH * OW * Cc)
    call("df_test_maxpool3x3s2", ptr(xc), ptr(out), Fr, H, W, OH, OW, Cc)
    got = take(out, Fr * OH * OW * Cc, (Fr, OH, OW, Cc))
    assert same_bits(got, op(ref).permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("Fr,H,W,Cc", [(3, 6, 10, 8), (2, 2, 2, 64), (1, 14, 4, 72)])
def test_subsample2(Fr, H, W, Cc):
    x = op(rnd((Fr, H, W, Cc), 72))
    xc, n = x.cuda(), Fr * (H // 2) * (W // 2) * Cc
    out = op_out(n)
    call("df_test_subsample2", ptr(xc), ptr(out), Fr, H, W, Cc)
    assert same_bits(take(out, n, (Fr, H // 2, W // 2, Cc)), x[:, ::2, ::2, :].contiguous())


@pytest.mark.parametrize("clips,T,HW,Cc", [(3, 1, 5, 8), (3, 2, 4, 64), (4, 5, 3, 72), (1, 5, 7, 8)])
def test_tcat3(clips, T, HW, Cc):
    """(x[t-1] | x[t] | x[t+1]) with zeros outside each clip: the first and last frame of EVERY clip must see zeros, not the
    neighbouring clip's frame (no value of x is zero, so a leak cannot hide)."""
    Fr = clips * T
    x = op(rnd((clips, T, HW, Cc), 73).abs() + 1.0)
    z = torch.zeros_like(x[:, :1])
    ref = torch.cat([torch.cat([z, x[:, :-1]], 1), x, torch.cat([x[:, 1:], z], 1)], dim=-1).reshape(Fr, HW, 3 * Cc)
    xc, out = x.cuda(), op_out(Fr * HW * 3 * Cc)
    call("df_test_tcat3", ptr(xc), ptr(out), Fr, T, HW, Cc)
    assert same_bits(take(out, Fr * HW * 3 * Cc, (Fr, HW, 3 * Cc)), ref.contiguous())


@pytest.mark.parametrize("B,T,Cc,k", [(2, 37, 10, 16), (3, 16, 512, 16), (1, 7, 3, 2), (2, 5, 64, 5)])
def test_maxpool_time(B, T, Cc, k):
    x = -(rnd((B, T, Cc), 74).abs() + 0.25)                # negative: an accumulator started at 0 would win
    To = T // k
    ref = x[:, :To * k].reshape(B, To, k, Cc).amax(2)
    xc, out = x.cuda(), f32_out(B * To * Cc)
    call("df_test_maxpool_time", ptr(xc), ptr(out), B, T, Cc, k)
    assert same_bits(take(out, B * To * Cc, (B, To, Cc)), ref.contiguous())


@pytest.mark.parametrize("rows,Cc", [(5, 100), (7, 512), (2, 64), (6, 3)])
def test_l2norm_rows(rows, Cc):
    """x / max(||x||, 1e-12) in place.  A term x_i^2 passes its product and at most C - 1 additions (all terms positive:
    relative error of the sum <= C 2^-24), the square root halves that, then sqrt, reciprocal and the final product round
    once each: <= (C / 2 + 3) 2^-24 relative, bounded here by K = max(C, 6).  A zero row stays exactly zero."""
    x = rnd((rows, Cc), 75) * 3
    x[rows // 2] = 0
    y64 = x.double() / x.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    buf = f32_out(rows * Cc)
    buf[:rows * Cc] = x.flatten().cuda()
    call("df_test_l2norm_rows", ptr(buf), rows, Cc)
    got = take(buf, rows * Cc, (rows, Cc))
    assert bool((got[rows // 2] == 0).all())
    within_f32(got, y64, max(Cc, 6), y64.abs(), "l2norm_rows")


@pytest.mark.parametrize("O,I,KT,KH,KW,KP", [(16, 8, 3, 1, 1, 64), (8, 3, 1, 7, 7, 192), (5, 16, 1, 3, 3, 144)])
def test_pack_conv3d_bn(O, I, KT, KH, KW, KP):
    """Weights: w gamma / sqrt(var + eps) within one operand ulp of float64, layout [O][(kt, ky, kx, i)] zero padded to KP.
    Bias fp32 = beta - mean sc: the term mean sc passes var + eps, the reciprocal square root (1 ulp = two round-offs), the
    products with gamma and mean and the subtraction: K = 6."""
    w = rnd((O, I, KT, KH, KW), 76)
    gamma, beta, mean = rnd((O,), 77) * 0.3 + 1, rnd((O,), 78), rnd((O,), 79)
    var, eps = rnd((O,), 80).abs() + 0.1, 1e-5
    K = KT * KH * KW * I
    sc = gamma.double() / torch.sqrt(var.double() + float(np.float32(eps)))
    w64 = torch.zeros(O, KP, dtype=torch.float64)
    w64[:, :K] = (w.double() * sc[:, None, None, None, None]).permute(0, 2, 3, 4, 1).reshape(O, K)
    out, bias = op_out(O * KP), f32_out(O)
    dev = [t.cuda() for t in (w, gamma, beta, mean, var)]
    call("df_test_pack_conv3d_bn", *[ptr(t) for t in dev], eps, ptr(out), ptr(bias), O, I, KT, KH, KW, KP)
    got = take(out, O * KP, (O, KP))
    assert bool((bits(got[:, K:]) == 0).all())
    err = (got.double() - w64).abs()
    assert bool((err <= ulp_op(w64, odt())).all()), float((err / ulp_op(w64, odt())).max())
    within_f32(take(bias, O), beta.double() - mean.double() * sc, 6, beta.double().abs() + (mean.double() * sc).abs(), "pack_conv3d_bn bias")


# ---------------------------------------------------------------------------------------------------------- casts and broadcasts
@pytest.mark.parametrize("n", [1, 3, 1001, 4096 * 256 + 77])
def test_cast_to_operand(n):
    x = rnd((n,), 81) * 5
    xc, out = x.cuda(), op_out(n)
    call("df_test_cast_bf16", ptr(xc), ptr(out), n)
    assert same_bits(take(out, n), op(x))


@pytest.mark.parametrize("rows,Cc,ld", [(37, 10, 14), (1, 2, 2), (300, 320, 960), (5, 64, 66)])
def test_cast_to_operand_2d(rows, Cc, ld):
    x = torch.full((rows, ld), float("nan"))
    x[:, :Cc] = rnd((rows, Cc), 82) * 5
    xc, out = x.cuda(), op_out(rows * Cc)
    call("df_test_cast_bf16_2d", ptr(xc), ld, ptr(out), rows, Cc)
    assert same_bits(take(out, rows * Cc, (rows, Cc)), op(x[:, :Cc]))


@pytest.mark.parametrize("rows,n", [(8, 1280), (1, 4), (3, 5124)])
def test_bcast_rows(rows, n):
    src = rnd((n,), 83)
    sc, dst = src.cuda(), f32_out(rows * n)
    call("df_test_bcast_rows", ptr(sc), ptr(dst), rows, n)
    assert same_bits(take(dst, rows * n, (rows, n)), src[None].expand(rows, n).contiguous())


@pytest.mark.parametrize("N,per", [(3, 1000), (1, 1), (4, 4096 * 64 + 5)])
def test_grad_scale_per_sample(N, per):
    """x[n] *= 1 - prob[n]: one subtraction and one product, both correctly rounded on either side: exact."""
    x, prob = rnd((N, per), 84), torch.rand(N, generator=torch.Generator().manual_seed(85))
    buf = f32_out(N * per)
    buf[:N * per] = x.flatten().cuda()
    pc = prob.cuda()
    call("df_test_grad_scale_per_sample", ptr(buf), ptr(pc), N, per)
    assert same_bits(take(buf, N * per, (N, per)), x * (1.0 - prob)[:, None])


# ---------------------------------------------------------------------------------------------------------- weight packing
@pytest.mark.parametrize("O,I,KH,KW,Ipad", [(6, 5, 3, 3, 8), (4, 4, 1, 1, 64), (7, 64, 3, 3, 64), (3, 1, 1, 1, 2)])
def test_pack_conv_weight(O, I, KH, KW, Ipad):
    w = rnd((O, I, KH, KW), 86) + 3.0
    ref = torch.zeros(O, KH, KW, Ipad)
    ref[..., :I] = w.permute(0, 2, 3, 1)
    wc, out = w.cuda(), op_out(O * KH * KW * Ipad)
    call("df_test_pack_conv_weight", ptr(wc), ptr(out), O, I, KH, KW, Ipad)
    got = take(out, O * KH * KW * Ipad, (O, KH, KW, Ipad))
    assert same_bits(got, op(ref))
    assert bool((bits(got[..., I:]) == 0).all())


@pytest.mark.parametrize("O,I,I2", [(5, 8, 12), (64, 64, 128), (3, 2, 1)])
def test_pack_conv_skip(O, I, I2):
    w, ws = rnd((O, I, 3, 3), 87), rnd((O, I2), 88)
    ref = torch.cat([w.permute(0, 2, 3, 1).reshape(O, 9 * I), ws], 1)
    wc, wsc, out = w.cuda(), ws.cuda(), op_out(O * (9 * I + I2))
    call("df_test_pack_conv_skip", ptr(wc), ptr(wsc), ptr(out), O, I, I2)
    assert same_bits(take(out, O * (9 * I + I2), (O, 9 * I + I2)), op(ref))


def _geglu_rows(half):
    """Source row of packed row p: blocks of (32 x rows | 32 gate rows)."""
    p = torch.arange(2 * half)
    blk, r = p // 64, p % 64
    return torch.where(r < 32, blk * 32 + r, half + blk * 32 + (r - 32))


@pytest.mark.parametrize("half,K", [(32, 7), (96, 64), (1280, 20)])
def test_pack_geglu(half, K):
    w, b = rnd((2 * half, K), 89), rnd((2 * half,), 90)
    src = _geglu_rows(half)
    wc, bc, wout, bout = w.cuda(), b.cuda(), op_out(2 * half * K), f32_out(2 * half)
    call("df_test_pack_geglu", ptr(wc), ptr(bc), ptr(wout), ptr(bout), half, K)
    assert same_bits(take(wout, 2 * half * K, (2 * half, K)), op(w[src]))
    assert same_bits(take(bout, 2 * half), b[src].contiguous())


@pytest.mark.parametrize("rows,K,row_off,geglu_half,has_bias", [(100, 320, 28, 0, 1), (128, 64, 0, 64, 1), (5, 70, 0, 0, 0),
                                                                (2560, 320, 0, 1280, 1)])
def test_pack_ln_linear(rows, K, row_off, geglu_half, has_bias):
    """wout = operand(gamma * w), the product in fp32, bit for bit, at row_off or GEGLU-interleaved; rows in front of row_off are
    not touched.  cs = sum of the ROUNDED operands and bb = beta . w + bias are fp32 sums of K (K + 1) terms."""
    w, gamma, beta = rnd((rows, K), 91), rnd((K,), 92) * 0.3 + 1, rnd((K,), 93)
    bias = rnd((rows,), 94) if has_bias else None
    if geglu_half:
        dst = torch.argsort(_geglu_rows(geglu_half))               # packed row p holds source row src[p]: dst is the inverse
    else:
        dst = row_off + torch.arange(rows)
    total = row_off + rows
    wg = op(gamma[None, :] * w)
    dev = [t.cuda() if t is not None else None for t in (w, bias, gamma, beta)]
    wout, cs, bb = op_out(total * K), f32_out(total), f32_out(total)
    call("df_test_pack_ln_linear", *[ptr(t) for t in dev], ptr(wout), ptr(cs), ptr(bb), rows, K, row_off, geglu_half)
    got_w, got_cs, got_bb = take(wout, total * K, (total, K)), take(cs, total), take(bb, total)
    assert same_bits(got_w[dst], wg)
    if row_off:
        assert bool((bits(got_w[:row_off]) == SENTINEL).all()) and bool(torch.isnan(got_cs[:row_off]).all())
    within_f32(got_cs[dst], wg.double().sum(1), K, wg.double().abs().sum(1), "pack_ln_linear cs")
    terms = beta.double()[None, :] * w.double()
    b64 = bias.double() if has_bias else torch.zeros(rows, dtype=torch.float64)
    within_f32(got_bb[dst], terms.sum(1) + b64, K + 1, terms.abs().sum(1) + b64.abs(), "pack_ln_linear bb")


# ---------------------------------------------------------------------------------------------------------- latent packing
def _latent_ref(x, rep):
    """NCHW [B][C][HW] -> NHWC rows, the batch repeated rep times back to back."""
    return x.permute(0, 2, 1).repeat(rep, 1, 1)


@pytest.mark.parametrize("B,Cc,HW,cpad,rep,in_scale", [(2, 1, 100, 8, 1, 0.5), (3, 4, 1024 + 7, 64, 2, 1.0 / 0.18215), (1, 8, 300, 8, 2, 3.0),
                                                      (2, 64, 70, 64, 1, 0.7), (2, 4, 37, 4, 1, 1.0)])
def test_pack_latent(B, Cc, HW, cpad, rep, in_scale):
    x = rnd((B, Cc, HW), 95) * 2
    s32 = torch.tensor(in_scale, dtype=torch.float32)
    ref = torch.zeros(rep * B, HW, cpad)
    ref[..., :Cc] = _latent_ref(x * s32, rep)
    xc, out = x.cuda(), op_out(rep * B * HW * cpad)
    call("df_test_pack_latent", ptr(xc), ptr(out), B, Cc, HW, cpad, rep, float(s32), None, None)
    got = take(out, rep * B * HW * cpad, (rep * B, HW, cpad))
    assert same_bits(got, op(ref))
    assert bool((bits(got[..., Cc:]) == 0).all())


@pytest.mark.parametrize("B,Cc,HW,cpad,rep,in_scale", [(2, 4, 1024 + 7, 64, 1, 1.0 / 0.18215), (1, 8, 300, 8, 2, 1.0), (3, 1, 50, 64, 1, 2.0)])
def test_pack_latent_post_quant(B, Cc, HW, cpad, rep, in_scale):
    """y = Wpq (x in_scale) + bpq per pixel, C <= 8 fp32 terms, rounded once: within one operand ulp of float64."""
    x, wpq, bpq = rnd((B, Cc, HW), 96) * 2, rnd((Cc, Cc), 97), rnd((Cc,), 98)
    s32 = torch.tensor(in_scale, dtype=torch.float32)
    y64 = torch.einsum("oc,bcp->bop", wpq.double(), x.double() * s32.double()) + bpq.double()[None, :, None]
    ref = torch.zeros(rep * B, HW, cpad, dtype=torch.float64)
    ref[..., :Cc] = _latent_ref(y64, rep)
    xc, wc, bc, out = x.cuda(), wpq.cuda(), bpq.cuda(), op_out(rep * B * HW * cpad)
    call("df_test_pack_latent", ptr(xc), ptr(out), B, Cc, HW, cpad, rep, float(s32), ptr(wc), ptr(bc))
    got = take(out, rep * B * HW * cpad, (rep * B, HW, cpad))
    assert bool((bits(got[..., Cc:]) == 0).all())
    err = (got.double() - ref).abs()
    assert bool((err <= ulp_op(ref, odt())).all()), float((err / ulp_op(ref, odt())).max())


@pytest.mark.parametrize("B,Cc,HW,cpad,rep,rows,n", [(4, 4, 1024, 64, 2, 8, 1280), (1, 8, 257, 8, 1, 3, 4), (2, 4, 1000, 64, 2, 2, 5124)])
def test_pack_latent_bcast_equals_its_two_launches(B, Cc, HW, cpad, rep, rows, n):
    x, src = rnd((B, Cc, HW), 99), rnd((n,), 100)
    xc, sc = x.cuda(), src.cuda()
    np_ = rep * B * HW * cpad
    o1, d1, o2, d2 = op_out(np_), f32_out(rows * n), op_out(np_), f32_out(rows * n)
    call("df_test_pack_latent_bcast", ptr(xc), ptr(o1), B, Cc, HW, cpad, rep, ptr(sc), ptr(d1), rows, n)
    call("df_test_pack_latent", ptr(xc), ptr(o2), B, Cc, HW, cpad, rep, 1.0, None, None)
    call("df_test_bcast_rows", ptr(sc), ptr(d2), rows, n)
    assert same_bits(take(o1, np_), take(o2, np_))
    assert same_bits(take(d1, rows * n), take(d2, rows * n))
    assert same_bits(take(d1, rows * n, (rows, n)), src[None].expand(rows, n).contiguous())


# ---------------------------------------------------------------------------------------------------------- pooling, embedding, softmax
@pytest.mark.parametrize("N,HW,Cc", [(2, 64, 512), (3, 1, 7), (1, 1000, 33)])
def test_avgpool(N, HW, Cc):
    """HW terms summed (HW - 1 additions) and one division: K = HW."""
    x = rnd((N, HW, Cc), 101) + 0.3
    xc, out = x.cuda(), f32_out(N * Cc)
    call("df_test_avgpool", ptr(xc), ptr(out), N, HW, Cc)
    within_f32(take(out, N * Cc, (N, Cc)), x.double().mean(1), max(HW, 2), x.double().abs().mean(1), "avgpool")


def _temb64(t, dim):
    """timestep_embedding of the reference model (sinusoidal, max_period 10000, [cos | sin]) in float64."""
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = t.double()[:, None] * f[None]
    return torch.cat([torch.cos(a), torch.sin(a)], -1), a


@pytest.mark.parametrize("dim", [128, 320, 1280])
def test_timestep_embedding(dim):
    """Per element |got - ref| <= (|t f| + 1) 2^-21: the argument t f passes about five fp32 roundings and a 2-ulp expf, and
    cos / sin have slope <= 1.  The operand-type variant (row n embeds t[n % t_B]) gets one operand ulp on top."""
    L = _eng().lib(PREC)
    t = torch.tensor([0.0, 1.0, 999.0, 1000.0, 500.5, 37.25, 0.125, 873.6181640625, 12.000244140625])
    N = t.numel()
    ref, a = _temb64(t, dim)
    bound = torch.cat([a.abs() + 1, a.abs() + 1], -1) * 2.0 ** -21
    tc, out = t.cuda(), f32_out(N * dim)
    call("df_test_timestep_embedding", ptr(tc), ptr(out), N, dim)
    err = (take(out, N * dim, (N, dim)).double() - ref).abs()
    print(f"MARGIN timestep_embedding dim {dim} {PREC} err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    t_B, N2 = 4, 10                                                          # CFG duplication folded in: t_B < N
    ref2, a2 = _temb64(t[:t_B][torch.arange(N2) % t_B], dim)
    bound2 = torch.cat([a2.abs() + 1, a2.abs() + 1], -1) * 2.0 ** -21 + ulp_op(ref2, odt())
    out2 = op_out(N2 * dim)
    call("df_test_timestep_embedding_b16", ptr(tc), t_B, ptr(out2), N2, dim)
    err2 = (take(out2, N2 * dim, (N2, dim)).double() - ref2).abs()
    print(f"MARGIN timestep_embedding_b16 dim {dim} {PREC} err/bound {float((err2 / bound2).max()):.3f}")
    assert bool((err2 <= bound2).all()), float((err2 / bound2).max())


@pytest.mark.parametrize("rows,T", [(7, 1), (5, 63), (8, 64), (3, 65), (6, 1000), (2, 4096), (1, 77)])
def test_softmax_rows(rows, T):
    """Every element within ulp_op(y64) + 8 delta of the float64 softmax, delta = max |y32 - y64| of torch's fp32 softmax on the
    same scores (the rule of tests/test_norm_forms_gpu.py: delta measures fp32 noise of the reference, the factor 8 the kernel's
    different but legitimate evaluation, here exp through the hardware exp2).  Columns [T, ldp) exactly zero; the last row's scores
    span more than 100 and must stay finite."""
    s = rnd((rows, T), 102) * 3
    if T > 1:
        s[-1] = torch.linspace(-70.0, 60.0, T)
    ldp = (T + 31) // 32 * 32 + 8
    y64, y32 = torch.softmax(s.double(), -1), torch.softmax(s, -1)
    delta = float((y32.double() - y64).abs().max())
    sc, out = s.cuda(), op_out(rows * ldp)
    call("df_test_softmax_rows", ptr(sc), ptr(out), rows, T, ldp)
    got = take(out, rows * ldp, (rows, ldp))
    assert bool((bits(got[:, T:]) == 0).all())
    g = got[:, :T].double()
    assert bool(torch.isfinite(g).all())
    err, u = (g - y64).abs(), ulp_op(y64, odt())
    if delta > 0:
        print(f"MARGIN softmax_rows T {T} {PREC} delta {delta:.3e} ratio {float(((err - u) / delta).max()):.3f}")
    assert bool((err <= u + 8 * delta).all()), float(((err - u) / max(delta, 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------- sampler arithmetic
N_BIG = 5 * 209921                # > 4096 * 256 elements and not a multiple of 4: walks the grid-stride loop and a ragged tail


@pytest.mark.parametrize("n", [1, 1000, N_BIG])
@pytest.mark.parametrize("nterms,alias", [(1, 0), (2, 1), (3, 0), (4, 3), (4, 0)])
def test_lincomb(n, nterms, alias):
    """out = sum coef_j in_j: a term passes its product and nterms - 1 additions (the first addition, to 0, is exact): K = nterms.
    alias > 0: out IS input alias - 1."""
    E = _eng()
    ins = [rnd((n,), 110 + j) for j in range(nterms)]
    coef = [0.3, -1.7, 2.0, 0.815][:nterms]
    c32 = [float(np.float32(c)) for c in coef]
    y64 = sum(c * t.double() for c, t in zip(c32, ins))
    terms = sum(abs(c) * t.double().abs() for c, t in zip(c32, ins))
    dev = [t.cuda() for t in ins]
    out = dev[alias - 1] if alias else None
    got = E.lincomb(list(zip(coef, dev)), out=out)
    torch.cuda.synchronize()
    if alias:
        assert got.data_ptr() == dev[alias - 1].data_ptr()
    within_f32(got.cpu(), y64, nterms, terms, f"lincomb {nterms}")


@pytest.mark.parametrize("n", [7, N_BIG])
def test_cfg_combine(n):
    """e = u + s (c - u): the term c passes the subtraction, the product and the addition: K = 3 over |u| + |s c| + |s u|."""
    E = _eng()
    e2, s = rnd((2, n), 115), float(np.float32(4.5))
    got = E.cfg_combine(e2.cuda(), s)
    torch.cuda.synchronize()
    u, c = e2[0].double(), e2[1].double()
    within_f32(got.cpu().reshape(n), u + s * (c - u), 3, u.abs() + abs(s) * c.abs() + abs(s) * u.abs(), "cfg_combine")


@pytest.mark.parametrize("n,with_noise", [(5, 1), (N_BIG, 1), (N_BIG, 0)])
def test_ddim_update(n, with_noise):
    """pred_x0 = (x - s1m e) / sqrt(a_t): the term s1m e passes product, subtraction, division: K = 3.
    x_prev = sqrt(a_prev) pred_x0 + dir e + sigma noise: that term then passes one product and two additions more: K = 6.
    The coefficients are the fp32 values the entry point derives (sqrtf is correctly rounded; sigma = 0.25 keeps sigma^2 exact)."""
    E = _eng()
    x, e, noise = rnd((n,), 116), rnd((n,), 117), rnd((n,), 118)
    a_t, a_prev, sigma, s1m = (np.float32(v) for v in (0.5123, 0.7311, 0.25 if with_noise else 0.0, (1 - 0.5123) ** 0.5))
    sa, sp = np.sqrt(a_t), np.sqrt(a_prev)
    dr = np.sqrt(np.float32(np.float32(np.float32(1.0) - a_prev) - np.float32(sigma * sigma)))
    assert sa.dtype == np.float32 and dr.dtype == np.float32
    sa, sp, dr, sg, s1 = (float(v) for v in (sa, sp, dr, sigma, s1m))
    xd, ed, nd = x.double(), e.double(), noise.double()
    p0 = (xd - s1 * ed) / sa
    t_p0 = (xd.abs() + abs(s1) * ed.abs()) / sa
    xp = sp * p0 + dr * ed + (sg * nd if with_noise else 0)
    t_xp = sp * t_p0 + dr * ed.abs() + (sg * nd.abs() if with_noise else 0)
    got_xp, got_p0 = E.ddim_update(x.cuda(), e.cuda(), float(a_t), float(a_prev), float(sigma), float(s1m),
                                   noise=noise.cuda() if with_noise else None)
    torch.cuda.synchronize()
    within_f32(got_p0.cpu(), p0, 3, t_p0, "ddim pred_x0")
    within_f32(got_xp.cpu(), xp, 6, t_xp, "ddim x_prev")


@pytest.mark.parametrize("B,Cc,H,W,mask_c", [(2, 4, 5, 7, 1), (2, 4, 5, 7, 4), (1, 5, 1, 209921, 1), (1, 5, 1, 209921, 5)])
def test_q_sample_blend(B, Cc, H, W, mask_c):
    """out = (a x0 + b noise) m + (1 - m) img: the terms a x0 m and b noise m pass two products and two additions: K = 4.
    mask [B][1][H][W] must broadcast over the channels of ITS sample only."""
    E = _eng()
    img, x0, noise = (rnd((B, Cc, H, W), s_) for s_ in (120, 121, 122))
    mask = torch.rand(B, mask_c, H, W, generator=torch.Generator().manual_seed(123))
    mask[0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])[:min(3, W)]
    a, b = float(np.float32(0.8366)), float(np.float32(0.5477))
    got = E.q_sample_blend(img.cuda(), x0.cuda(), noise.cuda(), mask.cuda(), a, b)
    torch.cuda.synchronize()
    m = mask.double().expand(B, Cc, H, W)
    y64 = (a * x0.double() + b * noise.double()) * m + (1 - m) * img.double()
    terms = (a * x0.double().abs() + b * noise.double().abs()) * m + (1 - m).abs() * img.double().abs()
    within_f32(got.cpu(), y64, 4, terms, "q_sample_blend")
