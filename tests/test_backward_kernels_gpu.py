"""GPU: each kernel of the classifier's hand-written input-gradient pass (csrc/backward.hip, the backward-data GEMM modes of
engine_cls_grad.hip:build_classifier_grad) on its own, through the df_test_* entry points, against torch autograd in FLOAT64 on the CPU of the
same op.  Operand inputs are rounded to the build's operand type first (bf16 / fp16, both builds via the `prec` fixture), so the
reference sees exactly the values the kernel reads.

Tolerances (u = unit roundoff of the operand type: bf16 2^-8, fp16 2^-11; one rounding to nearest costs at most u |v|):
  * fp32 outputs (dx of GroupNorm / LayerNorm, the backward-data conv, the head's dh): max |err| <= 2e-5 max |ref|.  The kernels reduce
    up to 50k fp32 terms (a few 2^-24 per level of the reduction tree) and use __expf / rsqrtf (2 ulp); 2e-5 leaves an order of
    magnitude over what that costs and stays five orders below a dropped term.  The large-mean GroupNorm case (x = 50 + 0.01 randn)
    loses log2(5000) ~ 12 bits to the fp32 mean: 5e-3 there.
  * operand-type outputs of fp32 arithmetic (GEGLU, the VALU attention forms): per element |err| <= 2u |ref| + a, a = the fp32
    arithmetic's absolute error (erf_as: 1.5e-7 absolute; attention: 1e-4 max |ref| + 2^-20 times the size of one dO . V * K product,
    since the softmax-gradient sums cancel -- with one key dQ is exactly zero) + 2^-24 (the fp16 subnormal spacing), and rel-L2 <= u.
  * the MFMA attention form rounds dO, P and dS to the operand type inside the kernel (three roundings of cancelling sums): rel-L2 <= 3u
    per output, max |err| <= 12u max |ref|.
  * operand copies (dx_b16, the conv's aux copy, dh_b16) must equal the operand rounding of the fp32 value BIT for bit, saturating at
    +-65504 on fp16; the weight packings are exact.
Input padding the kernels must not read holds NaN (Vt columns past Tk, stride gaps of strided inputs), and so does every output element
they must not write (stride gaps of dq / dk / dv / dx, rows behind dh); those must still be NaN afterwards."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from helpers import rnd, rel_l2

pytestmark = pytest.mark.gpu


def _eng():
    from diff_foley_amd import engine as E
    return E


PREC = "bf16"
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}


@pytest.fixture(params=["bf16", "fp16"], autouse=True)
def prec(request):
    global PREC
    PREC = request.param
    yield PREC
    PREC = "bf16"


def odt():
    return _eng().OPERAND_DTYPE[PREC]


def lib():
    return _eng().lib(PREC)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc):
    assert rc == 0, lib().df_last_error()
    torch.cuda.synchronize()


def _op(t):
    """t rounded to the operand type, as the kernels round: fp16 saturates at +-65504 instead of overflowing to inf."""
    if PREC == "fp16":
        t = t.clamp(-65504.0, 65504.0)
    return t.to(odt())


def _nan_op(shape):
    return torch.full(shape, float("nan"), dtype=odt(), device="cuda")


def _nan32(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _bits(t):
    return t.view(torch.int16)


def _max_rel(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check_op_elem(got, ref, a, what):
    """Operand-type output of fp32 arithmetic: |got - ref| <= 2u |ref| + a (+ the fp16 subnormal spacing), rel-L2 <= u."""
    got, ref = got.double(), ref.double()
    u = U[PREC]
    bound = 2 * u * ref.abs() + a + 2.0 ** -24
    over = float(((got - ref).abs() / bound).max())
    err = rel_l2(got, ref)
    print(f"{what} [{PREC}]: worst |err| / bound {over:.3f}, rel-L2 {err:.2e} (u {u:.1e})")
    assert over <= 1.0, (what, over)
    if float(ref.abs().max()) > 16 * float(torch.as_tensor(a).max()):    # not when the exact result is zero (dQ of one key)
        assert err <= u, (what, err)


# ---------------------------------------------------------------------------------------------------------------- GroupNorm
def _gn_ref(x, gamma, beta, eps, silu, dy, N, HW, C):
    """float64 autograd of GroupNorm(32)[+SiLU] on NHWC rows [N*HW][C]."""
    xx = x.double().reshape(N, HW, C).permute(0, 2, 1).contiguous().requires_grad_(True)
    y = F.group_norm(xx, 32, gamma.double(), beta.double(), eps)
    if silu:
        y = F.silu(y)
    y.backward(dy.double().reshape(N, HW, C).permute(0, 2, 1))
    return xx.grad.permute(0, 2, 1).reshape(N * HW, C)


@pytest.mark.parametrize("N,HW,C,silu,eps,addend,pad", [
    (1, 1, 64, 1, 1e-5, False, 0), (3, 16, 96, 0, 1e-6, True, 8), (5, 256, 128, 1, 1e-5, True, 4), (1, 1024, 256, 1, 1e-6, False, 32),
    (3, 3072, 512, 1, 1e-5, True, 0), (5, 37, 320, 0, 1e-5, False, 12), (1, 37, 64, 1, 1e-6, True, 64), (3, 1024, 320, 1, 1e-5, True, 4),
    (1, 3072, 96, 0, 1e-5, False, 0), (5, 16, 512, 0, 1e-6, True, 16)])
def test_groupnorm_bwd(N, HW, C, silu, eps, addend, pad):
    rows = N * HW
    ld, lddy, ldadd, lddx = C + pad, C + 2 * pad + 4, C + pad + 4, C + pad
    x = rnd((rows, C), 100 + C) * 2 + 0.5
    dy = rnd((rows, C), 101 + C)
    ad = rnd((rows, C), 102 + C) if addend else None
    g, b = rnd((C,), 103) * 0.5 + 1, rnd((C,), 104)
    ref = _gn_ref(x, g, b, eps, silu, dy, N, HW, C)
    if addend:
        ref = ref + ad.double()
    xs, dys = _nan32((rows, ld)), _nan32((rows, lddy))
    xs[:, :C], dys[:, :C] = x.cuda(), dy.cuda()
    ads = None
    if addend:
        ads = _nan32((rows, ldadd))
        ads[:, :C] = ad.cuda()
    dx, db = _nan32((rows, lddx)), _nan_op((rows, C))
    gc, bc = g.cuda(), b.cuda()
    _ok(lib().df_test_groupnorm_bwd(ptr(xs), ld, N, HW, C, ptr(gc), ptr(bc), eps, silu, ptr(dys), lddy, ptr(ads), ldadd, ptr(dx),
                                    lddx, ptr(db), stream()))
    assert torch.isnan(dx[:, C:]).all(), "groupnorm_bwd wrote into the stride gap of dx"
    got = dx[:, :C].cpu()
    assert torch.isfinite(got).all()
    err = _max_rel(got, ref)
    print(f"groupnorm_bwd {N}x{HW}x{C} silu {silu} [{PREC}]: max err / max ref {err:.2e}")
    assert err <= 2e-5, err
    assert torch.equal(_bits(db.cpu()), _bits(_op(dx[:, :C]).cpu())), "dx_b16 is not the operand rounding of dx"


def test_groupnorm_bwd_large_mean_small_variance():
    N, HW, C = 2, 256, 128
    x = 50 + 0.01 * rnd((N * HW, C), 110)
    dy = rnd((N * HW, C), 111)
    g, b = rnd((C,), 112) * 0.5 + 1, rnd((C,), 113)
    ref = _gn_ref(x, g, b, 1e-6, 1, dy, N, HW, C)
    xc, dyc, gc, bc = x.cuda(), dy.cuda(), g.cuda(), b.cuda()
    dx = _nan32((N * HW, C))
    _ok(lib().df_test_groupnorm_bwd(ptr(xc), C, N, HW, C, ptr(gc), ptr(bc), 1e-6, 1, ptr(dyc), C, None, 0, ptr(dx), C, None,
                                    stream()))
    err = _max_rel(dx.cpu(), ref)
    print(f"groupnorm_bwd large mean [{PREC}]: max err / max ref {err:.2e}")
    assert err <= 5e-3, err


def test_groupnorm_bwd_operand_copy_saturates():
    """Gradients beyond the fp16 range: the operand copy is +-65504 (fp16) / the bf16 rounding, never inf."""
    N, HW, C = 1, 64, 64
    x = rnd((N * HW, C), 120)
    dy = rnd((N * HW, C), 121) * 1e6
    g, b = torch.ones(C), torch.zeros(C)
    xc, dyc, gc, bc = x.cuda(), dy.cuda(), g.cuda(), b.cuda()
    dx, db = _nan32((N * HW, C)), _nan_op((N * HW, C))
    _ok(lib().df_test_groupnorm_bwd(ptr(xc), C, N, HW, C, ptr(gc), ptr(bc), 1e-5, 0, ptr(dyc), C, None, 0, ptr(dx), C, ptr(db),
                                    stream()))
    assert torch.isfinite(db.float()).all()
    assert torch.equal(_bits(db.cpu()), _bits(_op(dx).cpu()))
    if PREC == "fp16":
        assert (db.float().abs() == 65504).any()


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows,C,addend", [(1, 64, False), (3, 96, True), (4, 128, False), (5, 256, True), (77, 320, True),
                                           (1024, 512, False), (5, 1280, True), (77, 1280, False), (3, 64, True), (1024, 96, True),
                                           (1, 512, True), (4, 320, False)])
def test_layernorm_bwd(rows, C, addend):
    x = rnd((rows, C), 130 + C) * 3 - 1
    dy = rnd((rows, C), 131 + C)
    g = rnd((C,), 132) * 0.5 + 1
    ad = rnd((rows, C), 133) if addend else None
    xx = x.double().requires_grad_(True)
    F.layer_norm(xx, (C,), g.double(), None, 1e-5).backward(dy.double())
    ref = xx.grad + (ad.double() if addend else 0)
    xc, dyc, gc = x.cuda(), dy.cuda(), g.cuda()
    adc = ad.cuda() if addend else None
    dx, db = _nan32((rows + 4, C)), _nan_op((rows + 4, C))
    _ok(lib().df_test_layernorm_bwd(ptr(xc), rows, C, ptr(gc), 1e-5, ptr(dyc), ptr(adc), ptr(dx), ptr(db), stream()))
    assert torch.isnan(dx[rows:]).all() and torch.isnan(db[rows:].float()).all(), "layernorm_bwd wrote past its last row"
    err = _max_rel(dx[:rows].cpu(), ref)
    print(f"layernorm_bwd {rows}x{C} [{PREC}]: max err / max ref {err:.2e}")
    assert err <= 2e-5, err
    assert torch.equal(_bits(db[:rows].cpu()), _bits(_op(dx[:rows]).cpu()))


# ---------------------------------------------------------------------------------------------------------------- GEGLU
def _geglu_u(rows, H, seed):
    u = rnd((rows, 2 * H), seed) * 2
    special = torch.tensor([0.0, 1e-3, -1e-3, 6.0, -6.0, 7.5, -7.5, 10.0, -10.0, 3.0, -3.0, 0.5])
    u[:, H:H + special.numel()] = special       # gates where the erf / phi tails matter
    return u.to(_eng().OPERAND_DTYPE[PREC])


@pytest.mark.parametrize("rows,H", [(37, 320), (3, 40), (77, 1280), (1, 12), (129, 96)])
def test_geglu_fwd(rows, H):
    u = _geglu_u(rows, H, 140 + H)
    x64, g64 = u[:, :H].double(), u[:, H:].double()
    ref = x64 * F.gelu(g64)
    uc = u.cuda()
    y = _nan_op((rows + 1, H))
    _ok(lib().df_test_geglu_fwd(ptr(uc), ptr(y), rows, H, stream()))
    assert torch.isnan(y[rows:].float()).all()
    a = 3e-7 * x64.abs() * (g64.abs() + 1)
    _check_op_elem(y[:rows].cpu(), ref, a, f"geglu_fwd {rows}x{H}")


@pytest.mark.parametrize("rows,H", [(37, 320), (3, 40), (77, 1280), (1, 12), (129, 96)])
def test_geglu_bwd(rows, H):
    u = _geglu_u(rows, H, 150 + H)
    dy = rnd((rows, H), 151 + H)
    uu = u.double().requires_grad_(True)
    (uu[:, :H] * F.gelu(uu[:, H:])).backward(dy.double())
    ref = uu.grad
    uc, dyc = u.cuda(), dy.cuda()
    du = _nan_op((rows + 1, 2 * H))
    _ok(lib().df_test_geglu_bwd(ptr(uc), ptr(dyc), ptr(du), rows, H, stream()))
    assert torch.isnan(du[rows:].float()).all()
    x64, g64, d64 = u[:, :H].double().abs(), u[:, H:].double().abs(), dy.double().abs()
    a = 3e-7 * d64 * (x64 + 1) * (g64 + 1)
    got = du[:rows].cpu()
    _check_op_elem(got[:, :H], ref[:, :H], a, f"geglu_bwd dx {rows}x{H}")
    _check_op_elem(got[:, H:], ref[:, H:], a, f"geglu_bwd dgate {rows}x{H}")


# ---------------------------------------------------------------------------------------------------------------- attention
def _rup(v, m):
    return (v + m - 1) // m * m


def _form_predicted(D, Tq, Tk, lddk, lddv):
    """Host restatement of launch_attention_bwd's choice (csrc/backward.hip attn_bwd_mfma_lds / attn_bwd_valu_lds): 0 MFMA,
    1 VALU LDS-resident, 2 tiled pair."""
    nkt, nqt = -(-Tk // 32), -(-Tq // 32)
    mfma = (D == 32 and Tk <= 256 and lddk % 4 == 0 and lddv % 4 == 0 and
            (2 * nkt + 2 * nqt) * 32 * 40 * 2 + (3 * 8 * 32 + 3 * 32 + 8 * 32 * 33) * 4 <= 160 * 1024)
    valu = ((2 * Tk + 2 * Tq) * (D + 1) + 3 * Tq) * 4 <= 160 * 1024
    return {0: mfma, 1: valu, 2: True}, (0 if mfma else (1 if valu else 2))


class _Attn:
    """One attention-backward problem in the engine's layout: Q / K rows of 2C (ldq = ldk = 2C, the other half NaN), V^T with
    ldvt = rup(Tk, 32) (pad NaN), dO rows of C + 4 (gap NaN), dQ / dK / dV rows of 3C (gaps NaN)."""

    def __init__(self, N, heads, D, Tq, Tk, seed, spike=False, dq_only=False):
        self.N, self.heads, self.D, self.Tq, self.Tk, self.dq_only = N, heads, D, Tq, Tk, dq_only
        C_ = self.C = heads * D
        q = rnd((N, Tq, C_), seed).to(odt())
        k = rnd((N, Tk, C_), seed + 1).to(odt())
        v = rnd((N, Tk, C_), seed + 2).to(odt())
        if spike:        # one key far above the rest for one query, in a late key tile
            j = min(Tk - 1, 200)
            k[:, j] = (q[:, min(5, Tq - 1)].float() * 4).to(odt())
        self.q, self.k, self.v = q, k, v
        self.do = rnd((N, Tq, C_), seed + 3)
        self.scale = D ** -0.5
        self.ldq, self.lddo, self.ldd = 2 * C_, C_ + 4, 3 * C_
        self.ldvt = _rup(Tk, 32)
        Qb = torch.full((N * Tq, 2 * C_), float("nan"), dtype=odt())
        Qb[:, :C_] = q.reshape(N * Tq, C_)
        Kb = torch.full((N * Tk, 2 * C_), float("nan"), dtype=odt())
        Kb[:, :C_] = k.reshape(N * Tk, C_)
        Vt = torch.full((N, C_, self.ldvt), float("nan"), dtype=odt())
        Vt[:, :, :Tk] = v.permute(0, 2, 1)
        dO = torch.full((N * Tq, self.lddo), float("nan"))
        dO[:, :C_] = self.do.reshape(N * Tq, C_)
        self.Qb, self.Kb, self.Vt, self.dOb = Qb.cuda(), Kb.cuda(), Vt.cuda(), dO.cuda()

    def ref(self):
        N, h, D, Tq, Tk = self.N, self.heads, self.D, self.Tq, self.Tk
        sp = lambda t, T: t.double().reshape(N, T, h, D).permute(0, 2, 1, 3).requires_grad_(True)
        q, k, v = sp(self.q, Tq), sp(self.k, Tk), sp(self.v, Tk)
        o = torch.softmax(q @ k.transpose(-1, -2) * self.scale, dim=-1) @ v
        o.backward(self.do.double().reshape(N, Tq, h, D).permute(0, 2, 1, 3))
        back = lambda g, T: g.permute(0, 2, 1, 3).reshape(N * T, h * D)
        return back(q.grad, Tq), back(k.grad, Tk), back(v.grad, Tk)

    def run(self, form):
        N, Tq, Tk, C_ = self.N, self.Tq, self.Tk, self.C
        dq = _nan_op((N * Tq, self.ldd))
        dk = None if self.dq_only else _nan_op((N * Tk, self.ldd))
        dv = None if self.dq_only else _nan_op((N * Tk, self.ldd))
        ldk = 0 if self.dq_only else self.ldd
        rc = lib().df_test_attention_bwd(ptr(self.Qb), self.ldq, ptr(self.Kb), self.ldq, ptr(self.Vt), self.ldvt, ptr(self.dOb),
                                         self.lddo, ptr(dq), self.ldd, ptr(dk), ldk, ptr(dv), ldk, N, self.heads, self.D, Tq, Tk,
                                         self.scale, form, stream())
        torch.cuda.synchronize()
        if rc != 0:
            return None
        outs = [dq] + ([] if self.dq_only else [dk, dv])
        for t in outs:
            assert torch.isnan(t[:, C_:].float()).all(), "attention_bwd wrote into a stride gap"
        return [t[:, :C_].cpu() for t in outs]

    def term(self):
        m = max(float(t.float().abs().max()) for t in (self.q, self.k, self.v))
        return float(self.do.abs().max()) * m * m * self.D * self.scale

    def lddk(self):
        return 0 if self.dq_only else self.ldd


def _check_attn(got, ref, form, what, term):
    """term: the size of one product dO . V * K * scale, the scale of the fp32 sums' absolute rounding error (dQ of one key is
    exactly zero, its fp32 value a few 2^-24 of that)."""
    u = U[PREC]
    for name, g, r in zip(("dQ", "dK", "dV"), got, ref):
        g, r = g.double(), r.double()
        assert torch.isfinite(g).all(), (what, name)
        if form == 0:
            err, mx = rel_l2(g, r), _max_rel(g, r)
            print(f"attention_bwd {what} form 0 {name} [{PREC}]: rel-L2 {err:.2e} (<= {3 * u:.1e}), max {mx:.2e} (<= {12 * u:.1e})")
            assert err <= 3 * u and mx <= 12 * u, (what, name, err, mx)
        else:
            _check_op_elem(g, r, 1e-4 * float(r.abs().max()) + 2.0 ** -20 * term, f"attention_bwd {what} form {form} {name}")


# (N, heads, Tq, Tk): every Tk of the MFMA form's key tiles (1 .. 8 tiles, ragged last tile) against 1 .. 19 query tiles
_MFMA = [(1, 1, 1, 1), (3, 8, 33, 16), (1, 8, 256, 31), (3, 1, 600, 32), (1, 1, 33, 33), (3, 8, 1, 77), (1, 8, 256, 255),
         (3, 1, 33, 256), (1, 8, 600, 77), (3, 1, 256, 1), (1, 1, 600, 256), (3, 8, 256, 256), (1, 1, 1, 255), (3, 8, 600, 33)]


@pytest.mark.parametrize("N,heads,Tq,Tk", _MFMA)
def test_attention_bwd_mfma(N, heads, Tq, Tk):
    a = _Attn(N, heads, 32, Tq, Tk, 160)
    ok, pred = _form_predicted(32, Tq, Tk, a.lddk(), a.lddk())
    got = a.run(0)
    if not ok[0]:
        assert got is None, "the MFMA form took a shape it must refuse"
        got = a.run(-1)
        assert got is not None, lib().df_last_error()
        _check_attn(got, a.ref(), pred, f"{N}x{heads} {Tq}x{Tk} (refused by MFMA: form {pred})", a.term())
        return
    assert got is not None, lib().df_last_error()
    _check_attn(got, a.ref(), 0, f"{N}x{heads} {Tq}x{Tk}", a.term())
    again = a.run(0)
    for g, h in zip(got, again):     # "deterministic" (backward.hip: fixed-order reductions)
        assert torch.equal(_bits(g), _bits(h)), "MFMA attention backward differs from run to run"


@pytest.mark.parametrize("D,N,heads,Tq,Tk", [(32, 2, 4, 64, 64), (64, 1, 2, 100, 37), (32, 1, 8, 300, 1), (64, 2, 1, 77, 150),
                                             (32, 3, 2, 33, 300), (64, 1, 4, 1, 1), (64, 2, 2, 150, 150)])
def test_attention_bwd_valu_resident_and_tiled_agree(D, N, heads, Tq, Tk):
    """VALU LDS-resident form against the reference, and BIT-equal to the tiled pair ("same arithmetic, same summation order per
    row / key as the resident kernel", backward.hip)."""
    a = _Attn(N, heads, D, Tq, Tk, 170 + D)
    ok, _ = _form_predicted(D, Tq, Tk, a.lddk(), a.lddk())
    assert ok[1]
    res = a.run(1)
    assert res is not None, lib().df_last_error()
    _check_attn(res, a.ref(), 1, f"D{D} {N}x{heads} {Tq}x{Tk}", a.term())
    til = a.run(2)
    assert til is not None, lib().df_last_error()
    for name, g, h in zip(("dQ", "dK", "dV"), res, til):
        assert torch.equal(_bits(g), _bits(h)), f"{name}: VALU resident and tiled pair differ"


@pytest.mark.parametrize("D,N,heads,Tq,Tk", [(32, 1, 2, 257, 257), (64, 1, 2, 300, 512), (32, 2, 1, 512, 300), (64, 1, 1, 1024, 1024),
                                             (32, 1, 4, 1024, 257), (64, 2, 2, 257, 300), (32, 1, 1, 300, 1024)])
def test_attention_bwd_tiled(D, N, heads, Tq, Tk):
    a = _Attn(N, heads, D, Tq, Tk, 180 + D)
    ok, pred = _form_predicted(D, Tq, Tk, a.lddk(), a.lddk())
    got = a.run(2)
    assert got is not None, lib().df_last_error()
    _check_attn(got, a.ref(), 2, f"D{D} {N}x{heads} {Tq}x{Tk}", a.term())
    if not ok[1]:
        assert a.run(1) is None, "the VALU resident form took a shape it must refuse"


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("Tq", [64, 256, 1024])
@pytest.mark.parametrize("Tc", [1, 8, 31, 32, 33, 40, 77])
def test_attention_bwd_dq_only(D, Tq, Tc):
    """Cross attention (the context is a constant): dK == nullptr, every form that takes the shape, form -1 bit-equal to the
    predicted one."""
    a = _Attn(2, 2, D, Tq, Tc, 190 + Tc, dq_only=True)
    ok, pred = _form_predicted(D, Tq, Tc, 0, 0)
    ref = a.ref()
    outs = {}
    for form in (0, 1, 2):
        got = a.run(form)
        assert (got is not None) == ok[form], (form, ok, lib().df_last_error())
        if got is not None:
            _check_attn(got, ref[:1], form, f"dQ-only D{D} {Tq}x{Tc}", a.term())
            outs[form] = got
    auto = a.run(-1)
    assert torch.equal(_bits(auto[0]), _bits(outs[pred][0])), f"form -1 is not the predicted form {pred}"


@pytest.mark.parametrize("D,N,heads,T", [(32, 2, 8, 64), (32, 1, 4, 256), (32, 1, 2, 300), (64, 2, 2, 128), (64, 1, 2, 256),
                                         (64, 1, 1, 1024), (32, 3, 4, 16)])
def test_attention_bwd_default_form_is_the_predicted_one(D, N, heads, T):
    a = _Attn(N, heads, D, T, T, 200 + T)
    _, pred = _form_predicted(D, T, T, a.lddk(), a.lddk())
    auto, forced = a.run(-1), a.run(pred)
    assert auto is not None and forced is not None, lib().df_last_error()
    for g, h in zip(auto, forced):
        assert torch.equal(_bits(g), _bits(h)), f"form -1 is not the predicted form {pred}"
    _check_attn(auto, a.ref(), pred, f"default D{D} {N}x{heads} T{T}", a.term())


@pytest.mark.parametrize("form,D,T", [(0, 32, 256), (1, 64, 128), (2, 64, 256), (2, 32, 300)])
def test_attention_bwd_softmax_spike(form, D, T):
    """One key far above the rest for one query, in a late key tile (the forward's online-softmax rescale case)."""
    a = _Attn(1, 1, D, T, T, 210, spike=True)
    got = a.run(form)
    assert got is not None, lib().df_last_error()
    _check_attn(got, a.ref(), form, f"spike D{D} T{T}", a.term())


# ---------------------------------------------------------------------------------------------------------------- classifier head
@pytest.mark.parametrize("C_", [32, 64, 160, 256])
def test_cls_head_bwd(C_):
    N, HW = 4, 37
    Cp = _rup(C_, 64)
    prob = torch.tensor([0.0, 0.5, 1 - 1e-4, 1.0])
    w = rnd((C_,), 220) * 0.05
    ref = ((1 - prob.double())[:, None, None] * w.double()[None, None, :] / HW).expand(N, HW, C_).reshape(N * HW, C_)
    pc, wc = prob.cuda(), w.cuda()
    dh = _nan32((N * HW + 1, C_))
    db = _nan_op((N * HW, Cp))
    _ok(lib().df_test_cls_head_bwd(ptr(pc), ptr(wc), ptr(dh), ptr(db), N, HW, C_, Cp, stream()))
    assert torch.isnan(dh[N * HW:]).all()
    got = dh[:N * HW].cpu()
    err = _max_rel(got, ref)
    print(f"cls_head_bwd C {C_} [{PREC}]: max err / max ref {err:.2e}")
    assert err <= 2e-5 and torch.equal(got[-HW:], torch.zeros(HW, C_)), err      # p = 1: exactly zero
    assert torch.equal(_bits(db[:, C_:].cpu()), torch.zeros(N * HW, Cp - C_, dtype=torch.int16)), "pad columns not zero"
    assert torch.equal(_bits(db[:, :C_].cpu()), _bits(_op(dh[:N * HW]).cpu()))
    # prob == nullptr: the logit's cotangent is 1 (the gradient plan applies 1 - p at the end)
    _ok(lib().df_test_cls_head_bwd(None, ptr(wc), ptr(dh), ptr(db), N, HW, C_, Cp, stream()))
    ref1 = (w.double() / HW).expand(N * HW, C_)
    assert _max_rel(dh[:N * HW].cpu(), ref1) <= 2e-5
    assert torch.equal(_bits(db[:, :C_].cpu()), _bits(_op(dh[:N * HW]).cpu()))


# ---------------------------------------------------------------------------------------------------------------- weight packings
@pytest.mark.parametrize("O1,O2,I,extra", [(64, 64, 64, 0), (320, 320, 320, 8), (96, 32, 160, 4), (1, 3, 5, 0)])
def test_pack_linear_t_stacks(O1, O2, I, extra):
    """Two Linear weights [O][I] transposed into one [I][O1 + O2 (+ extra)] operand at column offsets 0 and O1 (w_stack_t, QKV)."""
    w1, w2 = rnd((O1, I), 230), rnd((O2, I), 231)
    ldo = O1 + O2 + extra
    out = _nan_op((I, ldo))
    w1c, w2c = w1.cuda(), w2.cuda()
    _ok(lib().df_test_pack_linear_t(ptr(w1c), ptr(out), O1, I, ldo, 0, stream()))
    _ok(lib().df_test_pack_linear_t(ptr(w2c), ptr(out), O2, I, ldo, O1, stream()))
    want = torch.cat([w1, w2], 0).t().contiguous().to(odt())
    assert torch.equal(_bits(out[:, :O1 + O2].cpu()), _bits(want))
    assert torch.isnan(out[:, O1 + O2:].float()).all()


@pytest.mark.parametrize("O,I", [(32, 64), (64, 64), (160, 320), (256, 128), (3, 5)])
def test_pack_conv_bwd_layout(O, I):
    """OIHW -> [I][ky'][kx'][Opad] with (ky', kx') = (2 - ky, 2 - kx) and zero rows O .. Opad."""
    Opad = _rup(O, 64)
    w = rnd((O, I, 3, 3), 240)
    out = _nan_op((I, 3, 3, Opad))
    wc = w.cuda()
    _ok(lib().df_test_pack_conv_bwd(ptr(wc), ptr(out), O, I, Opad, stream()))
    want = torch.zeros(I, 3, 3, Opad, dtype=odt())
    want[..., :O] = w.flip(2, 3).permute(1, 2, 3, 0).to(odt())
    assert torch.equal(_bits(out.cpu()), _bits(want))


# ---------------------------------------------------------------------------------------------------------------- backward-data conv
_TILES_S1 = [0, 1, 3, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16, 17, 18, 19, 20, 23, 24, 25, 26, 27, 28, 29]     # test_kernels_gpu.test_conv3x3
_TILES_S2 = [0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 14]       # generic tiles (the producer-specialised ones take MODE 0 / 1 only)


def _conv_bwd_data(NB, H, W, I, O, stride, tile, splitk, seed):
    Opad = _rup(O, 64)
    OH, OW = H // stride, W // stride
    dy = rnd((NB, O, OH, OW), seed).to(odt())
    w = rnd((O, I, 3, 3), seed + 1) / (3 * O ** 0.5)
    ref = torch.nn.grad.conv2d_input((NB, I, H, W), w.to(odt()).double(), dy.double(), stride=stride, padding=1)
    dyp = torch.zeros(NB, OH, OW, Opad, dtype=odt())
    dyp[..., :O] = dy.permute(0, 2, 3, 1)
    dyc, wc = dyp.cuda(), w.cuda()
    ws = _nan_op((I * 9 * Opad,))
    dx = _nan32((NB * H * W + 1, I))
    dxo = _nan_op((NB * H * W + 1, I))
    rc = lib().df_test_conv3x3_bwd_data(ptr(dyc), ptr(wc), ptr(ws), ptr(dx), ptr(dxo), NB, H, W, I, O, stride, tile, splitk, stream())
    if rc != 0 and b"refused" in lib().df_last_error():
        pytest.skip("tile / split-K combination does not exist for this problem")
    _ok(rc)
    assert torch.isnan(dx[-1]).all() and torch.isnan(dxo[-1].float()).all(), "conv backward-data wrote past its output"
    got = dx[:-1].cpu()
    assert torch.isfinite(got).all()
    err = _max_rel(got, ref.permute(0, 2, 3, 1).reshape(NB * H * W, I))
    print(f"conv3x3 bwd-data s{stride} {NB}x{H}x{W} {O}->{I} tile {tile} sk {splitk} [{PREC}]: max err / max ref {err:.2e}")
    assert err <= 2e-5, err
    assert torch.equal(_bits(dxo[:-1].cpu()), _bits(_op(dx[:-1]).cpu())), "aux operand copy is not the rounding of dX"


@pytest.mark.parametrize("tile", _TILES_S1)
@pytest.mark.parametrize("splitk", [1, 2, 4])
@pytest.mark.parametrize("NB,H,W,I,O", [(2, 2, 8, 64, 64), (1, 4, 16, 128, 160), (2, 16, 64, 64, 256), (3, 6, 10, 64, 32),
                                        (1, 2, 2, 128, 64)])
def test_conv3x3_bwd_data_stride1(tile, splitk, NB, H, W, I, O):
    _conv_bwd_data(NB, H, W, I, O, 1, tile, splitk, 250)


@pytest.mark.parametrize("tile", _TILES_S2)
@pytest.mark.parametrize("splitk", [1, 2, 4])
@pytest.mark.parametrize("NB,H,W,I,O", [(2, 4, 16, 64, 64), (1, 16, 64, 128, 128), (3, 2, 8, 64, 32), (1, 8, 12, 128, 256),
                                        (2, 2, 2, 64, 160)])
def test_conv3x3_bwd_data_stride2_zero_stuffed(tile, splitk, NB, H, W, I, O):
    """Downsample^T (down.bwd): conv over the zero-stuffed x2 grid of dY with the flipped taps (gemm_impl.h zstuff)."""
    _conv_bwd_data(NB, H, W, I, O, 2, tile, splitk, 260)
