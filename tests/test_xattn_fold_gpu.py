"""GPU: the folded cross-attention (engine_builder.hip context_px, st.xs, st.xo) kernel by kernel and as one chain, on both builds.

df_test_xattn_chain runs the plan's sequence -- ctx.kv, xattn_expand, the lnq_t packing, ctx.g, xattn_rowstats, the batched ctx.vo,
st.xs, st.xo -- and returns every intermediate.  Each is compared with its defining formula (csrc/elementwise.hip xattn_expand /
pack_lnq_t / xattn_rowstats) evaluated in float64 on the intermediates the kernels were given: copies bit-exact, products and sums
within fp32 round-off plus the rounding of an operand-type output.  The probabilities and the block output are compared with the
unfolded form, softmax(scale LN(x) Wq_h K_h^T) and x + to_out(attention(LN(x))), in float64.  Samples get different contexts, so a
row that read another sample's folded weights would fail.  The merged FF2 + proj_out packing (launch_pack_ffproj) is checked too."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from helpers import rnd

pytestmark = pytest.mark.gpu

PREC = "bf16"


@pytest.fixture(params=["bf16", "fp16"], autouse=True)
def prec(request):
    global PREC
    PREC = request.param
    yield PREC
    PREC = "bf16"


def _lib():
    from diff_foley_amd import engine as E
    return E.lib(PREC)


def odt():
    from diff_foley_amd import engine as E
    return E.OPERAND_DTYPE[PREC]


def op(t):
    return t.to(odt())


def p(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


U = 2.0 ** -24


def u_out():
    return 2.0 ** -8 if PREC == "bf16" else 2.0 ** -11


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def within(got, ref, bnd):
    """Largest |got - ref| / bnd (NaN = inf)."""
    err = (got.double() - ref).abs()
    r = torch.where(torch.isfinite(err), err / bnd, torch.full_like(err, float("inf")))
    return float(r.max())


def nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


# (C, heads, samples, Tc, tokens per sample, context width, st.xs tile, st.xo tile)
CHAIN = [(320, 8, 2, 1, 64, 128, 3, 13), (640, 8, 3, 17, 128, 64, 0, 1), (128, 2, 3, 32, 64, 128, 2, 3),
         (320, 8, 3, 32, 128, 64, 19, 28), (640, 8, 2, 17, 64, 128, 26, 12)]


@pytest.mark.parametrize("Cd,heads,NB,Tc,T,Dc,tile_xs,tile_xo", CHAIN)
def test_folded_cross_attention_chain(Cd, heads, NB, Tc, T, Dc, tile_xs, tile_xo):
    L = _lib()
    D, HT, M = Cd // heads, heads * 32, NB * T
    scale32 = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(D), dtype=torch.float32))
    scale = float(scale32)
    s0 = Cd + Tc
    ctx = op(rnd((NB * Tc, Dc), s0))
    Wkv = op(rnd((2 * Cd, Dc), s0 + 1) / Dc ** 0.5)
    Wq = rnd((Cd, Cd), s0 + 2) / Cd ** 0.5
    gamma, beta = 1 + 0.2 * rnd((Cd,), s0 + 3), 0.2 * rnd((Cd,), s0 + 4)
    bq = (Wq.double() @ beta.double()).float()
    Wo = op(rnd((Cd, Cd), s0 + 5) / Cd ** 0.5)
    bo = 0.1 * rnd((Cd,), s0 + 6)
    x = rnd((M, Cd), s0 + 7) * 1.5 + 0.5
    xb = op(x)
    xs = x.double().view(M, Cd // 64, 64)
    xst = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).float()
    dev = [t.cuda() for t in (ctx, Wkv, Wq, gamma, bq, Wo, bo, x, xb, xst)]
    kv, Kexp, Vexp = nan((NB * Tc, 2 * Cd), odt()), nan((NB, HT, Cd), odt()), nan((NB, HT, Cd), odt())
    WqT, G = nan((Cd, Cd), odt()), nan((NB, HT, Cd), odt())
    cs, bb = nan((NB, HT)), nan((NB, HT))
    Vo, P, out = nan((NB, Cd, HT), odt()), nan((M, HT), odt()), nan((M, Cd))
    rc = L.df_test_xattn_chain(*map(p, dev), NB, T, Tc, Dc, Cd, heads, *map(p, (kv, Kexp, Vexp, WqT, G, cs, bb, Vo, P, out)),
                               tile_xs, tile_xo, stream())
    assert rc == 0, L.df_last_error()
    torch.cuda.synchronize()
    kv, Kexp, Vexp, WqT, G, cs, bb, Vo, P, out = (t.cpu() for t in (kv, Kexp, Vexp, WqT, G, cs, bb, Vo, P, out))
    worst = {}

    def bounded(name, got, ref, absprod, K, rounded=True):
        bnd = 2 * K * U * absprod + (u_out() * ref.abs() if rounded else 4 * U * ref.abs()) + 1e-30
        worst[name] = within(got, ref, bnd)
        assert worst[name] <= 1, f"{name}: {worst[name]:.3g} x its bound"

    # ctx.kv
    c64, wkv64 = ctx.double(), Wkv.double()
    bounded("kv", kv, c64 @ wkv64.t(), c64.abs() @ wkv64.abs().t(), Dc)
    # xattn_expand: head h's columns of token tc in row (h, tc); zeros in the other heads' columns and in rows tc >= Tc
    ke = torch.zeros(NB, heads, 32, Cd, dtype=odt())
    ve = torch.zeros_like(ke)
    kvn = kv.view(NB, Tc, 2 * Cd)
    for h in range(heads):
        ke[:, h, :Tc, h * D:(h + 1) * D] = kvn[:, :, h * D:(h + 1) * D]
        ve[:, h, :Tc, h * D:(h + 1) * D] = kvn[:, :, Cd + h * D:Cd + (h + 1) * D]
    assert torch.equal(bits(Kexp), bits(ke.view(NB, HT, Cd))), "Kexp differs from the head-masked expansion of K"
    assert torch.equal(bits(Vexp), bits(ve.view(NB, HT, Cd))), "Vexp differs from the head-masked expansion of V"
    # lnq_t: round(fp32(scale * gamma[c]) * Wq[j][c]), the kernel's own multiplication order
    assert torch.equal(bits(WqT), bits(op((scale32 * gamma)[:, None] * Wq.t()))), "WqT is not round(fp32(scale gamma[c]) Wq[j][c])"
    # ctx.g: G' = Kexp WqT^T
    k64, q64 = Kexp.double(), WqT.double()
    bounded("G", G, k64 @ q64.t(), k64.abs() @ q64.abs().t(), Cd)
    # xattn_rowstats: cs = sum_c G'[row][c] (operand values), bb = scale sum_j Kexp[row][j] bq[j]
    g64 = G.double()
    bounded("cs", cs, g64.sum(-1), g64.abs().sum(-1), Cd, rounded=False)
    bq64 = bq.double()
    bounded("bb", bb, scale * (k64 @ bq64), scale * (k64.abs() @ bq64.abs()), Cd + 2, rounded=False)
    # ctx.vo: Vo[n] = Wo Vexp[n]^T
    wo64, v64 = Wo.double(), Vexp.double()
    bounded("Vo", Vo, torch.stack([wo64 @ v64[n].t() for n in range(NB)]),
            torch.stack([wo64.abs() @ v64[n].abs().t() for n in range(NB)]), Cd)
    # unfolded reference: LayerNorm -> q, scores against this sample's keys, softmax over the Tc real tokens, values, to_out
    ln = F.layer_norm(x.double(), (Cd,), gamma.double(), beta.double(), 1e-5)
    q = ln @ Wq.double().t()
    kvt = (c64 @ wkv64.t()).view(NB, Tc, 2 * Cd)
    smp = torch.arange(M) // T
    Kt, Vt = kvt[smp, :, :Cd], kvt[smp, :, Cd:]                     # [M][Tc][C] each row's own sample
    pr = torch.zeros(M, heads, 32, dtype=torch.float64)
    att = torch.zeros(M, Cd, dtype=torch.float64)
    for h in range(heads):
        sl = slice(h * D, (h + 1) * D)
        sc = scale * torch.einsum("md,mtd->mt", q[:, sl], Kt[:, :, sl])
        ph = torch.softmax(sc, -1)
        pr[:, h, :Tc] = ph
        att[:, sl] = torch.einsum("mt,mtd->md", ph, Vt[:, :, sl])
    ref_out = x.double() + att @ wo64.t() + bo.double()
    Pg = P.double().view(M, heads, 32)
    assert torch.equal(bits(P.view(M, heads, 32)[..., Tc:]), torch.zeros(M, heads, 32 - Tc, dtype=torch.int16)), \
        "probabilities of padding tokens are not +0"
    # operand roundings of xb, G', Kexp and P against the exact form: measured worst |dp| bf16 4.0e-3, fp16 4.3e-4
    tol_p = 1e-2 if PREC == "bf16" else 1.2e-3
    dp = (Pg - pr).abs().amax(-1).amax(-1)
    worst["P"] = float(dp.max())
    assert worst["P"] <= tol_p, f"row {int(dp.argmax())}: probabilities off by {worst['P']:.3g} (sample {int(dp.argmax()) // T})"
    # block output, per row relative to the attention branch: measured worst bf16 6.8e-3, fp16 8.0e-4
    tol_o = 1.5e-2 if PREC == "bf16" else 2e-3
    branch = (ref_out - x.double()).norm(dim=-1)
    eo = (out.double() - ref_out).norm(dim=-1) / branch
    worst["out"] = float(eo.max())
    assert torch.isfinite(out).all() and worst["out"] <= tol_o, f"row {int(eo.argmax())}: block output off by {worst['out']:.3g}"
    print(f"\nxattn C {Cd} heads {heads} NB {NB} Tc {Tc} [{PREC}]: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("Cd,Fd", [(320, 1280), (128, 512), (640, 2560)])
def test_pack_ffproj(Cd, Fd):
    """[Wp W2 | Wp] within one operand-type ulp of the float64 product, plus the fp32 accumulation bound 2 C u sum |Wp||W2| where
    the product cancels to far below its terms (there a bf16 ulp is smaller than any fp32 sum can resolve); Wp b2 + bp within fp32
    round-off."""
    L = _lib()
    Wp, W2 = rnd((Cd, Cd), 1) / Cd ** 0.5, rnd((Cd, Fd), 2) / Fd ** 0.5
    bp, b2 = 0.1 * rnd((Cd,), 3), 0.1 * rnd((Cd,), 4)
    wout, bout = nan((Cd, Fd + Cd), odt()), nan((Cd,))
    rc = L.df_test_pack_ffproj(*map(p, (Wp.cuda(), bp.cuda(), W2.cuda(), b2.cuda(), wout, bout)), Cd, Fd, stream())
    assert rc == 0, L.df_last_error()
    torch.cuda.synchronize()
    wout, bout = wout.cpu(), bout.cpu()
    ref = Wp.double() @ W2.double()
    _, e = torch.frexp(ref)
    mant = 8 if PREC == "bf16" else 11
    ulp = torch.ldexp(torch.ones_like(ref), (e - mant).clamp_min(-24 if PREC == "fp16" else -133))
    bnd = ulp + 2 * Cd * U * (Wp.double().abs() @ W2.double().abs())
    assert within(wout[:, :Fd], ref, bnd) <= 1, f"Wp W2: {within(wout[:, :Fd], ref, bnd):.3g} x (one ulp + fp32 accumulation)"
    assert torch.equal(bits(wout[:, Fd:]), bits(op(Wp))), "the Wp columns are not the operand-type copy of Wp"
    rb = Wp.double() @ b2.double() + bp.double()
    bnd = 2 * (Cd + 2) * U * ((Wp.double().abs() @ b2.double().abs()) + bp.double().abs()) + 1e-30
    assert within(bout, rb, bnd) <= 1, "Wp b2 + bp"
