"""GPU: every dispatch form of GroupNorm, LayerNorm and fused attention (tests/kernel_cases.py; tests/test_kernel_forms_cpu.py
proves the tables reach all of them) against float64 references, with per-element / per-row bounds, padded leading dimensions and
sentinel-filled outputs.  Both operand builds.

Norm bound (every element): |got - y64| <= ulp_op(y64) + 8 delta, y64 = float64 result on the exact fp32 inputs, delta = max
|y32 - y64| with y32 torch's own float32 CPU result of the same case (the fp32 evaluation noise of the reference, not of the
kernel), ulp_op = one unit in the last place of the operand type at |y64|.

Attention bound (every (batch, head, query) row): rel-L2 against the exact float64 softmax(QK^T)V <= 4 x the largest per-row
rel-L2 that a float64 evaluation with P and O rounded to the operand type where the kernel rounds them shows in the same case.

Measured margins on an MI355X, largest over the cases of a form and both builds -- norms: (err - ulp_op) / delta, bound 8;
attention: row rel-L2 / rounding floor, bound 4.

  GroupNorm form        plain   slabs     own
  PER  1               0.002   0.066   0.014
  PER  2               0.004   0.047   0.072
  PER  3               0.058   0.089   0.027
  PER  4               0.054   0.112   0.072
  PER  6               0.053   0.048   0.026
  PER  8               0.205   0.017   0.035
  PER 12               0.093   0.072   0.035
  PER 16               0.139   0.079   0.059
  PER 20               0.113   0.200   0.064
  streaming            0.232       -       -
  chunked              0.146       -       -
  LayerNorm, largest over the 32 widths: 0.103
  attention  <D,4,2> 1.033   <D,4> 1.115   <D,2> 1.060   <D,1> 1.043
The norm ratios are far below 8 because ulp_op allows a whole unit where round-to-nearest of an fp32-accurate value uses half:
(err - ulp) / delta stays near zero unless an error approaches one full ulp.  No form needed more than the factor 8.  The norm
tests therefore also assert the round-to-nearest form of the bound, |got - y64| <= ulp_op / 2 + 8 delta (check_elementwise), which
a store that truncates misses; measured (err - ulp / 2) / delta: at most 0.67 for every form except GroupNorm PER 1 plain at 1.04,
LayerNorm 0.25.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from helpers import rnd, rel_l2
import kernel_cases as KC

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A                 # operand-type bit pattern no kernel may overwrite (finite in both types)


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


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ulp_op(y, dt):
    """One unit in the last place of the operand type at |y| (float64 tensor); subnormal spacing below the smallest normal."""
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - mant)


def bits(t):
    return t.contiguous().view(torch.int16)


def sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(odt())


def is_sentinel(t):
    return bool((bits(t.cpu()) == SENTINEL).all())


def padded(t, ld, fill=float("nan")):
    """[rows][C] -> [rows][ld] with the pad columns poisoned: no kernel may read them into a result."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def check_elementwise(got, y64, y32, what):
    """|got - y64| <= ulp_op(y64) + 8 delta for EVERY element; returns the largest (err - ulp) / delta for the record."""
    delta = float((y32.double() - y64).abs().max())
    assert delta > 0
    err = (got.double() - y64).abs()
    u = ulp_op(y64, got.dtype)
    ratio = float(((err - u) / delta).max())
    print(f"MARGIN {what} {PREC} delta {delta:.3e} ratio {ratio:.3f}")
    bad = err > u + 8 * delta
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements beyond ulp + 8 delta (worst (err - ulp) / delta = {ratio:.2f})"
    # Tighter, and what catches truncation in place of round-to-nearest: a value within fp32 noise n of y64, rounded to nearest,
    # lies within ulp / 2 + n of it (ulp taken at the larger of |got|, |y64|: the two may sit on either side of a power of two),
    # with the same noise allowance n = 8 delta.  A truncating store is off by up to a whole ulp.
    half = ulp_op(torch.maximum(y64.abs(), got.double().abs()), got.dtype) / 2
    ratio_rn = float(((err - half) / delta).max())
    print(f"MARGIN-RN {what} {PREC} ratio {ratio_rn:.3f}")
    bad = err > half + 8 * delta
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements beyond ulp / 2 + 8 delta (worst (err - ulp / 2) / delta = {ratio_rn:.2f})"
    return ratio


# ------------------------------------------------------------------------------------------------------------------- GroupNorm
def _gn_id(c):
    return "-".join(str(v) for v in c)


@pytest.mark.parametrize("case", KC.GN_CASES, ids=_gn_id)
def test_groupnorm_every_form(case):
    """Each (form, mode) with ld > C, ldo > C and raw_out.  Checked: the per-element bound on the normalised operand; the pad
    columns [C, ldo) of out and raw_out keep the sentinel; raw_out is the finished input cast to the operand type bit for bit
    (slab modes: the slab sum + bias terms in the kernel's fp32 order); own-slab mode: x is written back bit-equal, its channels
    >= c_own and its pad columns are untouched; the NaN-poisoned pad columns of every input never reach a result."""
    E = _eng()
    L = E.lib(PREC)
    mode, N, HW, Cc, silu, eps, nslab, c_own = case
    rows, ld, ldo, ldrb = N * HW, Cc + 8, Cc + 16, Cc + 2
    form = L.df_test_groupnorm_form(N, HW, Cc, nslab if mode != "plain" else 0)
    g, b = rnd((Cc,), 7) * 0.5 + 1.0, rnd((Cc,), 8)
    keep = []                                   # device tensors stay alive: the ABI takes raw pointers
    dev = lambda t: (keep.append(t.cuda()), keep[-1])[1]
    args = dict(nslab=0, stride=0, bias=None, rowbias=None, own=None, c_own=0, res=None, ldr=0)
    if mode == "plain":
        full = rnd((rows, Cc), 6) * 2 + 0.5
        xdev = dev(padded(full, ld))
    elif mode == "slabs":
        slabs = rnd((nslab, rows, Cc), 61) * 0.9 + 0.2
        which = (N + HW + Cc) % 3                                        # both bias terms, the bias alone, the per-sample bias alone
        bias = rnd((Cc,), 62) if which != 2 else None
        rowbias = rnd((N, Cc), 63) if which != 1 else None
        full = slabs[0].clone()
        for s_ in range(1, nslab):
            full += slabs[s_]
        add = torch.zeros(N, Cc)
        if bias is not None:
            add = add + bias
        if rowbias is not None:
            add = add + rowbias
        full = (full.reshape(N, HW, Cc) + add[:, None, :]).reshape(rows, Cc)
        xdev = dev(torch.stack([padded(s_, ld) for s_ in slabs]))
        args.update(nslab=nslab, stride=rows * ld, bias=ptr(dev(bias)) if bias is not None else None,
                    rowbias=ptr(dev(padded(rowbias, ldrb))) if rowbias is not None else None)
    else:
        slabs = rnd((nslab, rows, c_own), 61) * 0.7
        bias, res = rnd((c_own,), 62), rnd((rows, c_own), 63)
        x0 = rnd((rows, Cc), 64) * 2 + 0.5
        fin = slabs[0].clone()
        for s_ in range(1, nslab):
            fin += slabs[s_]
        fin = fin + bias
        fin = fin + res
        full = x0.clone()
        full[:, :c_own] = fin
        xdev = dev(padded(x0, ld))
        args.update(nslab=nslab, stride=rows * c_own, bias=ptr(dev(bias)), own=ptr(dev(slabs)), c_own=c_own,
                    res=ptr(dev(padded(res, c_own + 6))), ldr=c_own + 6)
    nchw = lambda t: t.reshape(N, HW, Cc).permute(0, 2, 1)
    act = (lambda t: F.silu(t)) if silu else (lambda t: t)
    y64 = act(F.group_norm(nchw(full.double()), 32, g.double(), b.double(), eps))
    y32 = act(F.group_norm(nchw(full), 32, g, b, eps))
    out, raw = sentinel((rows + 1, ldo)), sentinel((rows + 1, ldo))      # one guard row behind the last pixel
    gc, bc = dev(g), dev(b)
    rc = L.df_test_groupnorm_ex(ptr(xdev), ld, N, HW, Cc, ptr(gc), ptr(bc), eps, silu, ptr(out), ldo, ptr(raw), args["nslab"], args["stride"],
                                args["bias"], args["rowbias"], ldrb, args["own"], args["c_own"], args["res"], args["ldr"], stream())
    assert rc == 0, L.df_last_error()
    torch.cuda.synchronize()
    oc, rw = out.cpu(), raw.cpu()
    assert is_sentinel(oc[:rows, Cc:]) and is_sentinel(oc[rows]), "out written beyond its C columns / its last row"
    assert is_sentinel(rw[:rows, Cc:]) and is_sentinel(rw[rows]), "raw_out written beyond its C columns / its last row"
    assert torch.equal(bits(rw[:rows, :Cc]), bits(full.to(odt()))), "raw_out is not the input rounded to nearest"
    xa = xdev.cpu()
    if mode == "own":
        assert torch.equal(xa[:, :Cc], full), "x was not finished bit-equal to the reduce"
        assert bool(torch.isnan(xa[:, Cc:]).all())
    else:
        x_first = xa if mode == "plain" else xa[0]
        assert torch.equal(x_first[:, :Cc], full if mode == "plain" else slabs[0])      # a plain / producer-slab input is read-only
    got = nchw(oc[:rows, :Cc])
    assert torch.isfinite(got.float()).all()
    assert rel_l2(got.float(), y64) < 4e-3
    check_elementwise(got, y64, y32, f"groupnorm {mode} form {form}")


def test_groupnorm_refusals_launch_nothing():
    """The smallest shape on the wrong side of each rule of the GroupNorm launcher: every such call returns non-zero with
    df_last_error() set and leaves out, raw_out and x bit-identical.  The one shape right next to a refusal that must run
    (input slabs at HW = 16384, C = 64: PER 16, the most the register kernels hold) is checked with the file's bound."""
    L = _eng().lib(PREC)
    keep = []
    dev = lambda t: (keep.append(t.cuda()), keep[-1])[1]

    def call(x, ld, N, HW, Cc, ldo, nslab=0, stride=0, bias=None, own=None, c_own=0, res=None, ldr=0):
        g, b = dev(rnd((Cc,), 7) * 0.5 + 1.0), dev(rnd((Cc,), 8))
        out, raw = sentinel((N * HW + 1, ldo)), sentinel((N * HW + 1, ldo))
        rc = L.df_test_groupnorm_ex(ptr(x), ld, N, HW, Cc, ptr(g), ptr(b), 1e-5, 1, ptr(out), ldo, ptr(raw), nslab, stride, ptr(bias),
                                    None, 0, ptr(own), c_own, ptr(res), ldr, stream())
        torch.cuda.synchronize()
        return rc, out.cpu(), raw.cpu()

    def refused(what, x, *a, **kw):
        before = x.clone()
        rc, out, raw = call(x, *a, **kw)
        assert rc != 0 and L.df_last_error(), f"{what}: not refused"
        assert is_sentinel(out) and is_sentinel(raw), f"{what}: a refused call wrote its outputs"
        assert torch.equal(x.view(torch.int32), before.view(torch.int32)), f"{what}: a refused call wrote x"

    # input slabs: one item more than the register kernels hold, then the largest shape they do hold
    slabs = rnd((2, 16385, 64), 61) * 0.9 + 0.2
    bias = rnd((64,), 62)
    xs, bs = dev(slabs), dev(bias)
    refused("slabs HW 16385", xs, 64, 1, 16385, 64, 64, nslab=2, stride=16385 * 64, bias=bs)
    assert L.df_test_groupnorm_form(1, 16384, 64, 2) == 16
    rc, out, raw = call(xs, 64, 1, 16384, 64, 64, nslab=2, stride=16385 * 64, bias=bs)
    assert rc == 0, L.df_last_error()
    assert torch.equal(xs.cpu(), slabs), "a producer's slabs are read-only"
    full = (slabs[0, :16384] + slabs[1, :16384]) + bias
    assert is_sentinel(out[16384]) and is_sentinel(raw[16384])
    assert torch.equal(bits(raw[:16384]), bits(full.to(odt()))), "raw_out is not the input rounded to nearest"
    nchw = lambda t: t.reshape(1, 16384, 64).permute(0, 2, 1)
    g, b = rnd((64,), 7) * 0.5 + 1.0, rnd((64,), 8)
    y64 = F.silu(F.group_norm(nchw(full.double()), 32, g.double(), b.double(), 1e-5))
    y32 = F.silu(F.group_norm(nchw(full), 32, g, b, 1e-5))
    check_elementwise(nchw(out[:16384]), y64, y32, "groupnorm slabs form 16 (HW 16384)")

    # own slabs: an odd c_own, a single slab, an odd residual leading dimension
    for what, c_own, nslab, ldr in (("c_own 31", 31, 2, 32), ("nslab 1", 32, 1, 32), ("ldr 33", 32, 2, 33)):
        own, ob, res = dev(rnd((nslab, 16, c_own), 61)), dev(rnd((c_own,), 62)), dev(rnd((16, ldr), 63))
        refused("own slabs " + what, dev(rnd((16, 64), 64)), 64, 1, 16, 64, 64, nslab=nslab, stride=16 * c_own, bias=ob, own=own,
                c_own=c_own, res=res, ldr=ldr)

    # plain: a chunked shape whose output rows are not 16-byte aligned; a channel count that is no multiple of 64
    assert L.df_test_groupnorm_form(1, 8193, 128, 0) == KC.GN_CHUNKED
    refused("chunked ldo C + 4", dev(rnd((8193, 128), 6)), 128, 1, 8193, 128, 132)
    refused("C 100", dev(rnd((16, 100), 6)), 100, 1, 16, 100, 100)


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows,Cc,ld", KC.LN_CASES)
def test_layernorm_every_width(rows, Cc, ld):
    E = _eng()
    L = E.lib(PREC)
    x = rnd((rows, Cc), 9) * 3 - 1
    g, b = rnd((Cc,), 10) * 0.5 + 1.0, rnd((Cc,), 11)
    y64 = F.layer_norm(x.double(), (Cc,), g.double(), b.double(), 1e-5)
    y32 = F.layer_norm(x, (Cc,), g, b, 1e-5)
    xc, gc, bc = padded(x, ld).cuda(), g.cuda(), b.cuda()
    out = sentinel((rows + 1, Cc))
    rc = L.df_test_layernorm_ex(ptr(xc), ld, rows, Cc, ptr(gc), ptr(bc), ptr(out), stream())
    assert rc == 0, L.df_last_error()
    torch.cuda.synchronize()
    oc = out.cpu()
    assert is_sentinel(oc[rows]), "a row past the last one was written"
    got = oc[:rows]
    assert torch.isfinite(got.float()).all()
    assert rel_l2(got.float(), y64) < 4e-3
    check_elementwise(got, y64, y32, f"layernorm NV {Cc // 64}")


# ------------------------------------------------------------------------------------------------------------------- attention
def _attn_refs(q, k, v, N, heads, D, Tq, Tk, scale, dt):
    """Exact float64 attention and the same with the kernel's two roundings: P = exp(s - max) (in [0, 1]) to the operand type
    before the P V product -- the row sum runs over the rounded P where the kernel takes it from the matrix pipe (D % 32 != 0) and
    over the unrounded p elsewhere -- and O to the operand type at the store.  Both [N][heads][Tq][D] float64."""
    sp = lambda t, T: t.double().reshape(N, T, heads, D).permute(0, 2, 1, 3)
    s = sp(q, Tq) @ sp(k, Tk).transpose(-1, -2) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    exact = (p @ sp(v, Tk)) / p.sum(-1, keepdim=True)
    pr = p.to(dt).double()
    l = pr.sum(-1, keepdim=True) if D % 32 else p.sum(-1, keepdim=True)
    emu = ((pr @ sp(v, Tk)) / l).to(dt).double()
    return exact, emu


def _attn_id(c):
    return "-".join(str(v) for v in c)


@pytest.mark.parametrize("case", KC.ATTN_CASES, ids=_attn_id)
def test_attention_every_form(case):
    E = _eng()
    L = E.lib(PREC)
    N, heads, D, Tq, Tk, fused = case
    C_ = heads * D
    form = L.df_test_attention_form(D, Tq, Tk)
    q, k, v = (rnd((N, T, C_), s_).to(odt()) for T, s_ in ((Tq, 12), (Tk, 13), (Tk, 14)))
    scale = D ** -0.5
    exact, emu = _attn_refs(q, k, v, N, heads, D, Tq, Tk, scale, odt())
    ldvt = (Tk + 31) // 32 * 32
    vt = torch.full((N, C_, ldvt), float("nan"), dtype=odt())      # padding deliberately poisoned
    vt[:, :, :Tk] = v.permute(0, 2, 1)
    if fused:                                                       # Q | K as column ranges of one [N*T][2C] buffer
        qk = torch.cat([q, k], dim=-1).contiguous().cuda()
        qp, kp, ldq, ldk = qk.data_ptr(), qk.data_ptr() + C_ * qk.element_size(), 2 * C_, 2 * C_
    else:
        qc, kc = q.cuda(), k.cuda()
        qp, kp, ldq, ldk = qc.data_ptr(), kc.data_ptr(), C_, C_
    vc = vt.cuda()
    ldo = C_ + 24
    o = sentinel((N * Tq + 1, ldo))                                  # pad columns and one guard row behind the last query
    rc = L.df_test_attention(C.c_void_p(qp), ldq, C.c_void_p(kp), ldk, ptr(vc), ldvt, ptr(o), ldo, N, heads, D, Tq, Tk, scale, stream())
    assert rc == 0, L.df_last_error()
    torch.cuda.synchronize()
    oc = o.cpu()
    assert is_sentinel(oc[:N * Tq, C_:]) and is_sentinel(oc[N * Tq]), "O written beyond heads * D columns / its last query row"
    got = oc[:N * Tq, :C_].double().reshape(N, Tq, heads, D).permute(0, 2, 1, 3)
    assert torch.isfinite(got).all()
    assert rel_l2(got, exact) < 1e-2
    norm = exact.norm(dim=-1)
    floor = float(((emu - exact).norm(dim=-1) / norm).max())
    rows = (got - exact).norm(dim=-1) / norm                        # every (batch, head, query) row
    ratio = float(rows.max()) / floor
    print(f"MARGIN attention form {form} D {D} {PREC} floor {floor:.3e} ratio {ratio:.3f}")
    assert bool((rows <= 4 * floor).all()), f"{int((rows > 4 * floor).sum())} rows beyond 4 x the rounding floor {floor:.3e} (worst {ratio:.2f} x)"
