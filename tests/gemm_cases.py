"""Case builders of tests/test_gemm_forms_gpu.py and tests/test_gemm_cases_cpu.py: every GEMM form of the shipped plan tables.

A form is what the tune-cache key (csrc/engine_tune.hip tune_key, M_N_K_taps_stride_ups_batch_geglu_eEPI) says about the kernel that
runs: (taps, stride, ups, batched, geglu, EPI bits).  The two tables under diff_foley_amd/tuned hold 28 forms; CASES has at least
one case per form, sized so that every (form, tile, split-K) triple a table ships is among the (tile, split-K) pairs the autotuner
would launch for some case of that form (tests/test_gemm_cases_cpu.py asserts both).  Nothing here needs a GPU: operands, the float64
reference, the per-element bounds and the checks live on the CPU; the GPU test only moves them and launches.

How a case is put together (all stages are plain functions of the case, so the CPU test can feed them other inputs):
    acc64 / absacc   sum_k A W and sum_k |A| |W| in float64 from operands rounded to the build's operand type
    epi(acc, dtype)  the epilogue on such an accumulator in float64 (the reference) or float32 (a stand-in for a kernel)
    pack(final)      the output buffers a launch leaves behind, from the epilogue's values: C with its NaN gaps and slack rows, the
                     operand copy, row statistics, V^T, CFG-duplicated rows
    check(outs, sk)  every element against its own bound; gaps, slack rows and padding still NaN; copies bit-equal

Bounds (u = 2^-24; derived, never fitted to a kernel's output):
    accumulation     2 K u sum|A||W|: fp32 summation of K exact products in any order, the split-K slab additions included
    additions        4 u (|v| + |bias| + |res|) for the epilogue's additions
    LayerNorm fold   rstd (acc - mean cs) + b from the producer's fp32 (sum, sum of squares) partials: 4 u (|acc| + |mean cs|) for the
                     subtraction and scaling, 16 u (s2/C)/var |core| for rstd out of the cancelling s2/C - mean^2 (as xs() of
                     tests/test_gemm_epilogues_gpu.py)
    SiLU             as dense() of that file
    GEGLU            x gelu(g): |gelu(g)| dx + |x| (1.13 dg + 3e-7 (|g| + 1)) + 4 u |x gelu(g)|.  1.13 >= max |gelu'|; 3e-7 (|g| + 1) is
                     csrc/common.h erf_as (Abramowitz-Stegun 7.1.26, abs err <= 1.5e-7, + v_rcp_f32 and __expf round-off, about 6 u on
                     values <= 1) through 0.5 g (1 + erf): 0.5 |g| 5e-7, and the fp32 rounding of the products
    operand stores   half an ulp of the stored value: u_out (|ref| + bound)
    row statistics   the sums of the bounds of a 64-column slot + 64 u of its absolute sum (as dense())

Measured worst error / bound over all tuner pairs (MI355X, bf16 / fp16 build; MEASURED at the end of this file has it per family):
fp32 outputs 0.003 (LayerNorm-folded 0.012); operand-type outputs 0.98 / 0.94, nearly all of it the half-ulp rounding the bound
states exactly.  No pair was refused by launch_gemm and no case failed.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from helpers import rnd

U = 2.0 ** -24
NAN = float("nan")
ODT = {"bf16": torch.bfloat16, "fp16": torch.float16}
U_OUT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
GELU_TAILS = (0.0, 1e-3, -1e-3, 6.0, -6.0, 7.5, -7.5, 10.0, -10.0, 3.0, -3.0, 0.5)     # gates where the erf tails matter (_geglu_u)
PTR_FIELDS = ("A", "W", "A2", "bias", "res", "ln_stats", "ln_cs")


def ups4_weights(w):
    """[a][b][O][dy][dx][I] from OIHW fp32: the 3x3 taps that land on one input pixel are summed (tests/test_kernels_gpu.py)."""
    S = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    O, I = w.shape[:2]
    out = torch.zeros(2, 2, O, 2, 2, I)
    for a in (0, 1):
        for b in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    out[a, b, :, dy, dx, :] = sum(w[:, :, ky, kx] for ky in S[a][dy] for kx in S[b][dx])
    return out


def _excess(got, ref, bnd):
    """Largest |got - ref| / bnd (NaN counts as infinite) and the first offending row."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bnd)
    ratio = torch.where(torch.isfinite(err), err / bnd, torch.full_like(err, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    row = int(bad.reshape(bad.shape[0], -1).any(1).nonzero()[0, 0]) if bool(bad.any()) else -1
    return worst, row


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _all_nan(t):
    return bool(torch.isnan(t.float()).all()) if t.numel() else True


class FormCase:
    """One GEMM form at one shape.  ins: descriptor pointer field -> CPU tensor; f: the other descriptor fields; out_shapes: name ->
    (shape, dtype) of the NaN-poisoned outputs (C, aux, stats, vt); r: reference tensors (moved with to())."""

    def __init__(self, name, prec):
        self.name, self.prec = name, prec
        self.f, self.ins, self.out_shapes, self.r = {}, {}, {}, {}
        self.batch, self.defer, self.mutants = 1, False, []

    # ---- descriptor
    def desc_fields(self, ptrs):
        """Descriptor fields with the pointer fields taken from `ptrs` (name -> address)."""
        f = dict(self.f)
        f.update({k: ptrs[k] for k in self.ins})
        return f

    def host_desc(self):
        """A descriptor for the host-only queries: dummy non-null pointers where validity looks at them."""
        from diff_foley_amd import engine as E
        f = self.desc_fields({k: 64 for k in self.ins})
        d = E.GemmDesc(**f)
        d.C = 64
        for k, fld in (("aux", "aux"), ("stats", "stats"), ("vt", "vt")):
            if k in self.out_shapes:
                setattr(d, fld, 64)
        d.batch = self.batch
        d.defer_reduce = 1 if self.defer else 0
        return d

    def key(self, L):
        buf = C.create_string_buffer(160)
        assert L.df_test_gemm_key(C.byref(self.host_desc()), self.batch, buf, 160) == 0, L.df_last_error()
        return buf.value.decode()

    def to(self, dev):
        self.r = {k: v.to(dev) for k, v in self.r.items()}
        return self

    # ---- outputs
    def blank(self, dev="cpu"):
        return {k: torch.full(s, NAN, dtype=dt, device=dev) for k, (s, dt) in self.out_shapes.items()}

    def pack(self, final):
        """The buffers a correct launch leaves behind when its epilogue values are `final` [batch][rows][cols] (any float type)."""
        o = self.blank()
        M, N = self.Mo, self.No
        odt = ODT[self.prec]
        c32 = final.float()
        cst = c32.to(odt) if self.out_operand else c32
        rows = [slice(0, M)] + ([slice(M, 2 * M)] if self.dup else [])
        nc = N if self.vt_col0 is None else self.vt_col0
        for rs in rows:
            o["C"][:, rs, :nc] = cst[:, :, :nc]
            if "aux" in o:
                o["aux"][rs, :N] = c32[0].to(odt)
            if "stats" in o:
                s = c32[0].reshape(M, N // 64, 64)
                o["stats"][rs] = torch.stack([s.sum(-1), (s * s).sum(-1)], -1)
        if "vt" in o:
            T, Cv = self.vt_T, self.N - self.vt_col0
            o["vt"][:, :, :T] = c32[0][:, self.vt_col0:].to(odt).reshape(M // T, T, Cv).permute(0, 2, 1)
        return o

    # ---- checks
    def check(self, outs, sk=1):
        """-> (failure messages, worst error / bound, [(output, first offending row)])"""
        fails, rows, worst = [], [], 0.0
        M, N, r = self.Mo, self.No, self.r
        uo = U_OUT[self.prec]
        odt = ODT[self.prec]

        def cmp(what, got, ref, bnd, operand):
            nonlocal worst
            b = bnd * (1 + uo) + uo * ref.abs() if operand else bnd
            w, row = _excess(got, ref, b)
            worst = max(worst, w)
            if row >= 0:
                fails.append(f"{what}: row {row} off by {w:.3g} x its bound")
                rows.append((what, row))

        c = outs["C"]
        nrows = M + (M if self.dup else 0)
        nc = N if self.vt_col0 is None else self.vt_col0
        for z in range(self.batch):
            cmp(f"C slice {z}" if self.batch > 1 else "C", c[z, :M, :nc], r["ref"][z][:, :nc], r["bnd"][z][:, :nc], self.out_operand)
        if not _all_nan(c[:, :, nc:]):
            fails.append("ldc gap written")
        if not _all_nan(c[:, nrows:]):
            fails.append("rows past M (+ dup_rows) written")
        if self.dup and not torch.equal(_bits(c[:, M:nrows, :nc]), _bits(c[:, :M, :nc])):
            fails.append("dup_rows copy of C differs from its original")
        if "aux" in outs:
            a = outs["aux"]
            if not self.out_operand and not torch.equal(_bits(a[:M, :N]), _bits(c[0, :M, :N].to(odt))):
                fails.append("aux is not the operand-type rounding of C")
            cmp("aux", a[:M, :N], r["ref"][0], r["bnd"][0], True)
            if not _all_nan(a[:, N:]) or not _all_nan(a[nrows:]):
                fails.append("aux gap / rows past M (+ dup_rows) written")
            if self.dup and not torch.equal(_bits(a[M:nrows, :N]), _bits(a[:M, :N])):
                fails.append("dup_rows copy of aux differs from its original")
        if "stats" in outs:
            s = outs["stats"]
            cmp("stats", s[:M], r["ref_st"], r["bnd_st"], False)
            if not _all_nan(s[nrows:]):
                fails.append("stats rows past M (+ dup_rows) written")
            if self.dup and not torch.equal(_bits(s[M:nrows]), _bits(s[:M])):
                fails.append("dup_rows copy of stats differs from its original")
        if "vt" in outs:
            v = outs["vt"]
            T = self.vt_T
            cmp("vt", v[:, :, :T], r["ref_vt"], r["bnd_vt"], True)
            if not _all_nan(v[:, :, T:]):
                fails.append("vt padding (columns T .. ldvt) written")
        return fails, worst, rows


# ------------------------------------------------------------------------------------------------------------------------------
def _conv_nhwc(a, w, stride):
    """a [NB][H][W][C], w [N][3][3][C] -> [NB * OH * OW][N] (pad 1)"""
    y = F.conv2d(a.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1, stride=stride)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def _zstuff_nhwc(dy, w_oihw):
    """dy [NB][h][w][O], w [O][I][3][3] -> the stride-2 conv's input gradient [NB * 2h * 2w][I]"""
    y = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w_oihw, stride=2, padding=1, output_padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w_oihw.shape[1])


def _ups4_nhwc(a, w4):
    """a [NB][H][W][C], w4 [2][2][N][2][2][C] -> nearest-x2 + conv3x3 as four 2x2 convs, [NB * 2H * 2W][N]"""
    NB, H, W, _ = a.shape
    N = w4.shape[2]
    xp = F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1))
    out = torch.empty(NB, N, 2 * H, 2 * W, dtype=a.dtype)
    for p in (0, 1):
        for q in (0, 1):
            out[:, :, p::2, q::2] = F.conv2d(xp[:, :, p:p + H + 1, q:q + W + 1], w4[p, q].permute(0, 3, 1, 2))
    return out.permute(0, 2, 3, 1).reshape(-1, N)


def form(name, prec, *, kind="lin", M=0, K=0, N=0, conv=None, O=0, Cin2=0, lda2_pad=0, batch=1, bias=True, res=False, aux=False,
         stats=False, dup=False, silu=False, defer=False, ln=None, T=0, out_operand=0, ld_pad=4, seed=0):
    """kind: lin | conv (3x3 stride 1) | s2 (3x3 stride 2) | zstuff (transposed stride-2 conv of the classifier gradient; conv = the
    stored dY map, O its real channel count) | ups4 (phase-decomposed upsample conv).  ln: plain | geglu | vt (fused QKV, N = 3C)."""
    cs = FormCase(name, prec)
    odt = ODT[prec]
    op = lambda t: t.to(odt)
    cs.batch, cs.defer, cs.dup, cs.kind, cs.ln = batch, defer, dup, kind, ln
    f = cs.f
    # ---- operands and the float64 accumulator
    if kind == "lin":
        K1 = K
        x = rnd((batch, M, K1), seed)
        if ln:
            x = x * (0.25 + 1.5 * (torch.arange(M) % 3 == 0).float())[None, :, None] + (torch.arange(M) % 5).float()[None, :, None]
        Aq = op(x)
        Ktot = K1 + Cin2
        Wq = op(rnd((batch, N, Ktot), seed + 1) / Ktot ** 0.5 * (2.0 if ln else 1.0))
        if ln == "geglu":            # group 0's first gates sit at the erf tails: no weights, the value is the bias
            Wq[0, 32:32 + len(GELU_TAILS)] = 0
        f.update(M=M, N=N, K=K1)
        if batch > 1:
            f.update(a_bs=M * K1, w_bs=N * Ktot)
        parts = [(Aq.double(), Wq[..., :K1].double())]
        Mo = M
    else:
        NB, H, Wd, Cin = conv
        taps = 4 if kind == "ups4" else 9
        Aq = op(rnd((NB, H, Wd, Cin), seed))
        if kind == "zstuff":
            Aq[..., O:] = 0                                            # Opad zero columns in dY
            w_oihw = op(rnd((O, N, 3, 3), seed + 1) / (3 * O ** 0.5))     # distinct taps
            Wq = torch.zeros(N, 3, 3, Cin, dtype=odt)
            Wq[..., :O] = w_oihw.flip(2, 3).permute(1, 2, 3, 0)         # launch_pack_conv_bwd: [I][2 - ky][2 - kx][Opad]
            cs.w_oihw = w_oihw
            Mo = NB * 4 * H * Wd
            f.update(conv=1, ups=1, zstuff=1, stride=1)
        elif kind == "ups4":
            w = rnd((N, Cin, 3, 3), seed + 1) / (3 * Cin ** 0.5)
            Wq = op(ups4_weights(w))                                   # [2][2][N][2][2][Cin]
            Mo = NB * 4 * H * Wd
            f.update(conv=2)
        else:
            st = 2 if kind == "s2" else 1
            Wq = op(rnd((N, 3, 3, Cin + 0), seed + 1) / (9 * Cin + Cin2) ** 0.5)
            Mo = NB * (H // st) * (Wd // st)
            f.update(conv=1, stride=st)
        f.update(NB=NB, H=H, Wd=Wd, Cin=Cin, N=N)
        Ktot = taps * Cin + Cin2
        M = Mo
    cs.A, cs.Wq = Aq, Wq
    if Cin2:
        rows2 = M
        lda2 = Cin2 + lda2_pad
        A2 = torch.zeros(rows2, lda2, dtype=odt)
        A2[:, :Cin2] = op(rnd((rows2, Cin2), seed + 7))
        if kind == "lin":
            W2 = Wq[0, :, K1:]
        else:
            W2 = op(rnd((N, Cin2), seed + 8) / Ktot ** 0.5)
            Wq = torch.cat([Wq.reshape(N, -1), W2], 1).contiguous()
        cs.A2, cs.W2 = A2, W2
        cs.ins["A2"] = A2
        f.update(lda2=lda2, Cin2=Cin2)
    cs.ins["A"], cs.ins["W"] = Aq, Wq

    def accumulate(dt, absolute=False, chunked=False, A=None, A2_=None, W_=None, taps_off=()):
        """sum_k A W in dtype dt.  chunked: K in 64-wide chunks, last chunk first (an independent summation order).  taps_off: 3x3
        taps (ky, kx) left out."""
        g = (lambda t: t.to(dt).abs()) if absolute else (lambda t: t.to(dt))
        a = g(cs.A if A is None else A)
        wq = cs.Wq if W_ is None else W_
        kc = a.shape[-1]
        spans = [(k0, k0 + 64) for k0 in range(0, kc, 64)][::-1] if chunked else [(0, kc)]
        tot = None
        for k0, k1 in spans:
            if kind == "lin":
                p = torch.stack([a[z, :, k0:k1] @ g(wq[z, :, k0:k1]).t() for z in range(batch)])
            elif kind == "zstuff":
                wz = g(cs.w_oihw if W_ is None else W_)
                if k0 >= wz.shape[0]:
                    continue
                p = _zstuff_nhwc(a[..., k0:min(k1, wz.shape[0])], wz[k0:k1])[None]
            elif kind == "ups4":
                p = _ups4_nhwc(a[..., k0:k1], g(wq[..., k0:k1]))[None]
            else:
                w3 = g(wq.reshape(N, -1)[:, :9 * Cin].reshape(N, 3, 3, Cin)[..., k0:k1]).clone()
                for ky, kx in taps_off:
                    w3[:, ky, kx] = 0
                p = _conv_nhwc(a[..., k0:k1], w3, 2 if kind == "s2" else 1)[None]
            tot = p if tot is None else tot + p
        if Cin2:
            a2 = g(cs.A2 if A2_ is None else A2_)[:, :Cin2]
            for k0 in (range(0, Cin2, 64)[::-1] if chunked else [0]):
                k1 = k0 + 64 if chunked else Cin2
                tot = tot + (a2[:, k0:k1] @ g(cs.W2[:, k0:k1]).t())[None]
        return tot

    cs.accumulate = accumulate
    acc = accumulate(torch.float64)
    absacc = accumulate(torch.float64, absolute=True)
    cs.acc64 = acc
    # ---- epilogue operands
    if ln:
        slots = K // 64
        s = x[0].double().reshape(M, slots, 64)
        stt = torch.stack([s.sum(-1), (s * s).sum(-1)], -1).float()
        csum = Wq[0].double().sum(-1).float()
        cs.ins["ln_stats"], cs.ins["ln_cs"] = stt, csum
        f.update(ln_slots=slots, ln_C=K, ln_eps=1e-5)
        sd1, sd2 = stt[..., 0].double().sum(1), stt[..., 1].double().sum(1)
        mean = sd1 / K
        var = sd2 / K - mean * mean
        rstd = (var + 1e-5).rsqrt()
        cm = mean[:, None] * csum.double()[None]
    b = None
    if bias:
        b = rnd((N,), seed + 2) * (0.5 if ln else 1.0)
        if ln == "geglu":
            b[32:32 + len(GELU_TAILS)] = torch.tensor(GELU_TAILS)
        cs.ins["bias"] = b
    r = None
    if res:
        ldr = N + ld_pad
        r = torch.full((batch, Mo, ldr), NAN)
        r[:, :, :N] = rnd((batch, Mo, N), seed + 4)
        cs.ins["res"] = r
        f.update(ldr=ldr, res_bs=Mo * ldr)

    def epi(a, dt, with_bound=False, no_cm_rows=(), swap_group=None):
        """The epilogue on accumulator `a` in dtype dt.  with_bound (float64 only): also the per-element bound.  Defects for the CPU
        test: no_cm_rows -- rows whose mean * colsum term is dropped; swap_group -- a GEGLU group whose x and gate are exchanged."""
        v = a.to(dt)
        bnd = 2 * Ktot * U * absacc if with_bound else None
        terms = v.abs()
        if ln:
            cmv = cm.to(dt).clone()
            if len(no_cm_rows):
                cmv[list(no_cm_rows)] = 0
            core = rstd.to(dt)[:, None] * (v - cmv[None])
            if with_bound:
                bnd = rstd[:, None] * (bnd + 4 * U * (v.abs() + cm.abs()[None])) + 16 * U * (sd2 / K / var)[:, None] * core.abs()
            v = core
            terms = v.abs()
        if b is not None:
            v = v + b.to(dt)
            terms = terms + b.to(dt).abs()
        if r is not None:
            v = v + r[:, :, :N].to(dt)
            terms = terms + r[:, :, :N].to(dt).abs()
        if with_bound:
            bnd = bnd + 4 * U * terms
        if silu:
            sv = F.silu(v)
            if with_bound:
                bnd = 1.1 * bnd + 4 * U * (v.abs() + 8) * sv.abs()
            v = sv
        if ln == "geglu":
            g4 = v.reshape(batch, M, N // 64, 2, 32)
            xv, gv = g4[..., 0, :], g4[..., 1, :]
            if swap_group is not None:
                xv, gv = xv.clone(), gv.clone()
                xv[:, :, swap_group], gv[:, :, swap_group] = g4[:, :, swap_group, 1], g4[:, :, swap_group, 0]
            out = xv * F.gelu(gv)
            if with_bound:
                b4 = bnd.reshape(batch, M, N // 64, 2, 32)
                bnd = (F.gelu(gv).abs() * b4[..., 0, :] + xv.abs() * (1.13 * b4[..., 1, :] + 3e-7 * (gv.abs() + 1)) + 4 * U * out.abs())
                bnd = bnd.reshape(batch, M, N // 2)
            v = out.reshape(batch, M, N // 2)
        return (v, bnd + 1e-30) if with_bound else v

    cs.epi = epi
    ref, bnd = epi(acc, torch.float64, with_bound=True)
    cs.r["ref"], cs.r["bnd"] = ref, bnd
    No = N // 2 if ln == "geglu" else N
    cs.Mo, cs.No, cs.N, cs.M, cs.K = Mo, No, N, M, Ktot
    cs.out_operand = 1 if (out_operand or ln in ("geglu", "vt")) else 0
    cs.vt_col0, cs.vt_T = None, 0
    f.update(out_operand=cs.out_operand)
    if silu:
        f["silu"] = 1
    if ln == "geglu":
        f["geglu"] = 1
    # ---- outputs
    R = Mo + (Mo if dup else 0) + 3
    cdt = odt if cs.out_operand else torch.float32
    if ln == "vt":
        Cq = N // 3
        cs.vt_col0, cs.vt_T = 2 * Cq, T
        ldc, ldvt = 2 * Cq + 8, T + 8
        cs.out_shapes["vt"] = ((M // T, Cq, ldvt), odt)
        f.update(vt_col0=2 * Cq, vt_T=T, ldvt=ldvt)
        cs.r["ref_vt"] = ref[0][:, 2 * Cq:].reshape(M // T, T, Cq).permute(0, 2, 1).contiguous()
        cs.r["bnd_vt"] = bnd[0][:, 2 * Cq:].reshape(M // T, T, Cq).permute(0, 2, 1).contiguous()
    else:
        ldc = No + (8 if cs.out_operand else ld_pad)
    f.update(ldc=ldc, c_bs=R * ldc)
    cs.out_shapes["C"] = ((batch, R, ldc), cdt)
    if dup:
        f["dup_rows"] = Mo
    if aux:
        f["ld_aux"] = No + ld_pad
        cs.out_shapes["aux"] = ((R, No + ld_pad), odt)
    if stats:
        slots_o = No // 64
        f["stats_slots"] = slots_o
        cs.out_shapes["stats"] = ((R, slots_o, 2), torch.float32)
        v0, b0 = ref[0].reshape(Mo, slots_o, 64), bnd[0].reshape(Mo, slots_o, 64)
        a0 = v0.abs()
        cs.r["ref_st"] = torch.stack([v0.sum(-1), (v0 * v0).sum(-1)], -1)
        cs.r["bnd_st"] = torch.stack([b0.sum(-1) + 64 * U * a0.sum(-1), (2 * a0 * b0 + b0 * b0).sum(-1) + 64 * U * (a0 * a0).sum(-1)],
                                     -1) + 1e-30
    if defer:
        cs.gn_g, cs.gn_b = rnd((N,), seed + 5), rnd((N,), seed + 6)
    _add_mutants(cs)
    return cs


# ------------------------------------------------------------------------------------------------------------------------------
def _add_mutants(cs):
    """Single-site defects a kernel could have, as functions -> the outputs such a kernel would leave (float64 arithmetic otherwise)."""
    kind, mk = cs.kind, cs.mutants
    acc = cs.acc64
    A64, W64 = cs.A.double(), cs.Wq.double()
    outs_of = lambda a, **kw: cs.pack(cs.epi(a, torch.float64, **kw))
    if kind in ("conv", "s2"):
        NB, H, Wd, Cin = cs.A.shape
        N = cs.N
        st = 2 if kind == "s2" else 1
        OH, OW = H // st, Wd // st
        w3 = W64.reshape(N, -1)[:, :9 * Cin].reshape(N, 3, 3, Cin)

        def tap_dropped():       # the bottom-right tap of sample 1's top-left output pixel (it reads an interior pixel)
            a = acc.clone()
            a[0, OH * OW] -= w3[:, 2, 2] @ A64[1, st * 0 + 1, st * 0 + 1]
            return outs_of(a)
        mk.append(("one tap dropped at a corner pixel", tap_dropped))

        def cross_sample():      # a padding row taken from the neighbouring sample instead of zeros
            a = acc.clone()
            if st == 1:          # sample 0's last pixel: tap (2, 1) reads sample 1's first row
                a[0, OH * OW - 1] += w3[:, 2, 1] @ A64[1, 0, Wd - 1]
            else:                # sample 1's first pixel: tap (0, 1) reads sample 0's last row
                a[0, OH * OW] += w3[:, 0, 1] @ A64[0, H - 1, 0]
            return outs_of(a)
        mk.append(("a sample's edge row reads the neighbouring sample", cross_sample))
    if kind == "zstuff":
        mk.append(("taps not flipped", lambda: outs_of(cs.accumulate(torch.float64, W_=cs.w_oihw.flip(2, 3)))))
    if kind == "ups4":
        def phase_swapped():
            w = cs.Wq.clone()
            w[0, 1], w[1, 0] = cs.Wq[1, 0], cs.Wq[0, 1]
            return outs_of(cs.accumulate(torch.float64, W_=w))
        mk.append(("one phase's weights swapped", phase_swapped))

        def tap_dropped4():      # tap (1, 1) of phase (0, 0) at sample 1's top-left pixel: it reads input pixel (0, 0)
            a = acc.clone()
            NB, H, Wd, _ = cs.A.shape
            a[0, 4 * H * Wd] -= W64[0, 0, :, 1, 1] @ A64[1, 0, 0]
            return outs_of(a)
        mk.append(("one tap dropped at a corner pixel", tap_dropped4))
    if hasattr(cs, "A2") and cs.W2.shape[1] > 64:      # (a 64-channel range rolled by 64 is itself)
        def skip_offset():
            a2 = cs.A2.clone()
            c2 = cs.W2.shape[1]
            a2[:, :c2] = torch.roll(cs.A2[:, :c2], 64, 1)
            return outs_of(cs.accumulate(torch.float64, A2_=a2))
        mk.append(("the second operand's range offset by 64 channels", skip_offset))
    if cs.ln:
        mk.append(("mean * colsum dropped in one row", lambda: outs_of(acc, no_cm_rows=(cs.M - 2,))))
    if cs.ln == "geglu":
        mk.append(("x and gate swapped in one 32-column group", lambda: outs_of(acc, swap_group=1)))
    if cs.ln == "vt":
        def vt_no_bias():
            o = outs_of(acc)
            c, t = 5, cs.vt_T - 1
            o["vt"][1, c, t] = (cs.r["ref"][0][cs.vt_T + t, cs.vt_col0 + c] - cs.ins["bias"][cs.vt_col0 + c].double()).to(o["vt"].dtype)
            return o
        mk.append(("bias missing on one V^T element", vt_no_bias))

        def vt_wrong_sample():
            o = outs_of(acc)
            good = o["vt"].clone()
            o["vt"][0, 3, 2], o["vt"][1, 3, 2] = good[1, 3, 2], good[0, 3, 2]
            return o
        mk.append(("V^T written at row % T of the wrong sample", vt_wrong_sample))
    if cs.defer:
        def slab_missing():
            if kind == "lin":
                k0 = cs.A.shape[-1] // 64 // 2 * 64
                a = acc - (A64[:, :, k0:] @ W64[:, :, k0:cs.A.shape[-1]].transpose(1, 2))
            else:                # the last of nine one-tap slabs
                a = cs.accumulate(torch.float64, taps_off=((2, 2),))
            return outs_of(a)
        mk.append(("one slab missing from a deferred reduce", slab_missing))


# ------------------------------------------------------------------------------------------------------------------------------
# One or more cases per form.  Conv maps: NB >= 2 (a patch never reads across samples), widths 16 k and not, ragged last M tiles,
# every border pixel is an output.  Cin up to 1536 so that split-K reaches what the tables ship (generic tiles need K / 64 >= 2 sk,
# halo tiles Cin / 64 >= sk); K / 64 divisible by the shipped factors where the shape allows, so that no slab is empty.
def _cases():
    c = {}

    def add(name, **kw):
        c[name] = lambda prec, name=name, kw=kw: form(name, prec, **kw)

    # ---- taps 1
    add("lin_e0", M=100, N=96, K=1536, seed=100)                                                  # e0, split-K to 12
    add("lin_e0_n33", M=70, N=33, K=256, bias=False, seed=101)                                    # e0: odd N (scalar epilogue)
    add("lin_batch3", M=80, N=64, K=256, batch=3, bias=False, seed=102)                           # e0 batched
    add("lin_silu", M=32, N=128, K=1536, silu=True, seed=103)                                     # e128: time-embedding MLP
    add("lin_aux", M=96, N=256, K=256, aux=True, seed=104)                                        # e8
    add("lin_aux_stats", M=72, N=320, K=1280, aux=True, stats=True, seed=105)                     # e10: producer without residual
    add("lin_res", M=72, N=256, K=1024, res=True, seed=106)                                       # e16
    add("lin_res_aux", M=200, N=256, K=128, res=True, aux=True, seed=107)                         # e24
    add("lin_prod", M=72, N=320, K=1280, res=True, aux=True, stats=True, seed=108)                # e26: st.attn1.out
    add("lin_prod_dup", M=96, N=320, K=320, res=True, aux=True, stats=True, dup=True, seed=109)   # e282: CFG prefix
    add("lin_res_defer", M=144, N=256, K=512, res=True, defer=True, seed=110)                     # e80
    # st.ffproj: K over two operand tensors (K1 = 4C, Cin2 = C), residual with a padded ldr; operand copy / deferred
    add("ffproj_c64", M=136, N=64, K=256, Cin2=64, res=True, aux=True, seed=120)                  # e56
    add("ffproj_c320", M=72, N=320, K=1280, Cin2=320, lda2_pad=8, res=True, aux=True, seed=121)   # e56, split-K to 12
    add("ffproj_c64_defer", M=136, N=64, K=256, Cin2=64, res=True, defer=True, seed=122)          # e112
    add("ffproj_c320_defer", M=72, N=320, K=1280, Cin2=320, res=True, defer=True, seed=123)       # e112, split-K to 12
    # LayerNorm-folded consumers: plain (own split-K reduce), fused QKV (vt_col0 = 2C a tile boundary for every BN), GEGLU
    add("ln_plain_c320", M=100, N=256, K=320, ln="plain", seed=130)                               # e1
    add("ln_plain_c1280", M=72, N=256, K=1280, ln="plain", seed=131)                              # e1, split-K to 8
    add("qkv_c128", M=2 * 96, N=384, K=128, ln="vt", T=96, seed=140)                              # e5
    add("qkv_c320", M=3 * 64, N=960, K=320, ln="vt", T=64, seed=141)
    add("qkv_c640", M=2 * 100, N=1920, K=640, ln="vt", T=100, seed=142)
    add("geglu_c320", M=200, N=2560, K=320, ln="geglu", seed=150)                                 # geglu e1: ragged last row tile
    add("geglu_c640", M=128, N=5120, K=640, ln="geglu", seed=151)                                 # M = one tile, 10 statistics slots
    add("geglu_c1280", M=72, N=1280 * 2, K=1280, ln="geglu", seed=152)                            # 20 statistics slots (tile 31)
    # ---- phase-decomposed upsample conv: odd map, N a multiple of 4 but not of 64 under split-K
    add("ups4_5x7", kind="ups4", conv=(2, 5, 7, 384), N=68, seed=160)                             # taps 4 e0, split-K to 12
    add("ups4_4x16", kind="ups4", conv=(2, 4, 16, 128), N=256, seed=161)
    # ---- 3x3 stride 1
    add("conv_e0", kind="conv", conv=(2, 8, 16, 256), N=64, seed=170)                             # e0, split-K to 16
    add("conv_e0_w8", kind="conv", conv=(3, 6, 8, 768), N=128, seed=171)                          # width 8: halo patches 8 wide
    add("conv_res", kind="conv", conv=(2, 6, 16, 256), N=128, res=True, seed=172)                 # e16
    add("conv_dup", kind="conv", conv=(2, 6, 16, 64), N=320, dup=True, seed=173)                  # e256
    add("conv_res_dup", kind="conv", conv=(2, 6, 16, 192), N=320, res=True, dup=True, seed=174)   # e272
    add("conv_defer", kind="conv", conv=(2, 8, 16, 1536), N=128, defer=True, seed=175)            # e64, split-K to 24 / 16 halo
    add("conv_defer_w8", kind="conv", conv=(2, 12, 8, 768), N=64, defer=True, seed=176)
    add("conv_res_defer", kind="conv", conv=(2, 8, 16, 768), N=128, res=True, defer=True, seed=177)   # e80, split-K to 12
    # folded 1x1 skip: Cin2 != Cin both ways, Cin2 / 64 of 1, 3 and >= 10 (the three-slot tail ring of tiles 23-25 wraps)
    add("skip_c2_64", kind="conv", conv=(2, 6, 16, 128), N=128, Cin2=64, seed=180)                # e32
    add("skip_c2_192", kind="conv", conv=(2, 6, 8, 64), N=128, Cin2=192, lda2_pad=8, seed=181)
    add("skip_aux", kind="conv", conv=(2, 4, 16, 1280), N=128, Cin2=2560, aux=True, seed=182)     # e40, split-K to 24 / 12 halo
    add("skip_defer", kind="conv", conv=(2, 6, 16, 768), N=128, Cin2=640, defer=True, seed=183)   # e96, split-K to 16 / 12 halo
    add("skip_defer_w8", kind="conv", conv=(2, 6, 8, 128), N=64, Cin2=320, defer=True, seed=184)
    add("skip_dup", kind="conv", conv=(2, 6, 16, 128), N=128, Cin2=192, res=True, aux=True, dup=True, seed=185)   # res.conv2 under CFG
    # ---- zero-stuffed transposed conv of the classifier gradient (operand copy): 96 real channels in 128
    add("zstuff", kind="zstuff", conv=(2, 3, 8, 128), O=96, N=128, bias=False, aux=True, seed=190)     # taps 9 ups 1 e8, split-K to 12
    add("zstuff_w5", kind="zstuff", conv=(2, 4, 5, 256), O=256, N=64, bias=False, aux=True, seed=191)
    # ---- 3x3 stride 2 (Downsample): even maps, OW not a multiple of 16
    add("s2_e0", kind="s2", conv=(2, 8, 24, 384), N=128, seed=200)                                # stride 2 e0, split-K to 8
    add("s2_defer", kind="s2", conv=(2, 8, 20, 768), N=128, defer=True, seed=201)                 # stride 2 e64, split-K to 24
    return c


CASES = _cases()

# Measured worst error / bound per case family over every tuner pair (MI355X): (bf16 build, fp16 build).
MEASURED = {
    "fp32 C: linear, two-operand K, 3x3 stride 1 / 2, folded skip, phase-decomposed, deferred": (0.003, 0.003),
    "fp32 C, LayerNorm-folded (ln_plain_*)": (0.012, 0.012),
    "operand copy (aux) of a linear / producer / ffproj GEMM": (0.977, 0.937),
    "operand copy of a conv: skip_aux, skip_dup, zstuff*": (0.874, 0.570),
    "fused QKV: y and V^T (qkv_*)": (0.966, 0.877),
    "GEGLU (geglu_*)": (0.879, 0.577),
}
