"""GPU: every GEMM epilogue the plan uses, on every (tile, split-K) pair the autotuner may pick for it.

autotune_plan (csrc/engine_tune.hip) times each GEMM on tiles 0 .. TILE_ALL-1 with split-K 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, where the
first split-K > 1 that gemm_tile_valid refuses ends that tile's walk; whichever pair is fastest becomes production code on that
machine.  Each case below is one plan epilogue (csrc/gemm.h GemmParams) at a small shape chosen so that its edges occur, run
through df_test_gemm_ex on exactly that set of pairs.

Reference: float64 on the CPU from operands rounded to the build's operand type.  Every element is held to its own bound: fp32
accumulation over K (2 K u |A||W|), fp32 round-off of the epilogue additions, and the rounding of an operand-type output (half an
ulp).  Outputs are NaN-poisoned before each launch, so gaps (ldc / ld_aux), rows outside [0, M + dup_rows) and buffers that must
stay untouched (no_c_store, cfg_out) are checked as well.  Bit-level invariants need no reference: every gm walk order and a
repeated launch give the same bits, a batch-n launch equals n single-slice launches, duplicated CFG rows equal their originals,
and split-K slabs left for a GroupNorm (defer_reduce) finish to the same bits as the GEMM's own reduce.

Measured worst error / bound over all pairs (MI355X): fp32 outputs 0.005; operand-type outputs (probabilities, aux copies, batched
operand output) 0.98 bf16 / 0.94 fp16, nearly all of it the half-ulp rounding the bound states exactly."""
import ctypes as C
import time

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


def _eng():
    from diff_foley_amd import engine as E
    return E


def lib():
    return _eng().lib(PREC)


def odt():
    return _eng().OPERAND_DTYPE[PREC]


def op(t):
    """Round to the build's operand type (what the kernel multiplies)."""
    return t.to(odt())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


U = 2.0 ** -24                       # fp32 unit round-off


def u_out():
    """Relative rounding of an operand-type store (round to nearest even: half an ulp)."""
    return 2.0 ** -8 if PREC == "bf16" else 2.0 ** -11


TILE_ALL = 35                        # csrc/gemm.h GemmTile
SKS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
GMS = (1, 2, 4, 8, 16)               # the in-plan walk orders autotune_plan tries besides 0
NAN = float("nan")


def tuner_pairs(d, batch):
    """The (tile, split-K) pairs autotune_plan launches for this GEMM, in its order."""
    L = lib()
    out = []
    for t in range(TILE_ALL):
        for sk in SKS:
            v = L.df_test_gemm_valid(C.byref(d), t, batch, sk)
            assert v >= 0, L.df_last_error()
            if not v:
                if sk > 1:
                    break
                continue
            out.append((t, sk))
    return out


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def all_nan(t):
    return bool(torch.isnan(t.float()).all()) if t.numel() else True


class Case:
    """One plan epilogue: device inputs, the descriptor fields, NaN-poisoned outputs and the float64 reference + bounds."""

    def __init__(self, name):
        self.name = name
        self.f = {}          # GemmDesc fields (ints / floats / device pointers)
        self.outs = {}       # name -> output tensor, NaN before every launch
        self.keep = []       # device inputs referenced by pointer
        self.batch = 1
        self.defer = False
        self.cfg = None

    def dev(self, t):
        t = t.cuda().contiguous()
        self.keep.append(t)
        return t

    def out(self, name, shape, dtype):
        self.outs[name] = torch.full(shape, NAN, dtype=dtype, device="cuda")
        return self.outs[name]

    def desc(self, tile, sk, gm, batch=None, **over):
        f = dict(self.f)
        f.update(over)
        d = _eng().GemmDesc(**f)
        d.tile, d.splitk, d.gm, d.batch = tile, sk, gm, self.batch if batch is None else batch
        return d

    def poison(self):
        for t in self.outs.values():
            t.fill_(NAN)

    def set_outs(self, d, sk):
        _set_outs(self, d, sk)

    def launch(self, d):
        self.poison()
        rc = lib().df_test_gemm_ex(C.byref(d), stream())
        return rc, (lib().df_last_error().decode() if rc else "")


def _excess(got, ref, bnd):
    """Largest |got - ref| / bnd (NaN counts as infinite) and the first offending row."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bnd)
    ratio = torch.where(torch.isfinite(err), err / bnd, torch.full_like(err, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    row = int(bad.reshape(bad.shape[0], -1).any(1).nonzero()[0, 0]) if bool(bad.any()) else -1
    return worst, row


def _slot_stats(v, slots):
    """(sum, sum of squares) of every 64-column slot of every row, float64."""
    s = v.reshape(v.shape[0], slots, 64)
    return s.sum(-1), (s * s).sum(-1)


# ------------------------------------------------------------------------------------------------------------------------------
# plain epilogues: linear / 3x3 conv, bias, FiLM row bias, residual, alpha, SiLU / ReLU, aux copy, row statistics, CFG-prefix row
# duplication, no_c_store, per-sample weights (w_rows), batched slices, NCHW store, CFG combine in the split-K reduce
def dense(name, *, N, M=0, K=0, conv=None, S=1, batch=1, alpha=1.0, bias=True, film=None, res=False, act=0, out_operand=0,
          aux=False, stats=False, dup=False, no_c_store=False, nchw=False, cfg=None, ldc_pad=4, ld_pad=4, defer=False, seed=0):
    cs = Case(name)
    cs.batch, cs.defer = batch, defer
    if conv:
        NB, H, Wd, Cin = conv
        M, K = NB * H * Wd, 9 * Cin
    Ws = rnd((batch * S, N, K), seed + 1) / K ** 0.5
    Wq = op(Ws)
    W64 = Wq.double()
    if conv:
        Aq = op(rnd((NB, H, Wd, Cin), seed))
        A64 = Aq.double()
        wc = W64[0].reshape(N, 3, 3, Cin).permute(0, 3, 1, 2)
        conv2 = lambda a, w: F.conv2d(a.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(M, N)
        acc = conv2(A64, wc)[None]
        absacc = conv2(A64.abs(), wc.abs())[None]
    else:
        Aq = op(rnd((batch, M, K), seed))
        A64 = Aq.double()
        Ms = M // S
        acc = torch.stack([torch.cat([A64[z, s * Ms:(s + 1) * Ms] @ W64[z * S + s].t() for s in range(S)]) for z in range(batch)])
        absacc = torch.stack([torch.cat([A64[z, s * Ms:(s + 1) * Ms].abs() @ W64[z * S + s].abs().t() for s in range(S)])
                              for z in range(batch)])
    v = alpha * acc
    bnd = 2 * K * U * abs(alpha) * absacc
    terms = v.abs()
    f = cs.f
    f.update(M=M, N=N, K=K, A=cs.dev(Aq).data_ptr(), W=cs.dev(Wq).data_ptr(), out_operand=out_operand, alpha=alpha)
    if conv:
        f.update(conv=1, NB=NB, H=H, Wd=Wd, Cin=Cin, stride=1)
    if batch > 1:
        f.update(a_bs=M * K, w_bs=N * K)
    if S > 1:
        f.update(w_rows=M // S, w_bs=N * K)
    if bias:
        b = rnd((N,), seed + 2)
        f["bias"] = cs.dev(b).data_ptr()
        v = v + b.double()
        terms = terms + b.double().abs()
    if film:
        mode, rps = film
        ldrb = N + ld_pad
        nrb = M // rps if mode == 1 else rps
        rb = torch.full((nrb, ldrb), NAN)
        rb[:, :N] = rnd((nrb, N), seed + 3)
        idx = torch.arange(M) // rps if mode == 1 else torch.arange(M) % rps
        rbr = rb[idx, :N].double()
        f.update(rowbias=cs.dev(rb).data_ptr(), ld_rowbias=ldrb, rows_per_sample=rps, rowbias_mode=mode)
        v = v + rbr
        terms = terms + rbr.abs()
    if res:
        ldr = N + ld_pad
        r = torch.full((batch, M, ldr), NAN)
        r[:, :, :N] = rnd((batch, M, N), seed + 4)
        f.update(res=cs.dev(r).data_ptr(), ldr=ldr, res_bs=M * ldr)
        v = v + r[:, :, :N].double()
        terms = terms + r[:, :, :N].double().abs()
    bnd = bnd + 4 * U * terms
    if act == 1:
        f["silu"] = 1
        sv = F.silu(v)
        bnd = 1.1 * bnd + 4 * U * (v.abs() + 8) * sv.abs()
        v = sv
    elif act == 2:
        f["relu"] = 1
        v = v.clamp_min(0)
    cs.ref, cs.bnd = v.cuda(), (bnd + 1e-30).cuda()
    cs.M, cs.N, cs.K, cs.dup, cs.no_c_store, cs.nchw, cs.cfg, cs.out_operand = M, N, K, dup, no_c_store, nchw, cfg, out_operand
    cs.A, cs.W, cs.elt = Aq, Wq, (2 if out_operand else 4)
    R = M + (M if dup else 0) + 3                     # rows past M (+ dup_rows) must stay NaN
    cdt = odt() if out_operand else torch.float32
    if nchw:
        HW = H * Wd
        f.update(store_nchw=1, hw_out=HW, ldc=N)
        cs.HW, cs.NB = HW, NB
        cs.out("C", (NB * N * HW + 64,), cdt)
        if cfg:
            cs.out("cfg", ((NB // 2) * N * HW + 64,), torch.float32)
            u_, c_ = v[0][:M // 2], v[0][M // 2:]
            cs.ref_cfg = (u_ + cfg * (c_ - u_)).cuda()
            bu, bc = bnd[0][:M // 2], bnd[0][M // 2:]
            cs.bnd_cfg = ((1 + cfg) * bu + cfg * bc + 4 * U * (u_.abs() + cfg * (c_ - u_).abs()) + 1e-30).cuda()
    else:
        ldc = N + ldc_pad
        f["ldc"] = ldc
        f["c_bs"] = R * ldc
        cs.R, cs.ldc = R, ldc
        cs.out("C", (batch, R, ldc), cdt)
        if dup:
            f["dup_rows"] = M
        if no_c_store:
            f["no_c_store"] = 1
    if aux:
        lda_ = N + ld_pad
        f.update(ld_aux=lda_)
        cs.ld_aux = lda_
        cs.out("aux", (R, lda_), odt())
    if stats:
        cs.slots = N // 64
        f["stats_slots"] = cs.slots
        cs.out("stats", (R, cs.slots, 2), torch.float32)
        s1, s2 = _slot_stats(v[0], cs.slots)
        b0 = bnd[0].reshape(M, cs.slots, 64)
        a0 = v[0].abs().reshape(M, cs.slots, 64)
        cs.ref_st = torch.stack([s1, s2], -1).cuda()
        cs.bnd_st = torch.stack([b0.sum(-1) + 64 * U * a0.sum(-1),
                                 (2 * a0 * b0 + b0 * b0).sum(-1) + 64 * U * (a0 * a0).sum(-1)], -1).cuda() + 1e-30
    if defer:
        cs.gn_x = torch.empty(M, N, device="cuda")
        cs.gn_out = torch.empty(M, N, dtype=odt(), device="cuda")
        cs.gn_g, cs.gn_b = cs.dev(rnd((N,), seed + 5)), cs.dev(rnd((N,), seed + 6))
    cs.check = lambda sk: _check_dense(cs, sk)
    return cs


def _set_outs(cs, d, sk):
    """Point the descriptor at this launch's outputs (cfg_out only where the plan sets it: split-K > 1)."""
    d.C = cs.outs["C"].data_ptr()
    if "aux" in cs.outs:
        d.aux = cs.outs["aux"].data_ptr()
    if "stats" in cs.outs:
        d.stats = cs.outs["stats"].data_ptr()
    if cs.cfg and sk > 1:
        d.cfg_out, d.cfg_scale = cs.outs["cfg"].data_ptr(), cs.cfg


def _check_dense(cs, sk):
    """-> (list of failures, worst error / bound)"""
    fails, worst = [], 0.0
    M, N = cs.M, cs.N
    c = cs.outs["C"]
    extra = u_out() if cs.out_operand else 0.0

    def cmp(what, got, ref, bnd):
        nonlocal worst
        w, row = _excess(got, ref, bnd + extra * ref.abs())
        worst = max(worst, w)
        if row >= 0:
            fails.append(f"{what}: row {row} off by {w:.3g} x its bound")

    if cs.nchw:
        HW, NB = cs.HW, cs.NB
        if cs.cfg and sk > 1:
            if not all_nan(c):
                fails.append("C written although cfg_out takes the guided output")
            g = cs.outs["cfg"]
            if not all_nan(g[(NB // 2) * N * HW:]):
                fails.append("cfg_out written past its end")
            got = g[:(NB // 2) * N * HW].view(NB // 2, N, HW).permute(0, 2, 1).reshape(M // 2, N)
            cmp("cfg_out", got, cs.ref_cfg, cs.bnd_cfg)
        else:
            if not all_nan(c[NB * N * HW:]):
                fails.append("NCHW store past the end of C")
            got = c[:NB * N * HW].view(NB, N, HW).permute(0, 2, 1).reshape(M, N)
            cmp("C (NCHW)", got, cs.ref[0], cs.bnd[0])
        return fails, worst
    rows = M + (M if cs.dup else 0)
    if cs.no_c_store:
        if not all_nan(c):
            fails.append("no_c_store: C written")
    else:
        for z in range(cs.batch):
            cmp(f"C slice {z}", c[z, :M, :N], cs.ref[z], cs.bnd[z])
        if not all_nan(c[:, :, N:]):
            fails.append("ldc gap written")
        if not all_nan(c[:, rows:]):
            fails.append("rows past M (+ dup_rows) written")
        if cs.dup and not same_bits(c[:, M:rows, :N], c[:, :M, :N]):
            fails.append("dup_rows copy of C differs from its original")
    if "aux" in cs.outs:
        a = cs.outs["aux"]
        if not cs.no_c_store and not cs.out_operand:
            if not same_bits(a[:M, :N], op(c[0, :M, :N])):
                fails.append("aux is not the operand-type rounding of C")
        else:
            w, row = _excess(a[:M, :N], cs.ref[0], cs.bnd[0] + u_out() * cs.ref[0].abs())
            worst = max(worst, w)
            if row >= 0:
                fails.append(f"aux: row {row} off by {w:.3g} x its bound")
        if not all_nan(a[:, N:]) or not all_nan(a[rows:]):
            fails.append("aux gap / rows past M (+ dup_rows) written")
        if cs.dup and not same_bits(a[M:rows, :N], a[:M, :N]):
            fails.append("dup_rows copy of aux differs from its original")
    if "stats" in cs.outs:
        s = cs.outs["stats"]
        w, row = _excess(s[:M], cs.ref_st, cs.bnd_st)
        worst = max(worst, w)
        if row >= 0:
            fails.append(f"stats: row {row} off by {w:.3g} x its bound")
        if not all_nan(s[rows:]):
            fails.append("stats rows past M (+ dup_rows) written")
        if cs.dup and not same_bits(s[M:rows], s[:M]):
            fails.append("dup_rows copy of stats differs from its original")
    return fails, worst


# ------------------------------------------------------------------------------------------------------------------------------
# cross-attention scores (EPI_XS): LayerNorm fold with per-sample column sums / bias, one weight matrix per sample (w_rows), a
# softmax over the first sm_valid columns of every 32-column head group, operand-type probabilities
def xs(name, *, S, T, heads, Cd, valid, seed=0):
    cs = Case(name)
    M, HT, K = S * T, heads * 32, Cd
    slots = K // 64
    x = rnd((M, K), seed) * 1.5 + 0.5                 # non-zero row means: the mean term of the fold must cancel them
    Aq = op(x)
    s1, s2 = _slot_stats(x.double(), slots)
    stt = torch.stack([s1, s2], -1).float()
    Gq = op(rnd((S, HT, K), seed + 1) * (2.0 / K ** 0.5))
    csum = Gq.double().sum(-1).float()
    bb = rnd((S, HT), seed + 2) * 0.5
    bb.view(S, heads, 32)[..., valid:] = 1e4         # padding columns must not matter: not even to the row maximum
    sd1, sd2 = stt[..., 0].double().sum(1), stt[..., 1].double().sum(1)
    mean = sd1 / K
    var = sd2 / K - mean * mean
    rstd = (var + 1e-5).rsqrt()
    A64, G64 = Aq.double(), Gq.double()
    acc = torch.cat([A64[s * T:(s + 1) * T] @ G64[s].t() for s in range(S)])
    absacc = torch.cat([A64[s * T:(s + 1) * T].abs() @ G64[s].abs().t() for s in range(S)])
    smp = torch.arange(M) // T
    cm = mean[:, None] * csum.double()[smp]
    core = rstd[:, None] * (acc - cm)
    logit = core + bb.double()[smp]
    # fp32: accumulation, the fold's subtraction and scaling, rstd from the fp32 partials (cancellation s2/C - mean^2)
    dl = rstd[:, None] * (2 * K * U * absacc + 4 * U * (acc.abs() + cm.abs())) + 4 * U * logit.abs() + \
        16 * U * (sd2 / K / var)[:, None] * core.abs()
    lg = logit.view(M, heads, 32)
    p = torch.zeros_like(lg)
    p[..., :valid] = torch.softmax(lg[..., :valid], -1)
    dlm = dl.view(M, heads, 32)[..., :valid].amax(-1, keepdim=True)
    # softmax of perturbed logits moves p by at most p (e^{2 dl} - 1); exp / reciprocal approximations ~16 ulp; operand rounding
    pb = p * (torch.expm1(2 * dlm) + 16 * U + u_out()) + 2.0 ** -24
    cs.ref, cs.bnd = p.reshape(M, HT).cuda(), pb.reshape(M, HT).cuda()
    cs.valid, cs.heads, cs.M, cs.N = valid, heads, M, HT
    ldc = HT + 4
    cs.f.update(M=M, N=HT, K=K, A=cs.dev(Aq).data_ptr(), W=cs.dev(Gq).data_ptr(), out_operand=1, ldc=ldc,
                bias=cs.dev(bb).data_ptr(), ln_stats=cs.dev(stt).data_ptr(), ln_slots=slots, ln_C=K, ln_eps=1e-5,
                ln_cs=cs.dev(csum).data_ptr(), w_rows=T, w_bs=HT * K, sm_w=32, sm_valid=valid)
    cs.out("C", (M + 3, ldc), odt())
    cs.check = lambda sk: _check_xs(cs)
    return cs


def _check_xs(cs):
    fails = []
    M, HT, valid = cs.M, cs.N, cs.valid
    c = cs.outs["C"]
    got = c[:M, :HT]
    worst, row = _excess(got, cs.ref, cs.bnd)
    if row >= 0:
        fails.append(f"probabilities: row {row} off by {worst:.3g} x its bound")
    g = got.view(M, cs.heads, 32)
    if valid < 32 and not bool((bits(g[..., valid:].contiguous()) == 0).all()):
        fails.append("padding columns of a head group are not +0")
    tot = g.double().sum(-1)
    tb = cs.bnd.view(M, cs.heads, 32).sum(-1)
    if not bool(((tot - 1).abs() <= tb).all()):
        fails.append(f"a head group sums to {float(tot.flatten()[((tot - 1).abs() - tb).flatten().argmax()]):.6f}, not 1")
    if not all_nan(c[:, HT:]) or not all_nan(c[M:]):
        fails.append("ldc gap / rows past M written")
    return fails, worst


# ------------------------------------------------------------------------------------------------------------------------------
CASES = {
    # ResBlock conv1: FiLM bias per sample, rows_per_sample = H * W a power of two (shift path) / not one (divide path)
    "film_conv_rps1024": lambda: dense("film_conv_rps1024", conv=(2, 16, 64, 64), N=64, film=(1, 1024), seed=10),
    "film_conv_rps1008": lambda: dense("film_conv_rps1008", conv=(2, 16, 63, 64), N=64, film=(1, 1008), seed=11),
    "film_linear_rps32": lambda: dense("film_linear_rps32", M=96, N=128, K=1024, film=(1, 32), seed=12),
    # cond stage: positional embedding as a per-position row bias, T a power of two / not one
    "posemb_T32": lambda: dense("posemb_T32", M=3 * 32, N=192, K=512, film=(2, 32), seed=13),
    "posemb_T40": lambda: dense("posemb_T40", M=3 * 40, N=192, K=512, film=(2, 40), seed=14),
    # cross-attention scores st.xs: w_rows (= T) equal to and larger than the tiles' BM, 2 and 3 samples, several heads
    "xs_valid1": lambda: xs("xs_valid1", S=2, T=128, heads=4, Cd=192, valid=1, seed=20),
    "xs_valid17": lambda: xs("xs_valid17", S=3, T=128, heads=2, Cd=320, valid=17, seed=21),
    "xs_valid31": lambda: xs("xs_valid31", S=2, T=256, heads=6, Cd=128, valid=31, seed=22),
    "xs_valid32": lambda: xs("xs_valid32", S=3, T=64, heads=8, Cd=192, valid=32, seed=23),
    # st.xo: probabilities x (Wo V^T) per sample, residual, operand copy + statistics, no fp32 store
    "xo_no_c_store": lambda: dense("xo_no_c_store", M=2 * 128, N=192, K=128, S=2, res=True, aux=True, stats=True, no_c_store=True,
                                   seed=30),
    "xo_no_c_store_k256": lambda: dense("xo_no_c_store_k256", M=3 * 64, N=128, K=256, S=3, res=True, aux=True, stats=True,
                                        no_c_store=True, seed=31),
    # CFG prefix: st.attn1.out (residual, operand copy, statistics) and a ResBlock conv2 (residual, operand copy) stored twice
    "dup_linear": lambda: dense("dup_linear", M=192, N=320, K=320, res=True, aux=True, stats=True, dup=True, seed=40),
    "dup_conv": lambda: dense("dup_conv", conv=(2, 8, 16, 128), N=128, res=True, aux=True, dup=True, seed=41),
    # UNetModel.out conv: N = 4, NCHW with hw_out = 96 (no tile's multiple); under CFG the split-K reduce forms the guided eps
    "nchw_conv": lambda: dense("nchw_conv", conv=(2, 8, 12, 128), N=4, nchw=True, seed=50),
    "cfg_conv": lambda: dense("cfg_conv", conv=(4, 8, 12, 128), N=4, nchw=True, cfg=4.5, seed=51),
    # vae.qk: alpha = 1/sqrt(ch), batched slices
    "alpha_batch2": lambda: dense("alpha_batch2", M=80, N=80, K=128, batch=2, alpha=128 ** -0.5, bias=False, seed=60),
    "alpha_batch3": lambda: dense("alpha_batch3", M=64, N=64, K=256, batch=3, alpha=0.0625, bias=False, out_operand=1, seed=61),
    # long K: every split-K up to 32 (reduce kernels 8 .. 32).  K = 6144 is 96 K steps, split evenly by every factor, so the
    # last slab is never empty (with K = 4096 it is for 12 and 24); time-embedding SiLU, and the producer epilogue with dup_rows
    "longk_silu": lambda: dense("longk_silu", M=32, N=128, K=6144, act=1, seed=70),
    "longk_prod_dup": lambda: dense("longk_prod_dup", M=64, N=128, K=4096, res=True, aux=True, stats=True, dup=True, seed=71),
    # unaligned leading dimensions: scalar epilogue and the scalar split-K reduce, alpha + ReLU + operand copy
    "unaligned_any": lambda: dense("unaligned_any", M=100, N=96, K=1024, alpha=0.5, act=2, res=True, aux=True, ldc_pad=3, ld_pad=1,
                                   seed=80),
    # split-K producer of a GroupNorm: slabs left for the norm (defer_reduce), finished by it
    "defer_conv": lambda: dense("defer_conv", conv=(2, 16, 16, 256), N=128, res=True, defer=True, seed=90),
}


def _defer_check(cs, tile, sk, own_c):
    """The same GEMM with defer_reduce, its slabs finished by the GroupNorm that owns them: bit-equal to its own reduce (both add
    the slabs in slab order, then bias, then the residual)."""
    M, N = cs.M, cs.N
    slabs = torch.full((sk, M, N), NAN, device="cuda")
    d = cs.desc(tile, sk, 0, defer_reduce=1, slabs_out=slabs.data_ptr())
    cs.set_outs(d, sk)
    rc, msg = cs.launch(d)
    if rc:
        return [f"defer_reduce launch failed: {msg}"]
    fails = []
    if not all_nan(cs.outs["C"]):
        fails.append("defer_reduce: C written")
    cs.gn_x.fill_(NAN)
    f = cs.f
    rc = lib().df_test_groupnorm_own_slabs(C.c_void_p(cs.gn_x.data_ptr()), N, 2, M // 2, N, C.c_void_p(cs.gn_g.data_ptr()),
                                           C.c_void_p(cs.gn_b.data_ptr()), 1e-5, 1, C.c_void_p(cs.gn_out.data_ptr()),
                                           C.c_void_p(slabs.data_ptr()), sk, N, C.c_void_p(f["bias"]), C.c_void_p(f.get("res")),
                                           f.get("ldr", 0), stream())
    if rc:
        return fails + ["groupnorm_own_slabs: " + lib().df_last_error().decode()]
    if not same_bits(cs.gn_x, own_c):
        diff = (cs.gn_x - own_c).abs()
        fails.append(f"slabs finished by the GroupNorm differ from the GEMM's own reduce (max {float(diff.max()):.3g})")
    return fails


def _slices_check(cs, tile, sk, snap):
    """A batch-n launch equals n single-slice launches (pointers advanced by a_bs / w_bs / c_bs / res_bs)."""
    f = cs.f
    cs.poison()
    esz = cs.outs["C"].element_size()
    for z in range(cs.batch):
        over = dict(A=f["A"] + 2 * z * f["a_bs"], W=f["W"] + 2 * z * f["w_bs"])
        if f.get("res"):
            over["res"] = f["res"] + 4 * z * f["res_bs"]
        d = cs.desc(tile, sk, 0, batch=1, **over)
        d.C = cs.outs["C"].data_ptr() + esz * z * f["c_bs"]
        rc = lib().df_test_gemm_ex(C.byref(d), stream())
        if rc:
            return [f"slice {z}: " + lib().df_last_error().decode()]
    return [] if same_bits(cs.outs["C"], snap["C"]) else ["batch launch differs from its single-slice launches"]


def run_on_every_tuner_pair(case, cs):
    """The loop of this file and of tests/test_gemm_forms_gpu.py.  Every (tile, split-K) pair autotune_plan may launch for the case:
    its check (float64 reference within the per-element bound, untouched gaps stay NaN), gm walk orders and a repeated launch
    bit-identical, the batch / defer_reduce invariants; prints pairs run / refused and the worst error / bound.  -> that worst."""
    t0 = time.time()
    d = cs.desc(0, 1, 0)
    cs.set_outs(d, 1)
    pairs = tuner_pairs(d, cs.batch)
    assert pairs, f"{case}: the tuner has no pair for this GEMM"
    failures, refused, worst, ran = [], [], 0.0, 0
    for tile, sk in pairs:
        where = f"tile {tile} split-K {sk}"
        d = cs.desc(tile, sk, 0)
        cs.set_outs(d, sk)
        rc, msg = cs.launch(d)
        if rc:
            # launch_gemm refuses only what gemm_tile_valid refuses (one function decides both): a refused tuner pair is a failure too
            (refused if "launch_gemm refused" in msg else failures).append(f"{where}: {msg}")
            continue
        ran += 1
        fl, w = cs.check(sk)
        worst = max(worst, w)
        failures += [f"{where}: {m}" for m in fl]
        snap = {k: t.clone() for k, t in cs.outs.items()}
        for gm in (0,) + GMS:                      # gm 0 again: the same launch repeated
            d = cs.desc(tile, sk, gm)
            cs.set_outs(d, sk)
            rc, msg = cs.launch(d)
            if rc:
                failures.append(f"{where} gm {gm}: {msg}")
                continue
            for k, t in cs.outs.items():
                if not same_bits(t, snap[k]):
                    failures.append(f"{where}: gm {gm} changes the bits of {k}")
        if cs.batch > 1:
            failures += [f"{where}: {m}" for m in _slices_check(cs, tile, sk, snap)]
        if cs.defer and sk > 1:
            failures += [f"{where}: {m}" for m in _defer_check(cs, tile, sk, snap["C"][0, :cs.M, :cs.N].contiguous())]
    torch.cuda.synchronize()
    print(f"\n{case} [{PREC}]: {len(pairs)} tuner pairs, {ran} ran, {len(refused)} refused by launch_gemm, worst error / bound "
          f"{worst:.3f}, {time.time() - t0:.1f} s")
    assert not refused, f"{case}: launch_gemm refused {len(refused)} pair(s) the tuner would try:\n" + "\n".join(refused[:10])
    assert not failures, f"{case} [{PREC}]: {len(failures)} failure(s) over {ran} pairs:\n" + "\n".join(failures[:40])
    return worst


@pytest.mark.parametrize("case", list(CASES))
def test_epilogue_on_every_tuner_pair(case):
    """Every (tile, split-K) pair autotune_plan may launch for this epilogue: float64 reference within the per-element bound,
    untouched gaps stay NaN, gm walk orders and a repeated launch bit-identical, the batch / dup_rows / defer_reduce invariants."""
    run_on_every_tuner_pair(case, CASES[case]())
