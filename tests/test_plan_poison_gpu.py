"""GPU: no op of a plan may read what its plan did not write (Engine.debug_poison, df_debug_poison).

The ownership rule: an op may read only bytes written earlier in the same run by an op of its plan, or a pinned zeroed
block (Plan::alloc_zeroed).  With the hook on, a block fresh from the allocator holds 0xFF bytes (NaN as fp32 / bf16 / fp16) instead
of zeros, every block is filled with the pattern again right behind the last op in front of its release, and the split-K scratch is
filled in front of every split-K GEMM.  An op that relies on the build-time zeros, on a previous tenant's bytes, or on its own
buffer after the release then gives NaN instead of a number that is a little wrong.

Every plan family, both operand builds, the tiny configurations (synth.*_TINY), no tuner: the call runs once unpoisoned and twice
poisoned -- the second run starts from the first one's leftovers and its poison fills -- and both poisoned outputs must be finite
and BIT-equal to the unpoisoned one (same plan, same tiles, same fp32 summation order: equality is a condition, not a tolerance).
The family's oracle comparison is then repeated on the poisoned output at the tolerance of the family's own test file, so that
"equal" cannot mean "equally wrong":
  UNet forward 2e-2 / 3e-3 (bf16 / fp16: test_path_gpu.py FWD_TOL, test_path_fp16_gpu.py), guided forward and DDIM latents
  5e-2 / 1e-2 (TRAJ_TOL; the fp16 samplers' bound), VAE decode and encode 2e-2 / 3e-3, cond stage 5e-3 / 2e-3 (test_path_gpu.py,
  test_vae_cond_cavp_fuzz_gpu.py), classifier probability atol 2e-2 / 3e-3 and gradient 5e-2 / 1e-2, CAVP features 1.5e-2 / 2e-3
  (test_cavp_gpu.py).

Index-like blocks (content read as an integer, an index or a pointer; they would go through Plan::alloc_index and are never
poisoned): every Plan::alloc site of engine_builder.hip, engine_nets.hip, engine_cls_grad.hip, engine.hip and engine_test_api.hip
was read before the first poisoned run -- there are none.  Plan workspaces hold fp32, float2 statistics and operand-type values
only; the one table of pointers a plan owns (Plan::chk_list of df_debug_checksums) is a hipMalloc of its own outside
alloc / release, like Etab / ttab / E's table rows and the context's raw / packed weight buffers, which the hook leaves alone.

The hook's own self-test (df_test_poison_selftest): a four-op plan with a planted defect -- 1: an op reads a buffer that was
released two ops earlier and recycled; 2: an op reads the tail of its oversized recycled block that it never wrote -- is finite
(silently wrong) with the hook off and non-finite with it on; the correct plan equals the float64 value of its arithmetic either
way.  The split-K defect of the same family (a reduce that sums one slab more than the K slices wrote) is not planted: the launch
route derives the slab count of the reduce from the GEMM's own split-K, so no plan can ask for it."""
import functools

import pytest
import torch

from helpers import rel_l2, rnd, tiny_classifier_sd
import vae_encoder_ref as R

pytestmark = pytest.mark.gpu

FWD = {"bf16": 2e-2, "fp16": 3e-3}
TRAJ = {"bf16": 5e-2, "fp16": 1e-2}
COND = {"bf16": 5e-3, "fp16": 2e-3}
CLS_P = {"bf16": 2e-2, "fp16": 3e-3}
CLS_G = {"bf16": 5e-2, "fp16": 1e-2}
CAVP = {"bf16": 1.5e-2, "fp16": 2e-3}


@functools.lru_cache(maxsize=None)
def _sd():
    from diff_foley_amd import synth
    return synth.make_state_dict(synth.state_dict_spec(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY, with_encoder=True), 0)


def _sub(prefix):
    from oracle import unet as ou
    return ou.sub_state_dict(_sd(), prefix)


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def tiny(request):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    m = P.LatentDiffusion(precision=request.param, **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    missing, unexpected = m.load_state_dict(_sd())
    assert missing == [] and unexpected == []
    m.cuda()
    assert not m.engine.autotune_on
    return m


@pytest.fixture(scope="module")
def cls(tiny):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    c = P.AlignmentClassifier(classifier_config=dict(params=dict(synth.CLS_TINY)))
    c.load_state_dict(tiny_classifier_sd())
    c.attach(tiny)
    return c


def _poisoned(eng, call, what):
    """call() unpoisoned, then twice poisoned: finite and bit-equal.  Returns the second poisoned output (CPU)."""
    eng.debug_poison(False)
    want = [t.cpu() for t in call()]
    eng.debug_poison(True)
    try:
        runs = [[t.cpu() for t in call()] for _ in range(2)]
    finally:
        eng.debug_poison(False)
    for k, got in enumerate(runs):
        for i, (g, w) in enumerate(zip(got, want)):
            bad = int((~torch.isfinite(g)).sum())
            assert bad == 0, f"{what}: poisoned run {k + 1}, output {i}: {bad} of {g.numel()} values are not finite"
            assert torch.equal(g, w), f"{what}: poisoned run {k + 1}, output {i} differs from the unpoisoned run (rel-L2 {rel_l2(g, w):.3e})"
    return runs[1]


# ------------------------------------------------------------------------------------------- UNet
@functools.lru_cache(maxsize=None)
def _unet_case(B, W, T):
    from diff_foley_amd import synth
    from oracle import unet as ou
    x, c = rnd((B, 4, 16, W), 7000 + 10 * B + W), rnd((B, T, 128), 7100 + 10 * B + T)
    t = (torch.arange(B) * 311 + 37).float()
    return x, c, t, ou.unet_forward(_sub("model.diffusion_model."), synth.UNET_TINY, x, t, c)


@pytest.mark.parametrize("T", [32, 40])           # 32: the folded cross-attention operands; 40: the K / V^T form
@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_unet_forward(tiny, B, W, T):
    x, c, t, ref = _unet_case(B, W, T)
    eng = tiny.engine
    xd, cd, td = x.cuda(), c.cuda(), t.cuda()

    def call():
        eng.set_context(cd)
        return [eng.unet_forward(xd, td)]

    y, = _poisoned(eng, call, f"unet_forward B {B} 16x{W} T {T}")
    err = rel_l2(y, ref)
    print(f"poisoned unet_forward [{tiny.precision}] B {B} 16x{W} T {T}: rel-L2 {err:.3e}")
    assert err < FWD[tiny.precision]


@pytest.mark.parametrize("HW", [(8, 8), (8, 16)])
def test_unet_forward_one_and_two_token_maps(tiny, HW):
    """Beside the shapes above: latents whose deepest maps hold 1 or 2 tokens -- the LayerNorm kernel with separate K|Q and V^T GEMMs
    instead of the fused QKV form, V^T rows of 32 columns of which 1 or 2 are written."""
    from diff_foley_amd import synth
    from oracle import unet as ou
    x, c, t = rnd((2, 4) + HW, 7200 + HW[1]), rnd((2, 32, 128), 7201 + HW[1]), torch.tensor([500.0, 37.0])
    ref = ou.unet_forward(_sub("model.diffusion_model."), synth.UNET_TINY, x, t, c)
    eng = tiny.engine
    xd, cd, td = x.cuda(), c.cuda(), t.cuda()

    def call():
        eng.set_context(cd)
        return [eng.unet_forward(xd, td)]

    y, = _poisoned(eng, call, f"unet_forward {HW[0]}x{HW[1]}")
    err = rel_l2(y, ref)
    print(f"poisoned unet_forward [{tiny.precision}] {HW[0]}x{HW[1]}: rel-L2 {err:.3e}")
    assert err < FWD[tiny.precision]


def test_unet_forward_cfg(tiny):
    """B = 2, 16 x 32: the deduplicated CFG prefix (dup_rows) and the guided split-K reduce of out.conv."""
    from diff_foley_amd import synth
    from oracle import unet as ou
    B = 2
    x, c = rnd((B, 4, 16, 32), 7310), rnd((B, 32, 128), 7410)
    uc, t = torch.zeros_like(c), torch.tensor([961.0, 961.0])
    e2 = ou.unet_forward(_sub("model.diffusion_model."), synth.UNET_TINY, torch.cat([x, x]), torch.cat([t, t]), torch.cat([uc, c]))
    ref = e2[:B] + 4.5 * (e2[B:] - e2[:B])
    eng = tiny.engine
    xd, cd, td = x.cuda(), torch.cat([uc, c]).cuda(), t.cuda()

    def call():
        eng.set_context(cd)
        return [eng.unet_forward_cfg(xd, td, 4.5)]

    y, = _poisoned(eng, call, "unet_forward_cfg")
    err = rel_l2(y, ref)
    print(f"poisoned unet_forward_cfg [{tiny.precision}]: rel-L2 {err:.3e}")
    assert err < TRAJ[tiny.precision]


def test_hoisted_timestep_table_ddim(tiny):
    """4-step DDIM with CFG 4.5: set_context's [0, n_ctx), set_timesteps' [op_t0, op_tl) and the steps' [op_tl, end).  Four steps
    because three do not exist: the reference's uniform discretisation (util.py:48-57, range(0, 1000, 1000 // S) + 1, kept by the
    product and by the oracle) makes the timesteps 1, 334, 667, 1000 for S = 3, the last one outside the 1000-entry schedule -- it
    raises.  S = 4 is the smallest run of at least three steps that the reference can make."""
    from diff_foley_amd import synth
    from oracle import samplers as osamp, schedule as osch, unet as ou, vae as ov
    B = 2
    xT = synth.synthetic_xT(B, seed=23, shape=(4, 16, 32))
    feats = synth.synthetic_cavp(B, 32, synth.COND_TINY["origin_dim"], seed=1234)
    c_ref = ov.cond_stage(_sub("cond_stage_model."), feats)
    usd = _sub("model.diffusion_model.")
    z_ref, _ = osamp.ddim_sample(lambda x, tt, cc: ou.unet_forward(usd, synth.UNET_TINY, x, tt, cc), osch.ddpm_schedule()["alphas_cumprod"],
                                 4, xT, c_ref, scale=4.5, uc=torch.zeros_like(c_ref))
    c = c_ref.cuda()
    uc = torch.zeros_like(c)

    def call():
        z, _ = tiny.sample_log_diff_sampler(c, B, "DDIM", 4, unconditional_guidance_scale=4.5, unconditional_conditioning=uc,
                                            x_T=xT.clone().cuda())
        return [z]

    z, = _poisoned(tiny.engine, call, "4-step CFG DDIM")
    err = rel_l2(z, z_ref)
    print(f"poisoned 4-step CFG DDIM [{tiny.precision}]: latent rel-L2 {err:.3e}")
    assert err < TRAJ[tiny.precision]


# ------------------------------------------------------------------------------------------- VAE, cond stage
@pytest.mark.parametrize("B", [1, 17])          # 17: one above vae_chunk (16 for the tiny map): a 16-sample slice and the remainder plan
def test_vae_decode(tiny, B):
    from diff_foley_amd import synth
    from oracle import vae as ov
    z = rnd((B, 4, 8, 8), 7500 + B)
    ref = ov.decode_first_stage(_sub("first_stage_model."), synth.VAE_TINY, z)
    zd = z.cuda()
    d, = _poisoned(tiny.engine, lambda: [tiny.decode_first_stage(zd)], f"vae_decode B {B}")
    err = rel_l2(d, ref)
    print(f"poisoned vae_decode [{tiny.precision}] B {B}: rel-L2 {err:.3e}")
    assert err < FWD[tiny.precision]


@pytest.mark.parametrize("B", [1, 3])
def test_vae_encode(tiny, B):
    from diff_foley_amd import synth
    x = R.mel_like((B, 3, 32, 64), 7600 + B)
    ref = R.vae_encode(R.sub_state_dict(_sd()), synth.VAE_TINY, x)
    xd = x.cuda()
    m, = _poisoned(tiny.engine, lambda: [tiny.engine.vae_encode(xd)], f"vae_encode B {B}")
    err = rel_l2(m, ref)
    print(f"poisoned vae_encode [{tiny.precision}] B {B}: rel-L2 {err:.3e}")
    assert err < FWD[tiny.precision]


@pytest.mark.parametrize("T", [1, 32, 40])
def test_cond_encode(tiny, T):
    from oracle import vae as ov
    f = rnd((2, T, 64), 7700 + T)
    ref = ov.cond_stage(_sub("cond_stage_model."), f)
    fd = f.cuda()
    c, = _poisoned(tiny.engine, lambda: [tiny.engine.cond_encode(fd)], f"cond_encode T {T}")
    err = rel_l2(c, ref)
    print(f"poisoned cond_encode [{tiny.precision}] T {T}: rel-L2 {err:.3e}")
    assert err < COND[tiny.precision]


# ------------------------------------------------------------------------------------------- classifier
@functools.lru_cache(maxsize=None)
def _cls_case(T):
    from diff_foley_amd import synth
    from oracle import samplers as osamp, unet as ou
    csd = ou.sub_state_dict(tiny_classifier_sd(), "model.")
    x = rnd((2, 4, 16, 32), 7800 + T)
    vf = synth.synthetic_cavp(2, T, synth.CLS_TINY["context_dim"], seed=4321 + T)
    t = torch.tensor([500.0, 37.0])
    fwd = lambda xx, tt, cc: ou.classifier_forward(csd, synth.CLS_TINY, xx, tt, cc)      # noqa: E731
    return x, vf, t, fwd(x, t, vf).detach(), osamp.classifier_grad(fwd, x, t, vf)


@pytest.mark.parametrize("T", [8, 33])
def test_classifier_forward(tiny, cls, T):
    x, vf, t, p_ref, _ = _cls_case(T)
    xd, vd, td = x.cuda(), vf.cuda(), t.cuda()
    p, = _poisoned(tiny.engine, lambda: [tiny.engine.classifier_forward(xd, td, vd)], f"classifier_forward T {T}")
    print(f"poisoned classifier_forward [{tiny.precision}] T {T}: p {p.flatten().tolist()} ref {p_ref.flatten().tolist()}")
    assert torch.allclose(p, p_ref, atol=CLS_P[tiny.precision])


@pytest.mark.parametrize("T", [8, 33])
def test_classifier_grad_with_a_feature_token(tiny, cls, T):
    """The same feature tensor in every call: the second poisoned call carries the first one's token and runs [n_feat, end) only,
    on the K / V^T buffers the first call wrote -- they must not be among the released (re-poisoned) blocks."""
    x, vf, t, p_ref, g_ref = _cls_case(T)
    eng = tiny.engine
    xd, vd, td = x.cuda(), vf.cuda(), t.cuda()
    tokens = []

    def call():
        out = eng.classifier_grad(xd, td, vd, want_prob=True)
        tokens.append(eng._cls_feat[2])
        return list(out)

    g, p = _poisoned(eng, call, f"classifier_grad T {T}")
    assert tokens[0] != 0 and len(set(tokens)) == 1
    err = rel_l2(g, g_ref)
    print(f"poisoned classifier_grad [{tiny.precision}] T {T}: grad rel-L2 {err:.3e}")
    assert torch.allclose(p, p_ref, atol=CLS_P[tiny.precision])
    assert err < CLS_G[tiny.precision]


# ------------------------------------------------------------------------------------------- CAVP
@functools.lru_cache(maxsize=None)
def _cavp_case():
    from diff_foley_amd import synth
    from oracle import cavp as ocavp
    sd = synth.make_state_dict(synth.cavp_spec(synth.CAVP_TINY))
    v = synth.synthetic_video(2, 5, 64, seed=78)
    return sd, v, ocavp.encode_video(sd, v, stage_blocks=tuple(synth.CAVP_TINY["stage_blocks"]))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_cavp_encode(prec):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    sd, v, ref = _cavp_case()
    m = P.CAVPInference(embed_dim=synth.CAVP_TINY["embed_dim"], stage_blocks=synth.CAVP_TINY["stage_blocks"], precision=prec)
    m.load_state_dict(sd)
    m.cuda()
    vd = v.cuda()
    f, = _poisoned(m.engine, lambda: [m.encode_video(vd, normalize=True, pool=False)], "cavp_encode")
    err = rel_l2(f, ref)
    print(f"poisoned cavp_encode [{prec}]: rel-L2 {err:.3e}")
    assert err < CAVP[prec]


# ------------------------------------------------------------------------------------------- the hook itself
def test_hook_detects_planted_defects(tiny):
    eng = tiny.engine
    i = torch.arange(1024, dtype=torch.float64)
    x = ((i % 37) - 18) / 8
    want = (1.5 * x[:512] + 3.0 * x[512:]).float()        # every term and sum is exact in fp32: equality below
    out = {}
    for on in (False, True):
        eng.debug_poison(on)
        try:
            for defect in (0, 1, 2):
                out[on, defect] = eng.poison_selftest(defect).cpu()
        finally:
            eng.debug_poison(False)
    assert torch.equal(out[False, 0], want) and torch.equal(out[True, 0], want)
    for defect in (1, 2):
        off, on = out[False, defect], out[True, defect]
        assert torch.isfinite(off).all() and not torch.equal(off, want), f"defect {defect}: not silent with the hook off"
        assert not torch.isfinite(on).any(), f"defect {defect}: {int(torch.isfinite(on).sum())} of 512 outputs finite with the hook on"


def test_hook_and_tuner_refuse_each_other(tiny):
    eng = tiny.engine
    eng.autotune(True)
    try:
        with pytest.raises(RuntimeError, match="df_autotune is on"):
            eng.debug_poison(True)
    finally:
        eng.autotune(False)
    eng.debug_poison(True)
    try:
        with pytest.raises(RuntimeError, match="df_debug_poison is on"):
            eng.autotune(True)
    finally:
        eng.debug_poison(False)
