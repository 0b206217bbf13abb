"""GPU: first_stage_model.encode / encode_first_stage / get_first_stage_encoding through the facade, both operand builds.

Against the reference's own outputs (G13, tests/golden/make_golden_vae_encoder.py): the tiny moments with the hooked stages and the
seeded sample, and the full-size moments, by rel-L2 under the project's bounds for the same op families at the same depth (the VAE
decode bounds of DESIGN.md section 4): < 2e-2 with bf16 operands, < 3e-3 with fp16.  Then what a plan family owes its callers --
batch invariance, stream hand-over, no interference with the decoder -- and a configuration fuzz against tests/vae_encoder_ref.py."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLD, fuzz_seeds, gold, rel_l2, rnd
import vae_encoder_ref as R

pytestmark = pytest.mark.gpu

BOUND = {"bf16": 2e-2, "fp16": 3e-3}
TINY_SEED, FULL_SEED, SAMPLE_SEED = 131, 132, 5


def g13():
    return {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in np.load(os.path.join(GOLD, "g13_vae_encoder.npz")).items()}


def _model(prec, vae, seed=0):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    spec = synth.state_dict_spec(synth.UNET_TINY, vae, synth.COND_TINY, with_encoder=True)
    sd = synth.make_state_dict(spec, seed)
    m = P.LatentDiffusion(precision=prec, **P.stage2_config(synth.UNET_TINY, vae, synth.COND_TINY))
    missing, unexpected = m.load_state_dict(sd)
    assert missing == [] and unexpected == []
    m.cuda()
    return m, sd


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def tiny(request):
    from diff_foley_amd import synth
    m, _ = _model(request.param, synth.VAE_TINY)
    return m


@pytest.fixture(scope="module")
def x_tiny():
    return R.mel_like((2, 3, 32, 64), TINY_SEED)


def test_tiny_moments_and_hooked_stages_vs_reference(tiny, x_tiny):
    g, bound = g13(), BOUND[tiny.precision]
    post = tiny.encode_first_stage(x_tiny.cuda())
    assert tuple(post.parameters.shape) == (2, 8, 8, 16) and post.parameters.dtype == torch.float32
    errs = {"moments": rel_l2(post.parameters.cpu(), g["tiny_moments"])}
    for name, tap, hwc, sl in (("conv_in", 0, (32, 64, 64), (slice(1, 2), slice(None), slice(None, None, 2), slice(None, None, 2))),
                               ("down0", 1, (16, 32, 64), (slice(1, 2),)), ("down1", 2, (8, 16, 128), (slice(1, 2),)),
                               ("mid", 100, (8, 16, 128), (slice(1, 2),))):
        mom, stage = tiny.engine.vae_encode_tap(x_tiny.cuda(), tap, hwc)
        # a plan of its own: the copy op stands between a GEMM and the GroupNorm that otherwise takes over its split-K reduce, so the
        # tap plan may sum in another order than the product plan -- its moments are held to the same bound, not to the same bits
        errs[name + " (moments of the tap plan)"] = rel_l2(mom.cpu(), g["tiny_moments"])
        errs[name] = rel_l2(stage.cpu()[sl], g["tiny_" + name])
    print(f"vae encoder tiny [{tiny.precision}]: " + ", ".join(f"{k} rel-L2 {v:.2e}" for k, v in errs.items()))
    assert errs["conv_in"] < 1e-6                                # fp32 VALU conv of unrounded inputs
    assert all(v < bound for v in errs.values()), errs
    # the posterior's members (stage1_autoencoder/model.py:34-44)
    mean, logvar = torch.chunk(post.parameters, 2, dim=1)
    assert torch.equal(post.mean, mean) and torch.equal(post.mode(), mean) and post.deterministic is False
    assert torch.equal(post.logvar, logvar.clamp(-30.0, 20.0))
    assert torch.equal(post.std, torch.exp(0.5 * post.logvar)) and torch.equal(post.var, torch.exp(post.logvar))
    assert tuple(post.kl().shape) == (2,) and tuple(post.nll(post.mean).shape) == (2,)
    from diff_foley_amd import engine as E
    assert torch.equal(E.posterior_sample(post.parameters, None, 1.0), mean.contiguous()), "mode() is the mean, bit-exact"
    assert torch.equal(tiny.first_stage_model.encode(x_tiny.cuda()).parameters, post.parameters)


def test_seeded_first_stage_encoding_vs_reference(tiny, x_tiny):
    g = g13()
    torch.manual_seed(SAMPLE_SEED)
    z = tiny.get_first_stage_encoding(tiny.encode_first_stage(x_tiny.cuda()))
    want = float(tiny.scale_factor) * g["tiny_sample"]
    err = rel_l2(z.cpu(), want)
    print(f"vae encoder tiny sample [{tiny.precision}]: rel-L2 {err:.2e}")
    assert tuple(z.shape) == (2, 4, 8, 16) and err < BOUND[tiny.precision]
    # the same noise through sample(): torch.manual_seed gives the reference's draw
    torch.manual_seed(SAMPLE_SEED)
    z1 = tiny.encode_first_stage(x_tiny.cuda()).sample()
    assert rel_l2(z1.cpu(), g["tiny_sample"]) < BOUND[tiny.precision]
    # a tensor is scaled; anything else is refused like the reference does
    t = rnd((2, 4, 8, 16), 77).cuda()
    assert torch.equal(tiny.get_first_stage_encoding(t), torch.tensor(float(tiny.scale_factor), dtype=torch.float32).cuda() * t)
    with pytest.raises(NotImplementedError):
        tiny.get_first_stage_encoding((t,))


def test_batch_invariance_and_stream_handover(tiny):
    """Row 0 of B = 3 has the bits of B = 1: an encoder plan chooses every tile and split-K for the per-sample problem and takes no
    entry of the tune table, whose keys carry the row count (whatever other tests of the process left in that table)."""
    x = R.mel_like((3, 3, 32, 64), 141).cuda()
    m3 = tiny.encode_first_stage(x).parameters
    m1 = tiny.encode_first_stage(x[:1].contiguous()).parameters
    assert torch.equal(m3[:1], m1), f"row 0 of B = 3 differs from B = 1: rel-L2 {rel_l2(m3[:1].cpu(), m1.cpu()):.2e}"
    # two back-to-back calls on different torch streams give the single-stream bits (Engine._on("vaeenc") hands the plan over)
    xa, xb = x[:2].contiguous(), R.mel_like((2, 3, 32, 64), 142).cuda()
    wa, wb = tiny.encode_first_stage(xa).parameters.clone(), tiny.encode_first_stage(xb).parameters.clone()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ga = tiny.encode_first_stage(xa).parameters
    with torch.cuda.stream(s2):
        gb = tiny.encode_first_stage(xb).parameters
    torch.cuda.synchronize()
    assert torch.equal(ga, wa) and torch.equal(gb, wb)


def test_decoder_goldens_still_met_after_an_encode(tiny, x_tiny):
    g = gold("g3_tiny_unet.npz")
    tiny.encode_first_stage(x_tiny.cuda())
    y = tiny.decode_first_stage(rnd((2, 4, 16, 64), 103).cuda())
    err = rel_l2(y.cpu(), g["decode"])
    assert err < BOUND[tiny.precision], err
    # and the round trip has the right shapes: mel -> posterior mode -> mel
    z = tiny.get_first_stage_encoding(tiny.encode_first_stage(x_tiny.cuda()).mode())
    assert tuple(tiny.decode_first_stage(z).shape) == (2, 3, 32, 64)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_full_size_moments_vs_reference(prec):
    from diff_foley_amd import synth
    m, _ = _model(prec, synth.VAE_FULL)
    mom = m.encode_first_stage(R.mel_like((1, 3, 128, 512), FULL_SEED).cuda()).parameters
    err = rel_l2(mom.cpu(), g13()["full_moments"])
    print(f"vae encoder full size [{prec}]: moments rel-L2 {err:.2e}")
    assert tuple(mom.shape) == (1, 8, 16, 64) and err < BOUND[prec], err


def test_edge_inputs(tiny):
    p = tiny.encode_first_stage(torch.zeros(0, 3, 32, 64).cuda())
    assert tuple(p.parameters.shape) == (0, 8, 8, 16) and tuple(p.mean.shape) == (0, 4, 8, 16)
    assert tuple(p.sample().shape) == (0, 4, 8, 16) and tuple(tiny.get_first_stage_encoding(p).shape) == (0, 4, 8, 16)
    for bad, what in ((torch.zeros(3, 32, 64), "4-D"), (torch.zeros(1, 2, 32, 64), "channels"), (torch.zeros(1, 3, 30, 64), "multiple"),
                      (torch.zeros(1, 3, 32, 66), "multiple")):
        with pytest.raises((ValueError, RuntimeError), match=what):
            tiny.encode_first_stage(bad.cuda())


# --------------------------------------------------------------------------------------------------------- configuration fuzz
# Which draws are admissible.  GroupNorm(32 groups) on a small map normalises a handful of values per group -- on the 1 x 1 latent of an
# f x f image with ch = 64 it is PAIRS of channels, i.e. sign(a - b) / sqrt(1 + eps / var): discontinuous where a ~ b.  Such a case is not
# a statement about any implementation: the fp32 reference ITSELF moves by O(1) when nothing but its conv weights are rounded to the
# operand type (seed 5's first draw: rel-L2 0.80 with bf16 weights, 3e-4 with fp16 weights; seed 1's 1 x 1 latent: 1.8e-3).  So a draw is
# judged by the reference alone, before the engine is asked anything: the restatement with its matmul weights rounded to bf16 (the
# coarser operand type; one case set for both builds) must stay within HALF the bf16 bound of the fp32 restatement -- every product of
# the network rounds two operands with the same unit round-off, its weight and its activation, so an implementation's error is about
# sqrt(2) times the weights-only figure, and a reference that spends more than half the bound on its weights alone leaves none for
# the activations.  A draw that does not is replaced by the next draw of the same seed (same rule, attempt + 1); f x f stays f x f.
_COND_LIMIT = BOUND["bf16"] / 2


def _draw(seed, attempt=0):
    r = np.random.default_rng(6500 + seed + 1000 * attempt)
    mults = ([1], [1, 2], [1, 1], [1, 2, 2], [1, 2, 4], [1, 1, 2, 2], [1, 2, 4, 4])
    cfg = dict(ch=int(r.choice([64, 128])), ch_mult=list(mults[int(r.integers(0, len(mults)))]), num_res_blocks=int(r.choice([1, 2])),
               in_channels=int(r.integers(1, 4)), z_channels=int(r.integers(1, 9)), out_ch=3)
    cfg["embed_dim"] = cfg["z_channels"]
    f = 2 ** (len(cfg["ch_mult"]) - 1)
    if seed % 4 == 1:
        H = W = f                                            # an f x f image: a 1 x 1 latent
    else:
        H, W = f * int(r.integers(1, 32 // f + 1)), f * int(r.integers(1, 96 // f + 1))
    return cfg, int(r.integers(1, 4)), H, W


_cases = {}


def _case(seed):
    """(cfg, state dict, x, fp32 reference moments, conditioning figure) of the first admissible draw of ``seed``."""
    from diff_foley_amd import synth
    if seed not in _cases:
        for attempt in range(16):
            cfg, B, H, W = _draw(seed, attempt)
            sd = synth.make_state_dict(synth.state_dict_spec(synth.UNET_TINY, cfg, synth.COND_TINY, with_encoder=True), 900 + seed)
            sub = R.sub_state_dict(sd)
            x = R.mel_like((B, cfg["in_channels"], H, W), 1000 + seed)
            ref = R.vae_encode(sub, cfg, x)
            rounded = {k: (v.to(torch.bfloat16).float() if v.ndim >= 2 and "conv_in" not in k and "quant_conv" not in k else v)
                       for k, v in sub.items()}                    # conv_in and quant_conv run in fp32 in every build
            cond = rel_l2(R.vae_encode(rounded, cfg, x), ref)
            if cond < _COND_LIMIT:
                _cases[seed] = (cfg, sd, x, ref, cond, attempt)
                break
        else:
            raise AssertionError(f"seed {seed}: no admissible draw in 16 attempts")
    return _cases[seed]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("seed", fuzz_seeds(8))
def test_encoder_configuration_fuzz_vs_restatement(seed, prec):
    import diff_foley_amd as P
    from diff_foley_amd import synth
    cfg, sd, x, ref, cond, attempt = _case(seed)
    B, _, H, W = x.shape
    m = P.LatentDiffusion(precision=prec, **P.stage2_config(synth.UNET_TINY, cfg, synth.COND_TINY))
    assert m.load_state_dict(sd) == ([], [])
    m.cuda()
    got = m.encode_first_stage(x.cuda()).parameters.cpu()
    f = 2 ** (len(cfg["ch_mult"]) - 1)
    assert got.shape == ref.shape == (B, 2 * cfg["z_channels"], H // f, W // f) and bool(torch.isfinite(got).all()), (cfg, B, H, W)
    err = rel_l2(got, ref)
    print(f"vae encoder case {seed} (draw {attempt}, reference with bf16 weights {cond:.1e}) [{prec}]: {cfg} B {B} {H}x{W} -> rel-L2 {err:.2e}")
    assert err < BOUND[prec], (cfg, B, H, W, err)
