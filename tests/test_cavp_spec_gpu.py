"""GPU: the CAVP spectrogram tower (CAVPInference.encode_spec -> df_cavp_spec_encode) and the audio / video similarity.

(i)   The full-width model against golden G15, the reference's own Cnn14 (tests/golden/make_golden_cavp_spec.py): features raw,
      normalised and pooled, the 72-frame clip whose fourth pool floors, and the hooked ConvBlocks through the plan's tap.
(ii)  Each kernel of csrc/cavp_spec.hip alone, element by element against float64, outputs pre-filled with a sentinel and padded
      leading dimensions.  Bounds (derived, none measured): a result stored in the operand type is the fp32 value rounded to nearest,
      |want| * u with u = 2^-8 (bf16) / 2^-11 (fp16), + 2^-24 absolute for fp16's subnormal steps; the fp32 value itself is off by
      at most n * 2^-24 * (sum of the magnitudes of its terms), n = the number of roundings on its longest chain, stated per kernel.
(iii) The tiny-width model against the float64 restatement (tests/cavp_spec_ref.py, pinned to G15 by test_cavp_spec_cpu.py): batch
      independence to the bit, two streams, no interference with the video tower.
(iv)  alignment_scores and the edge inputs.

Bounds of (i) and (iii): TOL / COS of tests/test_cavp_gpu.py, the bounds of this op family (BN-folded conv + ReLU chains)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import cavp_spec_ref as R
import diff_foley_amd as P
from diff_foley_amd import engine as E, synth
from helpers import gold, rel_l2
from test_cavp_gpu import COS, TOL

pytestmark = pytest.mark.gpu

SEED_64, SEED_72, SEED_256 = 151, 152, 153          # make_golden_cavp_spec.py
PRECS = ["bf16", "fp16"]
U_OP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
F32 = 2.0 ** -24
TINY_V, TINY_A = synth.CAVP_TINY, synth.CAVP_AUDIO_TINY


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _check(f, ref, prec, what):
    f, ref = f.detach().cpu(), ref.detach().cpu()
    assert f.shape == ref.shape, (what, f.shape, ref.shape)
    err = rel_l2(f, ref)
    cos = F.cosine_similarity(f.double(), ref.double(), dim=-1).min().item()
    print(f"cavp spec {what} [{prec}]: rel-L2 {err:.3e}  min cos {cos:.6f}")
    assert torch.isfinite(f).all()
    assert err < TOL[prec] and cos > COS[prec], (what, err, cos)


# ------------------------------------------------------------------------------------------------ (i) full width against G15
_full_sd = {}


def _full_state():
    if not _full_sd:
        _full_sd.update(synth.make_state_dict(synth.cavp_audio_spec(synth.CAVP_AUDIO_FULL)))
        _full_sd.update(synth.make_state_dict(synth.cavp_spec({**TINY_V, "embed_dim": 512})))      # a shallow video tower: not run here
    return _full_sd


@pytest.fixture(scope="module", params=PRECS)
def full_model(request):
    m = P.CAVPInference(embed_dim=512, stage_blocks=TINY_V["stage_blocks"], precision=request.param)
    missing, unexpected = m.load_state_dict(_full_state())
    assert not missing and not unexpected
    return m.cuda(), request.param


def test_full_width_features_vs_golden(full_model):
    m, prec = full_model
    g = gold("g15_cavp_spec.npz")
    mel = synth.synthetic_mel(2, 64, 128, SEED_64).cuda()
    _check(m.encode_spec(mel, normalize=False, pool=False), g["f64_raw"], prec, "full 64 frames raw")
    fn = m.encode_spec(mel, normalize=True, pool=False)
    assert torch.allclose(fn.norm(dim=-1).cpu(), torch.ones(2, 4), atol=1e-4)
    _check(fn, g["f64_norm"], prec, "full 64 frames normalised")
    _check(m.encode_spec(synth.synthetic_mel(1, 72, 128, SEED_72).cuda(), normalize=False, pool=False), g["f72_raw"], prec,
           "full 72 frames raw (floored pool)")
    mel = synth.synthetic_mel(2, 256, 128, SEED_256).cuda()
    _check(m.encode_spec(mel, normalize=False, pool=True), g["f256_pool"], prec, "full 256 frames pooled")
    _check(m.encode_spec(mel, normalize=True, pool=True), g["f256_pool_norm"], prec, "full 256 frames pooled normalised")


@pytest.mark.parametrize("tap, key", [(1, "f64_block1"), (4, "f64_block4"), (6, "f64_block6")])
def test_full_width_hooked_blocks_vs_golden(full_model, tap, key):
    m, prec = full_model
    g = gold("g15_cavp_spec.npz")
    mel = synth.synthetic_mel(2, 64, 128, SEED_64).cuda()
    feat, stage = m.engine.cavp_spec_encode_tap(mel, tap)
    stage = stage[1].cpu()                                   # clip 1, (C, t, mel)
    stage = {1: stage[:, ::2, ::2], 4: stage, 6: stage[::2]}[tap]
    ref = g[key]
    assert stage.shape == ref.shape
    err = rel_l2(stage, ref)
    print(f"cavp spec conv_block{tap} [{prec}]: rel-L2 {err:.3e}")
    assert err < TOL[prec], (tap, err)
    _check(feat, g["f64_raw"], prec, f"full 64 frames raw (tap {tap} plan)")


# ------------------------------------------------------------------------------------------------ (ii) the kernels alone
def _op(prec):
    return E.OPERAND_DTYPE[prec]


def _sentinel(shape, dtype):
    """0xFFFF bit patterns (a NaN as bf16 and fp16) / NaN: an element the kernel leaves out is seen."""
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), device=_dev())
    return torch.full(shape, -1, dtype=torch.int16, device=_dev()).view(dtype)


def _judge(got, want, mag, n_round, prec, what, exact_op=True):
    """|got - want| <= u |want| + n 2^-24 mag (+ 2^-24): see the module docstring.  got, want, mag: float64 CPU tensors."""
    u = U_OP[prec] if exact_op else 0.0
    bound = u * want.abs() + n_round * F32 * mag + (F32 if exact_op else 0.0)
    bad = (got - want).abs() > bound
    used = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    print(f"{what} [{prec}]: worst share of the bound {used:.3f}")
    assert not bool(bad.any()), (what, int(bad.sum()), used)


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T, NM, shift", [(16, 8, 0.05), (17, 128, 0.05), (33, 24, 0.05), (33, 24, 10.0)])
def test_spec_conv_in_kernel(prec, T, NM, shift):
    """Border rows and columns, odd sizes, more than one tile in both axes (tiles are 32 frames x 8 mels), the input BN applied before
    the zero padding: with the BN bias at 10 a border tap that read the shift instead of 0 would be off by ~10 |w|.
    Roundings on the longest chain: 5 for the normalised input, 4 for the folded weight and bias, 9 + 1 accumulations: n = 20."""
    L = E.lib(prec)
    B, C1, ldo = 2, 64, 72
    g = torch.Generator().manual_seed(7 * T + NM)
    spec = torch.rand(B, NM, T, generator=g)
    bn0 = [1 + 0.2 * torch.rand(NM, generator=g), shift * (2 * torch.rand(NM, generator=g) - 1) + (shift if shift > 1 else 0.0),
           0.4 + 0.2 * torch.rand(NM, generator=g), 0.5 + torch.rand(NM, generator=g)]
    w = (2 * torch.rand(C1, 1, 3, 3, generator=g) - 1) * 0.8
    bn1 = [1 + 0.2 * torch.rand(C1, generator=g), 0.2 * (2 * torch.rand(C1, generator=g) - 1), 0.1 * torch.rand(C1, generator=g),
           0.5 + torch.rand(C1, generator=g)]
    d = [t.to(_dev()) for t in [spec] + bn0 + [w] + bn1]
    out = _sentinel((B, T, NM, ldo), _op(prec))
    E._chk(L.df_test_spec_conv_in(d[0].data_ptr(), _ptrs(d[1:5]), d[5].data_ptr(), _ptrs(d[6:10]), 1e-5, out.data_ptr(), ldo, B, NM, T,
                                  C1, None), L)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[..., C1:].view(torch.int16) == -1).all()), "pad columns written"
    # float64: BN over the mel axis BEFORE the padding, conv, folded bn1, ReLU; and the magnitudes of the terms
    f8 = lambda t: t.double()
    sc0 = f8(bn0[0]) / torch.sqrt(f8(bn0[3]) + 1e-5)
    x = f8(spec).permute(0, 2, 1).unsqueeze(1)                                      # (B, 1, T, NM)
    xn = (x - f8(bn0[2])) * sc0 + f8(bn0[1])
    xmag = (x - f8(bn0[2])).abs() * sc0.abs() + f8(bn0[1]).abs()
    sc1 = (f8(bn1[0]) / torch.sqrt(f8(bn1[3]) + 1e-5)).view(1, C1, 1, 1)
    b1 = f8(bn1[1]).view(1, C1, 1, 1) - f8(bn1[2]).view(1, C1, 1, 1) * sc1
    pre = F.conv2d(xn, f8(w), padding=1) * sc1 + b1
    mag = F.conv2d(xmag, f8(w).abs(), padding=1) * sc1.abs() + f8(bn1[1]).abs().view(1, C1, 1, 1) + (f8(bn1[2]).view(1, C1, 1, 1) * sc1).abs()
    want = F.relu(pre).permute(0, 2, 3, 1)                                          # (B, T, NM, C1)
    _judge(out[..., :C1].double(), want, mag.permute(0, 2, 3, 1), 20, prec, f"spec_conv_in T {T} mels {NM} shift {shift}")
    if shift > 1:     # the folded form (BN shift seen by the border taps) is far outside the bound: the test would see it
        folded = F.relu(F.conv2d(F.pad(xn, (1, 1, 1, 1), value=float(f8(bn0[1]).mean())), f8(w)) * sc1 + b1).permute(0, 2, 3, 1)
        assert float((folded - want).abs().max()) > 1.0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ph, pw", [(2, 2), (1, 2)])
@pytest.mark.parametrize("H, W", [(2, 2), (3, 5), (9, 4)])
def test_avgpool_nhwc_kernel(prec, H, W, ph, pw):
    """Floor semantics on odd maps, both pool shapes.  ph * pw - 1 additions and one exact scaling by a power of two: n = 3."""
    L = E.lib(prec)
    B, Cc, ldx, ldo = 2, 24, 28, 32
    g = torch.Generator().manual_seed(100 * H + 10 * W + ph)
    x = torch.randn(B, H, W, ldx, generator=g)
    out = _sentinel((B, H // ph, W // pw, ldo), _op(prec))
    xd = x.to(_dev())
    E._chk(L.df_test_avgpool_nhwc(xd.data_ptr(), ldx, out.data_ptr(), ldo, B, H, W, Cc, ph, pw, None), L)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[..., Cc:].view(torch.int16) == -1).all()), "pad columns written"
    x8 = x[..., :Cc].double().permute(0, 3, 1, 2)
    want = F.avg_pool2d(x8, (ph, pw)).permute(0, 2, 3, 1)
    mag = F.avg_pool2d(x8.abs(), (ph, pw)).permute(0, 2, 3, 1)
    assert want.shape == out[..., :Cc].shape
    _judge(out[..., :Cc].double(), want, mag, 3, prec, f"avgpool_nhwc {H}x{W} ({ph},{pw})")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_spec_head_pool_kernel(prec, T, W):
    """Two clips: a frame's neighbours stay inside its clip; max pads with -inf, the average with zeros and always divides by 3.
    W - 1 additions and a division for a mean, two additions, a division and the final addition: n = W + 4."""
    L = E.lib(prec)
    B, Cc, ldx, ldo = 2, 20, 24, 28
    g = torch.Generator().manual_seed(10 * T + W)
    x = torch.randn(B, T, W, ldx, generator=g) - 1.0          # mostly negative: a zero-padded max would show
    out = _sentinel((B * T, ldo), _op(prec))
    xd = x.to(_dev())
    E._chk(L.df_test_spec_head_pool(xd.data_ptr(), ldx, out.data_ptr(), ldo, B, T, W, Cc, None), L)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[:, Cc:].view(torch.int16) == -1).all()), "pad columns written"
    m = x[..., :Cc].double().mean(dim=2).permute(0, 2, 1)                         # (B, C, T)
    ma = x[..., :Cc].double().abs().mean(dim=2).permute(0, 2, 1)
    want = (F.max_pool1d(m, 3, 1, 1) + F.avg_pool1d(m, 3, 1, 1)).permute(0, 2, 1).reshape(B * T, Cc)
    mag = (F.max_pool1d(ma, 3, 1, 1) + F.avg_pool1d(ma, 3, 1, 1)).permute(0, 2, 1).reshape(B * T, Cc)
    _judge(out[:, :Cc].double(), want, mag, W + 4, prec, f"spec_head_pool T' {T} W {W}")


@pytest.mark.parametrize("Bv, Bs, T, D", [(1, 1, 1, 64), (2, 3, 5, 512), (1, 8, 32, 512)])
def test_cavp_similarity_kernel(Bv, Bs, T, D):
    """fp32 in and out.  A lane's chain is ceil(T / 4) frames x ceil(D / 256) steps x 4 fused multiply-adds; then 6 levels of the wavefront
    reduction, 4 wavefront totals, the scale / T factor and its product: n = chain + 12."""
    L = E.lib()
    g = torch.Generator().manual_seed(T * D + Bs)
    v, s = torch.randn(Bv, T, D, generator=g), torch.randn(Bs, T, D, generator=g)
    scale = 14.2857
    out = _sentinel((Bv, Bs), torch.float32)
    vd, sdv = v.to(_dev()), s.to(_dev())
    E._chk(L.df_cavp_similarity(vd.data_ptr(), sdv.data_ptr(), out.data_ptr(), Bv, Bs, T, D, scale, None), L)
    torch.cuda.synchronize()
    want = R.similarity(v, s, scale)
    mag = scale * torch.einsum("itd,jtd->ij", v.double().abs(), s.double().abs()) / T
    n = -(-T // 4) * -(-D // 256) * 4 + 12
    _judge(out.cpu().double(), want, mag, n, "fp32", f"cavp_similarity {Bv}x{Bs}x{T}x{D}", exact_op=False)


# ------------------------------------------------------------------------------------------------ (iii) tiny width vs the restatement
_tiny_sd = {}


def _tiny_state():
    if not _tiny_sd:
        _tiny_sd.update(synth.make_state_dict(synth.cavp_spec(TINY_V)))
        _tiny_sd.update(synth.make_state_dict(synth.cavp_audio_spec(TINY_A)))
    return _tiny_sd


def _tiny_model(prec, with_tower=True):
    m = P.CAVPInference(embed_dim=TINY_A["embed_dim"], stage_blocks=TINY_V["stage_blocks"], spec_channels=TINY_A["channels"],
                        spec_fc_dim=TINY_A["fc_dim"], spec_n_mels=TINY_A["n_mels"], precision=prec)
    sd = _tiny_state()
    if not with_tower:
        sd = {k: v for k, v in sd.items() if k != "spec_encoder.fc1.bias"}
    missing, unexpected = m.load_state_dict(sd)
    assert not missing and bool(unexpected) == (not with_tower)
    return m.cuda()


@pytest.fixture(scope="module", params=PRECS)
def tiny_model(request):
    return _tiny_model(request.param), request.param


@pytest.mark.parametrize("T", [16, 40, 72])
def test_tiny_vs_restatement_and_batch_independence(tiny_model, T):
    m, prec = tiny_model
    mel = synth.synthetic_mel(3, T, TINY_A["n_mels"], seed=200 + T)
    for norm in (False, True):
        ref = R.encode_spec(_tiny_state(), mel, normalize=norm, pool=False)
        f3 = m.encode_spec(mel.cuda(), normalize=norm, pool=False)
        assert f3.shape == (3, R.out_rows(T), TINY_A["embed_dim"])
        _check(f3, ref, prec, f"tiny 3 x {T} frames normalize={norm}")
        f1 = m.encode_spec(mel[:1].cuda(), normalize=norm, pool=False)
        assert torch.equal(f1[0], f3[0]), "a clip's features depend on its batch-mates"


def test_tiny_batch_beyond_one_slice(tiny_model):
    """df_cavp_spec_encode runs more than 16 clips as slices: the clips of the second slice have the bits they have on their own."""
    m, prec = tiny_model
    mel = synth.synthetic_mel(18, 16, TINY_A["n_mels"], seed=77).cuda()
    f18 = m.encode_spec(mel, normalize=True, pool=False)
    assert f18.shape == (18, 1, TINY_A["embed_dim"]) and bool(torch.isfinite(f18).all())
    assert torch.equal(f18[16:], m.encode_spec(mel[16:], normalize=True, pool=False))
    assert torch.equal(f18[:1], m.encode_spec(mel[:1], normalize=True, pool=False))


def test_tiny_two_streams_give_the_single_stream_bits(tiny_model):
    m, prec = tiny_model
    mels = [synth.synthetic_mel(2, 40, TINY_A["n_mels"], seed=s).cuda() for s in (301, 302)]
    want = [m.encode_spec(x, normalize=True, pool=False).clone() for x in mels]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for x, st in zip(mels, streams):
        with torch.cuda.stream(st):
            got.append(m.encode_spec(x, normalize=True, pool=False))
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_tiny_video_tower_is_undisturbed(tiny_model):
    m, prec = tiny_model
    v = synth.synthetic_video(1, 4, 64, seed=77).cuda()
    before = m.encode_video(v, normalize=True, pool=False).clone()
    m.encode_spec(synth.synthetic_mel(2, 40, TINY_A["n_mels"], seed=5).cuda(), normalize=True, pool=False)
    after = m.encode_video(v, normalize=True, pool=False)
    assert torch.equal(before, after)


def test_tiny_pooled_and_forward(tiny_model):
    m, prec = tiny_model
    mel = synth.synthetic_mel(2, 256, TINY_A["n_mels"], seed=41)
    for norm in (False, True):
        _check(m.encode_spec(mel.cuda(), normalize=norm), R.encode_spec(_tiny_state(), mel, normalize=norm, pool=True), prec,
               f"tiny pooled normalize={norm}")
    raw = m.encode_spec(synth.synthetic_mel(1, 512, TINY_A["n_mels"], seed=42).cuda(), normalize=False, pool=True)
    assert raw.shape == (1, TINY_A["embed_dim"], 2)                      # two windows: the reference's (B, C, T' / 16) layout
    with pytest.raises(NotImplementedError):
        m.encode_spec(synth.synthetic_mel(1, 512, TINY_A["n_mels"], seed=42).cuda(), normalize=True, pool=True)
    with pytest.raises(RuntimeError, match="fewer than"):
        m.encode_spec(mel[:, :, :128].cuda(), normalize=False, pool=True)
    video = synth.synthetic_video(2, 16, 64, seed=3).cuda()
    out = m.forward(video, mel.cuda())
    assert set(out) == {"video_features", "spec_features", "logit_scale"}
    assert out["video_features"].shape == out["spec_features"].shape == (2, TINY_A["embed_dim"])
    assert float(out["logit_scale"]) == pytest.approx(float(_tiny_state()["logit_scale"].exp()), rel=1e-6)
    tup = m.forward(video, mel.cuda(), output_dict=False)
    assert torch.equal(tup[1], out["spec_features"]) and torch.equal(tup[0], out["video_features"])


# ------------------------------------------------------------------------------------------------ (iv) scores and edge inputs
def _candidates():
    """Four mels whose restatement scores against the direction below lie 0.1 or more apart: a smooth field, the lower half of the
    bands on, one loud frame in sixteen, silence."""
    nm = TINY_A["n_mels"]
    base = synth.synthetic_mel(1, 256, nm, seed=31)[0]
    halves = torch.zeros(nm, 256)
    halves[: nm // 2] = 1.0
    ticks = torch.zeros(nm, 256)
    ticks[:, ::16] = 1.0
    return torch.stack([ticks, base, torch.zeros(nm, 256), halves])


def test_alignment_scores(tiny_model):
    m, prec = tiny_model
    cands = _candidates()
    ref_f = R.encode_spec(_tiny_state(), cands, normalize=True, pool=False)            # (4, 16, D) float64
    video = F.normalize(ref_f[1:2] - ref_f[2:3], dim=-1).float()                         # unit rows: from silence towards the smooth field
    want = R.similarity(video, ref_f)
    # |score error| <= mean_t |v_t| |ds_t| <= rel-L2 of the normalised features (unit rows, Cauchy-Schwarz) < TOL: the ranking of
    # candidates whose scores are more than 2 TOL apart is decided
    gaps = want[0].sort().values.diff()
    assert float(gaps.min()) > 2 * TOL[prec], gaps
    scores = m.alignment_scores(video.cuda(), cands.cuda())
    assert scores.shape == (1, 4)
    print(f"alignment scores [{prec}]: {scores.cpu().tolist()} restatement {want.tolist()}")
    assert float((scores.cpu().double() - want).abs().max()) < TOL[prec]
    assert scores.argsort(dim=1).cpu().tolist() == want.argsort(dim=1).tolist()
    assert int(scores.argmax()) == 1
    # features in place of mels, and torch's own einsum on the same device features
    sf = m.encode_spec(cands.cuda(), normalize=True, pool=False)
    again = m.alignment_scores(video.cuda(), sf)
    assert torch.equal(again, scores)
    ein = torch.einsum("itd,jtd->ij", video.cuda(), sf) / sf.shape[1]
    assert float((scores - ein).abs().max()) < 1e-6
    two = torch.cat([video, -video]).cuda()
    s2 = m.alignment_scores(two, sf)
    assert s2.shape == (2, 4) and torch.equal(s2[0], scores[0]) and torch.equal(s2[1], -scores[0])
    with pytest.raises(RuntimeError, match="frames"):
        m.alignment_scores(video[:, :15].cuda(), cands.cuda())
    with pytest.raises(RuntimeError, match="frames"):
        m.alignment_scores(video.cuda(), sf[:, :8])


def test_edge_inputs(tiny_model):
    m, prec = tiny_model
    nm, emb = TINY_A["n_mels"], TINY_A["embed_dim"]
    with pytest.raises(RuntimeError, match="no output row"):
        m.encode_spec(torch.zeros(1, nm, 15).cuda(), pool=False)
    with pytest.raises(RuntimeError, match="mel bins"):
        m.encode_spec(torch.zeros(1, nm + 8, 32).cuda(), pool=False)
    with pytest.raises(RuntimeError, match="must be"):
        m.encode_spec(torch.zeros(nm, 32).cuda(), pool=False)
    empty = m.encode_spec(torch.zeros(0, nm, 40).cuda(), normalize=True, pool=False)
    assert empty.shape == (0, 2, emb) and empty.is_cuda
    # the C ABI refuses what the facade answers or rejects: no frames for a row, another mel height, an empty batch
    L, h = m.engine.L, m.engine._h
    x, o = torch.zeros(1, nm, 64).cuda(), torch.zeros(1, 4, emb).cuda()
    for B, M, T, word in ((1, nm, 15, b"no output row"), (1, nm + 8, 32, b"configured for"), (0, nm, 32, b"empty input")):
        assert L.df_cavp_spec_encode(h, x.data_ptr(), o.data_ptr(), B, M, T, 0, None) != 0
        assert word in L.df_last_error(), L.df_last_error()
    assert L.df_cavp_similarity(x.data_ptr(), x.data_ptr(), o.data_ptr(), 0, 1, 4, 64, 1.0, None) != 0
    assert L.df_cavp_similarity(x.data_ptr(), x.data_ptr(), o.data_ptr(), 1, 1, 4, 6, 1.0, None) != 0
    assert float(o.abs().max()) == 0.0


@pytest.mark.parametrize("prec", PRECS)
def test_model_without_the_tower_refuses(prec):
    m = _tiny_model(prec, with_tower=False)
    with pytest.raises(NotImplementedError, match="spec_encoder.fc1.bias"):
        m.encode_spec(torch.zeros(1, TINY_A["n_mels"], 32).cuda(), pool=False)
    with pytest.raises(NotImplementedError):
        m.forward(synth.synthetic_video(1, 16, 64, seed=3).cuda(), torch.zeros(1, TINY_A["n_mels"], 256).cuda())
    v = synth.synthetic_video(1, 4, 64, seed=77).cuda()
    assert m.encode_video(v, normalize=True, pool=False).shape == (1, 4, TINY_V["embed_dim"])
