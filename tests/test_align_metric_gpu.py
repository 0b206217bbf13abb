"""GPU: the Align-Acc metric model (diff_foley_amd.AlignmentClassifierMetric, df_align_verdict) against the reference's own outputs,
G16 (tests/golden/make_golden_align_metric.py), on both operand builds.

Bounds.  ``moments`` and ``z`` by rel-L2 under the bound tests/test_vae_encoder_gpu.py holds the encoder to (< 2e-2 with bf16 operands,
< 3e-3 with fp16); the cond stage's output under the existing cond bound of the golden comparisons (rel-L2 < 5e-3,
tests/test_path_gpu.py).  The probability bound P_BOUND is MEASURED against the reference, not fixed beforehand: the G16 comparisons
were run once per build on an MI355X, the largest |p - p_ref| over all cases taken, and the bound is twice that, rounded up to one
significant digit (the factor covers plan choices and summation orders that differ between boxes and batches).  Measured: 1.11e-3
with bf16 operands (the tiny replay), 1.05e-4 with fp16 (tiny, 32 frames); full size alone 1.99e-4 / 7.59e-5.  Bounds: 3e-3 / 3e-4,
next to the classifier's existing 5e-3 (fp16; 8x that for bf16) of tests/test_classifier_config_fuzz_gpu.py.

Verdicts.  ``pred`` must equal the reference's on EVERY committed case.  What makes that fair is decided by the reference alone: the
generator keeps only cases at a margin min |p - 0.5| (full size 0.0149, tiny 0.0451, the tiny replay 0.0395, asserted there), and a
bound may take at most a third of its configuration's margin (asserted here)."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLD, gold, rel_l2
import align_metric_cases as K

pytestmark = pytest.mark.gpu

ENC_BOUND = {"bf16": 2e-2, "fp16": 3e-3}
COND_BOUND = 5e-3
# largest |p - p_ref| over all G16 cases (tiny 8 / 32 frames, the tiny replay, full size) measured on an MI355X: 1.11e-3 with bf16
# operands, 1.05e-4 with fp16 -> twice that, rounded up to one significant digit
P_BOUND = {"bf16": 3e-3, "fp16": 3e-4}


def g16():
    return {k: (torch.from_numpy(v) if v.dtype.kind == "f" and v.ndim else v) for k, v in np.load(os.path.join(GOLD, "g16_align_metric.npz")).items()}


def _model(prec, which):
    import diff_foley_amd as P
    m = P.AlignmentClassifierMetric(precision=prec, **P.align_metric_config(*K.CFG[which]))
    missing, unexpected = m.load_state_dict(K.state_dict(which, bias=g16()[which + "_bias"]))
    assert missing == [] and unexpected == []
    m.cuda()
    assert m.engine.precision == prec, "the range probe moved the model to another build"
    return m


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def tiny(request):
    return _model(request.param, "tiny")


def _chain_vs_g16(m, g, tag, which, frames, rows, worst):
    """moments, z, cond, p and pred of the kept cases ``rows`` (positions in G16's kept list) in ONE call each, against G16."""
    from diff_foley_amd import engine as E
    prec = m.engine.precision
    x, feats, noise = K.inputs(which, frames)
    kept = torch.as_tensor(g[tag + "_kept"])[rows]
    x, feats, noise = x[kept].cuda(), feats[kept].cuda(), noise[kept].cuda()
    post = m.encode_first_stage(x)
    z = E.posterior_sample(post.parameters, noise, m.scale_factor)
    c = m.cond_model(feats)
    p = m.probabilities(x, feats, noise=noise)
    assert tuple(p.shape) == (len(rows), 1) and p.dtype == torch.float32 and p.is_cuda
    # the same chain through the reference's calling conventions: bit-equal, it is the same plans
    t = torch.tensor(0).reshape(1,).repeat(len(rows)).to(m.device).long()
    assert torch.equal(m.model(z, context=c, timesteps=t), p) and torch.equal(m(z, c, t), p) and torch.equal(m.encode_cond(feats), c)
    c_ref = g[tag + "_cond"][rows]
    errs = dict(moments=rel_l2(post.parameters.cpu(), g[tag + "_moments"][rows]), z=rel_l2(z.cpu(), g[tag + "_z"][rows]),
                cond=rel_l2(c.cpu()[:, ::4] if which == "full" else c.cpu(), c_ref),
                p=float((p.cpu() - g[tag + "_p"][rows]).abs().max()))
    print(f"align metric {tag} rows {list(rows)} [{prec}]: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f"; p {p.cpu().reshape(-1).tolist()} ref {g[tag + '_p'][rows].reshape(-1).tolist()}")
    worst[prec] = max(worst.get(prec, 0.0), errs["p"])
    assert errs["moments"] < ENC_BOUND[prec] and errs["z"] < ENC_BOUND[prec], errs
    assert errs["cond"] < COND_BOUND, errs
    assert errs["p"] < P_BOUND[prec], errs
    counts = torch.zeros(2, dtype=torch.int64, device=m.device)
    pred = E.align_verdict(p, None, counts)
    assert torch.equal(pred.cpu(), g[tag + "_pred"][rows]), (pred.cpu().reshape(-1).tolist(), g[tag + "_pred"][rows].reshape(-1).tolist())
    assert counts.tolist() == [int(g[tag + "_pred"][rows].sum()), len(rows)]


_worst = {}


def test_a_bound_takes_at_most_a_third_of_its_margin():
    g = g16()
    for prec, b in P_BOUND.items():
        assert b <= float(g["full_margin"]) / 3 and b <= float(g["tiny_margin"]) / 3 and b <= float(g["tiny32_replay_margin"]) / 3, (prec, b)


@pytest.mark.parametrize("frames", K.TINY_FRAMES)
def test_tiny_chain_vs_reference(tiny, frames):
    _chain_vs_g16(tiny, g16(), f"tiny{frames}", "tiny", frames, [0, 2, 4], _worst)      # batch 3: the lowest, the middle, the highest


@pytest.mark.parametrize("frames", K.TINY_FRAMES)
def test_tiny_remaining_kept_cases_vs_reference(tiny, frames):
    _chain_vs_g16(tiny, g16(), f"tiny{frames}", "tiny", frames, [1, 3], _worst)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_full_chain_vs_reference(prec):
    """eval_classifier.yaml's model at full size: batch 2 (one case of each verdict) and the remaining six in one call of batch 6."""
    m = _model(prec, "full")
    g = g16()
    _chain_vs_g16(m, g, "full", "full", 32, [0, 7], _worst)
    _chain_vs_g16(m, g, "full", "full", 32, [1, 2, 3, 4, 5, 6], _worst)
    print(f"align metric: largest |p - p_ref| so far {_worst}")
    with pytest.raises(NotImplementedError, match="encoder only"):
        m.first_stage_model.decode(torch.zeros(1, 4, 16, 64).cuda())
    with pytest.raises(RuntimeError, match="vae not configured"):
        m.engine.vae_decode(torch.zeros(1, 4, 16, 64).cuda())


# ---------------------------------------------------------------------------------------------------------- the fp16 range guard
GEGLU_FACTOR = 3.0e4          # the factor tests/test_path_fp16_gpu.py scales LatentDiffusion's GEGLU projection by


def _saturating_sd():
    """The tiny model's weights with the GEGLU projection of the backbone's first SpatialTransformer scaled by GEGLU_FACTOR."""
    sd = K.state_dict("tiny", bias=g16()["tiny_bias"])
    key = sorted(k for k in sd if k.startswith("model.") and k.endswith("transformer_blocks.0.ff.net.0.proj.weight"))[0]
    sd[key] = sd[key] * GEGLU_FACTOR
    return sd


def _new_metric(sd, **kw):
    import diff_foley_amd as P
    m = P.AlignmentClassifierMetric(**kw, **P.align_metric_config(*K.CFG["tiny"]))
    m.load_state_dict(sd)
    return m


def _probe_left_nothing_behind(m):
    """The saturation counters are off after a probe, and a normal call still runs."""
    x, feats, noise = K.inputs("tiny", 8)
    assert m.engine.debug_saturations_read() == []
    p = m.probabilities(x[:2].cuda(), feats[:2].cuda(), noise=noise[:2].cuda())
    assert torch.isfinite(p).all()
    assert m.engine.debug_saturations_read() == []
    return p


def test_fp16_range_guard_of_the_metric_model(monkeypatch):
    """The guard behind AlignmentClassifierMetric's load_state_dict + .cuda(): one saturation-counted pass of the Align-Acc chain.
    Procedural weights: silent.  With the GEGLU projection of model.input_blocks.3.1 scaled by 3.0e4 the fp16 build warns, names the ops
    and the bf16 fallback, and warns again when the same weights are loaded into the live model; the bf16 build has no range to guard
    and DF_RANGE_CHECK=0 switches the probe off.  The factor was fixed on the commit before the guard was folded into one template:
    there 3.0e4 flags 2 ops of the probe pass on an MI355X, that block's GEGLU and the projection behind it
    (cls_1_16_64_32#30:st.ff1: 65802 stores at +-65504, cls_1_16_64_32#31:st.ffproj: 4935)."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        m = _new_metric(K.state_dict("tiny", bias=g16()["tiny_bias"]), precision="fp16").cuda()
        assert m._range_check() == []
    _probe_left_nothing_behind(m)
    sd = _saturating_sd()
    m = _new_metric(sd, precision="fp16")
    with pytest.warns(RuntimeWarning, match=r"fp16 operands saturated.*Align-Acc chain.*precision='bf16'") as rec:
        m.cuda()
    print(f"metric range guard: {[str(w.message) for w in rec]}")
    assert m.engine.precision == "fp16"                       # an explicit precision is obeyed: warning only
    with pytest.warns(RuntimeWarning, match="saturated") as again:     # re-loading weights into a live engine probes again
        m.load_state_dict(sd)
    # both load paths name the caller's line, not one inside the package
    assert [os.path.basename(w.filename) for w in list(rec) + list(again)] == [os.path.basename(__file__)] * 2
    _probe_left_nothing_behind(m)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        _new_metric(sd, precision="bf16").cuda()
        monkeypatch.setenv("DF_RANGE_CHECK", "0")
        _new_metric(sd, precision="fp16").cuda()


def test_unrequested_precision_moves_the_metric_model_to_bf16_when_fp16_saturates(monkeypatch):
    """No operand type requested: the saturating weights give ONE warning, the model is on the bf16 build afterwards and its
    probabilities equal the explicit bf16 model's bit for bit.  A model that was tuning when the weights arrived keeps tuning on its
    new engine (the flag only: no forward runs here, so nothing is tuned)."""
    import warnings
    monkeypatch.delenv("DF_PRECISION", raising=False)
    sd = _saturating_sd()
    m = _new_metric(sd)
    with pytest.warns(RuntimeWarning, match="now runs on the bf16 build") as rec:
        m.cuda()
    print(f"metric range guard: {[str(w.message) for w in rec]}")
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert m.precision == m.engine.precision == "bf16"
    p = _probe_left_nothing_behind(m)
    mb = _new_metric(sd, precision="bf16").cuda()
    x, feats, noise = K.inputs("tiny", 8)
    assert torch.equal(p, mb.probabilities(x[:2].cuda(), feats[:2].cuda(), noise=noise[:2].cuda()))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        mt = _new_metric(K.state_dict("tiny", bias=g16()["tiny_bias"])).cuda()
    assert mt.engine.precision == "fp16"
    mt.autotune(True)
    old = mt.engine
    with pytest.warns(RuntimeWarning, match="now runs on the bf16 build"):
        mt.load_state_dict(sd)
    assert mt.engine is not old and mt.engine.precision == "bf16" and mt.engine.autotune_on is True
    assert mt.engine.debug_saturations_read() == []


# ---------------------------------------------------------------------------------------------------------- df_align_verdict alone
def _probs(B, seed):
    r = np.random.default_rng(seed)
    p = r.random(B, dtype=np.float32)
    half = np.float32(0.5)
    special = [half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)), np.float32(0), np.float32(1), np.float32(1.5),
               np.float32(2.5), np.float32("nan"), np.nextafter(np.float32(1), np.float32(0))]
    for i, v in enumerate(special[:B]):
        p[(i * 7) % B] = v
    return p


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_align_verdict_kernel_is_exact(B):
    from diff_foley_amd import engine as E
    E.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    want_c = want_t = 0
    for call, with_labels in enumerate((False, True, True)):          # the counters accumulate over three calls
        p = _probs(B, 10 * B + call)
        labels = np.random.default_rng(B + call).integers(0, 2, B).astype(np.float32) if with_labels else None
        buf = torch.full((B + 16,), -7.0, device=dev)                # sentinel-filled: pred is written for b < B and nowhere else
        shape = (B, 1) if call == 1 else (B,)
        pred = E.align_verdict(torch.from_numpy(p).to(dev).reshape(shape), None if labels is None else torch.from_numpy(labels),
                               counts, pred=buf[:B].reshape(shape))
        ref_pred, c, t = K.verdict(p, labels)
        want_c, want_t = want_c + c, want_t + t
        got = pred.reshape(-1).cpu().numpy()
        assert all((a == b) or (a != a and b != b) for a, b in zip(got.tolist(), ref_pred)), (B, call)
        assert bool((buf[B:] == -7.0).all())
        assert counts.tolist() == [want_c, want_t], (B, call, counts.tolist(), want_c, want_t)
    with pytest.raises(ValueError):
        E.align_verdict(torch.zeros(4, device=dev), torch.zeros(3), counts)
    with pytest.raises(ValueError):
        E.align_verdict(torch.zeros(4, device=dev), None, counts.int())
    assert tuple(E.align_verdict(torch.zeros(0, device=dev), None, counts).shape) == (0,) and counts.tolist() == [want_c, want_t]


# ---------------------------------------------------------------------------------------------------------- the loop
def _kept32(g):
    """G16's five kept 32-frame clips: (images (5, 3, 32, 64), features, the reference's noise rows)."""
    x, feats, noise = K.inputs("tiny", 32)
    kept = torch.as_tensor(g["tiny32_kept"])
    return x[kept], feats[kept], noise[kept]


def test_align_acc_loop(tiny, monkeypatch):
    """Five tiny clips (G16's kept 32-frame cases) in slices of 2, the last one ragged: both input layouts give the same counts, equal to
    the sum over round(p) of single calls and to the reference's verdicts; the counters stay on the device -- one host synchronisation,
    counted through the tensor methods that make one."""
    g = g16()
    images, feats, noise = _kept32(g)
    assert torch.equal(images[:, 0], images[:, 1]) and torch.equal(images[:, 0], images[:, 2])
    mel = torch.cat([images[:, 0], torch.full((5, 32, 8), 9.0)], dim=2)       # one-channel mels; toy cut of 64 columns below
    images, feats, noise = images.cuda(), feats.cuda(), noise.cuda()
    ref_pred = g["tiny32_pred"].reshape(-1)
    singles = [tiny.probabilities(images[i:i + 1], feats[i:i + 1], noise=noise[i:i + 1]) for i in range(5)]
    assert [K.round_half_even(float(p)) for p in singles] == ref_pred.tolist()
    want = (int(ref_pred.sum()), 5)
    assert tiny.align_acc(images, feats, batch_size=2, noise=noise) == want
    assert tiny.align_acc(mel[:, :, :64].cuda(), feats, batch_size=2, noise=noise) == want          # (N, n_mels, T) mels
    assert tiny.align_acc(mel[:, :, :64], feats.cpu(), batch_size=2, noise=noise.cpu()) == want     # ... from host memory
    assert tiny.align_acc(images, feats, batch_size=64, noise=noise) == want and tiny.align_acc(images[:0], feats[:0]) == (0, 0)
    labels = torch.tensor([0, 1, 0, 1, 1])
    assert tiny.align_acc(images, feats, labels=labels, batch_size=2, noise=noise) == (int((ref_pred == labels).sum()), 5)
    assert tiny.align_acc(images, feats, labels=1 - ref_pred, batch_size=3, noise=noise) == (0, 5)
    # the 512-column cut and the channel repeat are the loop's own (evaluation/dataset.py:99-107)
    from diff_foley_amd import ldm
    assert torch.equal(ldm.align_acc_specs(mel, columns=64).contiguous(), images.cpu())
    with pytest.raises(RuntimeError, match="feature sequences"):
        tiny.align_acc(images, feats[:4])
    # the default draw (the device's generator): the same loop, and no .item() / .cpu() / synchronize inside it
    calls = {"item": 0, "cpu": 0, "tolist": 0, "sync": 0}
    for name in ("item", "cpu", "tolist"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    sync = torch.cuda.synchronize

    def counted_sync(*a, **kw):
        calls["sync"] += 1
        return sync(*a, **kw)
    monkeypatch.setattr(torch.cuda, "synchronize", counted_sync)
    correct, total = tiny.align_acc(images, feats, batch_size=2)
    monkeypatch.undo()
    assert total == 5 and 0 <= correct <= 5
    assert calls == {"item": 0, "cpu": 1, "tolist": 1, "sync": 0}, calls


def model_inference(model, batch):
    """evaluation/align_acc.py:67-87 in this test's words: the calls a reference user makes, keyword arguments as written there."""
    bs = batch["spec"].shape[0]
    labels = torch.ones(bs).to(model.device)
    with torch.no_grad():
        spec = batch["spec"].to(model.device)
        video_feat = batch["video_feat"].to(model.device)
        encode_spec = model.encode_spec_z(spec)
        encode_cond = model.cond_model(video_feat)
        t = torch.tensor(0).reshape(1,).repeat(spec.shape[0]).to(model.device).long()
        prob_logits = model.model(encode_spec, context=encode_cond, timesteps=t)
        predicted = torch.round(prob_logits)
        correct_num = ((predicted == labels.float().unsqueeze(1)).sum()).item()
    return correct_num, predicted.shape[0], prob_logits


def test_model_inference_sequence_gives_the_references_count(tiny):
    g = g16()
    x, feats, _ = _kept32(g)
    model = tiny.eval()
    torch.manual_seed(int(g["tiny32_replay_seed"]))              # the reference draws posterior.sample() from the CPU generator
    correct, n, p = model_inference(model, dict(spec=x, video_feat=feats))
    err = float((p.cpu() - g["tiny32_replay_p"]).abs().max())
    print(f"align metric model_inference [{tiny.engine.precision}]: max |p - p_ref| {err:.2e}")
    assert err < P_BOUND[tiny.engine.precision]
    assert (correct, n) == (int(g["tiny32_replay_correct"]), 5)


def test_command_line_tool_prints_the_references_accuracy(tiny, tmp_path, capsys):
    """tools/align_acc.py on a folder written from G16's inputs (the five kept 32-frame clips as one-channel mels, one batch, the
    replay's seed): the reference's closing line with the reference's count."""
    import importlib.util
    import yaml
    import diff_foley_amd as P
    g = g16()
    x, feats, _ = _kept32(g)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec_dir, feat_dir = tmp_path / "generated", tmp_path / "feat"
    spec_dir.mkdir()
    feat_dir.mkdir()
    for i in range(5):
        np.save(spec_dir / f"clip_{i:02d}_sample_0.npy", x[i, 0].numpy())
        np.savez(feat_dir / f"clip_{i:02d}.npz", feat=torch.cat([feats[i], torch.zeros(3, 64)]).numpy())      # rows past 32 are dropped
    cfg = dict(model=dict(target="diff_foley_amd.ldm.AlignmentClassifierMetric", params=P.align_metric_config(*K.CFG["tiny"])))
    (tmp_path / "eval.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"state_dict": K.state_dict("tiny", bias=g["tiny_bias"])}, tmp_path / "eval.ckpt")
    spec = importlib.util.spec_from_file_location("align_acc_tool", os.path.join(root, "tools", "align_acc.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    acc, total = tool.main(["--config", str(tmp_path / "eval.yaml"), "--ckpt", str(tmp_path / "eval.ckpt"), "--specs", str(spec_dir),
                            "--feats", str(feat_dir), "--seed", str(int(g["tiny32_replay_seed"])), "--precision", tiny.engine.precision])
    want = int(g["tiny32_replay_correct"]) / 5
    assert total == 5 and acc == want
    assert f"Metric =====> Avg ACC: {want}   Total Num: 5" in capsys.readouterr().out


def test_missing_classifier_keys_raise_and_name_them(tiny):
    import diff_foley_amd as P
    sd = {k: v for k, v in K.state_dict("tiny").items() if not k.startswith("model.middle_block.")}
    m = P.AlignmentClassifierMetric(precision=tiny.engine.precision, **P.align_metric_config(*K.CFG["tiny"])).cuda()
    with pytest.raises(RuntimeError, match=r"Missing key\(s\).*model\.middle_block\.0\.in_layers\.0\.weight"):
        m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m.probabilities(torch.zeros(1, 3, 32, 64).cuda(), torch.zeros(1, 8, 64).cuda())


def test_decoder_free_and_decoder_carrying_state_dicts_score_alike(tiny):
    """A state dict without decoder tensors loads and scores (every fixture of this module); one WITH them scores to the same bits and
    reports them as unexpected: the decoder is not on the path and is not uploaded."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    g = g16()
    sd = K.state_dict("tiny", bias=g["tiny_bias"])
    assert not any(k.startswith(("first_stage_model.decoder.", "first_stage_model.post_quant_conv.")) for k in sd)
    dec = synth.make_state_dict(synth.vae_decoder_spec(synth.VAE_TINY, "first_stage_model."), 0)
    m = P.AlignmentClassifierMetric(precision=tiny.engine.precision, **P.align_metric_config(*K.CFG["tiny"]))
    missing, unexpected = m.load_state_dict(dict(sd, **dec))
    assert missing == [] and sorted(unexpected) == sorted(dec)
    m.cuda()
    x, feats, noise = K.inputs("tiny", 8)
    x, feats, noise = x[:3].cuda(), feats[:3].cuda(), noise[:3].cuda()
    assert torch.equal(m.probabilities(x, feats, noise=noise), tiny.probabilities(x, feats, noise=noise))


def test_latent_diffusion_beside_a_metric_model():
    """An ordinary LatentDiffusion still meets the tiny DDIM golden after a metric model was built and used in the process, and the two
    contexts do not share plans."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    from helpers import tiny_state_dict
    metric = _model("bf16", "tiny")
    x, feats, noise = K.inputs("tiny", 8)
    metric.probabilities(x[:2].cuda(), feats[:2].cuda(), noise=noise[:2].cuda())
    m = P.LatentDiffusion(precision="bf16", **P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    m.load_state_dict(tiny_state_dict())
    m.cuda()
    assert m.engine is not metric.engine
    before = metric.engine.plan_count()[0]
    assert before >= 3 and m.engine.plan_count()[0] == 0
    B = 2
    xT = synth.synthetic_xT(B, seed=21)
    c = m.get_learned_conditioning(synth.synthetic_cavp(B, 32, 64, seed=1234).cuda())
    z, _ = m.sample_log_diff_sampler(c, B, "DDIM", 25, unconditional_guidance_scale=4.5, unconditional_conditioning=torch.zeros_like(c),
                                     x_T=xT.clone())
    assert rel_l2(z.cpu(), gold("g5_tiny_samplers.npz")["DDIM_25_z"]) < 5e-2
    assert metric.engine.plan_count()[0] == before and m.engine.plan_count()[0] >= 2
    p0 = metric.probabilities(x[:2].cuda(), feats[:2].cuda(), noise=noise[:2].cuda())
    metric2 = _model("bf16", "tiny")
    assert torch.equal(p0, metric2.probabilities(x[:2].cuda(), feats[:2].cuda(), noise=noise[:2].cuda()))
