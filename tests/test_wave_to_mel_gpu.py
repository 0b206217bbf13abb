"""GPU: waveform -> normalised log-mel in libdfengine (csrc/vocoder.hip wave_to_mel_kernel, df_wave_to_mel) against the float64
restatement tests/wave_to_mel_ref.py.  PARITY UNPINNED: librosa 0.8.0 is not importable here (see that file's header).

The bound.  Every output element must lie in [f(ref - d), f(ref + d)] widened by 2 ulp of the output, where f is the
normalisation chain (monotone: the floor and the clip need no special case, no element is left out), ref the float64 linear mel
and d = K * eps32 * |frame * window|_2 * sum_k A[m, k]: the error of any FFT bin is bounded by a multiple of eps * |x|_2.

K is NOT taken from the kernel.  A float32 restatement on the CPU (scipy's float32 rfft, float32 filterbank product:
wave_to_mel_ref.linear_mel_f32) measured against float64 on this file's own inputs, in those units, worst element per case:

    index lengths (noise + tone, 15 lengths)   8.16        noise 0.1          3.04  3.73
    n_mels 80                                  6.28        tone 440 Hz       17.14 17.53
    n_mels 1                                   1.34        chirp 100-7500 Hz 19.77 20.96
    sr 22050                                   9.97        burst in 1e-6      3.90  3.38
    single-bin rows (24 rows, 100-400 Hz)      2.87        noise 1e-4         3.15  3.65

K = 4 x the worst of them (20.96).  The factor 4: ten radix-2 stages with fp32 table twiddles round more often than pocketfft's
mixed radix, and sqrt / fma contraction differ.  tests/test_wave_to_mel_cpu.py re-measures the short cases against K / 4."""
import ctypes as C

import numpy as np
import pytest
import torch

import wave_to_mel_ref as R

pytestmark = pytest.mark.gpu

K = 4 * 20.96
SR = 16000


def _fb(n_mels=128, sr=SR, fmin=125.0, fmax=7600.0):
    from oracle import vocoder as ov
    return ov.mel_filterbank(n_mels, sr=sr, fmin=fmin, fmax=fmax)


def _judge(out, y, what, **kw):
    """out (n_mels, T) float32 from the GPU for the clip y: every element inside the bound; prints how much of it was used."""
    ref_out, lin, norms = R.wave_to_mel_ref(y, **kw)
    A = _fb(**kw).astype(np.float64)
    assert out.shape == ref_out.shape and out.dtype == np.float32, (out.shape, ref_out.shape, out.dtype)
    o = out.astype(np.float64)
    assert np.isfinite(o).all()
    unit = R.EPS32 * A.sum(1)[:, None] * norms[None, :]
    lo, hi = R.normalise(lin - K * unit), R.normalise(lin + K * unit)
    ulp = np.spacing(np.abs(out)).astype(np.float64)
    inner = (o > 0) & (o < 1) & (unit > 0)                       # where the output still tells the linear value
    used = np.abs(10.0 ** ((o * 100.0 - 80.0) / 20.0) - lin)[inner] / unit[inner] if inner.any() else np.zeros(1)
    print(f"{what}: worst |mel - ref| = {used.max():.2f} units of eps32 |frame w| sum A (bound K = {K:.2f}; output rounding included), "
          f"worst |out - ref| = {np.abs(o - ref_out).max():.2e}, {(ref_out == 0).mean():.0%} of the reference at 0.0")
    bad = (o < lo - 2 * ulp) | (o > hi + 2 * ulp)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), o[bad][:4], lo[bad][:4], hi[bad][:4])
    return ref_out


def _gpu(y, **kw):
    from diff_foley_amd import vocoder as V
    return V.wave_to_mel(torch.from_numpy(np.ascontiguousarray(y)).cuda(), **kw).cpu().numpy()


def _tile():
    from diff_foley_amd import engine as E
    ft = E.lib().df_wave_to_mel_tile()
    assert ft >= 2 and ft % 2 == 0
    return ft


def test_lengths_at_which_indexing_can_go_wrong():
    """L = 1, 2, around one hop, around the 512-sample reflect pad (the pad equals / exceeds the clip: more than one reflection),
    around n_fft, a tile minus one / a full tile / a tile plus one frame, an odd and an even frame count above two tiles."""
    ft = _tile()
    for i, L in enumerate(R.index_lengths(ft)):
        y = R.noise_tone(L, 100 + i)
        out = _gpu(y)
        assert out.shape == (1, 128, 1 + L // 256)
        _judge(out[0], y, f"L = {L}")


def test_batch_row_stride_and_every_element_written():
    from diff_foley_amd import engine as E, vocoder as V
    L, B, gap = 256 * _tile() + 77, 3, 37
    ys = np.stack([R.noise_tone(L, 200 + b, hz=500.0 * (b + 1)) for b in range(B)])
    buf = torch.full((B, L + gap), 1e30, dtype=torch.float32)   # a sentinel in the gap: reading it would wreck a frame
    buf[:, :L] = torch.from_numpy(ys)
    buf = buf.cuda()
    view = buf[:, :L]
    assert view.stride(0) == L + gap and view.data_ptr() == buf.data_ptr()
    out = V.wave_to_mel(view)
    assert out.shape == (B, 128, 1 + L // 256)
    # the same through the C entry into an output pre-filled with a sentinel: every element must be overwritten
    c = V._get_fwd_consts(SR, 128, 125.0, 7600.0, buf.device)
    raw = torch.full_like(out, float("nan"))
    p = lambda t: C.c_void_p(t.data_ptr())
    lib = E.lib()
    E._chk(lib.df_wave_to_mel(p(buf), L + gap, B, L, p(c.A), p(c.bands), 128, p(c.tw), p(c.window), 1e-5, p(raw), E._stream()), lib)
    assert not torch.isnan(raw).any() and torch.equal(raw, out)
    assert torch.equal(buf[:, L:].cpu(), torch.full((B, gap), 1e30))
    o = out.cpu().numpy()
    for b in range(B):
        _judge(o[b], ys[b], f"B = 3, clip {b}")
        one = _gpu(ys[b])                                         # B = 1, contiguous: the same bits
        assert one.shape == (1, 128, 1 + L // 256) and np.array_equal(one[0], o[b])
    assert np.array_equal(_gpu(ys[0][None])[0], o[0]) and np.array_equal(V.wave_to_mel(ys[1]).cpu().numpy()[0], o[1])   # (L,) = B 1


@pytest.mark.parametrize("kw", [dict(n_mels=80), dict(n_mels=1), dict(sr=22050), dict(n_mels=24, fmin=100.0, fmax=400.0)],
                         ids=["n_mels80", "n_mels1", "sr22050", "single_bin_rows"])
def test_other_filterbanks(kw):
    from diff_foley_amd import vocoder as V
    if "fmin" in kw:
        assert (V.mel_bands(V.mel_filterbank(sr=SR, **kw))[:, 1] == 1).any()        # rows whose band is a single bin
    y = R.noise_tone(4196, 77)                                    # T = 17: an odd count, a last tile of one frame
    full = dict(n_mels=128, sr=SR, fmin=125.0, fmax=7600.0)
    full.update(kw)
    out = _gpu(y, **full)
    _judge(out[0], y, str(kw), **full)


def test_exact_ends():
    rng = np.random.default_rng(5)
    L = 256 * 2 * _tile() + 300
    silence = np.zeros((2, L), np.float32)
    ref = R.wave_to_mel_ref(silence[0])[0]
    assert (ref == 0.0).all()
    out = _gpu(silence)
    assert out.shape == (2, 128, 1 + L // 256) and (out == 0.0).all()
    loud = (1000.0 * rng.uniform(-1, 1, (2, L))).astype(np.float32)
    out = _gpu(loud)
    for b in range(2):
        ref, lin, _ = R.wave_to_mel_ref(loud[b])
        assert (ref == 1.0).all() and lin.min() > 10.0
        assert (out[b] == 1.0).all()


@pytest.fixture(scope="module")
def content():
    return R.content_cases()


@pytest.mark.parametrize("name", ["noise_0.1", "tone_440", "chirp_100_7500", "burst_in_1e-6", "noise_1e-4"])
def test_content_at_the_models_size(content, name):
    """L = 131071 -> T = 512, B = 2.  The burst puts loud and silent frames into one tile; noise 1e-4 straddles the point where the
    chain clips to 0.0 (about 40 % of the reference sits there)."""
    y = content[name]
    assert y.shape == (2, R.MODEL_L)
    out = _gpu(y)
    assert out.shape == (2, 128, 512)
    for b in range(2):
        ref = _judge(out[b], y[b], f"{name}[{b}]")
        if name == "noise_1e-4":
            assert 0.3 < (ref == 0).mean() < 0.5 and ref.max() > 0.05
        if name == "burst_in_1e-6":
            assert (ref == 0).mean() > 0.9 and ref.max() > 0.5


def test_determinism_and_streams(content):
    from diff_foley_amd import vocoder as V
    y = torch.from_numpy(content["chirp_100_7500"]).cuda()
    a = V.wave_to_mel(y)
    b = V.wave_to_mel(y)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = V.wave_to_mel(y)
    side.synchronize()
    assert torch.equal(a, c)


def test_facade(content):
    import diff_foley_amd as P
    from diff_foley_amd import vocoder as V
    wav = content["noise_0.1"][0]
    full = np.concatenate([wav, wav[:5000]])                      # longer than length: cut
    y, mel = P.get_spectrogram(full, 131072)
    assert y.shape == (131071,) and np.array_equal(y, full[:131071])
    assert mel.shape == (128, 512) and mel.dtype == np.float32
    direct = P.wave_to_mel(torch.from_numpy(full[:131071])[None].cuda())
    assert direct.is_cuda and direct.dtype == torch.float32 and np.array_equal(mel, direct[0].cpu().numpy())
    y2, mel2 = P.get_spectrogram(wav[:100000], 131072)            # shorter: zero-padded
    assert y2.shape == (131071,) and not y2[100000:].any() and mel2.shape == (128, 512)
    assert np.array_equal(mel2[:, :380], mel[:, :380]) and (mel2[:, 400:] == 0).all()
    empty = P.wave_to_mel(torch.zeros(0, 4096).cuda())
    assert tuple(empty.shape) == (0, 128, 17) and empty.is_cuda
    moved = P.wave_to_mel(torch.from_numpy(wav[:8192]))           # a CPU tensor is moved, as inverse_op moves its input
    assert moved.is_cuda and torch.equal(moved, P.wave_to_mel(wav[:8192].astype(np.float64)))
    assert torch.equal(moved, P.wave_to_mel(torch.from_numpy(wav[:8192]).cuda()))
    with pytest.raises(ValueError):
        P.wave_to_mel(torch.zeros(2, 0).cuda())


def test_c_entry_rejects_bad_arguments():
    from diff_foley_amd import engine as E, vocoder as V
    dev = torch.device("cuda", torch.cuda.current_device())
    c = V._get_fwd_consts(SR, 128, 125.0, 7600.0, dev)
    wav, out = torch.zeros(2, 1024, device=dev), torch.zeros(2, 128, 5, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    lib = E.lib()

    def call(B=2, L=1024, n_mels=128, wav_p=p(wav), out_p=p(out), stride=1024):
        return lib.df_wave_to_mel(wav_p, stride, B, L, p(c.A), p(c.bands), n_mels, p(c.tw), p(c.window), 1e-5, out_p, E._stream())
    assert call() == 0
    for bad in (dict(B=0), dict(L=0), dict(n_mels=0), dict(n_mels=129), dict(wav_p=None), dict(out_p=None), dict(stride=1000)):
        assert call(**bad) != 0, bad
        assert b"wave_to_mel" in lib.df_last_error()
    torch.cuda.synchronize()


def test_feeds_encode_first_stage():
    """wave_to_mel -> 3-channel repeat -> encode_first_stage on the tiny encoder state of tests/test_vae_encoder_gpu.py."""
    import diff_foley_amd as P
    from diff_foley_amd import synth
    spec = synth.state_dict_spec(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY, with_encoder=True)
    m = P.LatentDiffusion(**P.stage2_config(synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY))
    m.load_state_dict(synth.make_state_dict(spec, 0))
    m.cuda()
    wav = np.stack([R.noise_tone(256 * 63 + 9, 300 + b) for b in range(2)])
    mel = P.wave_to_mel(wav, n_mels=32)                           # the tiny VAE's image: 32 x 64
    assert tuple(mel.shape) == (2, 32, 64)
    post = m.encode_first_stage(mel[:, None].repeat(1, 3, 1, 1))
    assert tuple(post.parameters.shape) == (2, 8, 8, 16) and torch.isfinite(post.parameters).all()
    z = m.get_first_stage_encoding(post.mode())
    assert tuple(z.shape) == (2, 4, 8, 16)


def test_inverse_on_the_same_basis():
    """mel_to_stft(wave_to_mel(y, sr=16000), sr=16000): A_16k S reproduces the linear mel, judged by the residual bound
    tests/test_vocoder_gpu.py uses for the default basis."""
    from diff_foley_amd import vocoder as V
    from oracle import vocoder as ov
    y = np.stack([R.noise_tone(256 * 23 + 5, 400 + b, hz=700.0 * (b + 1)) for b in range(2)])
    mel = V.wave_to_mel(y, sr=16000)
    m = mel.cpu().numpy()
    assert m.shape == (2, 128, 24) and m.min() > 0 and m.max() < 1          # nothing clipped: the chain is invertible here
    amp = ov.undo_mel_normalisation(m.astype(np.float64)).astype(np.float32)
    S = V.mel_to_stft(mel, sr=16000).cpu().numpy()
    assert S.shape == (2, 24, 513) and (S >= 0).all() and np.isfinite(S).all()
    A = ov.mel_filterbank(128, sr=16000)
    for b in range(2):
        lin = R.wave_to_mel_ref(y[b])[1]
        assert np.abs(amp[b] / lin - 1).max() < 1e-4                        # the undone chain is the linear mel
        res = np.linalg.norm(A @ S[b].T - amp[b]) / np.linalg.norm(amp[b])
        Xo = ov.nnls_lbfgs(A, amp[b])
        res_o = np.linalg.norm(A @ Xo - amp[b]) / np.linalg.norm(amp[b])
        print(f"NNLS residual on the sr-16000 basis: engine {res:.2e}   oracle {res_o:.2e}")
        assert res < 1e-2 and res < 3.0 * res_o + 2e-3
        wrong = np.linalg.norm(ov.mel_filterbank(128) @ S[b].T - amp[b]) / np.linalg.norm(amp[b])
        assert wrong > 10 * res                                             # and it is the 16 kHz basis that was inverted
