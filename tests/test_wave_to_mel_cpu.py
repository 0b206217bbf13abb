"""CPU: the host side of waveform -> mel (diff_foley_amd/vocoder.py: wave_to_mel, get_spectrogram, the ``sr`` keyword of the
inverse) and the float64 reference the GPU kernel is judged by (tests/wave_to_mel_ref.py).  PARITY UNPINNED: librosa 0.8.0 is
not importable here, so nothing below comes from the reference's own run (see the header of wave_to_mel_ref.py)."""
import os
import re

import numpy as np
import pytest
import torch

import wave_to_mel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_exists_and_header_declares_the_entry():
    import diff_foley_amd as P
    from diff_foley_amd import engine as E, vocoder as V
    assert P.get_spectrogram is V.get_spectrogram and P.wave_to_mel is V.wave_to_mel
    hdr = open(os.path.join(ROOT, "include", "df_engine.h")).read()
    assert re.search(r"\bint\s+df_wave_to_mel\s*\(", hdr)
    assert "wav2spec.py:145-155" in hdr and "170-189" in hdr              # every export cites what it replaces
    assert "df_wave_to_mel" in E.exported_symbols()
    src = open(os.path.join(ROOT, "diff_foley_amd", "csrc", "vocoder.hip")).read()
    assert "wave_to_mel_kernel" in src


@pytest.mark.parametrize("kw", [dict(n_mels=128, sr=16000), dict(n_mels=80, sr=16000), dict(n_mels=1, sr=16000),
                                dict(n_mels=128, sr=22050), dict(n_mels=24, sr=16000, fmin=100.0, fmax=400.0)])
def test_host_filterbank_equals_the_oracle_bit_for_bit(kw):
    from diff_foley_amd import vocoder as V
    from oracle import vocoder as ov
    a, b = V.mel_filterbank(**kw), ov.mel_filterbank(**kw)
    assert a.dtype == np.float32 and a.shape == (kw["n_mels"], 513)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_band_table_covers_exactly_the_nonzeros_of_every_row():
    from diff_foley_amd import vocoder as V
    for kw in (dict(n_mels=128, sr=16000), dict(n_mels=80, sr=16000), dict(n_mels=1, sr=16000), dict(n_mels=128, sr=22050),
               dict(n_mels=24, sr=16000, fmin=100.0, fmax=400.0)):
        A = V.mel_filterbank(**kw)
        bands = V.mel_bands(A)
        assert bands.dtype == np.int32 and bands.shape == (kw["n_mels"], 2)
        for m, (k0, n) in enumerate(bands):
            inside = np.zeros(513, bool)
            inside[k0:k0 + n] = True
            assert 0 <= k0 and k0 + n <= 513
            assert not A[m][~inside].any()                                  # nothing outside the span
            if n:
                assert A[m, k0] != 0 and A[m, k0 + n - 1] != 0              # and the span is tight
            else:
                assert not A[m].any()
    A = V.mel_filterbank(128, sr=16000)                                     # the figures the kernel's header quotes
    bands = V.mel_bands(A)
    assert np.count_nonzero(A) == 944 and bands[:, 0].min() == 9 and (bands[:, 0] + bands[:, 1]).max() == 487
    assert bands[:, 1].max() == 22
    assert V.mel_bands(np.zeros((2, 513), np.float32)).tolist() == [[0, 0], [0, 0]]
    single = V.mel_bands(V.mel_filterbank(24, sr=16000, fmin=100.0, fmax=400.0))
    assert (single[:, 1] == 1).any()                                        # the GPU test's single-bin bank has such rows


@pytest.mark.parametrize("L", [1, 255, 256, 131071, 163839])
def test_frame_count(L):
    from diff_foley_amd import vocoder as V
    out, lin, norms = R.wave_to_mel_ref(R.noise_tone(L, 3), n_mels=4)
    assert V.n_frames(L) == 1 + L // 256 == out.shape[1] == lin.shape[1] == norms.shape[0]
    assert out.shape[0] == 4
    if L == 131071:
        assert out.shape[1] == 512                                          # the model's mel width
    if L == 163839:
        assert out.shape[1] == 640                                          # "ensure: 640 spec"


def test_reference_on_a_pure_tone_peaks_in_the_row_that_holds_it():
    from oracle import vocoder as ov
    A = ov.mel_filterbank(128, sr=16000)
    for hz in (440.0, 1000.0, 3000.0):
        y = 0.3 * np.sin(2 * np.pi * hz * np.arange(8192) / 16000.0)
        out, lin, _ = R.wave_to_mel_ref(y)
        k = int(round(hz / (16000.0 / 1024)))
        want = int(np.argmax(A[:, k]))
        assert A[want, k] > 0
        assert (np.argmax(lin[:, 2:-2], axis=0) == want).all()              # frames clear of the reflected ends
        assert (np.argmax(out[:, 2:-2], axis=0) == want).all()
    assert R.normalise(np.array([0.0, 1e-5, 1e-4, 1.0, 10.0, 1e3])).tolist() == [0.0, 0.0, 0.0, 0.8, 1.0, 1.0]


def test_float32_cpu_restatement_stays_within_a_quarter_of_the_gpu_bound():
    """K of tests/test_wave_to_mel_gpu.py is 4 x the worst ratio of the float32 CPU restatement: re-measured here on the short cases."""
    import test_wave_to_mel_gpu as G
    from oracle import vocoder as ov
    A = ov.mel_filterbank(128, sr=16000)
    src = open(os.path.join(ROOT, "diff_foley_amd", "csrc", "vocoder.hip")).read()
    ft = int(re.search(r"^#define WTM_FT (\d+)", src, re.M).group(1))        # the GPU test's lengths follow the kernel's tile
    for i, L in enumerate(R.index_lengths(ft)):
        y = R.noise_tone(L, 100 + i)
        _, lin, norms = R.wave_to_mel_ref(y)
        assert R.error_units(R.linear_mel_f32(y), lin, norms, A) <= G.K / 4


def test_get_spectrogram_pad_cut_rule(monkeypatch, tmp_path):
    from diff_foley_amd import vocoder as V
    seen = []

    def fake(wav, sr=16000, **kw):                                          # the reference in place of the GPU kernel
        wav = np.asarray(wav)
        seen.append((wav.shape, wav.dtype, sr))
        return torch.from_numpy(np.stack([R.wave_to_mel_ref(w, sr=sr)[0] for w in wav]).astype(np.float32))
    monkeypatch.setattr(V, "wave_to_mel", fake)
    length = 2048
    rng = np.random.default_rng(0)
    short, exact, long_ = (0.1 * rng.standard_normal(n).astype(np.float32) for n in (1500, length, 5000))
    y, mel = V.get_spectrogram(short, length)                               # zero-padded, then [:length - 1]
    assert y.shape == (length - 1,) and y.dtype == np.float64
    assert np.array_equal(y[:1500], short.astype(np.float64)) and not y[1500:].any()
    assert mel.shape == (128, 8) and mel.dtype == np.float32
    assert np.array_equal(mel, R.wave_to_mel_ref(y)[0].astype(np.float32))
    y, mel = V.get_spectrogram(long_, length)                               # cut
    assert y.shape == (length - 1,) and y.dtype == np.float32 and np.array_equal(y, long_[:length - 1])
    assert mel.shape == (128, 8)
    y, _ = V.get_spectrogram(exact, length)
    assert np.array_equal(y, exact[:length - 1])
    y, _ = V.get_spectrogram(torch.from_numpy(long_)[None], length)        # a tensor, any shape: reshape(-1)
    assert np.array_equal(y, long_[:length - 1])
    assert all(s == ((1, length - 1), np.float32, 16000) for s in seen)
    np.save(tmp_path / "clip.npy", long_)
    y, _ = V.get_spectrogram(str(tmp_path / "clip.npy"), length)            # wav2spec.py:173
    assert np.array_equal(y, long_[:length - 1])
    with pytest.raises(ValueError, match="caller"):
        V.get_spectrogram("clip.wav", length)


def test_sr_keyword_of_the_inverse_reaches_the_filterbank(monkeypatch):
    from diff_foley_amd import vocoder as V
    import inspect
    for fn in (V.mel_to_stft, V.mel_to_wave):
        assert inspect.signature(fn).parameters["sr"].default == 22050
    real, seen = V.mel_filterbank, []

    def spy(n_mels, sr=V.SR, **kw):
        seen.append(sr)
        return real(n_mels, sr=sr, **kw)
    monkeypatch.setattr(V, "mel_filterbank", spy)
    monkeypatch.setattr(V, "_consts", {})
    c_def = V._get_consts(8, 4, "cpu")
    c_16k = V._get_consts(8, 4, "cpu", sr=16000)
    assert seen == [22050, 16000] and c_def is not c_16k
    assert V._get_consts(8, 4, "cpu") is c_def and V._get_consts(8, 4, "cpu", 22050) is c_def
    assert np.array_equal(c_def.A.numpy().view(np.uint32), real(8).view(np.uint32))        # the default: the same bits as before
    assert np.array_equal(c_16k.A.numpy().view(np.uint32), real(8, sr=16000).view(np.uint32))
    assert not np.array_equal(c_def.A.numpy(), c_16k.A.numpy())


def test_wave_to_mel_rejects_bad_arguments_before_touching_the_device():
    from diff_foley_amd import vocoder as V
    with pytest.raises(ValueError):
        V.wave_to_mel(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        V.wave_to_mel(np.zeros(1000, np.float32), n_mels=129)
    with pytest.raises(ValueError):
        V.wave_to_mel(np.zeros(1000, np.float32), n_mels=0)
