"""TEST INFRASTRUCTURE ONLY (never imported by diff_foley_amd/).  **PARITY UNPINNED.**

Float64 restatement of the waveform -> mel transform of data_preprocess/wav2spec.py:145-155 (``TRANSFORMS``):

    S    = |librosa.stft(y, n_fft=1024, hop_length=256)|          hann (periodic), centred, np.pad(mode="reflect") by 512
    mel  = librosa.filters.mel(sr=16000, n_fft=1024, fmin=125, fmax=7600, n_mels=128) @ S
    out  = clip((20 * log10(max(1e-5, mel)) - 20 + 100) / 100, 0, 1)

librosa 0.8.0 cannot be imported here and the reference holds no golden vector for this path, so -- as oracle/vocoder.py says
for the inverse -- parity to librosa itself is unpinned: what the GPU kernel is judged against is this restatement, with
``np.fft.rfft`` in float64 and the oracle's Slaney filterbank (oracle.vocoder.mel_filterbank, float32 entries as librosa
returns them, multiplied in float64).

Also here, shared by the CPU and the GPU tests: the float32 CPU restatement whose distance to float64 sets the GPU test's bound,
and the seeded signals both are run on."""
import numpy as np

from oracle import vocoder as ov

N_FFT, HOP, FLOOR = 1024, 256, 1e-5
EPS32 = float(np.finfo(np.float32).eps)


def normalise(mel, floor=FLOOR):
    """LowerThresh, Log10, Multiply(20), Subtract(20), Add(100), Divide(100), Clip(0, 1): monotone in ``mel``."""
    return np.clip((20.0 * np.log10(np.maximum(floor, mel)) - 20.0 + 100.0) / 100.0, 0.0, 1.0)


def _windowed_frames(y, dtype):
    y = np.asarray(y, dtype=dtype).reshape(-1)
    yp = np.pad(y, N_FFT // 2, mode="reflect")
    T = 1 + (len(yp) - N_FFT) // HOP
    idx = HOP * np.arange(T)[:, None] + np.arange(N_FFT)[None, :]
    return yp[idx] * ov.hann(N_FFT).astype(dtype)[None, :]                      # [T][1024]


def wave_to_mel_ref(y, sr=16000, n_mels=128, fmin=125.0, fmax=7600.0):
    """y (L,) -> (out (n_mels, T) float64 normalised log-mel, lin (n_mels, T) float64 linear mel, norms (T,) = |frame * window|_2)."""
    fw = _windowed_frames(y, np.float64)
    S = np.abs(np.fft.rfft(fw, axis=1))                                          # [T][513]
    A = ov.mel_filterbank(n_mels, sr=sr, fmin=fmin, fmax=fmax).astype(np.float64)
    lin = A @ S.T
    return normalise(lin), lin, np.linalg.norm(fw, axis=1)


def linear_mel_f32(y, sr=16000, n_mels=128, fmin=125.0, fmax=7600.0):
    """The same in float32 on the CPU: float32 frames, scipy's float32 rfft (pocketfft), float32 filterbank product -> (n_mels, T)."""
    from scipy import fft as sfft
    fw = _windowed_frames(y, np.float32)
    X = sfft.rfft(fw, axis=1)
    assert X.dtype == np.complex64
    return ov.mel_filterbank(n_mels, sr=sr, fmin=fmin, fmax=fmax) @ np.abs(X).T


def error_units(lin, lin64, norms, A):
    """|lin - lin64| in units of eps32 * |frame * window|_2 * sum_k A[m, k], worst element (rows / frames with a zero unit left out)."""
    unit = EPS32 * A.astype(np.float64).sum(1)[:, None] * norms[None, :]
    ok = unit > 0
    return float((np.abs(lin.astype(np.float64) - lin64)[ok] / unit[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------- the seeded signals (sr 16000)
def noise_tone(L, seed, amp=0.1, hz=1000.0, sr=16000):
    """Seeded uniform noise plus a tone, peak amplitude ``amp``."""
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    return (amp * (0.7 * rng.uniform(-1, 1, L) + 0.3 * np.sin(2 * np.pi * hz * n / sr))).astype(np.float32)


def index_lengths(ft):
    """Lengths at which indexing can go wrong for a tile of ``ft`` frames."""
    return [1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 256 * ft - 1, 256 * ft, 256 * (ft + 1),
            256 * (2 * ft + 2) + 17,           # T = 2 ft + 3: odd, above two tiles
            256 * (2 * ft + 3) + 100]          # T = 2 ft + 4: even


MODEL_L = 131071                               # get_spectrogram(audio, 131072): T = 512, the model's mel width


def content_cases(L=MODEL_L, sr=16000):
    """name -> (2, L) float32: two clips per kind of content."""
    rng = np.random.default_rng(1234)
    n = np.arange(L)
    t = n / sr
    out = {}
    out["noise_0.1"] = 0.1 * rng.uniform(-1, 1, (2, L))
    out["tone_440"] = np.stack([0.5 * np.sin(2 * np.pi * 440.0 * t), 0.05 * np.sin(2 * np.pi * 440.0 * t + 1.0)])
    k = (7500.0 - 100.0) / (L / sr)
    up = 0.3 * np.sin(2 * np.pi * (100.0 * t + 0.5 * k * t * t))
    out["chirp_100_7500"] = np.stack([up, up[::-1]])
    burst = 1e-6 * rng.uniform(-1, 1, (2, L))                                    # 10 ms = 160 samples, loud, in 1e-6 noise
    burst[0, 40000:40160] += 0.5 * rng.uniform(-1, 1, 160)
    burst[1, 70001:70161] += 0.5 * rng.uniform(-1, 1, 160)                       # not on a hop boundary
    out["burst_in_1e-6"] = burst
    out["noise_1e-4"] = 1e-4 * rng.standard_normal((2, L))       # straddles the floor: ~40 % of the reference is clipped to 0.0
    return {k_: v.astype(np.float32) for k_, v in out.items()}
