"""TEST INFRASTRUCTURE ONLY (never imported by diff_foley_amd/).  **PARITY UNPINNED.**

Float64 restatements, stage by stage, of the mel -> waveform kernels of csrc/vocoder.hip (nnls_fista_kernel, gl_init_angles_kernel,
gl_ifft_kernel, gl_ola_kernel, gl_stft_kernel), written from the formulas of oracle/vocoder.py and the kernels' comments in plain
numpy.  librosa 0.8.0 cannot be imported here (see the oracle's header), so parity to librosa itself stays unpinned: these functions
are what the GPU kernels are judged against, element by element (tests/test_vocoder_kernels_gpu.py), and tests/test_vocoder_ref_cpu.py
ties them to the oracle.

Layouts are the device's: S [..][T][513] magnitudes, angles / rebuilt complex [..][T][513], frames [..][T][1024], wav [..][256 (T-1)],
phase0 [..][513][T], mel [..][n_mels][T]; leading dimensions are batch.

Every stage function has a float32 twin (``*_f32``: float32 arrays, scipy.fft in float32, float32 accumulation).  The twins are not
the kernel: their distance to float64 on the GPU test's own inputs, times 4, is the GPU test's bound K, so that no constant comes
from the kernel.  The ``judge_*`` functions turn a stage's output and the float64 reference into a per-element verdict in the
stage's own unit (eps32 = 2^-24):

    init angles      eps32, each component of a unit vector
    gl_ifft          eps32 * |irfft frame|_2 * window[n]              (window[0] = 0: that sample must be exactly 0)
    gl_ola           4 * eps32 * sum |terms| / wss                    (derived: at most three additions and one division; no K)
    gl_stft rebuilt  eps32 * |frame * window|_2, each component of a bin
    gl_stft angles   eps32 * (1 + (|rb| + m |prev|) / |a|), m = momentum / (1 + momentum); an element whose bound reaches 0.1
                     tells nothing, and at most 0.1 % of a case's elements may be such
    NNLS             eps32 * max_k x64[k, t] for each frame t; and exactly 0 where the float64 iterate is 0 and the float64
                     pre-clip value lies below -K units

Also here, shared by the CPU and the GPU tests: the seeded inputs and shapes both run on."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import vocoder as ov

N_FFT, HOP, N_BIN = 1024, 256, 513
EPS32 = 2.0 ** -24
TINY32 = float(np.finfo(np.float32).tiny)
SILENT_BOUND, SILENT_CAP = 0.1, 1e-3


# ---------------------------------------------------------------------------------------- the tables the host hands the kernels
def window32():
    """Periodic hann as diff_foley_amd.vocoder._Consts builds it: float64, rounded once to float32."""
    return ov.hann(N_FFT).astype(np.float32)


def wss32(T):
    """Window sum-square of T frames, float32 accumulation of float32 squares, as _Consts builds it: [1024 + 256 (T - 1)]."""
    wss = np.zeros(N_FFT + HOP * (T - 1), dtype=np.float32)
    wsq = (ov.hann(N_FFT) ** 2).astype(np.float32)
    for i in range(T):
        wss[i * HOP:i * HOP + N_FFT] += wsq
    return wss


def as_complex(buf):
    """Device complex buffer read back as float32 [..][2] -> complex128 [..]."""
    buf = np.asarray(buf)
    return buf[..., 0].astype(np.float64) + 1j * buf[..., 1].astype(np.float64)


def _win(window, dtype):
    return (ov.hann(N_FFT) if window is None else np.asarray(window)).astype(dtype)


# ---------------------------------------------------------------------------------------- Griffin-Lim stages
def init_angles(phase0):
    """phase0 [..][513][T] in [0, 1) -> exp(2 pi i u), complex128 [..][T][513]."""
    return np.swapaxes(np.exp(2j * np.pi * np.asarray(phase0, dtype=np.float64)), -1, -2)


def init_angles_f32(phase0):
    a = np.float32(2 * np.pi) * np.asarray(phase0, dtype=np.float32)
    return np.swapaxes((np.cos(a) + 1j * np.sin(a)).astype(np.complex64), -1, -2)


def synth_frames(S, angles, window=None):
    """Spectrum S * angles with the imaginary parts of DC and Nyquist ignored -> irfft(n = 1024) -> periodic hann.
    Returns (frames [..][T][1024], |irfft frame|_2 [..][T])."""
    spec = np.asarray(S, dtype=np.float64) * np.asarray(angles, dtype=np.complex128)
    spec[..., 0] = spec[..., 0].real
    spec[..., N_BIN - 1] = spec[..., N_BIN - 1].real
    x = np.fft.irfft(spec, n=N_FFT, axis=-1)
    return x * _win(window, np.float64), np.linalg.norm(x, axis=-1)


def synth_frames_f32(S, angles, window=None):
    from scipy import fft as sfft
    spec = (np.asarray(S, dtype=np.float32) * np.asarray(angles, dtype=np.complex64)).astype(np.complex64)
    spec[..., 0] = spec[..., 0].real
    spec[..., N_BIN - 1] = spec[..., N_BIN - 1].real
    x = sfft.irfft(spec, n=N_FFT, axis=-1)
    assert x.dtype == np.float32
    return x * _win(window, np.float32)


def overlap_add(frames, wss, T, n=None, t0=0, dtype=np.float64):
    """Gather form: sample n of the trimmed signal sums frames[t][n + 512 - 256 t] over the frames that cover it (ascending t) and
    divides by wss[n + 512] where that exceeds float32 tiny.  ``n``: the samples wanted (default all 256 (T - 1)); ``frames[.., 0]``
    is frame ``t0`` of the clip (a slice of a long clip).  Returns (y [..][len(n)], sum |terms| / wss: the unit of the bound)."""
    frames = np.asarray(frames, dtype=dtype)
    n = np.arange(HOP * (T - 1)) if n is None else np.asarray(n)
    pos = n + N_FFT // 2
    thi = pos // HOP
    acc = np.zeros(frames.shape[:-2] + n.shape, dtype=dtype)
    mass = np.zeros_like(acc)
    for j in (3, 2, 1, 0):                                        # a sample lies in at most 1024 / 256 = 4 frames
        t = thi - j
        ok = (t >= 0) & (t <= T - 1)
        term = frames[..., np.where(ok, t - t0, 0), pos - HOP * t] * ok.astype(dtype)
        acc = acc + term
        mass = mass + np.abs(term)
    w = np.asarray(wss)[pos].astype(dtype)
    big = w > TINY32
    div = np.where(big, w, 1).astype(dtype)
    return np.where(big, acc / div, acc), mass / div


def overlap_add_f32(frames, wss, T, n=None, t0=0):
    return overlap_add(frames, wss, T, n, t0, dtype=np.float32)[0]


def _padded_frames(y, T, window, dtype):
    y = np.asarray(y, dtype=dtype)
    assert y.shape[-1] == HOP * (T - 1), (y.shape, T)
    yp = np.pad(y, [(0, 0)] * (y.ndim - 1) + [(N_FFT // 2, N_FFT // 2)], mode="reflect")     # reflects as often as the pad needs
    idx = HOP * np.arange(T)[:, None] + np.arange(N_FFT)[None, :]
    return yp[..., idx] * _win(window, dtype)


def stft_frames(y, T, window=None):
    """np.pad(mode="reflect") by 512 (more than one reflection when the clip is shorter than the pad), window, rfft.
    Returns (spectrum complex [..][T][513], |frame * window|_2 [..][T])."""
    fw = _padded_frames(y, T, window, np.float64)
    return np.fft.rfft(fw, axis=-1), np.linalg.norm(fw, axis=-1)


def stft_frames_f32(y, T, window=None):
    from scipy import fft as sfft
    X = sfft.rfft(_padded_frames(y, T, window, np.float32), axis=-1)
    assert X.dtype == np.complex64
    return X


def angle_update(rebuilt, prev, momentum):
    """a = rebuilt - momentum / (1 + momentum) * prev ; a / (|a| + 1e-16)."""
    a = np.asarray(rebuilt, dtype=np.complex128) - (momentum / (1.0 + momentum)) * np.asarray(prev, dtype=np.complex128)
    return a / (np.abs(a) + 1e-16)


def angle_update_f32(rebuilt, prev, momentum):
    m = np.float32(momentum) / (np.float32(1) + np.float32(momentum))
    a = (np.asarray(rebuilt, dtype=np.complex64) - m * np.asarray(prev, dtype=np.complex64)).astype(np.complex64)
    return (a / (np.abs(a) + np.float32(1e-16))).astype(np.complex64)


# ---------------------------------------------------------------------------------------- NNLS by FISTA
def fista_path(A, Pt, mel, inv_L, iters, dtype=np.float64, At=None):
    """The kernel's iteration restated; ``iters``: the iteration counts wanted.  A [n_mels][513] (dense works as well), Pt [n_mels][513]
    = pinv(A)^T, mel [..][n_mels][T].  ``At`` [513][n_mels]: the matrix of the gradient product (the kernel takes it separately;
    default A^T).  Returns {count: (x [..][T][513], pre-clip value of the last projection [..][T][513])}.

        b = 10 ** ((mel * 100 - 100 + 20) / 20) ;  x0 = max(Pt^T b, 0) ;  t_0 = 1
        t_{n+1} = (1 + sqrt(1 + 4 t_n^2)) / 2 ;  beta = (t_n - 1) / t_{n+1}
        x+ = max(y - inv_L A^T (A y - b), 0) ;  y+ = x+ + beta (x+ - x)"""
    want = sorted({int(i) for i in np.atleast_1d(iters)})
    f = dtype
    A, Pt, mel = np.asarray(A, dtype=f), np.asarray(Pt, dtype=f), np.asarray(mel, dtype=f)
    At = A.T if At is None else np.asarray(At, dtype=f)
    b = f(10) ** ((mel * f(100) - f(100) + f(20)) / f(20))
    with _one_blas_thread():
        return _fista_loop(A, At, Pt, b, f(inv_L), want, f)


def _one_blas_thread():
    """How OpenBLAS splits a float32 product among its threads changes the last bits, and 200 iterations amplify them: the twin's
    figures are measured, and re-measured, with one thread whatever the environment says."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        import contextlib
        return contextlib.nullcontext()
    return threadpool_limits(limits=1, user_api="blas")


def _fista_loop(A, At, Pt, b, inv_L, want, f):
    pre = Pt.T @ b                                                # [..][513][T]
    x = np.maximum(pre, f(0))
    y, tn, out = x, f(1), {}
    for it in range(want[-1] + 1):
        if it in want:
            out[it] = (np.swapaxes(x, -1, -2).copy(), np.swapaxes(pre, -1, -2).copy())
        r = A @ y - b
        tnext = f(0.5) * (f(1) + np.sqrt(f(1) + f(4) * tn * tn))
        beta = (tn - f(1)) / tnext
        pre = y - inv_L * (At @ r)
        xn = np.maximum(pre, f(0))
        y = xn + beta * (xn - x)
        x, tn = xn, tnext
        assert x.dtype == f
    return out


def fista(A, Pt, mel, inv_L, iters):
    return fista_path(A, Pt, mel, inv_L, [iters])[int(iters)][0]


def fista_f32(A, Pt, mel, inv_L, iters):
    return fista_path(A, Pt, mel, inv_L, [iters], dtype=np.float32)[int(iters)][0]


def amplitude(mel):
    """b of the NNLS problem in float64: the undone log-mel normalisation, [..][n_mels][T]."""
    return 10.0 ** ((np.asarray(mel, dtype=np.float64) * 100.0 - 100.0 + 20.0) / 20.0)


# ---------------------------------------------------------------------------------------- judges
class Judgement(namedtuple("Judgement", "bad used silent")):
    """bad: per-element fail mask; used: worst |got - ref| as a fraction of the bound; silent: share of elements that tell nothing."""
    @property
    def ok(self):
        return not self.bad.any() and self.silent <= SILENT_CAP

    def __str__(self):
        where = np.argwhere(self.bad)[:4].tolist()
        return f"{int(self.bad.sum())} of {self.bad.size} elements outside the bound (first at {where}), worst used {self.used:.3g} of " \
               f"the bound, {self.silent:.2%} silent"


def _verdict(err, bound, silent=None):
    err, bound = np.broadcast_arrays(err, bound)
    listen = np.ones(err.shape, bool) if silent is None else ~silent
    bad = ~(err <= bound) & listen                                # NaN in got: err is NaN, the element fails
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    frac = np.where(np.isnan(err), np.inf, frac)[listen]
    return Judgement(bad, float(frac.max()) if frac.size else 0.0, 0.0 if silent is None else float(silent.mean()))


def _components(z):
    z = np.asarray(z, dtype=np.complex128)
    return np.stack([z.real, z.imag], -1)


def judge_init(got, phase0, K):
    return _verdict(np.abs(_components(got) - _components(init_angles(phase0))), K * EPS32)


def judge_frames(got, S, angles, window, K):
    ref, norms = synth_frames(S, angles, window)
    return _verdict(np.abs(np.asarray(got, dtype=np.float64) - ref), K * EPS32 * norms[..., None] * _win(window, np.float64))


def judge_ola(got, frames, wss, T, n=None, t0=0):
    ref, mass = overlap_add(frames, wss, T, n, t0)
    return _verdict(np.abs(np.asarray(got, dtype=np.float64) - ref), 4 * EPS32 * mass)


def judge_rebuilt(got, y, T, window, K):
    ref, norms = stft_frames(y, T, window)
    return _verdict(np.abs(_components(got) - _components(ref)), K * EPS32 * norms[..., None, None])


def judge_angles(got, rebuilt, prev, momentum, K):
    rb, pv = np.asarray(rebuilt, dtype=np.complex128), np.asarray(prev, dtype=np.complex128)
    m = momentum / (1.0 + momentum)
    num = np.abs(rb) + m * np.abs(pv)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(num > 0, num / np.abs(rb - m * pv), 0.0)
    bound = np.where(num > 0, K * EPS32 * (1.0 + ratio), 0.0)     # rebuilt = prev = 0 (a silent clip): the angle is exactly 0
    bound = np.broadcast_to(bound[..., None], bound.shape + (2,))
    return _verdict(np.abs(_components(got) - _components(angle_update(rb, pv, momentum))), bound, silent=bound >= SILENT_BOUND)


def judge_nnls(got, A, Pt, mel, inv_L, iters, K, At=None, ref=None):
    """``ref``: fista_path(...)[iters] of the same arguments, where the caller has it already."""
    x, pre = fista_path(A, Pt, mel, inv_L, [iters], At=At)[int(iters)] if ref is None else ref
    got = np.asarray(got, dtype=np.float64)
    bound = K * EPS32 * x.max(axis=-1, keepdims=True)
    j = _verdict(np.abs(got - x), bound)
    unclipped = (x == 0) & (pre < -bound) & (got != 0)            # the projection must really clip
    return Judgement(j.bad | unclipped, j.used, 0.0)


# ---------------------------------------------------------------------------------------- the seeded inputs of the GPU test
GL_SHAPES = [(2, 1), (3, 2), (4, 1), (5, 3), (17, 2), (33, 1)]      # T = 2, 3: the pad is longer than the clip; 4: one reflection
GL_KINDS = ["white", "dc_nyquist", "frame_first", "frame_last", "frame_middle", "zero_and_loud"]
GL_MOMENTA = (0.99, 0.5, 0.0)


def gl_inputs(kind, T, B):
    """-> (S [B'][T][513] float32, phase0 [B'][513][T] float32); B' = max(B, 2) for ``zero_and_loud``, else B.
    white: flat |N(0, 1)|, bin 512 weighs what bin 1 does; dc_nyquist: energy in bins 0 and 512 only; frame_*: one non-zero frame;
    zero_and_loud: clip 0 all zero, the others 1000 x white."""
    rng = np.random.default_rng([77, T, B, GL_KINDS.index(kind)])
    if kind == "zero_and_loud":
        B = max(B, 2)
    white = np.abs(rng.standard_normal((B, T, N_BIN))).astype(np.float32)
    phase0 = rng.random((B, N_BIN, T), dtype=np.float32)
    S = np.zeros_like(white)
    if kind == "white":
        S[:] = white
    elif kind == "dc_nyquist":
        S[..., 0], S[..., N_BIN - 1] = white[..., 0], white[..., N_BIN - 1]
    elif kind == "zero_and_loud":
        S[1:] = 1000.0 * white[1:]
    else:
        t = {"frame_first": 0, "frame_last": T - 1, "frame_middle": T // 2}[kind]
        S[:, t] = white[:, t]
    return S, phase0


NNLS_SHAPES = [(1, 1), (15, 2), (16, 1), (17, 3), (33, 2)]          # the kernel's tile is 16 frames
NNLS_ITERS = (0, 1, 2, 5, 20, 200)
NNLS_BANKS = ["slaney128", "slaney80", "slaney64", "slaney128_sr16000", "dense16", "zero_row", "zero_column"]
ZERO_ROW, ZERO_COLUMNS = 40, (6, 100)


@lru_cache(maxsize=None)
def nnls_bank(name):
    """-> (A float32 [n_mels][513], Pt float32 [n_mels][513] = pinv(A)^T, inv_L), the latter two as vocoder._Consts derives them.
    dense16: a dense random matrix (the kernel derives its spans from A: full ones here); zero_row / zero_column: the 128-row
    bank with row 40 / columns 6 (the lowest non-zero one) and 100 cleared: empty spans."""
    if name == "dense16":
        A = np.random.default_rng(16).standard_normal((16, N_BIN)).astype(np.float32)
    elif name == "slaney128_sr16000":
        A = ov.mel_filterbank(128, sr=16000)
    elif name in ("zero_row", "zero_column"):
        A = ov.mel_filterbank(128).copy()
        if name == "zero_row":
            A[ZERO_ROW] = 0
        else:
            assert not A[:, :ZERO_COLUMNS[0]].any() and A[:, ZERO_COLUMNS[0]].any()
            A[:, list(ZERO_COLUMNS)] = 0
    else:
        A = ov.mel_filterbank(int(name[len("slaney"):]))
    A64 = A.astype(np.float64)
    Pt = np.ascontiguousarray(np.linalg.pinv(A64).T).astype(np.float32)
    for a in (A, Pt):
        a.setflags(write=False)
    return A, Pt, float(1.0 / np.linalg.norm(A64, 2) ** 2)


def nnls_mel(bank, T, B):
    """Normalised log-mel [B][n_mels][T] float32 in [0, 1] of a decaying random spectrum, made inconsistent by multiplicative noise
    (as tests/test_vocoder_gpu.py does).  In every fourth frame (t = 1, 5, ...) about 3 % of the values sit at exactly 0.0 and 3 % at
    exactly 1.0: amplitudes of 1e-4 and 10 beside neighbours near 0.1."""
    A = nnls_bank(bank)[0].astype(np.float64)
    rng = np.random.default_rng([88, T, B, NNLS_BANKS.index(bank)])
    St = np.abs(rng.standard_normal((B, N_BIN, T))) * np.exp(-np.arange(N_BIN) / 150.0)[None, :, None]
    amp = np.einsum("mf,bft->bmt", np.abs(A), St) * np.exp(0.35 * rng.standard_normal((B, A.shape[0], T)))
    mel = np.clip((20.0 * np.log10(np.maximum(amp, 1e-4)) - 20.0 + 100.0) / 100.0, 0.0, 1.0).astype(np.float32)
    u = rng.random(mel.shape)
    edge = (np.arange(T) % 4 == 1)[None, None, :]
    mel[(u < 0.03) & edge] = 0.0
    mel[(u > 0.97) & edge] = 1.0
    return mel


OBJECTIVE_GAP = 1e-4          # of |b|: the bound of test_vocoder_gpu.test_mel_to_stft_objective_vs_exact_nnls_per_frame
OBJECTIVE_TELLS = 2.0 / 3     # share of a case's frames on which the float64 iteration itself has converged, at least


@lru_cache(maxsize=None)
def nnls_exact_residuals(bank, T, B):
    """min over x >= 0 of |A x - b| for every frame of nnls_mel(bank, T, B), from scipy.optimize.nnls (Lawson-Hanson, exact): [B][T]."""
    from scipy.optimize import nnls
    A64, b = nnls_bank(bank)[0].astype(np.float64), amplitude(nnls_mel(bank, T, B))
    return np.array([[nnls(A64, b[bi, :, t], maxiter=20000)[1] for t in range(T)] for bi in range(B)])


def objective_gaps(S, bank, T, B):
    """(|A x - b| - exact minimum) / |b| of every frame of S [B][T][513]: [B][T]; asserts that nothing beats the exact minimum."""
    A64, b = nnls_bank(bank)[0].astype(np.float64), amplitude(nnls_mel(bank, T, B))
    r = np.linalg.norm(np.einsum("mf,btf->bmt", A64, np.asarray(S, dtype=np.float64)) - b, axis=1)
    r_exact = nnls_exact_residuals(bank, T, B)
    assert (r >= r_exact * (1 - 1e-6) - 1e-9).all()
    return (r - r_exact) / np.linalg.norm(b, axis=1)


def judge_objective(got, bank, T, B, ref200):
    """The 200th iterate's objective against the exact minimum, frame by frame, at the bound the suite already uses.  200 FISTA
    iterations do not reach that bound on every frame even in float64 (measured: more than 9 plain frames in 10 do, about half of the
    frames with planted extremes).  A frame on which the float64 restatement ``ref200`` itself is not within a quarter of the bound
    tells nothing about the kernel here -- every element of it is still judged by judge_nnls -- and at least two thirds of a case's
    frames must tell.  Returns (Judgement over the frames, share of the frames that tell)."""
    ref_gap, gap = objective_gaps(ref200, bank, T, B), objective_gaps(got, bank, T, B)
    tells = ref_gap <= OBJECTIVE_GAP / 4
    j = _verdict(gap, OBJECTIVE_GAP, silent=~tells)
    share = float(tells.mean())
    return Judgement(j.bad | (share < OBJECTIVE_TELLS), j.used, 0.0), share


def nnls_objective_gap(S, A, mel):
    """Worst frame of (|A x - b| - exact minimum) / |b|, the minimum from scipy.optimize.nnls (Lawson-Hanson); also asserts that
    nothing beats the exact minimum.  S [B][T][513], mel [B][n_mels][T]."""
    from scipy.optimize import nnls
    A64, b_all = np.asarray(A, dtype=np.float64), amplitude(mel)
    worst = 0.0
    for bi in range(b_all.shape[0]):
        for t in range(b_all.shape[2]):
            b = b_all[bi, :, t]
            _, r_exact = nnls(A64, b, maxiter=20000)
            r = np.linalg.norm(A64 @ np.asarray(S[bi, t], dtype=np.float64) - b)
            assert r >= r_exact * (1 - 1e-6) - 1e-9, (bi, t, r, r_exact)
            worst = max(worst, (r - r_exact) / np.linalg.norm(b))
    return worst


# ---------------------------------------------------------------------------------------- the twins, measured in the judges' units
def measure_gl_twin(kind, T, B):
    """Runs the float32 twins as the GPU test runs the kernels -- n_iter = 2 at each momentum, every stage's float64 reference computed
    from the twin's own output of the stage before -- and returns {stage: worst error in the stage's unit} plus ``silent``, the
    worst share of angle elements that tell nothing.  The derived overlap-add bound is asserted for the twin on the way."""
    S, ph = gl_inputs(kind, T, B)
    win, wss = window32(), wss32(T)
    out = dict(init=0.0, ifft=0.0, stft=0.0, angles=0.0, silent=0.0)

    def note(stage, j):
        out[stage] = max(out[stage], j.used)
        out["silent"] = max(out["silent"], j.silent)
    a0 = init_angles_f32(ph)
    note("init", judge_init(a0, ph, 1.0))
    for mom in GL_MOMENTA:
        angles, prev = a0, np.zeros_like(a0)
        for it in range(3):
            frames = synth_frames_f32(S, angles, win)
            note("ifft", judge_frames(frames, S, angles, win, 1.0))
            assert not frames[..., 0].any()
            y = overlap_add_f32(frames, wss, T)
            j = judge_ola(y, frames, wss, T)
            assert j.ok, (kind, T, B, str(j))
            if it == 2:
                break
            rb = stft_frames_f32(y, T, win)
            note("stft", judge_rebuilt(rb, y, T, win, 1.0))
            angles = angle_update_f32(rb, prev, mom)
            note("angles", judge_angles(angles, rb, prev, mom, 1.0))
            prev = rb
    return out


def measure_nnls_twin(bank, T, B, K=None):
    """{iteration count: worst error of the float32 twin in NNLS units}.  With ``K`` ({count: bound}) the twin must also pass the
    whole judgement, the exact zeros included."""
    A, Pt, inv_L = nnls_bank(bank)
    mel = nnls_mel(bank, T, B)
    ref = fista_path(A, Pt, mel, inv_L, NNLS_ITERS)
    twin = fista_path(A, Pt, mel, inv_L, NNLS_ITERS, dtype=np.float32)
    for it in (NNLS_ITERS if K else ()):
        j = judge_nnls(twin[it][0], A, Pt, mel, inv_L, it, K[it], ref=ref[it])
        assert j.ok, (bank, T, B, it, str(j))
    return {it: judge_nnls(twin[it][0], A, Pt, mel, inv_L, it, 1.0, ref=ref[it]).used for it in NNLS_ITERS}
