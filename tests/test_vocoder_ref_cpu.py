"""CPU: the float64 restatements the vocoder kernels are judged by (tests/vocoder_ref.py) -- tied to the oracle (oracle/vocoder.py) and to
scipy's exact NNLS, the constants of tests/test_vocoder_kernels_gpu.py re-measured on that file's own inputs, and the proof that its
bounds can tell: each subtly wrong kernel below, applied to the float64 restatement and judged by the GPU test's own judge with the GPU
test's own K on its own inputs, is rejected.  PARITY UNPINNED, as everywhere around the vocoder (librosa 0.8.0 is not importable)."""
import numpy as np
import pytest

import test_vocoder_kernels_gpu as G
import vocoder_ref as R


def _norm_logmel(amp):
    return ((20.0 * np.log10(amp) - 20.0) + 100.0) / 100.0


# ---------------------------------------------------------------------------------------- the restatement against the oracle
def _compose(S, ph, n_iter, momentum=0.99):
    """The stage functions composed into griffinlim; oracle layout S, ph [513][T] -> wav."""
    T = S.shape[1]
    St, wss = S.T[None], R.wss32(T)
    angles, prev = R.init_angles(ph[None]), 0.0
    for _ in range(n_iter):
        y = R.overlap_add(R.synth_frames(St, angles)[0], wss, T)[0]
        rb = R.stft_frames(y, T)[0]
        angles, prev = R.angle_update(rb, prev, momentum), rb
    return R.overlap_add(R.synth_frames(St, angles)[0], wss, T)[0][0]


@pytest.mark.parametrize("T", [2, 3, 20])
def test_stages_composed_reproduce_the_oracle(T):
    from oracle import vocoder as ov
    rng = np.random.default_rng(6)
    if T == 20:                                   # the input of test_griffinlim_matches_oracle_sample_by_sample
        y = (np.sin(2 * np.pi * 523.25 * np.arange(256 * (T - 1)) / ov.SR) + 0.3 * rng.standard_normal(256 * (T - 1))).astype(np.float32)
        S = np.abs(ov.stft(y)).astype(np.float32)
    else:
        S = np.abs(rng.standard_normal((513, T))).astype(np.float32)
    ph = rng.random((513, T)).astype(np.float32)
    for n_iter in (0, 1):
        ref = ov.griffinlim(S, ph, n_iter=n_iter)
        got = _compose(S, ph, n_iter)
        assert got.shape == ref.shape == (256 * (T - 1),)
        e = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print(f"T = {T}, n_iter = {n_iter}: restatement vs oracle rel-L2 {e:.2e}")
        assert e < 1e-4                           # the oracle rounds to complex64 / float32 on the way


def test_tables_are_the_hosts():
    from diff_foley_amd import vocoder as V
    for T in (2, 5, 33):
        c = V._Consts(8, T, "cpu")
        assert np.array_equal(c.window.numpy().view(np.uint32), R.window32().view(np.uint32))
        assert np.array_equal(c.wss.numpy().view(np.uint32), R.wss32(T).view(np.uint32))
    A, Pt, inv_L = R.nnls_bank("slaney80")
    c = V._Consts(80, 4, "cpu")
    assert np.array_equal(c.A.numpy(), A) and np.array_equal(c.Pt.numpy(), Pt) and c.inv_L == inv_L
    assert np.array_equal(R.nnls_bank("slaney128_sr16000")[0], V._Consts(128, 4, "cpu", sr=16000).A.numpy())


def test_fista_reaches_the_exact_nnls_objective():
    """The setup of test_vocoder_gpu.test_mel_to_stft_objective_vs_exact_nnls_per_frame, the restatement in the engine's place."""
    from oracle import vocoder as ov
    rng = np.random.default_rng(11)
    A = ov.mel_filterbank(128)
    T = 16
    St = np.abs(rng.standard_normal((1, 513, T))) * np.exp(-np.arange(513) / 150.0)[None, :, None]
    amp = np.einsum("mf,bft->bmt", A.astype(np.float64), St) * np.exp(0.35 * rng.standard_normal((1, 128, T)))
    mel = _norm_logmel(np.maximum(amp, 1e-4).astype(np.float32)).astype(np.float32)
    _, Pt, inv_L = R.nnls_bank("slaney128")
    x = R.fista(A, Pt, mel, inv_L, 200)
    assert x.shape == (1, T, 513) and (x >= 0).all()
    gap = R.nnls_objective_gap(x, A, mel)
    print(f"float64 FISTA-200, objective gap to scipy's exact NNLS: {gap:.2e} of |b|")
    assert gap < R.OBJECTIVE_GAP
    assert np.array_equal(R.fista_f32(A, Pt, mel, inv_L, 3), R.fista_path(A, Pt, mel, inv_L, [3], dtype=np.float32)[3][0])


def test_fista_descends_with_a_dense_matrix():
    """Strictly down while the objective is large; FISTA's momentum is not a descent method, so once the objective has fallen by
    six orders it may ripple: measured 5e-7 of the start at iteration 10, allowed 1e-5.  16 equations in 513 unknowns: the minimum is 0."""
    A, Pt, inv_L = R.nnls_bank("dense16")
    mel = R.nnls_mel("dense16", 16, 1)
    path = R.fista_path(A, Pt, mel, inv_L, range(201))
    b = R.amplitude(mel)
    obj = np.array([np.sum((A.astype(np.float64) @ np.swapaxes(path[i][0], -1, -2) - b) ** 2) for i in range(201)])
    assert (np.diff(obj[:10]) < 0).all() and obj[9] < 1e-4 * obj[0]
    assert (np.diff(obj) <= 1e-5 * obj[0]).all(), np.argwhere(np.diff(obj) > 1e-5 * obj[0])[:4]
    assert obj[200] < 1e-12 * obj[0]


# ---------------------------------------------------------------------------------------- the constants
@pytest.mark.parametrize("kind", R.GL_KINDS)
def test_float32_twins_stay_within_a_quarter_of_the_griffinlim_bounds(kind):
    for T, B in R.GL_SHAPES:
        m = R.measure_gl_twin(kind, T, B)
        for stage, k in G.K_GL[kind].items():
            assert m[stage] <= k / 4, (kind, T, B, stage, m[stage], k / 4)
        assert m["silent"] <= R.SILENT_CAP, (kind, T, B, m["silent"])


@pytest.mark.parametrize("bank", R.NNLS_BANKS)
def test_float32_twin_stays_within_a_quarter_of_the_nnls_bounds(bank):
    for T, B in R.NNLS_SHAPES:
        m = R.measure_nnls_twin(bank, T, B, K=G.K_NNLS[bank])
        for it in R.NNLS_ITERS:
            assert m[it] <= G.K_NNLS[bank][it] / 4, (bank, T, B, it, m[it], G.K_NNLS[bank][it] / 4)


@pytest.mark.parametrize("bank", R.NNLS_BANKS)
def test_objective_judge_on_the_gpu_tests_inputs(bank):
    """On enough frames of the GPU test's inputs the float64 iteration has converged to a quarter of the objective bound, and the
    judge built on those frames rejects an iterate that has not: the 20th (the 5th with the dense matrix, whose minimum is 0)."""
    A, Pt, inv_L = R.nnls_bank(bank)
    T, B = 15, 2
    early = 5 if bank == "dense16" else 20
    path = R.fista_path(A, Pt, R.nnls_mel(bank, T, B), inv_L, [early, 200])
    j, share = R.judge_objective(path[200][0], bank, T, B, path[200][0])
    print(f"{bank}: {share:.0%} of the frames tell, the float64 iterate uses {j.used:.3f} of the bound")
    assert j.ok and share >= R.OBJECTIVE_TELLS and j.used <= 0.25
    assert not R.judge_objective(path[early][0], bank, T, B, path[200][0])[0].ok


# ---------------------------------------------------------------------------------------- the bounds can tell: Griffin-Lim
@pytest.fixture(scope="module")
def chain():
    """T, B -> the float64 pipeline on the GPU test's white input: what each stage is handed and what it gives."""
    def make(T, B):
        S, ph = R.gl_inputs("white", T, B)
        win, wss = R.window32(), R.wss32(T)
        c = dict(S=S, ph=ph, win=win, wss=wss, T=T, ang0=R.init_angles(ph))
        c["fr0"] = R.synth_frames(S, c["ang0"], win)[0]
        c["y0"] = R.overlap_add(c["fr0"], wss, T)[0]
        c["rb1"] = R.stft_frames(c["y0"], T, win)[0]
        c["ang1"] = R.angle_update(c["rb1"], 0.0, 0.99)
        c["y1"] = R.overlap_add(R.synth_frames(S, c["ang1"], win)[0], wss, T)[0]
        c["rb0"] = R.stft_frames(c["y1"], T, win)[0]
        return c
    return {tb: make(*tb) for tb in [(2, 1), (3, 2), (5, 3)]}


def _irfft_packed(spec):
    """irfft(n = 1024) as one 512-point complex transform of z[n] = x[2n] + i x[2n+1] (the halving wave_to_mel_kernel uses forwards).
    It does NOT ignore the imaginary parts of DC and Nyquist: they leak into Z[0]."""
    k = np.arange(512)
    Xk, Xc = spec[..., :512], np.conj(spec[..., 512:0:-1])
    Z = 0.5 * (Xk + Xc) + 0.5j * (Xk - Xc) * np.exp(2j * np.pi * k / 1024)
    z = np.fft.ifft(Z, axis=-1)
    return np.stack([z.real, z.imag], -1).reshape(spec.shape[:-1] + (1024,))


def _ifft_mutants(c):
    spec = c["S"].astype(np.float64) * c["ang0"]
    clean = spec.copy()
    clean[..., 0], clean[..., 512] = clean[..., 0].real, clean[..., 512].real
    assert np.abs(_irfft_packed(clean) - np.fft.irfft(clean, n=1024, axis=-1)).max() < 1e-12
    out = {}
    m = clean.copy()
    m[..., 512] = 0
    out["nyquist bin dropped"] = np.fft.irfft(m, n=1024, axis=-1)
    m = clean.copy()
    m[..., 512] = spec[..., 512]
    out["nyquist imaginary part kept"] = _irfft_packed(m)
    m = clean.copy()
    m[..., 0] = spec[..., 0]
    out["dc imaginary part kept"] = _irfft_packed(m)
    full = np.concatenate([clean, clean[..., 511:0:-1]], -1)         # the upper half without the conjugation
    out["conjugate half with the wrong sign"] = np.fft.ifft(full, axis=-1).real
    return {k: v * c["win"].astype(np.float64) for k, v in out.items()}


def test_bounds_reject_wrong_inverse_transforms(chain):
    c = chain[(5, 3)]
    K = G.K_GL["white"]["ifft"]
    assert R.judge_frames(c["fr0"], c["S"], c["ang0"], c["win"], K).ok
    assert R.judge_frames(c["fr0"].astype(np.float32), c["S"], c["ang0"], c["win"], K).ok
    for name, frames in _ifft_mutants(c).items():
        j = R.judge_frames(frames, c["S"], c["ang0"], c["win"], K)
        print(f"{name}: {j}")
        assert not j.ok, name
    nan = c["fr0"].copy()
    nan[1, 2, 700] = np.nan                                           # an element left unwritten
    assert not R.judge_frames(nan, c["S"], c["ang0"], c["win"], K).ok


def _stft_with_index(y, T, win, index):
    """STFT of y [B][L] whose padded signal is y[index(i)] for i in [-512, L + 512)."""
    L = y.shape[-1]
    yp = y[..., index(np.arange(-512, L + 512), L)]
    idx = 256 * np.arange(T)[:, None] + np.arange(1024)[None, :]
    return np.fft.rfft(yp[..., idx] * win.astype(np.float64), axis=-1)


def _reflect_once(i, L):                  # each end mirrored a single time; what still lies outside is clamped
    i = np.where(i < 0, -i, np.where(i >= L, 2 * (L - 1) - i, i))
    return np.clip(i, 0, L - 1)


def _symmetric(i, L):                     # the edge sample repeated: period 2 L
    i = np.mod(i, 2 * L)
    return np.where(i >= L, 2 * L - 1 - i, i)


def test_bounds_reject_wrong_padding(chain):
    K = G.K_GL["white"]["stft"]
    for tb, c in chain.items():
        y, T = c["y0"], c["T"]
        assert R.judge_rebuilt(c["rb1"], y, T, c["win"], K).ok
        assert not R.judge_rebuilt(_stft_with_index(y, T, c["win"], _symmetric), y, T, c["win"], K).ok, ("symmetric", tb)
    c = chain[(2, 1)]
    j = R.judge_rebuilt(_stft_with_index(c["y0"], 2, c["win"], _reflect_once), c["y0"], 2, c["win"], K)
    print(f"single reflection, T = 2: {j}")
    assert not j.ok


def test_single_reflection_at_three_frames():
    """At T = 3 the clip is exactly as long as the pad: a single reflection goes wrong in ONE sample per side, padded index -512 (under
    window[0] = 0: no weight at all) and L + 511 (under window[1023] = 9.4e-6).  On a white waveform that is 0.3 of the round-off bound:
    no float32 comparison can see it, here or on the GPU.  It is seen where the clip's second sample carries weight, so that is
    the input this mutant is judged on."""
    win, T, L = R.window32(), 3, 512
    y = np.random.default_rng(3).standard_normal((2, L))
    wrong = _reflect_once(np.arange(-512, L + 512), L) != np.pad(np.arange(L), 512, mode="reflect")
    assert np.flatnonzero(wrong).tolist() == [0, L + 1023]
    y[:, 1] = 1000.0
    K = G.K_GL["white"]["stft"]
    assert R.judge_rebuilt(R.stft_frames(y, T, win)[0], y, T, win, K).ok
    j = R.judge_rebuilt(_stft_with_index(y, T, win, _reflect_once), y, T, win, K)
    print(f"single reflection, T = 3, a loud second sample: {j}")
    assert not j.ok


def _ola_mutant(frames, wss, T, drop=None, offset=512):
    n = np.arange(256 * (T - 1))
    pos = n + 512
    acc = np.zeros(frames.shape[:-2] + n.shape)
    ts = [pos // 256 - j for j in (3, 2, 1, 0)]
    valid = [(t >= 0) & (t <= T - 1) for t in ts]
    first = np.argmax(np.stack(valid), 0)                              # which of the four is the first / last covering frame
    last = 3 - np.argmax(np.stack(valid[::-1]), 0)
    for i, (t, ok) in enumerate(zip(ts, valid)):
        keep = ok & ~((drop == "first") & (first == i)) & ~((drop == "last") & (last == i))
        acc += frames[..., np.where(ok, t, 0), pos - 256 * t] * keep
    with np.errstate(divide="ignore", invalid="ignore"):               # wss[0] = 0 without the offset
        return acc / wss[n + offset].astype(np.float64)


def test_bounds_reject_wrong_overlap_adds(chain):
    for tb, c in chain.items():
        fr, wss, T = c["fr0"], c["wss"], c["T"]
        assert R.judge_ola(c["y0"], fr, wss, T).ok and R.judge_ola(c["y0"].astype(np.float32), fr, wss, T).ok
        assert R.judge_ola(_ola_mutant(fr, wss, T), fr, wss, T).ok                 # the mutant's own form, unmutated
        for kw in (dict(drop="first"), dict(drop="last"), dict(offset=0)):
            j = R.judge_ola(_ola_mutant(fr, wss, T, **kw), fr, wss, T)
            assert not j.ok, (tb, kw)
        y = c["y0"].copy()
        y[..., -1] = y[..., -2]                                           # the last sample of a clip
        j = R.judge_ola(y, fr, wss, T)
        assert not j.ok and j.bad.sum() == y.shape[0]
        y = c["y0"].copy()
        y[-1, -1] = np.nan
        assert not R.judge_ola(y, fr, wss, T).ok


def test_bounds_reject_wrong_angle_updates(chain):
    K = G.K_GL["white"]["angles"]
    for tb, c in chain.items():
        rb0, rb1 = c["rb0"], c["rb1"]
        for mom in (0.99, 0.5):
            m = mom / (1 + mom)
            assert R.judge_angles(R.angle_update(rb0, rb1, mom), rb0, rb1, mom, K).ok
            a = rb0 - mom * rb1
            assert not R.judge_angles(a / (np.abs(a) + 1e-16), rb0, rb1, mom, K).ok, ("momentum in place of m / (1 + m)", tb)
            assert not R.judge_angles(R.angle_update(rb0, 0.0, mom), rb0, rb1, mom, K).ok, ("prev and cur not swapped", tb)
            assert not R.judge_angles(rb0 - m * rb1, rb0, rb1, mom, K).ok, ("not renormalised", tb)
        # prev and cur not swapped, the buffers at n_iter = 2: reb0 still holds the memset, reb1 the second STFT
        assert not R.judge_rebuilt(np.zeros_like(rb0), c["y1"], c["T"], c["win"], G.K_GL["white"]["stft"]).ok
        assert not R.judge_init(np.conj(c["ang0"]), c["ph"], G.K_GL["white"]["init"]).ok
        assert R.judge_init(R.init_angles_f32(c["ph"]), c["ph"], G.K_GL["white"]["init"]).ok


def test_an_angle_that_tells_nothing_is_counted_not_judged():
    rb = np.full((1, 1, 2000), 1.0 + 0.0j)
    pv = np.zeros_like(rb)
    pv[..., :3] = (1.0 + 1e-9) / (0.99 / 1.99)                        # a = rb - m prev cancels to 1e-9 of rb: bound above 0.1
    got = R.angle_update(rb, pv, 0.99)
    got[..., :3] = 1j                                                 # anything
    j = R.judge_angles(got, rb, pv, 0.99, 8.0)
    assert not j.bad.any() and j.silent == 3 / 2000 and not j.ok      # 0.15 % silent: over the cap
    pv[..., 2] = 0
    got[..., 2] = 1.0
    j = R.judge_angles(got, rb, pv, 0.99, 8.0)
    assert j.ok and j.silent == 2 / 2000
    z = np.zeros_like(rb)
    assert R.judge_angles(z, z, z, 0.99, 8.0).ok and not R.judge_angles(z + 1e-30, z, z, 0.99, 8.0).ok   # silence: exactly 0


# ---------------------------------------------------------------------------------------- the bounds can tell: NNLS
def _fista_mutant(A, Pt, mel, inv_L, iters, clip_start=True, beta_from_tnext=False, A_res=None, At_grad=None):
    A = np.asarray(A, np.float64)
    A_res = A if A_res is None else A_res
    At_grad = A.T if At_grad is None else At_grad
    b = R.amplitude(mel)
    x = Pt.astype(np.float64).T @ b
    if clip_start:
        x = np.maximum(x, 0)
    y, tn = x, 1.0
    for _ in range(iters):
        tnext = 0.5 * (1 + np.sqrt(1 + 4 * tn * tn))
        beta = (tnext - 1) / tnext if beta_from_tnext else (tn - 1) / tnext
        xn = np.maximum(y - inv_L * (At_grad @ (A_res @ y - b)), 0)
        y, x, tn = xn + beta * (xn - x), xn, tnext
    return np.swapaxes(x, -1, -2)


def _short_spans(A, axis, end):
    """A with the first (end = 0) or last (end = -1) non-zero of every row (axis = 1) / column (axis = 0) cleared."""
    out = A.astype(np.float64).copy()
    M = out if axis == 1 else out.T
    for row in M:
        nz = np.flatnonzero(row)
        if nz.size:
            row[nz[end]] = 0
    return out


def test_bounds_reject_wrong_nnls_iterations():
    bank, T, B = "slaney128", 17, 3
    A, Pt, inv_L = R.nnls_bank(bank)
    mel = R.nnls_mel(bank, T, B)
    ref = R.fista_path(A, Pt, mel, inv_L, R.NNLS_ITERS)

    def judge(got, it):
        return R.judge_nnls(got, A, Pt, mel, inv_L, it, G.K_NNLS[bank][it], ref=ref[it])
    for it in R.NNLS_ITERS:
        same = _fista_mutant(A, Pt, mel, inv_L, it)                                        # the mutant's own form, unmutated
        assert np.abs(same - ref[it][0]).max() <= 1e-9 * ref[it][0].max() and judge(same, it).ok
        assert judge(ref[it][0].astype(np.float32), it).ok
    mutants = {
        "start not clipped": (dict(clip_start=False), (0, 1, 2, 5)),
        "beta from t_{n+1} alone": (dict(beta_from_tnext=True), (2, 5, 20)),
        "row spans short at the low end": (dict(A_res=_short_spans(A, 1, 0)), (1, 2, 5, 20, 200)),
        "row spans short at the high end": (dict(A_res=_short_spans(A, 1, -1)), (1, 2, 5, 20, 200)),
        "column spans short at the low end": (dict(At_grad=_short_spans(A, 0, 0).T), (1, 2, 5, 20, 200)),
        "column spans short at the high end": (dict(At_grad=_short_spans(A, 0, -1).T), (1, 2, 5, 20, 200)),
    }
    for name, (kw, its) in mutants.items():
        for it in its:
            j = judge(_fista_mutant(A, Pt, mel, inv_L, it, **kw), it)
            print(f"{name}, iters = {it}: {j}")
            assert not j.ok, (name, it)
    for it in R.NNLS_ITERS:
        x = ref[it][0]
        assert not judge(np.concatenate([x[:1], x[:1], x[2:]]), it).ok, "clip 1 of a batch reading clip 0's mel"
        leak = x.copy()
        hit = (x == 0) & (ref[it][1] < -1e-3 * x.max(-1, keepdims=True))
        assert hit.any()
        leak[tuple(np.argwhere(hit)[0])] = 1e-30                                           # the projection did not clip
        assert not judge(leak, it).ok
    # a ragged last tile (15 of 16 frames) whose frames are shifted by one
    bank, T, B = "slaney128", 15, 2
    mel = R.nnls_mel(bank, T, B)
    for it in R.NNLS_ITERS:
        r = R.fista_path(A, Pt, mel, inv_L, [it])[it]
        shifted = r[0][:, np.minimum(np.arange(T) + 1, T - 1)]
        assert R.judge_nnls(r[0], A, Pt, mel, inv_L, it, G.K_NNLS[bank][it], ref=r).ok
        assert not R.judge_nnls(shifted, A, Pt, mel, inv_L, it, G.K_NNLS[bank][it], ref=r).ok
