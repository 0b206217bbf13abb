"""GPU: every mel -> waveform kernel of csrc/vocoder.hip (nnls_fista_kernel, gl_init_angles_kernel, gl_ifft_kernel, gl_ola_kernel,
gl_stft_kernel) element by element against the float64 restatements of tests/vocoder_ref.py.  PARITY UNPINNED: librosa 0.8.0 is not
importable here (see the header of oracle/vocoder.py); the yardstick is the restatement, which tests/test_vocoder_ref_cpu.py ties to
the oracle.

The tests call df_griffinlim / df_mel_to_stft with buffers of their own, pre-filled with NaN (an element left unwritten is seen), and
stop the pipeline after n_iter = 0, 1, 2.  A stage's reference is computed from the DEVICE's output of the stage before, read back and
widened to float64: no stage is blamed for its predecessor's round-off, nothing is amplified across iterations.  Units and judges:
the header of vocoder_ref.py.

No constant comes from the kernel.  K of a stage = 4 x the worst error of the float32 CPU twin against float64 (vocoder_ref.*_f32:
scipy's float32 pocketfft, float32 accumulation on one BLAS thread), in the stage's unit, on this file's own inputs, every shape and
momentum; the factor 4: ten radix-2 stages with fp32 table twiddles round more often than pocketfft, fma contraction and rsqrt /
exp10f differ.  The overlap-add bound is derived (three additions, one division), not measured.  tests/test_vocoder_ref_cpu.py
re-measures the twins against K / 4 and shows that the bounds reject a list of subtly wrong kernels.

Twin, worst over the shapes, in the stage's unit (rounded up; K = 4 x), and beside it the share of the bound K that the kernels used
on an MI355X (worst element of every shape, n_iter and momentum):

    Griffin-Lim input   init angles     gl_ifft         gl_stft rebuilt   gl_stft angles    gl_ola (derived bound)
    white               6.89   0.030    0.423  0.273    7.34   0.296      1.54   0.201             0.724
    dc_nyquist          6.93   0.030    0.101  0.248    50.8   0.207      1.74   0.213             0.726
    frame_first         6.93   0.029    0.372  0.339    7.23   0.284      1.55   0.203             0.249
    frame_last          6.92   0.031    0.383  0.336    6.50   0.356      1.45   0.198             0.248
    frame_middle        6.97   0.030    0.383  0.366    6.69   0.421      1.48   0.202             0.246
    zero_and_loud       6.93   0.030    0.471  0.291    8.34   0.270      1.54   0.196             0.717
    grid stride (K of white)   0.031                                                               0.756
    (no input of the twin has an angle element that tells nothing; the cap of 0.1 % is asserted on the kernels' inputs as well)

    NNLS bank           iters 0         1               2               5               20              200            objective
    slaney128           10.9   0.174    8.01   0.200    7.91   0.203    7.32   0.250    19.2   0.250    1380   0.226   0.224
    slaney80            9.66   0.250    9.78   0.232    8.91   0.250    8.60   0.282    18.2   0.249    1510   0.218   0.138
    slaney64            9.99   0.250    8.67   0.250    8.63   0.243    8.60   0.249    20.2   0.208    2070   0.236   0.097
    slaney128_sr16000   9.01   0.246    8.21   0.246    8.84   0.230    8.65   0.216    26.7   0.249    1590   0.253   0.193
    dense16             2.53   0.250    2.45   0.201    2.57   0.223    4.55   0.223    16.9   0.404    1550   0.249   0.005
    zero_row            9.22   0.250    7.90   0.241    7.96   0.240    8.92   0.217    19.5   0.206    1270   0.287   0.209
    zero_column         8.77   0.249    8.61   0.216    8.96   0.211    9.72   0.201    17.3   0.225    1160   0.320   0.243
    (objective: the 200th iterate's gap to scipy's exact NNLS as a share of 1e-4 |b|, on the frames where the float64 iteration
    itself has converged -- vocoder_ref.judge_objective; at least 75 % of a case's frames were such)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import vocoder_ref as R

pytestmark = pytest.mark.gpu

TWIN_GL = {
    "white": dict(init=6.89, ifft=0.423, stft=7.34, angles=1.54),
    "dc_nyquist": dict(init=6.93, ifft=0.101, stft=50.8, angles=1.74),
    "frame_first": dict(init=6.93, ifft=0.372, stft=7.23, angles=1.55),
    "frame_last": dict(init=6.92, ifft=0.383, stft=6.5, angles=1.45),
    "frame_middle": dict(init=6.97, ifft=0.383, stft=6.69, angles=1.48),
    "zero_and_loud": dict(init=6.93, ifft=0.471, stft=8.34, angles=1.54),
}
TWIN_NNLS = {
    "slaney128": {0: 10.9, 1: 8.01, 2: 7.91, 5: 7.32, 20: 19.2, 200: 1380},
    "slaney80": {0: 9.66, 1: 9.78, 2: 8.91, 5: 8.6, 20: 18.2, 200: 1510},
    "slaney64": {0: 9.99, 1: 8.67, 2: 8.63, 5: 8.6, 20: 20.2, 200: 2070},
    "slaney128_sr16000": {0: 9.01, 1: 8.21, 2: 8.84, 5: 8.65, 20: 26.7, 200: 1590},
    "dense16": {0: 2.53, 1: 2.45, 2: 2.57, 5: 4.55, 20: 16.9, 200: 1550},
    "zero_row": {0: 9.22, 1: 7.9, 2: 7.96, 5: 8.92, 20: 19.5, 200: 1270},
    "zero_column": {0: 8.77, 1: 8.61, 2: 8.96, 5: 9.72, 20: 17.3, 200: 1160},
}
K_GL = {kind: {stage: 4 * v for stage, v in row.items()} for kind, row in TWIN_GL.items()}
K_NNLS = {bank: {it: 4 * v for it, v in row.items()} for bank, row in TWIN_NNLS.items()}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nan(*shape, dev=None):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev or torch.device("cuda", torch.cuda.current_device()))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Used(dict):
    """stage -> worst used fraction of its bound within one test; printed for the header's table."""
    def take(self, stage, j, what):
        assert j.ok, f"{what}, {stage}: {j}"
        self[stage] = max(self.get(stage, 0.0), j.used)

    def show(self, what):
        print("USED", what, " ".join(f"{k}={v:.3f}" for k, v in self.items()))


# ---------------------------------------------------------------------------------------- Griffin-Lim
def _gl_call(S, ph, n_iter, momentum, bufs=None):
    """df_griffinlim on device tensors S [B][T][513], ph [B][513][T] into NaN-filled buffers of this test's own."""
    from diff_foley_amd import engine as E, vocoder as V
    B, T, _ = S.shape
    c = V._get_consts(128, T, S.device)
    if bufs is None:
        bufs = dict(angles=_nan(B, T, R.N_BIN, 2), reb0=_nan(B, T, R.N_BIN, 2), reb1=_nan(B, T, R.N_BIN, 2), frames=_nan(B, T, R.N_FFT),
                    wav=_nan(B, R.HOP * (T - 1)))
    lib = E.lib()
    E._chk(lib.df_griffinlim(_p(S), _p(ph), B, T, n_iter, momentum, _p(c.tw), _p(c.window), _p(c.wss), _p(bufs["angles"]),
                             _p(bufs["reb0"]), _p(bufs["reb1"]), _p(bufs["frames"]), _p(bufs["wav"]), E._stream()), lib)
    torch.cuda.synchronize()
    return bufs


def _gl(S, ph, n_iter, momentum):
    return {k: v.cpu().numpy() for k, v in _gl_call(S, ph, n_iter, momentum).items()}


@pytest.fixture(scope="module")
def tables():
    """The window and the sum-squares the kernels are handed, read back: float32 tables the host builds (vocoder._Consts)."""
    from diff_foley_amd import vocoder as V
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    for T in sorted({T for T, _ in R.GL_SHAPES}):
        c = V._get_consts(128, T, dev)
        win, wss = c.window.cpu().numpy(), c.wss.cpu().numpy()
        assert np.array_equal(_bits(win), _bits(R.window32())) and np.array_equal(_bits(wss), _bits(R.wss32(T)))
        out[T] = (win, wss)
    return out


@pytest.mark.parametrize("kind", R.GL_KINDS)
@pytest.mark.parametrize("T,B", R.GL_SHAPES)
def test_griffinlim_stage_by_stage(tables, T, B, kind):
    S_h, ph_h = R.gl_inputs(kind, T, B)
    S, ph = torch.from_numpy(S_h).cuda(), torch.from_numpy(ph_h).cuda()
    win, wss = tables[T]
    K, used, what = K_GL[kind], _Used(), f"{kind} T={T} B={S_h.shape[0]}"
    zero_clip = kind == "zero_and_loud"

    def tail(o, tag):                    # gl_ifft from the device's angles, gl_ola from the device's frames
        used.take("ifft", R.judge_frames(o["frames"], S_h, R.as_complex(o["angles"]), win, K["ifft"]), f"{what} {tag}")
        assert not o["frames"][..., 0].any(), f"{what} {tag}: window[0] = 0, sample 0 of a frame is exactly 0"
        used.take("ola", R.judge_ola(o["wav"], o["frames"], wss, T), f"{what} {tag}")
        if zero_clip:
            assert not o["frames"][0].any() and not o["wav"][0].any() and np.abs(o["wav"][1:]).max() > 1.0

    # n_iter = 0: the init angles, frames, wav; rebuilt = 0.0 before the first iteration; reb1 untouched
    o0 = _gl(S, ph, 0, 0.99)
    again = _gl(S, ph, 0, 0.99)
    for k in o0:
        assert np.array_equal(_bits(o0[k]), _bits(again[k])), f"{what}: {k} differs between two n_iter = 0 runs"
    used.take("init", R.judge_init(R.as_complex(o0["angles"]), ph_h, K["init"]), f"{what} n_iter=0")
    assert not _bits(o0["reb0"]).any() and np.isnan(o0["reb1"]).all()
    tail(o0, "n_iter=0")

    # n_iter = 1: reb1 = STFT(wav of the n_iter = 0 call), first update against prev = 0
    o1 = _gl(S, ph, 1, 0.99)
    used.take("stft", R.judge_rebuilt(R.as_complex(o1["reb1"]), o0["wav"], T, win, K["stft"]), f"{what} n_iter=1")
    assert not _bits(o1["reb0"]).any()
    zeros = np.zeros(o1["reb1"].shape[:-1])
    used.take("angles", R.judge_angles(R.as_complex(o1["angles"]), R.as_complex(o1["reb1"]), zeros, 0.99, K["angles"]), f"{what} n_iter=1")
    tail(o1, "n_iter=1")

    # n_iter = 2: reb0 = STFT(wav of the n_iter = 1 call) with reb1 kept: the second update and the buffer swap
    for mom in R.GL_MOMENTA:
        o2, tag = _gl(S, ph, 2, mom), f"n_iter=2 momentum={mom}"
        assert np.array_equal(_bits(o2["reb1"]), _bits(o1["reb1"])), f"{what} {tag}: reb1 is not the first iteration's STFT"
        used.take("stft", R.judge_rebuilt(R.as_complex(o2["reb0"]), o1["wav"], T, win, K["stft"]), f"{what} {tag}")
        used.take("angles", R.judge_angles(R.as_complex(o2["angles"]), R.as_complex(o2["reb0"]), R.as_complex(o2["reb1"]), mom,
                                           K["angles"]), f"{what} {tag}")
        if zero_clip:
            assert not _bits(np.abs(o2["angles"][0])).any() and not _bits(np.abs(o2["reb0"][0])).any()
        tail(o2, tag)
    used.show(what)


def _segments(lo, hi, per_clip):
    """Flat element range [lo, hi) of a [B][per_clip] buffer -> (clip, first, end) pieces."""
    out = []
    while lo < hi:
        b, n0 = divmod(lo, per_clip)
        n1 = min(per_clip, n0 + hi - lo)
        out.append((b, n0, n1))
        lo += n1 - n0
    return out


def test_grid_stride_second_pass():
    """gl_init_angles and gl_ola cap their grids at 65535 blocks of 256 and stride: B = 2, T = 32770 reaches the second pass of both
    (about 1.4 GB of device buffers).  Judged on the first and last 2^20 elements of angles and wav and 4096 on either side of
    element 65535 * 256, the reference built for those slices only."""
    from diff_foley_amd import vocoder as V
    B, T, span, edge = 2, 32770, 1 << 20, 65535 * 256
    dev = torch.device("cuda", torch.cuda.current_device())
    L, nspec = R.HOP * (T - 1), B * T * R.N_BIN
    assert nspec > edge + 4096 and B * L > edge                  # both kernels need a second pass
    g = torch.Generator(device=dev).manual_seed(9)
    S = torch.rand(B, T, R.N_BIN, device=dev, generator=g)
    ph = torch.rand(B, R.N_BIN, T, device=dev, generator=g)
    key = (128, T, dev, V.SR)
    try:
        o = _gl_call(S, ph, 0, 0.99)
        wss = V._get_consts(128, T, dev).wss.cpu().numpy()
    finally:
        V._consts.pop(key, None)
    assert np.array_equal(_bits(wss), _bits(R.wss32(T)))
    used = _Used()
    ang = o["angles"].view(-1, 2)
    for lo, hi in ((0, span), (nspec - span, nspec), (edge - 4096, edge + 4096)):
        e = np.arange(lo, hi)
        k, bt = e % R.N_BIN, e // R.N_BIN
        idx = torch.from_numpy((bt // T * R.N_BIN + k) * T + bt % T).to(dev)
        u = ph.view(-1)[idx].cpu().numpy()
        got = R.as_complex(ang[lo:hi].cpu().numpy())
        used.take("init", R.judge_init(got[:, None, None], u[:, None, None], K_GL["white"]["init"]), f"angles[{lo}:{hi}]")
    for lo, hi in ((0, span), (B * L - span, B * L), (edge - 4096, min(edge + 4096, B * L))):
        for b, n0, n1 in _segments(lo, hi, L):
            tlo, thi = max((n0 + 512) // R.HOP - 3, 0), min((n1 - 1 + 512) // R.HOP, T - 1)
            fr = o["frames"][b, tlo:thi + 1].cpu().numpy()
            assert not np.isnan(fr).any()
            got = o["wav"][b, n0:n1].cpu().numpy()
            used.take("ola", R.judge_ola(got, fr, wss, T, n=np.arange(n0, n1), t0=tlo), f"wav[{b}][{n0}:{n1}]")
    used.show("grid stride B=2 T=32770")


# ---------------------------------------------------------------------------------------- NNLS
def _nnls_call(mel, A, Pt, inv_L, iters, dev):
    from diff_foley_amd import engine as E
    B, NM, T = mel.shape
    mel_d, A_d, At_d, Pt_d = (torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(dev) for a in (mel, A, A.T, Pt))
    S = _nan(B, T, R.N_BIN, dev=dev)
    lib = E.lib()
    with torch.cuda.device(dev):                  # the operands stay referenced until the launch has finished
        E._chk(lib.df_mel_to_stft(_p(mel_d), B, NM, T, _p(A_d), _p(At_d), _p(Pt_d), inv_L, iters, _p(S), E._stream()), lib)
        torch.cuda.synchronize()
    return S.cpu().numpy()


def _nnls_case(bank, T, B, dev, iters=R.NNLS_ITERS):
    A, Pt, inv_L = R.nnls_bank(bank)
    mel = R.nnls_mel(bank, T, B)
    assert mel.min() >= 0 and mel.max() <= 1 and (mel.size < 1000 or ((mel == 0.0).any() and (mel == 1.0).any()))
    ref = R.fista_path(A, Pt, mel, inv_L, iters)
    used, what = _Used(), f"{bank} T={T} B={B} {dev}"
    for it in iters:
        S = _nnls_call(mel, A, Pt, inv_L, it, dev)
        used.take(f"iters{it}", R.judge_nnls(S, A, Pt, mel, inv_L, it, K_NNLS[bank][it], ref=ref[it]), f"{what} iters={it}")
        if it == 200:
            j, share = R.judge_objective(S, bank, T, B, ref[it][0])
            print(f"{what}: objective gap to scipy's exact NNLS, {share:.0%} of the frames tell")
            used.take("objective", j, f"{what} iters={it}")
    used.show(what)


@pytest.mark.parametrize("bank", R.NNLS_BANKS)
@pytest.mark.parametrize("T,B", R.NNLS_SHAPES)
def test_nnls_every_element_of_every_iterate(T, B, bank):
    _nnls_case(bank, T, B, torch.device("cuda", torch.cuda.current_device()))


def test_nnls_banks_have_the_spans_they_claim():
    A = R.nnls_bank("zero_row")[0]
    assert not A[R.ZERO_ROW].any() and A[R.ZERO_ROW - 1].any()
    A = R.nnls_bank("zero_column")[0]
    assert not A[:, list(R.ZERO_COLUMNS)].any() and A[:, R.ZERO_COLUMNS[1] - 1].any() and A[:, R.ZERO_COLUMNS[1] + 1].any()
    assert np.count_nonzero(R.nnls_bank("dense16")[0]) == 16 * R.N_BIN


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible devices")
def test_nnls_on_a_second_device_of_the_same_process():
    """launch_mel_to_stft raises the kernel's dynamic-LDS limit (82 KB) once and remembers that it did: the first call on another
    device of the same process must launch as well."""
    _nnls_case("slaney128", 17, 3, torch.device("cuda", 0), iters=(200,))
    _nnls_case("slaney128", 17, 3, torch.device("cuda", 1), iters=(200,))


# ---------------------------------------------------------------------------------------- refusals
def _refused(rc, lib, names, outs):
    assert rc != 0
    msg = lib.df_last_error().decode()
    assert all(n in msg for n in names), (names, msg)
    torch.cuda.synchronize()
    for o in outs:
        assert torch.isnan(o).all(), f"{names}: an output was touched ({msg})"


def test_mel_to_stft_names_what_it_refuses():
    from diff_foley_amd import engine as E
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, B, T = E.lib(), 2, 5
    A = torch.zeros(129, R.N_BIN, device=dev)
    At, Pt, mel, S = torch.zeros(R.N_BIN, 129, device=dev), torch.zeros(129, R.N_BIN, device=dev), torch.zeros(B, 129, T, device=dev), \
        _nan(B, T, R.N_BIN)

    def call(B=B, n_mels=128, T=T, iters=3, mel=mel, A=A, At=At, Pt=Pt, S=S):
        return lib.df_mel_to_stft(_p(mel), B, n_mels, T, _p(A), _p(At), _p(Pt), 0.5, iters, _p(S), E._stream())
    for bad, names in ((dict(n_mels=129), ["n_mels", "129"]), (dict(n_mels=0), ["mel bins"]), (dict(B=0), ["clips"]),
                       (dict(T=0), ["frames"]), (dict(iters=-1), ["iters", "-1"])) + \
            tuple(({k: None}, [f": {k} is a null pointer"]) for k in ("mel", "A", "At", "Pt", "S")):
        _refused(call(**bad), lib, ["mel_to_stft"] + names, [S])
    assert call(iters=0) == 0                                       # and what it takes: no iterations (the clipped start), 128 rows
    torch.cuda.synchronize()
    assert not torch.isnan(S).any()


def test_griffinlim_names_what_it_refuses():
    from diff_foley_amd import engine as E, vocoder as V
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, B, T = E.lib(), 2, 3
    c = V._get_consts(128, T, dev)
    t = dict(S=torch.ones(B, T, R.N_BIN, device=dev), phase0=torch.zeros(B, R.N_BIN, T, device=dev), twiddles=c.tw, window=c.window,
             wss=c.wss, angles=_nan(B, T, R.N_BIN, 2), reb0=_nan(B, T, R.N_BIN, 2), reb1=_nan(B, T, R.N_BIN, 2), frames=_nan(B, T, R.N_FFT),
             wav=_nan(B, R.HOP * (T - 1)))
    outs = [t[k] for k in ("angles", "reb0", "reb1", "frames", "wav")]

    def call(B=B, T=T, n_iter=1, momentum=0.99, **ptr):
        a = dict(t, **ptr)
        return lib.df_griffinlim(_p(a["S"]), _p(a["phase0"]), B, T, n_iter, momentum, _p(a["twiddles"]), _p(a["window"]), _p(a["wss"]),
                                 _p(a["angles"]), _p(a["reb0"]), _p(a["reb1"]), _p(a["frames"]), _p(a["wav"]), E._stream())
    cases = [(dict(B=0), ["clips"]), (dict(T=0), ["frames"]), (dict(T=1), ["T = 1"]), (dict(n_iter=-1), ["n_iter", "-1"]),
             (dict(momentum=1.0), ["momentum"]), (dict(momentum=-0.01), ["momentum"]), (dict(momentum=float("nan")), ["momentum"])]
    cases += [({k: None}, [f": {k} is a null pointer"]) for k in t]
    for bad, names in cases:
        _refused(call(**bad), lib, ["griffinlim"] + names, outs)
    assert call(n_iter=0, momentum=0.0) == 0
    torch.cuda.synchronize()
    assert not any(torch.isnan(t[k]).any() for k in ("angles", "reb0", "frames", "wav")) and torch.isnan(t["reb1"]).all()
