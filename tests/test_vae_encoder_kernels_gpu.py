"""GPU: the three new pieces of the VAE encoder, each alone through the C ABI, both operand builds.

  conv3x3_fewin        the encoder's conv_in (csrc/elementwise.hip): fp32 VALU, inputs NOT rounded to the operand type
  asymmetric stride-2  GemmParams::pad = 0 on every MODE-2 tile x every split-K the route accepts (csrc/gemm_impl.h)
  df_posterior_sample  DiagonalGaussianDistribution.sample() with the scale folded in

Every conv element is judged against float64 within the derived bound of tests/gemm_cases.py for a K-term fp32 dot product in any
summation order plus the epilogue's roundings:  2 K u sum|a||w| + 4 u (|v| + |bias|),  u = 2^-24, K = 9 Cin."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from helpers import rnd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PREC = "bf16"


def _eng():
    from diff_foley_amd import engine as E
    return E


@pytest.fixture(params=["bf16", "fp16"], autouse=True)
def prec(request):
    global PREC
    PREC = request.param
    yield PREC
    PREC = "bf16"


def lib():
    return _eng().lib(PREC)


def odt():
    return _eng().OPERAND_DTYPE[PREC]


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    L = lib()
    rc = getattr(L, name)(*args, stream())
    assert rc == 0, L.df_last_error()
    torch.cuda.synchronize()


def excess(got, ref, bnd):
    """max over elements of |got - ref| / bound (<= 1 passes); NaN anywhere fails."""
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return float(((got.double() - ref).abs() / bnd.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------- conv3x3_fewin
_fewin_ref = {}


def fewin_case(Cin, Cout, H, W):
    key = (Cin, Cout, H, W)
    if key not in _fewin_ref:
        B = 2
        x = rnd((B, Cin, H, W), 9000 + Cin * 131 + H).contiguous()
        w = (rnd((Cout, Cin, 3, 3), 9100 + Cout + Cin) / (3.0 * Cin ** 0.5)).contiguous()
        b = rnd((Cout,), 9200 + Cout).contiguous()
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)                      # the kernel rounds neither x nor w
        mag = F.conv2d(x.double().abs(), w.double().abs(), None, padding=1)
        bnd = 2 * 9 * Cin * U * mag + 4 * U * (ref.abs() + b.double().abs().view(1, -1, 1, 1))
        _fewin_ref[key] = (x, w, b, ref.permute(0, 2, 3, 1).reshape(B * H * W, Cout), bnd.permute(0, 2, 3, 1).reshape(B * H * W, Cout))
    return _fewin_ref[key]


@pytest.mark.parametrize("H, W", [(4, 8), (5, 36), (32, 64)])       # all border / ragged patch in both axes / several whole patches
@pytest.mark.parametrize("Cout", [64, 128, 256])
@pytest.mark.parametrize("Cin", [1, 3])
def test_conv3x3_fewin_alone(Cin, Cout, H, W):
    x, w, b, ref, bnd = fewin_case(Cin, Cout, H, W)
    rows, slack, ldo = 2 * H * W, 5, Cout + 8
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    runs = []
    for _ in range(2):
        out = torch.full((rows + slack, ldo), float("nan"), device="cuda")
        call("df_test_conv3x3_fewin", ptr(xd), ptr(wd), ptr(bd), ptr(out), ldo, 2, H, W, Cin, Cout)
        runs.append(out.cpu())
    out = runs[0]
    assert bool(torch.isnan(out[rows:]).all()), "slack rows behind the output were written"
    assert bool(torch.isnan(out[:, Cout:]).all()), "columns behind Cout were written"
    e = excess(out[:rows, :Cout], ref, bnd)
    print(f"fewin {Cin}->{Cout} {H}x{W} [{PREC}]: max error / bound = {e:.3f}")
    assert e <= 1.0
    assert torch.equal(runs[0][:rows, :Cout].view(torch.int32), runs[1][:rows, :Cout].view(torch.int32)), "not bit-equal on a repeat"


def test_conv3x3_fewin_refuses_what_it_does_not_build():
    L = lib()
    z = torch.zeros(16, device="cuda")
    for Cin, Cout, ldo in ((5, 64, 64), (0, 64, 64), (3, 96, 96), (3, 64, 60), (3, 64, 66)):
        assert L.df_test_conv3x3_fewin(ptr(z), ptr(z), None, ptr(z), ldo, 1, 1, 1, Cin, Cout, stream()) != 0
        assert b"refused" in L.df_last_error()


# ---------------------------------------------------------------------------------------------------- asymmetric stride-2 conv
_down_ref = {}


def down_case(C_, H, W):
    key = (PREC, C_, H, W)
    if key not in _down_ref:
        B = 2
        x = rnd((B, C_, H, W), 9300 + C_ + H).to(odt())
        w = (rnd((C_, C_, 3, 3), 9400 + C_) / (3.0 * C_ ** 0.5)).to(odt())
        b = rnd((C_,), 9500 + C_)
        xd, wd = x.double(), w.double()
        ref = F.conv2d(F.pad(xd, (0, 1, 0, 1)), wd, b.double(), stride=2)
        mag = F.conv2d(F.pad(xd.abs(), (0, 1, 0, 1)), wd.abs(), None, stride=2)
        bnd = 2 * 9 * C_ * U * mag + 4 * U * (ref.abs() + b.double().abs().view(1, -1, 1, 1))
        rows = B * (H // 2) * (W // 2)
        sym = F.conv2d(xd, wd, b.double(), stride=2, padding=1)
        _down_ref[key] = (x.permute(0, 2, 3, 1).contiguous().cuda(), w.permute(0, 2, 3, 1).contiguous().cuda(), b.cuda(),
                          ref.permute(0, 2, 3, 1).reshape(rows, C_), bnd.permute(0, 2, 3, 1).reshape(rows, C_),
                          sym.permute(0, 2, 3, 1).reshape(rows, C_))
    return _down_ref[key]


def mode2_tiles():
    return sorted(t for t, info in _eng().gemm_tiles(lib()).items() if 2 in info["modes"])


@pytest.mark.parametrize("H, W", [(4, 6), (8, 12), (32, 48)])      # 32 x 48 -> 768 rows: several row tiles, a sample boundary inside one
@pytest.mark.parametrize("C_", [64, 128])
def test_asymmetric_downsample_conv_on_every_mode2_tile_and_split(C_, H, W):
    L = lib()
    a, w, b, ref, bnd, sym = down_case(C_, H, W)
    rows = ref.shape[0]
    # the cases are the smallest at which the wrong padding shows: the symmetric conv differs from the reference far beyond the bound
    assert float(((sym - ref).abs() / bnd).median()) > 100.0
    tiles = mode2_tiles()
    assert tiles, "no MODE 2 tile in the table"
    worst, n = 0.0, 0
    for tile in tiles:
        for sk in range(1, 9 * C_ // 64 + 1):
            if L.df_test_conv3x3_down_valid(2, H, W, C_, C_, 0, tile, sk) != 1:
                continue
            out = torch.full((rows + 3, C_), float("nan"), device="cuda")
            call("df_test_conv3x3_down", ptr(a), ptr(w), ptr(b), ptr(out), 2, H, W, C_, C_, 0, tile, sk)
            o = out.cpu()
            assert bool(torch.isnan(o[rows:]).all()), (tile, sk, "slack rows written")
            e = excess(o[:rows], ref, bnd)
            assert e <= 1.0, (tile, sk, e)
            worst, n = max(worst, e), n + 1
    print(f"asym down {C_} {H}x{W} [{PREC}]: {n} (tile, split-K) pairs on tiles {tiles}, worst error / bound = {worst:.3f}")
    assert n >= len(tiles), "every MODE 2 tile must take the case unsplit"


def test_pad_one_through_the_new_entry_is_the_existing_stride2_form():
    """GemmParams::pad = 1 changed nothing: bit-equal to df_test_conv3x3(stride 2) on every MODE 2 tile, unsplit and split."""
    L = lib()
    C_, H, W = 64, 8, 12
    a, w, b, *_ = down_case(C_, H, W)
    rows = 2 * (H // 2) * (W // 2)
    for tile in mode2_tiles():
        for sk in (1, 3):
            if L.df_test_conv3x3_down_valid(2, H, W, C_, C_, 1, tile, sk) != 1:
                continue
            new = torch.full((rows, C_), float("nan"), device="cuda")
            old = torch.full((rows, C_), float("nan"), device="cuda")
            call("df_test_conv3x3_down", ptr(a), ptr(w), ptr(b), ptr(new), 2, H, W, C_, C_, 1, tile, sk)
            call("df_test_conv3x3", ptr(a), ptr(w), ptr(b), ptr(old), 2, H, W, C_, C_, 2, 0, tile, sk)
            assert bool(torch.isfinite(old).all())
            assert torch.equal(new.view(torch.int32), old.view(torch.int32)), (tile, sk)
    assert L.df_test_conv3x3_down_valid(2, H, W, C_, C_, 2, mode2_tiles()[0], 1) == 0          # pad is 0 or 1


# ------------------------------------------------------------------------------------------------------------ posterior sample
@pytest.mark.parametrize("HW", [1, 3, 1024])
@pytest.mark.parametrize("zc", [1, 4, 7])
def test_posterior_sample(zc, HW):
    """z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise).  Without noise: scale * mean, one rounding, bit-exact.  With
    noise, against float64 on the same fp32 inputs (0.5 * clamp(logvar) is exact in fp32, so the exp's argument carries no error):
    the product, the sum and the scaling round once each (3 u of the larger intermediate, asserted as 4 u), and the device exp is
    expf of the HIP device library, documented at 1 ulp = 2 u relative, which enters through std * noise."""
    L = lib()
    B, scale = 2, 0.18215
    n = B * zc * HW
    mean = rnd((B, zc, HW), 9600 + zc + HW)
    lv = 8.0 * rnd((B, zc, HW), 9700 + zc + HW)
    special = torch.tensor([-40.0, -30.0, 0.0, 20.0, 25.0])
    lv.view(-1)[:min(5, n)] = special[:min(5, n)]
    if n < 5:                                   # the smallest shapes: the special values ride in the second sample / later channels
        lv.view(-1)[-min(5, n):] = special[-min(5, n):]
    noise = rnd((B, zc, HW), 9800 + zc + HW)
    mom = torch.cat([mean, lv], dim=1).contiguous().cuda()
    z = torch.full((n + 8,), float("nan"), device="cuda")
    assert L.df_posterior_sample(ptr(mom), None, ptr(z), B, zc, HW, scale, stream()) == 0, L.df_last_error()
    got = z.cpu()
    assert bool(torch.isnan(got[n:]).all())
    want = (torch.tensor(scale, dtype=torch.float32) * mean).reshape(-1)
    assert torch.equal(got[:n].view(torch.int32), want.view(torch.int32)), "mode(): scale * mean, bit-exact"
    z = torch.full((n + 8,), float("nan"), device="cuda")
    nd = noise.cuda()
    assert L.df_posterior_sample(ptr(mom), ptr(nd), ptr(z), B, zc, HW, scale, stream()) == 0, L.df_last_error()
    got = z.cpu()
    assert bool(torch.isnan(got[n:]).all())
    s64 = float(torch.tensor(scale, dtype=torch.float32))
    sn = torch.exp(0.5 * lv.double().clamp(-30.0, 20.0)) * noise.double()
    ref = s64 * (mean.double() + sn)
    bnd = 4 * U * abs(s64) * (mean.double().abs() + sn.abs()) + 2 * U * abs(s64) * sn.abs()
    e = excess(got[:n].reshape(B, zc, HW), ref, bnd)
    print(f"posterior sample zc {zc} HW {HW} [{PREC}]: max error / bound = {e:.3f}")
    assert e <= 1.0
    for bad in ((0, zc, HW), (B, 0, HW), (B, zc, 0)):
        assert L.df_posterior_sample(ptr(mom), None, ptr(z), *bad, scale, stream()) != 0
