"""GPU: the prologue arithmetic of the GEMM-family kernels -- tile walk, split-K ranges, row decomposition -- from the launch constants
of the host (csrc/gemm.h GemmLaunch), and the weights-first request order of the conv kernels.

Every case goes through df_test_gemm_ex (the asymmetric Downsample through df_test_conv3x3_down, the one entry that sets pad 0) with
the float64 reference and the per-element bounds of tests/test_gemm_epilogues_gpu.py / tests/gemm_cases.py (2 K u sum|A||W| for the
fp32 accumulation, 4 u per epilogue addition, half an ulp of an operand-type store; derived there, not fitted).  The shapes are the
smallest that reach each branch of the arithmetic: a ragged last M tile and several N tiles under every gm walk order (full row
groups and a short last one), five K tiles split 1 .. 4 ways (uneven slabs; at 4 the last slab is one tile), per-sample weights,
batch 3 on odd maps (a sample boundary inside a tile, a patch count that is no multiple of the patches per block), a folded skip
dealt to the splits, an empty trailing split on the halo tiles (3 splits of 2 channel slices), both paddings of the stride-2 conv,
the four phases of the upsample conv, and a ragged last tile of each wide GEGLU tile.  Outputs are NaN-poisoned before every launch
(gaps, slack rows and padding must stay NaN), and every gm order and a repeated launch must give the same bits."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as G
import test_gemm_epilogues_gpu as TG
from helpers import rnd
from test_gemm_forms_gpu import DevForm

pytestmark = pytest.mark.gpu

GMS = (0, 1, 2, 3)


@pytest.fixture(params=["bf16", "fp16"], autouse=True)
def prec(request):
    TG.PREC = request.param
    yield request.param
    TG.PREC = "bf16"


def run(name, cs, tiles, sks, gms=GMS):
    """Every (tile, split-K) of tiles x sks -- launch_gemm must take each -- at gm 0: the case's check; then every gm of `gms` and gm 0
    again bit-equal to it."""
    L = TG.lib()
    failures, worst, ran = [], 0.0, 0
    for tile in tiles:
        for sk in sks:
            where = f"tile {tile} split-K {sk}"
            d = cs.desc(tile, sk, 0)
            cs.set_outs(d, sk)
            buf = C.create_string_buffer(200)
            assert L.df_test_gemm_why(C.byref(d), tile, cs.batch, sk, buf, 200) in (0, 1), f"{name} {where}: refused ({buf.value.decode()})"
            rc, msg = cs.launch(d)
            assert rc == 0, f"{name} {where}: {msg}"
            fl, w = cs.check(sk)
            worst, ran = max(worst, w), ran + 1
            failures += [f"{where}: {m}" for m in fl]
            snap = {k: t.clone() for k, t in cs.outs.items()}
            for gm in tuple(gms) + (0,):
                d = cs.desc(tile, sk, gm)
                cs.set_outs(d, sk)
                rc, msg = cs.launch(d)
                assert rc == 0, f"{name} {where} gm {gm}: {msg}"
                failures += [f"{where}: gm {gm} changes the bits of {k}" for k, t in cs.outs.items() if not TG.same_bits(t, snap[k])]
    torch.cuda.synchronize()
    print(f"\n{name} [{TG.PREC}]: {ran} (tile, split-K) pairs x {len(gms) + 2} launches, worst error / bound {worst:.3f}")
    assert not failures, f"{name} [{TG.PREC}]: {len(failures)} failure(s):\n" + "\n".join(failures[:40])


def test_linear_tile_walk_and_split_ranges():
    """M = 200, N = 192, K = 320: 4 x 3 tiles of 64 x 64 (2 x 3, 2 x 2 of the larger ones) with a ragged last row tile -- gm 3 walks one
    full row group and a short one, gm 2 two full ones -- and five K tiles in slabs of 5 | 3 + 2 | 2 + 2 + 1 | 2 + 2 + 1 + 0."""
    cs = TG.dense("prologue_lin", M=200, N=192, K=320, res=True, seed=300)
    run("linear", cs, (3, 26, 28, 0), (1, 2, 3, 4))


def test_per_sample_weights():
    """w_rows = 64, M = 192: the weight matrix of a tile is (M tile) / (w_rows / BM), a multiply-high by a launch constant."""
    cs = TG.dense("prologue_wrows", M=192, N=192, K=320, S=3, seed=301)
    run("per-sample weights", cs, (3, 26), (1, 2))


@pytest.mark.parametrize("hw", [(5, 7), (6, 10)])
def test_mode1_rows_on_odd_maps(hw):
    """Batch 3 on 5 x 7 and 6 x 10 maps, Cin = 128, generic and producer-specialised 64 x 64 tiles: rows -> (sample, y, x) by the
    host's magic numbers with sample boundaries inside a tile; with and without the folded skip (Cin2 = 64, split 1 .. 3 ways)."""
    H, Wd = hw
    run(f"conv {H}x{Wd}", TG.dense("prologue_conv", N=128, conv=(3, H, Wd, 128), seed=310 + H), (3, 26), (1, 2, 3))
    skip = DevForm(G.form("prologue_skip", TG.PREC, kind="conv", conv=(3, H, Wd, 128), N=128, Cin2=64, seed=320 + H))
    run(f"conv + skip {H}x{Wd}", skip, (3, 26), (1, 2, 3))


@pytest.mark.parametrize("hw", [(8, 16), (4, 16)])
def test_halo_conv_weights_first(hw):
    """The same convs on 8 x 16 and 4 x 16 maps, batch 3, on the producer-specialised halo tiles 23, 24, 25: the weight ring is
    requested in front of the halo-row table, the patch count (3 or 6 per sample) is no multiple of the patches per block, and 3
    splits of 2 channel slices leave an empty trailing split (the skip's slices go to the two splits that own conv slices)."""
    H, Wd = hw
    run(f"halo conv {H}x{Wd}", TG.dense("prologue_halo", N=128, conv=(3, H, Wd, 128), seed=330 + H), (23, 24, 25), (1, 2, 3))
    skip = DevForm(G.form("prologue_halo_skip", TG.PREC, kind="conv", conv=(3, H, Wd, 128), N=128, Cin2=64, seed=340 + H))
    run(f"halo conv + skip {H}x{Wd}", skip, (23, 24, 25), (1, 2, 3))


def test_halo_conv_symmetric_tiles():
    """The symmetric halo tiles (5: 128 x 64, 17: 192 x 64) take the same weights-first prologue with their own counted waits."""
    run("halo conv, symmetric tiles", TG.dense("prologue_halo_sym", N=128, conv=(3, 8, 16, 128), seed=350), (5, 17), (1, 2))


@pytest.mark.parametrize("pad", [1, 0])
def test_mode2_downsample_both_paddings(pad):
    """6 x 10 -> 3 x 5, batch 3, C = 128, stride 2 with pad 1 (the UNet's Downsample) and pad 0 (the VAE encoder's F.pad(0, 1, 0, 1)
    + padding-0 conv), unsplit and split, against float64 with the bound of tests/test_vae_encoder_kernels_gpu.py."""
    L = TG.lib()
    NB, H, Wd, C_ = 3, 6, 10, 128
    x = rnd((NB, C_, H, Wd), 360).to(TG.odt())
    w = (rnd((C_, C_, 3, 3), 361) / (3.0 * C_ ** 0.5)).to(TG.odt())
    b = rnd((C_,), 362)
    xd, wd = x.double(), w.double()
    pd = (lambda t: F.pad(t, (0, 1, 0, 1))) if pad == 0 else (lambda t: F.pad(t, (1, 1, 1, 1)))
    ref = F.conv2d(pd(xd), wd, b.double(), stride=2)[:, :, :H // 2, :Wd // 2]
    mag = F.conv2d(pd(xd.abs()), wd.abs(), None, stride=2)[:, :, :H // 2, :Wd // 2]
    bnd = 2 * 9 * C_ * TG.U * mag + 4 * TG.U * (ref.abs() + b.double().abs().view(1, -1, 1, 1))
    rows = NB * (H // 2) * (Wd // 2)
    ref, bnd = (t.permute(0, 2, 3, 1).reshape(rows, C_).cuda() for t in (ref, bnd))
    a, wq, bq = x.permute(0, 2, 3, 1).contiguous().cuda(), w.permute(0, 2, 3, 1).contiguous().cuda(), b.cuda()
    for tile in (3, 4):
        for sk in (1, 2, 3):
            assert L.df_test_conv3x3_down_valid(NB, H, Wd, C_, C_, pad, tile, sk) == 1, (tile, sk)
            outs = []
            for rep in range(2):
                out = torch.full((rows + 3, C_), float("nan"), device="cuda")
                rc = L.df_test_conv3x3_down(a.data_ptr(), wq.data_ptr(), bq.data_ptr(), out.data_ptr(), NB, H, Wd, C_, C_, pad, tile, sk, TG.stream())
                assert rc == 0, L.df_last_error()
                outs.append(out)
            assert TG.all_nan(outs[0][rows:]), (tile, sk, "slack rows written")
            e, row = TG._excess(outs[0][:rows], ref, bnd)
            assert row < 0, f"pad {pad} tile {tile} split-K {sk}: row {row} off by {e:.3g} x its bound"
            assert TG.same_bits(outs[0], outs[1]), (tile, sk, "a repeated launch changes the bits")


def test_mode3_phases():
    """The phase-decomposed upsample conv on a 4 x 6 map, batch 3: four phases in grid z next to the split, rows by the same magic
    numbers, split 1 and 2 ways."""
    cs = DevForm(G.form("prologue_ups4", TG.PREC, kind="ups4", conv=(3, 4, 6, 128), N=64, seed=370))
    run("ups4 4x6", cs, (3, 8), (1, 2))


@pytest.mark.parametrize("tile, M", [(34, 64), (34, 50), (33, 128), (33, 100), (32, 256), (32, 200)])
def test_wide_geglu(tile, M):
    """Each wide GEGLU tile (BM = 64 / 128 / 256) on exactly one row tile and on a ragged one, two 320-column N tiles."""
    cs = DevForm(G.form("prologue_wide", TG.PREC, M=M, N=640, K=320, ln="geglu", seed=380 + M))
    run(f"wide GEGLU tile {tile} M {M}", cs, (tile,), (1,))
