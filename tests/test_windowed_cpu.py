"""CPU: the geometry of the overlapped-window construction (diff_foley_amd/windows.py) against its restatement
(tests/windowed_ref.py), the restatement's own invariants, and the argument errors.  No GPU."""
import numpy as np
import pytest
import torch

import diff_foley_amd as P
from diff_foley_amd import synth, windows as W
from helpers import rnd, tiny_state_dict
import windowed_ref as R

CASES = [(32, 16), (33, 16), (48, 16), (50, 16), (40, 1), (64, 32), (95, 7)]      # (T, hop)
WC, RR = 64, 2


@pytest.mark.parametrize("T,hop", CASES)
def test_planner_equals_the_restatement(T, hop):
    starts, r = W.plan_windows(T, hop, WC)
    want = R.starts_ref(T, R.F, hop)
    assert r == RR and starts == want and len(starts) == len(want)
    assert len(starts) == (1 if T == 32 else -(-(T - 32) // hop) + 1)
    cols = [r * s for s in starts]
    k_first, k_count, n, inv_n = W.column_tables(cols, WC, r * T)
    rf, rc, rn = R.tables_ref(cols, WC, r * T)
    assert k_first.tolist() == rf and k_count.tolist() == rc and n.tolist() == rn
    assert min(rc) >= 1 and min(rn) > 0                       # every column covered
    assert inv_n.dtype == np.float32 and np.array_equal(inv_n, (1.0 / np.asarray(rn, dtype=np.float64)).astype(np.float32))
    # the windows covering a column are consecutive, which is what (k_first, k_count) can express
    for x in range(r * T):
        assert [k for k, s in enumerate(cols) if 0 <= x - s < WC] == list(range(rf[x], rf[x] + rc[x]))


@pytest.mark.parametrize("T,hop", CASES)
def test_partition_of_unity(T, hop):
    """blend(gather(f)) == f exactly in float64: the weights of a column sum to n, and n / n is 1."""
    cols = [RR * s for s in R.starts_ref(T, R.F, hop)]
    f = torch.randint(-2 ** 20, 2 ** 20, (2, 3, 5, RR * T), generator=torch.Generator().manual_seed(T)).double()
    win = R.gather_ref(f, cols, WC)
    assert win.shape == (2 * len(cols), 3, 5, WC)
    assert torch.equal(R.blend_ref(win, cols, WC, RR * T), f)


def test_odd_geometry_tables():
    k_first, k_count, n, _ = W.column_tables([0, 3, 5], 6, 11)
    rf, rc, rn = R.tables_ref([0, 3, 5], 6, 11)
    assert (k_first.tolist(), k_count.tolist(), n.tolist()) == (rf, rc, rn)
    with pytest.raises(ValueError):
        W.column_tables([0, 7], 6, 13)          # column 6 uncovered
    with pytest.raises(ValueError):
        W.column_tables([3, 0], 6, 9)           # not ascending


def test_one_window_restatement_is_the_plain_oracle_sampler():
    """K = 1: the windowed callable is the plain call, so the oracle's DDIM on the windowed conditioning has the bits of the oracle's
    DDIM on the plain one."""
    from oracle import unet as ou, vae as ov, samplers as osamp, schedule as osch
    sd = tiny_state_dict()
    usd, csd = ou.sub_state_dict(sd, "model.diffusion_model."), ou.sub_state_dict(sd, "cond_stage_model.")
    feats = synth.synthetic_cavp(1, 32, synth.COND_TINY["origin_dim"], seed=5)
    xT = rnd((1, 4, 16, 64), 6)
    unet = lambda x, t, c: ou.unet_forward(usd, synth.UNET_TINY, x, t, c)
    cw, starts = R.windowed_cond_ref(csd, feats, 16)
    assert starts == [0] and cw.shape[:3] == (1, 1, 32)
    c = ov.cond_stage(csd, feats)
    assert torch.equal(cw[:, 0], c)
    acp = osch.ddpm_schedule()["alphas_cumprod"]
    za, _ = osamp.ddim_sample(R.windowed_apply_model(unet, starts, 64), acp, 2, xT, cw, scale=4.5, uc=torch.zeros_like(cw))
    zb, _ = osamp.ddim_sample(unet, acp, 2, xT, c, scale=4.5, uc=torch.zeros_like(c))
    assert torch.equal(za, zb)


def _cond(B, T, hop=16, size_len=64, embed=8):
    starts, _ = W.plan_windows(T, hop, size_len)
    return W.WindowedConditioning(torch.zeros(B, len(starts), 32, embed), starts, hop, T, size_len)


def test_argument_errors():
    with pytest.raises(ValueError):
        W.plan_windows(31, 16, 64)              # T < 32
    for hop in (0, 33, -1):
        with pytest.raises(ValueError):
            W.plan_windows(48, hop, 64)
    for size_len in (48, 0, 16):
        with pytest.raises(ValueError):
            W.plan_windows(48, 16, size_len)    # size_len % 32
    c = _cond(2, 48)
    assert c.K == 2 and c.size_len_total == 96 and c.shape == (2, 48, 8) and c.col_starts == [0, 32]
    c.check_latent((2, 4, 16, 96))
    with pytest.raises(ValueError, match="columns"):
        c.check_latent((2, 4, 16, 64))          # wrong latent width
    with pytest.raises(ValueError, match="cap is 32"):
        _cond(11, 64).check_latent((11, 4, 16, 128))     # 11 x 3 = 33 window rows
    _cond(16, 33).check_latent((16, 4, 16, 66))          # 32 window rows: the cap itself
    z = c.zeros_like()
    assert isinstance(z, P.WindowedConditioning) and z.same_geometry(c) and not z.c.any()
    with pytest.raises(ValueError):
        c.uncond_rows(_cond(2, 50), 2)          # another geometry
    with pytest.raises(ValueError):
        c.uncond_rows(torch.zeros(2, 31, 8), 2)
    assert c.uncond_rows(torch.zeros(1, 32, 8), 2).shape == (4, 32, 8) and c.rows(2).shape == (4, 32, 8)


def test_new_symbols_are_in_the_header_and_the_binding():
    import os
    from diff_foley_amd import engine as E
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "df_engine.h")).read()
    for name in ("df_window_gather", "df_window_blend"):
        assert name + "(" in hdr and name in E.exported_symbols()
        for prec in ("bf16", "fp16"):
            assert hasattr(E.lib(prec), name)
