"""The restatement of the overlapped-window construction in plain torch on the CPU: test infrastructure only.

It states the semantics independently of diff_foley_amd/windows.py and csrc/windows.hip -- loops over windows and columns, float64
blend -- on top of the oracle's UNet, cond stage, decoder and samplers, which take an ``apply_model(x, t, c)`` callable.  The windowed
callable receives the (..., K, F, embed) conditioning, cuts the K windows out of the long latent, evaluates the oracle UNet on each
and blends the K predictions with the integer tent in float64.

  F = 32 frames per window, Wc latent columns per window, r = Wc // F columns per frame, W = r * T
  K = 1 if T == F else ceil((T - F) / hop) + 1;  s_k = k * hop for k < K - 1, s_{K-1} = T - F
  w(j) = min(j + 1, Wc - j);  n(x) = sum_k w(x - r s_k) over the windows covering x
  e(b, c, y, x) = (sum_k w(x - r s_k) e_k(b, c, y, x - r s_k)) / n(x)
"""
import math

import torch

F = 32


def starts_ref(total, width, hop):
    if total < width:
        raise ValueError("shorter than one window")
    if not 1 <= hop <= width:
        raise ValueError("hop outside 1..width")
    if total == width:
        return [0]
    K = math.ceil((total - width) / hop) + 1
    return [k * hop for k in range(K - 1)] + [total - width]


def weight(j, width):
    return min(j + 1, width - j)


def tables_ref(starts, width, total):
    """(k_first, k_count, n) per column, by the definition: a loop over columns and windows."""
    k_first, k_count, n = [], [], []
    for x in range(total):
        cover = [k for k, s in enumerate(starts) if 0 <= x - s < width]
        k_first.append(cover[0] if cover else -1)
        k_count.append(len(cover))
        n.append(sum(weight(x - starts[k], width) for k in cover))
    return k_first, k_count, n


def gather_ref(x, starts, width):
    """(B, C, H, W) -> (B * K, C, H, width), row b * K + k."""
    B = x.shape[0]
    return torch.stack([x[b, :, :, s:s + width] for b in range(B) for s in starts])


def blend_ref(win, starts, width, total):
    """(B * K, C, H, width) -> (B, C, H, total) in float64: the tent-weighted mean of the windows covering every column."""
    K = len(starts)
    B = win.shape[0] // K
    win = win.double().reshape(B, K, *win.shape[1:])
    acc = torch.zeros(B, win.shape[2], win.shape[3], total, dtype=torch.float64)
    n = torch.zeros(total, dtype=torch.float64)
    w = torch.tensor([weight(j, width) for j in range(width)], dtype=torch.float64)
    for k, s in enumerate(starts):
        acc[..., s:s + width] += w * win[:, k]
        n[s:s + width] += w
    return acc / n


def windowed_cond_ref(csd, video_feat, hop=16):
    """(B, K, F, embed): the oracle's cond stage on video_feat[:, s_k : s_k + F], every window at positions 0..F-1."""
    from oracle import vae as ov
    starts = starts_ref(video_feat.shape[1], F, hop)
    return torch.stack([ov.cond_stage(csd, video_feat[:, s:s + F]) for s in starts], 1), starts


def windowed_apply_model(unet, starts, Wc):
    """apply_model(x, t, c) for c of shape (N, K, F, embed) and x of shape (N, C, H, r T): per window the callable ``unet(x, t, c)``
    (the oracle's UNet), then the float64 blend, rounded to fp32 once.  One window: the plain call."""
    r = Wc // F
    cols = [r * s for s in starts]

    def apply_model(x, t, c):
        if len(starts) == 1:
            return unet(x, t, c[:, 0])
        assert x.shape[3] == cols[-1] + Wc and c.shape[1] == len(starts)
        e = torch.stack([unet(x[..., s:s + Wc].contiguous(), t, c[:, k]) for k, s in enumerate(cols)], 1)      # (N, K, C, H, Wc)
        return blend_ref(e.reshape(-1, *e.shape[2:]), cols, Wc, x.shape[3]).float()
    return apply_model


def decode_windowed_ref(vsd, vae_cfg, z, hop_cols=None, Wc=64, scale_factor=0.18215):
    """The windowed decode: the oracle's decode_first_stage per latent window, images blended with the tent over f * Wc columns."""
    from oracle import vae as ov
    f = 2 ** (len(vae_cfg["ch_mult"]) - 1)
    starts = starts_ref(z.shape[3], Wc, Wc // 2 if hop_cols is None else hop_cols)
    if len(starts) == 1:
        return ov.decode_first_stage(vsd, vae_cfg, z, scale_factor)
    img = torch.stack([ov.decode_first_stage(vsd, vae_cfg, z[..., s:s + Wc].contiguous(), scale_factor) for s in starts], 1)
    return blend_ref(img.reshape(-1, *img.shape[2:]), [f * s for s in starts], f * Wc, f * z.shape[3]).float()
