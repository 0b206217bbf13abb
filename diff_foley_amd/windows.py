"""Videos longer than one window: the host side of the overlapped-window construction.

A clip of ``T`` CAVP frames is covered by ``K`` windows of ``FRAMES`` = 32 frames (the length the model was trained on) at a hop of
``hop`` frames, the last one flush right.  At every solver step the guided noise prediction is evaluated on the K windows of the long
latent -- each under its own window's conditioning, positions 0..31 -- and the K predictions are blended column by column with an
integer tent weight; the solver update then runs on the long latent.  This module holds the geometry (plain integers, no device) and
the conditioning object the samplers recognise; the two device operations are ``engine.window_gather`` / ``engine.window_blend``.
"""
import math

import numpy as np
import torch

FRAMES = 32          # frames per window: the cond stage's training length (truncate_len of the reference notebook)
MAX_ROWS = 32        # window rows (B * K) of one UNet call: its CFG batch of 64 is the largest the engine's plans are built for


def window_starts(total, width, hop):
    """Starts of the windows of ``width`` units at a hop of ``hop`` over ``total`` units: k * hop, the last one total - width."""
    total, width, hop = int(total), int(width), int(hop)
    if total < width:
        raise ValueError(f"{total} is shorter than one window of {width}")
    if not 1 <= hop <= width:
        raise ValueError(f"hop = {hop}: expected 1 <= hop <= {width} (a larger hop leaves a gap between windows)")
    K = 1 if total == width else math.ceil((total - width) / hop) + 1
    return [k * hop for k in range(K - 1)] + [total - width]


def plan_windows(frames, hop=16, size_len=64):
    """(starts in frames, columns per frame r) of a clip of ``frames`` CAVP frames with ``size_len`` latent columns per window."""
    if int(size_len) < FRAMES or int(size_len) % FRAMES:
        raise ValueError(f"size_len = {size_len}: the latent columns of one window must be a positive multiple of its {FRAMES} frames")
    if int(frames) < FRAMES:
        raise ValueError(f"{frames} frames: a windowed conditioning needs at least one window of {FRAMES} frames")
    return window_starts(frames, FRAMES, hop), int(size_len) // FRAMES


def tent(width):
    """w(j) = min(j + 1, width - j), j = 0 .. width - 1."""
    j = np.arange(int(width), dtype=np.int64)
    return np.minimum(j + 1, int(width) - j)


def column_tables(starts, width, total):
    """Per column of [0, total): (k_first, k_count, n, inv_n) -- the first window that covers it, how many do (consecutive: starts
    ascend), the integer sum of their tent weights and fp32(1 / n) with the reciprocal taken in float64.  The tables the blend kernel
    reads (csrc/windows.hip builds the same on the host of the C entry)."""
    starts = [int(s) for s in starts]
    width, total = int(width), int(total)
    if not starts or width < 1 or total < width or starts != sorted(starts) or starts[0] < 0 or starts[-1] + width > total:
        raise ValueError(f"windows {starts} of {width} over {total}: starts must ascend inside [0, {total - width}]")
    k_first = np.full(total, -1, dtype=np.int32)
    k_count = np.zeros(total, dtype=np.int32)
    n = np.zeros(total, dtype=np.int64)
    w = tent(width)
    for k, s in enumerate(starts):
        cols = slice(s, s + width)
        k_first[cols] = np.where(k_first[cols] < 0, k, k_first[cols])
        k_count[cols] += 1
        n[cols] += w
    if (k_count == 0).any():
        raise ValueError(f"windows {starts} of {width} over {total}: column {int(np.argmin(k_count))} is covered by none")
    return k_first, k_count, n, (1.0 / n.astype(np.float64)).astype(np.float32)


def check_window_rows(batch, K):
    if int(batch) * int(K) > MAX_ROWS:
        raise ValueError(f"{batch} samples x {K} windows = {int(batch) * int(K)} window rows in one UNet call, the cap is {MAX_ROWS}: "
                         "sample fewer candidates at a time, or use a larger hop (fewer windows)")


class WindowedConditioning:
    """The conditioning of a clip longer than one window (``LatentDiffusion.get_windowed_conditioning``).

    ``c``               (B, K, 32, embed): the cond stage applied to ``video_feat[:, s_k : s_k + 32]``, window by window
    ``starts``          s_k in frames; ``col_starts`` = r * s_k in latent columns
    ``hop`` ``frames``  the hop asked for and T
    ``size_len``        latent columns of one window (Wc); ``size_len_total`` = r * T, the width of the long latent
    ``shape``           (B, T, embed): what a plain conditioning of the whole clip would have
    Hand it to a sampler in place of the conditioning tensor, with ``size_len=cond.size_len_total`` / a shape of that width."""

    def __init__(self, c, starts, hop, frames, size_len):
        if c.ndim != 4 or c.shape[1] != len(starts) or c.shape[2] != FRAMES:
            raise ValueError(f"windowed conditioning of shape {tuple(c.shape)}: expected (B, {len(starts)}, {FRAMES}, embed)")
        self.c = c
        self.starts = [int(s) for s in starts]
        self.hop, self.frames, self.size_len = int(hop), int(frames), int(size_len)
        self.r = self.size_len // FRAMES
        self.size_len_total = self.r * self.frames
        self.col_starts = [self.r * s for s in self.starts]
        self.shape = (int(c.shape[0]), self.frames, int(c.shape[3]))

    @property
    def K(self):
        return len(self.starts)

    @property
    def device(self):
        return self.c.device

    def zeros_like(self):
        """The notebook's unconditional side (torch.zeros_like(c)) with this geometry."""
        return WindowedConditioning(torch.zeros_like(self.c), self.starts, self.hop, self.frames, self.size_len)

    def same_geometry(self, other):
        return (self.starts, self.frames, self.size_len) == (other.starts, other.frames, other.size_len) and \
            tuple(self.c.shape) == tuple(other.c.shape)

    def check_latent(self, size):
        """``size`` = (B, C, H, W) of the long latent this conditioning is about to guide."""
        B, _, _, W = (int(v) for v in size)
        if W != self.size_len_total:
            raise ValueError(f"the latent is {W} columns wide, the windowed conditioning covers {self.frames} frames = "
                             f"{self.size_len_total} columns ({self.r} per frame): pass size_len=cond.size_len_total")
        if self.c.shape[0] not in (1, B):
            raise ValueError(f"{self.c.shape[0]} windowed conditionings for a batch of {B}")
        check_window_rows(B, self.K)

    def rows(self, batch):
        """(batch * K, 32, embed): the context rows of the window batch, row b * K + k."""
        c = self.c if self.c.shape[0] == batch else self.c.expand(batch, *self.c.shape[1:])
        return c.reshape(batch * self.K, FRAMES, self.c.shape[3])

    def uncond_rows(self, uc, batch):
        """The unconditional context rows of the window batch from ``uc``: a windowed object of the same geometry, or one tensor
        (1 | B, 32, embed) used for every window."""
        if isinstance(uc, WindowedConditioning):
            if not self.same_geometry(uc):
                raise ValueError("the unconditional windowed conditioning has another geometry than the conditional one")
            return uc.rows(batch)
        if uc.ndim != 3 or tuple(uc.shape[1:]) != (FRAMES, self.c.shape[3]) or uc.shape[0] not in (1, batch):
            raise ValueError(f"unconditional conditioning of shape {tuple(uc.shape)}: expected (1 | {batch}, {FRAMES}, {self.c.shape[3]}), "
                             "one window's worth used for every window, or a windowed conditioning of the same geometry")
        return uc.to(self.c.device, torch.float32)[:, None].expand(batch, self.K, FRAMES, self.c.shape[3]).reshape(
            batch * self.K, FRAMES, self.c.shape[3])
