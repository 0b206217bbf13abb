#!/usr/bin/env python
"""Measure waveform -> mel (df_wave_to_mel) on the GPU beside a composite of stock torch ops on the same device.

    python tools/wave_to_mel_bench.py [--batches 1,4,64] [--samples 100] [--inner 10] [--out profiles/wave_to_mel_bench.txt]

  * diff_foley_amd.wave_to_mel at L = 131071 (T = 512, the model's mel width) for each batch: HIP events around `inner`
    back-to-back calls, `samples` such windows after 20 warm-up calls; microseconds per call as median / min / max of the windows.
    The call includes the facade (output allocation, ctypes), as a user pays for it;
  * the composite, alternating with it window by window: torch.stft (hann, centred, reflect) -> abs -> filterbank matmul ->
    clamp / log10 / affine / clamp.  Where torch.stft does not run in this build the line says so and the kernel stands alone;
  * the largest |difference| of the two results, for orientation (nothing is asserted here: tests/test_wave_to_mel_gpu.py judges).
The library under test is the loaded one (DF_LIB_OVERRIDE selects a variant build, e.g. another tile: -DWTM_FT=8); every line
carries its tile (df_wave_to_mel_tile).  Prints one JSON line per measurement.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diff_foley_amd import engine as E, vocoder as V  # noqa: E402

L = 131071


def window_us(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def stats(ts):
    return dict(us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,64")
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wave_to_mel_bench: needs the GPU (there is no CPU path and no fallback)")
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    dev = torch.device("cuda", torch.cuda.current_device())
    tile = E.lib().df_wave_to_mel_tile()
    c = V._get_fwd_consts(V.WAV2SPEC_SR, 128, V.FMIN, V.FMAX, dev)
    g = torch.Generator().manual_seed(7)
    for B in [int(v) for v in a.batches.split(",")]:
        wav = (0.1 * torch.randn(B, L, generator=g)).to(dev)

        def fused():
            return V.wave_to_mel(wav)

        def composite():
            S = torch.stft(wav, 1024, hop_length=256, window=c.window, center=True, pad_mode="reflect", return_complex=True).abs()
            mel = torch.matmul(c.A, S)
            return ((20.0 * torch.log10(torch.clamp(mel, min=V.MEL_FLOOR)) - 20.0 + 100.0) / 100.0).clamp(0.0, 1.0)
        ref, why = None, None
        try:
            ref = composite()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001 -- reported, not hidden: the kernel is then timed alone
            why = f"{type(e).__name__}: {e}"[:200]
        for _ in range(20):
            fused()
            if ref is not None:
                composite()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(a.samples):
            tf.append(window_us(fused, a.inner))
            if ref is not None:
                tc.append(window_us(composite, a.inner))
        out = fused()
        rec = dict(what="wave_to_mel", tile=tile, B=B, L=L, frames=int(out.shape[2]), samples=a.samples, inner=a.inner, **stats(tf))
        if ref is not None:
            rec.update(composite={"ops": "torch.stft+abs+matmul+pointwise", **stats(tc)},
                       max_abs_diff_to_composite=float((out - ref).abs().max()))
        else:
            rec.update(composite=None, composite_error=why)
        emit(**rec)
    if a.out:
        path = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
