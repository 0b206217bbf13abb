#!/usr/bin/env python
"""Measure the CAVP spectrogram tower (df_cavp_spec_encode) on the GPU: call time and per-op time.

    python tools/cavp_spec_bench.py [--precision fp16] [--batches 1,4,8] [--frames 512] [--iters 20] [--out profiles/cavp_spec_bench.txt]

  * CAVPInference.encode_spec(normalize=True, pool=False) of the full-width Cnn14 (synth.CAVP_AUDIO_FULL, procedural weights) at each
    batch on a 128 x `frames` mel, HIP events around `iters` warmed calls; the tower's multiply-adds and weight bytes beside it;
  * per-op milliseconds of one profiled call (df_profile_begin / _end / _dump), summed per op tag;
  * df_cavp_similarity of one video against the batch's features.
Prints one JSON line per measurement; nothing is asserted.  Needs the GPU: there is no CPU path."""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diff_foley_amd as P  # noqa: E402
from diff_foley_amd import synth  # noqa: E402


def ev_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def tower_macs(cfg, frames):
    """Multiply-adds of one clip and the 2-byte weight volume of the GEMM-family ops."""
    h, w, cin, macs, wbytes = frames, cfg["n_mels"], 1, 0, 0
    for i, co in enumerate(cfg["channels"]):
        macs += h * w * 9 * (cin * co + co * co)
        wbytes += 2 * 9 * ((cin * co if i else 0) + co * co)
        cin = co
        if i < 5:
            h, w = (h // 2 if i < 4 else h), w // 2
    macs += h * (2 * cin * cfg["fc_dim"] + cfg["fc_dim"] * cfg["embed_dim"])
    wbytes += 2 * (cin * cfg["fc_dim"] + cfg["fc_dim"] * cfg["embed_dim"])
    return macs, wbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    cfg, vcfg = synth.CAVP_AUDIO_FULL, {**synth.CAVP_TINY, "embed_dim": 512}      # the video tower is not run: a shallow one
    m = P.CAVPInference(embed_dim=512, stage_blocks=vcfg["stage_blocks"], precision=a.precision)
    sd = synth.make_state_dict(synth.cavp_spec(vcfg))
    sd.update(synth.make_state_dict(synth.cavp_audio_spec(cfg)))
    m.load_state_dict(sd)
    m.cuda()
    eng = m.engine
    macs, wbytes = tower_macs(cfg, a.frames)
    for B in [int(v) for v in a.batches.split(",")]:
        mel = synth.synthetic_mel(B, a.frames, cfg["n_mels"], seed=7).cuda()
        ts = ev_ms(lambda: m.encode_spec(mel, normalize=True, pool=False), a.iters)
        med = statistics.median(ts)
        emit(what="df_cavp_spec_encode", precision=a.precision, B=B, frames=a.frames, ms_median=med, ms_min=min(ts), iters=a.iters,
             gmac_per_clip=macs / 1e9, weight_MB=wbytes / 1e6, tflops_median=2 * macs * B / med / 1e9)
        eng.profile_begin()
        feat = m.encode_spec(mel, normalize=True, pool=False)
        fam = eng.profile_end()
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "ops.csv")
            eng.profile_dump(path)
            per, shapes = {}, {}
            for i, r in enumerate(csv.DictReader(open(path))):
                key = f"{i:02d} {r['tag']}"
                per[key] = float(r["ms"])
                shapes[key] = f"{r['M']}x{r['N']}x{r['K']} tile {r['tile']} sk {r['splitk']}"
        emit(what="per_op_ms", B=B, families={k: round(v["ms"], 4) for k, v in fam.items()}, ops={k: round(v, 4) for k, v in per.items()},
             gemms={k: v for k, v in shapes.items() if not v.startswith("0x0x0")})
        video = torch.nn.functional.normalize(torch.randn(1, feat.shape[1], feat.shape[2], device=feat.device), dim=-1)
        ts = ev_ms(lambda: eng.cavp_similarity(video, feat, 1.0), a.iters)
        emit(what="df_cavp_similarity", Bv=1, Bs=B, T=feat.shape[1], D=feat.shape[2], ms_median=statistics.median(ts), ms_min=min(ts))
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
