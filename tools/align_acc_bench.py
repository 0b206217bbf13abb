#!/usr/bin/env python
"""Measure one AlignmentClassifierMetric.probabilities call (the Align-Acc chain) on the GPU.

    python tools/align_acc_bench.py [--precision fp16] [--batches 1,8,64] [--iters 20] [--out profiles/align_acc_bench_fp16.txt]

eval_classifier.yaml's model at full size (procedural weights): B mels of 3 x 128 x 512 and B x 32 x 512 CAVP features go through the VAE
encoder + quant_conv, the posterior sample (noise given, so the device's generator is not in the figure), the cond stage and the
classifier at t = 0 -- the existing plans back to back on one stream.  HIP events around `iters` warmed calls: median, min and max; the
parts of the chain are timed the same way beside it, and one df_align_verdict launch.  A cold call (plan building, operand packing) is
not measured.  Prints one JSON line per measurement; nothing is asserted.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diff_foley_amd as P  # noqa: E402
from diff_foley_amd import engine as E, synth  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    m = P.AlignmentClassifierMetric(precision=a.precision, **P.align_metric_config())
    m.load_state_dict(synth.make_state_dict(synth.align_metric_spec(), 0))
    m.cuda()
    eng = m.engine
    for B in [int(v) for v in a.batches.split(",")]:
        spec = synth.synthetic_mel(B, 512, 128, seed=99)[:, None].repeat(1, 3, 1, 1).cuda()
        feats = synth.synthetic_cavp(B, 32, 512, seed=1234).cuda()
        noise = torch.randn(B, 4, 16, 64, generator=torch.Generator().manual_seed(5)).cuda()
        t0 = torch.zeros(B, device=spec.device)
        parts = {"probabilities": lambda: m.probabilities(spec, feats, noise=noise),
                 "vae_encode": lambda: eng.vae_encode(spec)}
        mom = eng.vae_encode(spec)
        z = E.posterior_sample(mom, noise, m.scale_factor)
        c = eng.cond_encode(feats)
        p = eng.classifier_forward(z, t0, c)
        counts = torch.zeros(2, dtype=torch.int64, device=spec.device)
        parts.update({"posterior_sample": lambda: E.posterior_sample(mom, noise, m.scale_factor),
                      "cond_encode": lambda: eng.cond_encode(feats),
                      "classifier_forward": lambda: eng.classifier_forward(z, t0, c),
                      "align_verdict": lambda: E.align_verdict(p, None, counts)})
        for what, fn in parts.items():
            ts = ev_ms(fn, a.iters)
            emit(what=what, precision=m.engine.precision, B=B, ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4),
                 ms_max=round(max(ts), 4), iters=a.iters)
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
