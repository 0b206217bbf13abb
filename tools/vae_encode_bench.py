#!/usr/bin/env python
"""Measure the VAE encoder (df_vae_encode) on the GPU: call time, per-op time, and the conv_in A/B.

    python tools/vae_encode_bench.py [--precision fp16] [--batches 1,4] [--iters 30] [--out profiles/vae_encode_bench.txt]

  * df_vae_encode at each batch on 3 x 128 x 512 (the Stage-2 mel), HIP events around `iters` warmed calls; df_vae_decode of the
    matching 16 x 64 latent beside it for orientation;
  * per-op milliseconds of one profiled call (df_profile_begin / _end / _dump), summed per op tag;
  * vaeenc.conv_in both ways, alternating in the same run: the dedicated kernel (df_test_conv3x3_fewin) and the route it replaces
    (df_test_conv3x3_fewin_gemm: pack to 64 operand-type channels + implicit GEMM; that entry also re-packs the 74 k weight
    elements per call, one extra small launch).  The op's floor is writing the output once: H * W * Cout * 4 bytes per sample
    (33.5 MB at 128 x 512 x 128).
Prints one JSON line per measurement; nothing is asserted.  Needs the GPU: there is no CPU path."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

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
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    vae = synth.VAE_FULL
    spec = synth.state_dict_spec(synth.UNET_TINY, vae, synth.COND_TINY, with_encoder=True)
    m = P.LatentDiffusion(precision=a.precision, **P.stage2_config(synth.UNET_TINY, vae, synth.COND_TINY))
    m.load_state_dict(synth.make_state_dict(spec, 0))
    m.cuda()
    eng = m.engine
    H, W, Cin, Cout = 128, 512, 3, vae["ch"]
    g = torch.Generator().manual_seed(3)
    for B in [int(v) for v in a.batches.split(",")]:
        x = (0.5 * torch.randn(B, Cin, H, W, generator=g)).clamp_(-1, 1).cuda()
        z = torch.randn(B, 4, 16, 64, generator=g).cuda()
        enc = ev_ms(lambda: eng.vae_encode(x), a.iters)
        dec = ev_ms(lambda: eng.vae_decode(z), a.iters)
        emit(what="df_vae_encode", precision=a.precision, B=B, shape=[Cin, H, W], ms_median=statistics.median(enc), ms_min=min(enc),
             decode_ms_median=statistics.median(dec), decode_ms_min=min(dec), iters=a.iters)
        eng.profile_begin()
        eng.vae_encode(x)
        fam = eng.profile_end()
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "ops.csv")
            eng.profile_dump(path)
            per = {}
            for r in csv.DictReader(open(path)):
                per[r["tag"]] = per.get(r["tag"], 0.0) + float(r["ms"])
        emit(what="per_op_ms", B=B, families={k: round(v["ms"], 4) for k, v in fam.items()},
             ops={k: round(v, 4) for k, v in sorted(per.items(), key=lambda kv: -kv[1])})
        # ---- conv_in A/B, alternating
        L = eng.L
        sd = m._state
        w = sd["first_stage_model.encoder.conv_in.weight"].cuda().contiguous()
        b = sd["first_stage_model.encoder.conv_in.bias"].cuda().contiguous()
        out = torch.empty(B * H * W, Cout, device="cuda")
        xpad = torch.empty(B * H * W * 64, dtype=torch.int16, device="cuda")
        wpad = torch.empty(Cout * 9 * 64, dtype=torch.int16, device="cuda")
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())

        def fewin():
            E._chk(L.df_test_conv3x3_fewin(p(x), p(w), p(b), p(out), Cout, B, H, W, Cin, Cout, st()), L)

        def gemm():
            E._chk(L.df_test_conv3x3_fewin_gemm(p(x), p(w), p(b), p(out), p(xpad), p(wpad), B, H, W, Cin, Cout, st()), L)
        fewin(), gemm()
        ta, tb = [], []
        for _ in range(a.iters):
            ta += ev_ms(fewin, 1, warm=0)
            tb += ev_ms(gemm, 1, warm=0)
        bytes_out = B * H * W * Cout * 4
        emit(what="vaeenc.conv_in", B=B, fewin_ms_median=statistics.median(ta), fewin_ms_min=min(ta),
             padded_gemm_ms_median=statistics.median(tb), padded_gemm_ms_min=min(tb), out_MB=bytes_out / 1e6,
             fewin_write_GBps=bytes_out / 1e6 / statistics.median(ta))
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
