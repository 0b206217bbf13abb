#!/usr/bin/env python
"""Measure one LatentDiffusion.p_losses call (the validation loss of a batch) on the GPU, beside the same chain assembled from what
the package had before df_q_sample / df_diffusion_loss existed.

    python tools/p_losses_bench.py [--precision fp16] [--batches 4,64] [--iters 20] [--out profiles/p_losses_bench_fp16.txt]

Stage2_LDM.yaml's model at full size (procedural weights), B latents of 4 x 16 x 64 with B x 32 x 512 CAVP features already through
the cond stage, per-sample timesteps and the noise given (so the device's generator is not in the figure).  Subjects:

  p_losses      df_q_sample -> apply_model -> df_diffusion_loss, one device-to-host copy of five floats at the end
  torch_chain   the reference's expressions (ddpm.py:279-282, 1061-1079) as torch ops on the device around the same apply_model,
                its loss_dict read the way the reference reads it: one .item() per entry
  apply_model   the UNet alone, which both contain

HIP events around `iters` warmed calls: median, min and max.  A cold call (plan building, operand packing) is not measured.  The
launch counts are kernel launches of ONE call, counted with torch.profiler where it records device activity (null where it does
not); the UNet plan's own count is the engine's.  Prints one JSON line per measurement; nothing is asserted.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

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


def launches(fn):
    """Kernel launches of one call of fn (warmed), or None where the profiler records no device activity."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "emcpy" not in e.name
                and "emset" not in e.name)
        return n or None
    except Exception as ex:      # a tool's convenience figure: the timings do not depend on it
        print(f"# launch count unavailable: {type(ex).__name__}: {ex}", file=sys.stderr)
        return None


def torch_chain(m, x0, cond, t, noise):
    """p_losses of the reference, line by line, on device tensors (what a caller had to write before)."""
    shape = (x0.shape[0], 1, 1, 1)
    x_noisy = m.sqrt_alphas_cumprod[t].reshape(shape) * x0 + m.sqrt_one_minus_alphas_cumprod[t].reshape(shape) * noise
    out = m.apply_model(x_noisy, t, cond)
    loss_simple = torch.nn.functional.mse_loss(noise, out, reduction="none").mean([1, 2, 3])
    d = {"val/loss_simple": loss_simple.mean().item()}
    logvar_t = m.logvar[t]
    loss = m.l_simple_weight * (loss_simple / torch.exp(logvar_t) + logvar_t).mean()
    loss_vlb = (m.lvlb_weights[t] * loss_simple).mean()
    d["val/loss_vlb"] = loss_vlb.item()
    loss = loss + m.original_elbo_weight * loss_vlb
    d["val/loss"] = loss.item()
    return loss, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--batches", default="4,64")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    m = P.LatentDiffusion(precision=a.precision, **P.stage2_config())
    m.load_state_dict(synth.make_state_dict(synth.state_dict_spec(), 0))
    m.cuda()
    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator().manual_seed(5)
        x0 = torch.randn(B, 4, 16, 64, generator=g).cuda()
        noise = torch.randn(B, 4, 16, 64, generator=g).cuda()
        t = torch.randint(0, m.num_timesteps, (B,), generator=g).cuda()
        cond = m.get_learned_conditioning(synth.synthetic_cavp(B, 32, 512, seed=1234).cuda())
        x_noisy = m.q_sample(x0, t, noise)
        subjects = {"p_losses": lambda: m.p_losses(x0, cond, t, noise=noise),
                    "torch_chain": lambda: torch_chain(m, x0, cond, t, noise),
                    "apply_model": lambda: m.apply_model(x_noisy, t, cond)}
        fused, plain = subjects["p_losses"]()[1], subjects["torch_chain"]()[1]
        emit(what="agreement", B=B, p_losses=fused, torch_chain=plain)
        plan = m.engine.plan_stats()["launches"]
        for what, fn in subjects.items():
            ts = ev_ms(fn, a.iters)
            emit(what=what, precision=m.engine.precision, B=B, ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4),
                 ms_max=round(max(ts), 4), iters=a.iters, launches=launches(fn), unet_plan_launches=plan)
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
