#!/usr/bin/env python
"""Measure DPM_Solver.sample on the GPU for each method of the family, and DPM-Solver++(2M) as DPMSolverSampler.sample selects it.

    python tools/dpm_family_bench.py [--precision fp16] [--batch 4] [--iters 10] [--steps2m 50] [--out profiles/dpm_family_bench_fp16.txt]

Stage2_LDM.yaml's model at full size (procedural weights), B latents of 4 x 16 x 64, B x 32 x 512 CAVP features already through the
cond stage, classifier-free guidance 4.5 against a zero unconditional context, x_T given (the device's generator is not in the
figure).  Every subject is LatentDiffusion.dpm_solver(...).sample(...) on the fast route:

  per method   ms of one sample() (HIP events around `iters` warmed calls: median), the guided UNet evaluations it makes, evaluations
               per second ("steps/s"), and the ms outside the UNet: the median minus evaluations x the median of one guided evaluation
               with a hoisted time embedding, measured alone in the same process.  For 'adaptive' the evaluation count is the run's own
               and the embedding is computed in the step, so its UNet figure is the in-step evaluation's.
  2M           DPMSolverSampler.sample at --steps2m: DPM_Solver(multistep, order 2, time_uniform, predict_x0) behind the samplers'
               call surface, with the start latent and the solver built inside the figure.

Prints one JSON line per measurement; nothing is asserted.  Needs the GPU."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diff_foley_amd as P  # noqa: E402
from diff_foley_amd import dpm_solver as D, synth  # noqa: E402

METHODS = {
    "singlestep order 3, 15 evaluations, time_uniform": dict(steps=15, order=3, method="singlestep", skip_type="time_uniform"),
    "singlestep order 3, 15 evaluations, logSNR": dict(steps=15, order=3, method="singlestep", skip_type="logSNR"),
    "singlestep order 3 taylor, 15 evaluations": dict(steps=15, order=3, method="singlestep", skip_type="time_uniform", solver_type="taylor"),
    "singlestep_fixed order 2, 20 evaluations": dict(steps=20, order=2, method="singlestep_fixed", skip_type="time_uniform"),
    "multistep order 3, 20 evaluations": dict(steps=20, order=3, method="multistep"),
    "multistep order 2, 20 evaluations": dict(steps=20, order=2, method="multistep"),
    "multistep order 1, 20 evaluations": dict(steps=20, order=1, method="multistep"),
    "multistep order 2 + thresholding + denoise_to_zero, 21 evaluations": dict(steps=20, order=2, method="multistep", denoise_to_zero=True),
    "adaptive order 2": dict(order=2, method="adaptive"),
    "adaptive order 3": dict(order=3, method="adaptive"),
}


def ev_ms(fn, iters, warm=2):
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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps2m", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    m = P.LatentDiffusion(precision=a.precision, **P.stage2_config())
    m.load_state_dict(synth.make_state_dict(synth.state_dict_spec(), 0))
    m.cuda()
    B = a.batch
    x = synth.synthetic_xT(B).cuda()
    c = m.get_learned_conditioning(synth.synthetic_cavp(B, 32, 512, seed=1234).cuda())
    uc = torch.zeros_like(c)
    scale = 4.5

    # one guided evaluation alone: hoisted embedding (a 15-entry table) and in-step
    sol = m.dpm_solver(c, scale, uc)
    times = list(sol._time_steps("time_uniform", 1.0, 1e-3, 14))
    ses = D._FastSession(sol.model, tuple(x.shape), times)
    hoisted = statistics.median(ev_ms(lambda: ses(x, times[3]), 3 * a.iters))
    ses = D._FastSession(sol.model, tuple(x.shape), None)
    instep = statistics.median(ev_ms(lambda: ses(x, times[3]), 3 * a.iters))
    emit(what="guided evaluation", precision=m.engine.precision, B=B, ms_hoisted=round(hoisted, 4), ms_in_step=round(instep, 4))

    calls = []
    plain = D._FastSession.__call__
    D._FastSession.__call__ = lambda self, xx, t: (calls.append(1), plain(self, xx, t))[1]
    for what, kw in METHODS.items():
        sol = m.dpm_solver(c, scale, uc, thresholding="thresholding" in what)

        def run():
            with contextlib.redirect_stdout(io.StringIO()):
                return sol.sample(x, **kw)
        del calls[:]
        run()
        evals = len(calls)
        ts = ev_ms(run, a.iters)
        med = statistics.median(ts)
        unet = instep if kw["method"] == "adaptive" else hoisted
        emit(what=what, precision=m.engine.precision, B=B, evaluations=evals, ms_median=round(med, 3), ms_min=round(min(ts), 3),
             ms_max=round(max(ts), 3), steps_per_s=round(1000.0 * evals / med, 1), ms_outside_unet=round(med - evals * unet, 3),
             iters=a.iters)
    D._FastSession.__call__ = plain

    # the 2M configuration, through the sampler that selects it
    St = a.steps2m
    run2m = lambda: P.DPMSolverSampler(m).sample(St, B, (4, 16, 64), c, unconditional_guidance_scale=scale, unconditional_conditioning=uc, x_T=x)
    ts = ev_ms(run2m, a.iters)
    med = statistics.median(ts)
    emit(what="2M", precision=m.engine.precision, B=B, steps=St, ms_median=round(med, 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
         steps_per_s=round(1000.0 * St / med, 1), iters=a.iters)
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
