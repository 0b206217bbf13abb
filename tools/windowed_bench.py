#!/usr/bin/env python
"""Full-size timing of a clip longer than one window: a windowed DDIM with CFG 4.5 at B = 4,
T = 64 frames, hop = 16 (K = 3 windows, 12 window rows per UNet call), the two kernels of csrc/windows.hip on that step's shapes, and
beside it the reference notebook's way for the same clip -- K' = T // 32 = 2 independent 32-frame calls at B = 4, one after another.

    python tools/windowed_bench.py [--steps 25] [--repeats 3] [--precision fp16] [--batch 4] [--frames 64] [--hop 16]

Needs the GPU (there is no CPU path).  Procedural weights (synth.make_state_dict, seed 0): the timing does not depend on the values.
Every figure is a host clock around work that ends in a device synchronise, after one warm-up run of the same shapes; the kernel
times are HIP events around 200 back-to-back launches.  Prints one JSON line.  Nothing is asserted: this tool records what the
construction costs, it claims no speed-up."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--hop", type=int, default=16)
    ap.add_argument("--tiny", action="store_true", help="the tiny configuration of the tests (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()

    import torch
    import diff_foley_amd as P
    from diff_foley_amd import engine as E, synth
    if not torch.cuda.is_available():
        raise SystemExit("windowed_bench: no GPU (there is no CPU path, and a CPU time would say nothing)")
    cfgs = (synth.UNET_TINY, synth.VAE_TINY, synth.COND_TINY) if a.tiny else (None, None, None)
    spec = synth.state_dict_spec(*cfgs) if a.tiny else synth.state_dict_spec()
    m = P.LatentDiffusion(precision=a.precision, **P.stage2_config(*cfgs))
    m.load_state_dict(synth.make_state_dict(spec, 0))
    m.cuda()
    B, T = a.batch, a.frames
    dim = m.cond_cfg["origin_dim"]
    feats = synth.synthetic_cavp(B, T, dim).cuda()
    cw = m.get_windowed_conditioning(feats, hop=a.hop)
    W = cw.size_len_total
    xT = torch.randn(B, m.channels, 16, W, generator=torch.Generator().manual_seed(3)).cuda()

    def timed(fn):
        fn()                                  # warm-up: plans, code objects, the tables of the geometry
        torch.cuda.synchronize()
        best = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best.append(time.perf_counter() - t0)
        return best

    def windowed():
        return m.sample_log_diff_sampler(cw, B, "DDIM", a.steps, size_len=W, unconditional_guidance_scale=4.5,
                                         unconditional_conditioning=cw.zeros_like(), x_T=xT)[0]

    n_calls = T // 32                          # the notebook: window_num = feat_len // 32, the tail frames dropped
    conds = [m.get_learned_conditioning(feats[:, i * 32:(i + 1) * 32]) for i in range(n_calls)]
    x64 = [xT[..., i * 64:(i + 1) * 64].contiguous() for i in range(n_calls)]

    def notebook():
        return [m.sample_log_diff_sampler(c, B, "DDIM", a.steps, unconditional_guidance_scale=4.5,
                                          unconditional_conditioning=torch.zeros_like(c), x_T=x)[0] for c, x in zip(conds, x64)]

    tw, tn = timed(windowed), timed(notebook)

    # the two kernels alone, on the step's shapes
    n_it = 200
    win = E.window_gather(xT, cw.col_starts, cw.size_len)
    E.window_blend(win, cw.col_starts, W)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(n_it):
        E.window_gather(xT, cw.col_starts, cw.size_len)
    ev[1].record()
    for _ in range(n_it):
        E.window_blend(win, cw.col_starts, W)
    ev[2].record()
    torch.cuda.synchronize()
    gather_us, blend_us = ev[0].elapsed_time(ev[1]) * 1e3 / n_it, ev[1].elapsed_time(ev[2]) * 1e3 / n_it

    step_ms = min(tw) * 1e3 / a.steps
    print(json.dumps(dict(
        tool="windowed_bench", config="tiny" if a.tiny else "full", precision=m.engine.precision, batch=B, frames=T, hop=a.hop,
        windows=cw.K, window_rows=B * cw.K, latent_width=W, ddim_steps=a.steps, repeats=a.repeats,
        windowed_s=[round(v, 4) for v in tw], windowed_steps_per_s=round(a.steps / min(tw), 2), windowed_step_ms=round(step_ms, 3),
        gather_us_per_call=round(gather_us, 2), blend_us_per_call=round(blend_us, 2),
        window_kernels_share_of_step=round((gather_us + blend_us) * 1e-3 / step_ms, 4),
        notebook_calls=n_calls, notebook_frames_covered=32 * n_calls, notebook_s=[round(v, 4) for v in tn],
        notebook_steps_per_s=round(a.steps / min(tn), 2),
        note="steps/s = solver steps of the whole clip per second; the notebook's way runs its calls one after another")))


if __name__ == "__main__":
    main()
