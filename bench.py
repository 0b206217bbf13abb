#!/usr/bin/env python
"""bench.py -- denoise steps/s of the Stage-2 sampling path on MI355X (BASELINE.json metric).

One "step" = one DDIM denoise step of one batch: CFG UNet evaluation on N = 2B latents (batch duplication, UNet
forward, guidance combine) + the DDIM update, exactly the body of ddim.py:206-227.  Workload = BASELINE.json
configs[1]: B = 4 per GPU, 8 s audio latent (4x16x64), 32 CAVP context frames, guidance 4.5, 16-bit MFMA operands (fp16
headline -- the operand type that meets the north-star tolerance -- with the bf16 build timed beside it in `modes`),
procedurally generated weights of the full 860 M-parameter UNet (no checkpoint is reachable offline).
The engine is the PRODUCT's: no tuning call, plans from the shipped table of the GPU (diff_foley_amd/tuned/).

A plain run sets up, warms up, times the K steps and prints the headline line (`value`, `ms_per_step`, `dtype`, ...).
Everything else moves behind --full: the instrumented per-kernel-family pass (`roofline`, `kernel_ms_per_step`,
`north_star_families`, --dump-ops), `sampler_loop` (the same workload through LatentDiffusion.sample_log_diff_sampler),
`vae_decode_roofline`, `batch8`, `config2_classifier_guided`, `modes` (the other operand type, the in-bench golden check and
`modes.untuned`: the cost-model plans in a child process) and `cpu_baseline`; the --no-* switches trim that set.
--dump-outputs DIR writes what the last timed step computed (latent, pred_x0, guided eps) as float32 .npy files; the inputs
are seeded, so two builds run with the same arguments can be compared output for output.

    python bench.py --gpus 1 --steps 25 --warmup 3 [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import diff_foley_amd as P  # noqa: E402
from diff_foley_amd import engine as E, parallel, synth  # noqa: E402
from diff_foley_amd.schedule import DDIMTables  # noqa: E402

GFLOP_PER_SAMPLE = 177.86          # one UNet forward (SURVEY.md section 6 / BASELINE.md section 3)
GEMM_GFLOP_PER_SAMPLE = 169.83     # conv 110.99 + Linear 58.85 (the MFMA implicit-GEMM kernel family)
PEAK_BF16_TFLOPS = 2500.0          # dense MFMA bf16 (MI355X_MICROARCH.md)


def cpu_baseline(sd, nsteps):
    """The oracle (CPU restatement of the reference sampler, fp32) timed on this box's host cores:
    BASELINE.json configs[0]: B=1, CFG 4.5 (UNet batch 2), DDIM.  Bounded sample: `nsteps` steps at the fastest thread
    count (32: measured on the 128-core GPU box -- 8: 0.5, 16: 0.78, 32: 0.80, 64: 0.46, 128: 0.20 steps/s) and, side by
    side, nsteps/2 steps on 8 threads, the thread count of the build container's reference probe."""
    from oracle import unet as ou, vae as ov, schedule as osch
    usd = ou.sub_state_dict(sd, "model.diffusion_model.")
    csd = ou.sub_state_dict(sd, "cond_stage_model.")
    c = ov.cond_stage(csd, synth.synthetic_cavp(1))
    uc = torch.zeros_like(c)
    sch = osch.ddim_schedule(osch.ddpm_schedule()["alphas_cumprod"], 25)
    steps = np.flip(sch["timesteps"])

    def one(i, x):
        idx = 25 - i - 1
        ts = torch.full((2,), int(steps[i]), dtype=torch.long)
        e_u, e_c = ou.unet_forward(usd, synth.UNET_FULL, torch.cat([x, x]), ts, torch.cat([uc, c])).chunk(2)
        e = e_u + 4.5 * (e_c - e_u)
        a_t, a_p = float(sch["alphas"][idx]), float(sch["alphas_prev"][idx])
        p0 = (x - float(sch["sqrt_one_minus_alphas"][idx]) * e) / a_t ** 0.5
        return a_p ** 0.5 * p0 + (1 - a_p) ** 0.5 * e

    def timed(threads, n):
        torch.set_num_threads(min(threads, os.cpu_count() or 1))
        x = one(0, synth.synthetic_xT(1))          # warm-up (thread pools, allocator)
        t0 = time.perf_counter()
        for i in range(1, 1 + n):
            x = one(i, x)
        return n / (time.perf_counter() - t0), time.perf_counter() - t0, torch.get_num_threads()
    v32, dt32, th32 = timed(32, nsteps)
    v8, dt8, th8 = timed(8, max(2, nsteps // 2))
    return dict(value=v32, unit="denoise_steps/s at B=1 (UNet batch 2)", cores=th32, kind="port",
                sample=f"{nsteps} DDIM steps of BASELINE config[0] (B=1, CFG 4.5, fp32, oracle/unet.py), {dt32:.1f} s of CPU "
                       f"work on {th32} threads; side by side: {max(2, nsteps // 2)} steps on {th8} threads, {dt8:.1f} s",
                threads_8={"value": v8, "cores": th8}, host_cores=os.cpu_count())


def pmc_traffic(key="gemm_bytes_per_step"):
    """HBM-side bytes per GEMM launch (FETCH_SIZE x2 per the gfx950 calibration + WRITE_SIZE, separate --pmc passes of
    this same command; tools/pmc_traffic.sh).  rocprofv3 cannot run inside the timed process, so the number is read
    from the committed profile of the current round; null when absent."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            return json.load(f)[key]
    except Exception:
        return None


def sq_counters():
    """MFMA-pipe busy fraction per kernel family from the SQ counters of this same command (tools/sq_counters.sh: two rocprofv3
    --pmc passes; SQ_VALU_MFMA_BUSY_CYCLES / (32 x SQ_BUSY_CYCLES)), read from the committed profile of the current round."""
    try:
        with open(os.path.join(ROOT, "profiles", "sq_counters.json")) as f:
            d = json.load(f)
        return {k: round(v["mfma_busy"], 4) for k, v in d["families"].items() if v.get("mfma_busy") is not None}
    except Exception:
        return None


def measured_peak():
    """MFMA issue peak measured on an MI355X by tools/peaks.py (profiles/peaks.json), next to the nominal one."""
    try:
        with open(os.path.join(ROOT, "profiles", "peaks.json")) as f:
            return json.load(f)["mfma_bf16_tflops"]
    except Exception:
        return None


GOLD = os.path.join(ROOT, "tests", "golden", "g5_full_samplers.npz")


def golden_mel_mae(model, dev):
    """North-star parity metric, measured inside the bench: 25-step DDIM (CFG 4.5, B=1, seed 21) + decode_first_stage
    against the REFERENCE's own output for the same inputs (tests/golden/g5_full_samplers.npz, made by
    tests/golden/make_golden.py from /root/reference; a fixture, not the oracle).  Mean absolute error of the mel."""
    if not os.path.exists(GOLD):
        return None
    g = np.load(GOLD)
    xT = synth.synthetic_xT(1, seed=21).to(dev)
    c = model.get_learned_conditioning(synth.synthetic_cavp(1, 32, 512, seed=1234).to(dev))
    z, _ = model.sample_log_diff_sampler(c, 1, "DDIM", 25, unconditional_guidance_scale=4.5,
                                         unconditional_conditioning=torch.zeros_like(c), x_T=xT)
    mel = model.decode_first_stage(z)[:, 0].cpu().numpy()
    ref = g["ddim25_mel_21"]
    mae = float(np.abs(mel - ref).mean())
    span = float(ref.max() - ref.min())
    # parity_ok is the north-star bound as BASELINE.json words it: MAE < 1e-3 in mel units (absolute).  The fp16 operand
    # build meets it; the bf16 build (2^-9 per operand) does not and says so.  The range-normalised figure (MAE below 1e-3
    # of the mel range of this random-weight model; training mels live in [0, 1]) is the regression tripwire both builds
    # must pass (tests/test_path_gpu.py::test_full_ddim25_mel_mae).
    ok_abs = mae < 1e-3
    ok_rng = mae / span < 1e-3
    if not ok_rng:
        print(f"bench.py: PARITY REGRESSION -- mel MAE {mae:.3e} over a range of {span:.2f} exceeds 1e-3 of the range",
              file=sys.stderr, flush=True)
    return dict(mel_mae=mae, mel_range=span, mel_std=float(ref.std()), parity_ok=bool(ok_abs),
                parity_ok_range_normalised=bool(ok_rng),
                z_rel_l2=float(np.linalg.norm(z.cpu().numpy() - g["ddim25_z_21"]) / np.linalg.norm(g["ddim25_z_21"])))


def run_mode(precision, sd_dev, a, dev, rank, world, lo, hi, barrier, dump_ops=""):
    """Builds the engine for one MFMA operand type and times K denoise steps of this rank's shard."""
    B = a.batch
    t0 = time.perf_counter()
    model = P.LatentDiffusion(precision=precision, **P.stage2_config())
    if rank == 0:
        model.load_state_dict(sd_dev)
    model.cuda(dev)
    # The product default (round 6): the plans come from the shipped table of this GPU model (diff_foley_amd/tuned/, imported by
    # Engine.__init__) -- no tuning call, exactly what a notebook user gets.  --autotune re-tunes in this process instead.
    if rank == 0 and a.autotune:
        model.autotune(True)
    dist_info = None
    if world > 1:      # rank 0 packs ONCE, one broadcast of the packed operand blob (RCCL over xGMI), the others import
        dist_info = parallel.broadcast_packed_model(model, B, src=0)
        if rank != 0 and a.autotune:
            model.autotune(True)
    feats = synth.synthetic_cavp(B * world)[lo:hi].to(dev)
    x = synth.synthetic_xT(hi - lo, first_index=lo).to(dev)
    c = model.get_learned_conditioning(feats)
    uc = torch.zeros_like(c)
    eng = model.engine
    eng.set_context(torch.cat([uc, c]))
    tb = DDIMTables(model.alphas_cumprod, 25)
    steps = np.flip(tb.timesteps)
    t_all = torch.tensor(steps.copy(), dtype=torch.float32, device=dev)[:, None].expand(25, B).contiguous()
    # like the context, the time embedding of the 25 steps is announced before the loop (what DDIMSampler.sample does):
    # it depends on t only; a step then looks its row up (df_unet_set_timesteps / df_unet_forward_cfg_ts)
    hoist = not a.no_time_hoist
    if hoist:
        eng.set_timesteps([float(v) for v in steps], B, 16, 64, True)

    last = {}       # the last step's other results (fresh tensors every step), for --dump-outputs

    def step(i, x):
        i = i % 25
        idx = 25 - i - 1
        e = eng.unet_forward_cfg(x, t_all[i], 4.5, ts_index=i if hoist else None)
        xn, p0 = E.ddim_update(x, e, tb.alphas[idx], tb.alphas_prev[idx], 0.0, tb.sqrt_one_minus_alphas[idx])
        last["pred_x0"], last["eps"] = p0, e
        return xn

    for i in range(a.warmup):
        x = step(i, x)
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0
    barrier()
    t0 = time.perf_counter()
    for i in range(a.steps):
        x = step(a.warmup + i, x)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    assert torch.isfinite(x).all() or os.environ.get("DF_GEMM_DBG")
    outputs = {"latent": x, "pred_x0": last["pred_x0"], "eps": last["eps"]}
    if not a.full:
        return dict(model=model, dt=dt, outputs=outputs, stats=eng.plan_stats(), t_setup=t_setup,
                    dist=gather_dist_info(dist_info, dev, rank, world), plan_source=plan_source_of(a, eng))

    # ---- per-kernel-family time: HIP events on the launch stream around every op of the same K steps (second,
    # instrumented pass; the events themselves cost ~2 us per op, so the family times are NORMALISED to the
    # un-instrumented step time before any rate is derived from them)
    eng.profile_begin()
    for i in range(a.steps):
        x = step(a.warmup + i, x)
    prof = eng.profile_end()
    sub = None
    if rank == 0:
        import csv
        import tempfile
        dump = dump_ops or os.path.join(tempfile.gettempdir(), f"df_ops_{os.getpid()}.csv")
        eng.profile_dump(dump)
        rows = list(csv.DictReader(open(dump)))
        if rows and len(rows) % a.steps == 0:
            n = len(rows) // a.steps
            for i in range(n):
                rows[i]["ms"] = "%.5f" % (sum(float(rows[i + k * n]["ms"]) for k in range(a.steps)) / a.steps)
            rows = rows[:n]
            if dump_ops:
                with open(dump, "w", newline="") as f:
                    w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
                    w.writeheader()
                    w.writerows(rows)
            st_ms = sum(float(r["ms"]) for r in rows if r["tag"].startswith(("st.", "attn.")) or r["tag"] == "layernorm")
            rc_ms = sum(float(r["ms"]) for r in rows if r["tag"] in ("res.conv1", "res.conv2"))
            sub = {"st_ms": st_ms, "rc_ms": rc_ms, "st_launches": sum(1 for r in rows if r["tag"].startswith(("st.", "attn.")) or r["tag"] == "layernorm")}
        if not dump_ops:
            os.remove(dump)
    # ---- the same workload through the reference-shaped entry point (LatentDiffusion.sample_log_diff_sampler: Python DDIM
    # loop, set_context once per call, intermediates bookkeeping): 4 calls x 25 steps, reported beside the headline
    loop = None
    if rank == 0:
        x0 = synth.synthetic_xT(hi - lo, first_index=lo).to(dev)
        model.sample_log_diff_sampler(c, hi - lo, "DDIM", 25, unconditional_guidance_scale=4.5, unconditional_conditioning=uc, x_T=x0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ncall = 4
        for _ in range(ncall):
            model.sample_log_diff_sampler(c, hi - lo, "DDIM", 25, unconditional_guidance_scale=4.5, unconditional_conditioning=uc, x_T=x0)
        torch.cuda.synchronize()
        dl = time.perf_counter() - t1
        loop = {"steps": 25 * ncall, "steps_per_s": round(25 * ncall / dl, 3), "ms_per_step": round(dl / (25 * ncall) * 1e3, 4),
                "what": "LatentDiffusion.sample_log_diff_sampler('DDIM', 25 steps, CFG 4.5) x 4 calls incl. set_context per call"}
    return dict(model=model, dt=dt, outputs=outputs, prof=prof, sub=sub, stats=eng.plan_stats(), t_setup=t_setup,
                dist=gather_dist_info(dist_info, dev, rank, world), loop=loop, plan_source=plan_source_of(a, eng))


def gather_dist_info(dist_info, dev, rank, world):
    """N > 1: every rank's pack / broadcast / import seconds in the one JSON line (first real SCALE run shows them)."""
    if world == 1:
        return dist_info
    infos = [None] * world
    # what each rank saw of the job: the world size of its process group on its backend ("nccl" = RCCL), the device it
    # computes on and that device's PCI bus id -- a SCALE run with two ranks on one GPU, or a rank that fell back to gloo,
    # shows in the line itself
    try:
        bus = torch.cuda.get_device_properties(dev).pci_bus_id
    except Exception:
        bus = None
    seen = dict(rccl_world_seen=torch.distributed.get_world_size(), pg_backend=torch.distributed.get_backend(),
                cuda_device=torch.cuda.current_device(), pci_bus_id=bus, gpu_name=torch.cuda.get_device_name(dev))
    torch.distributed.all_gather_object(infos, dict(rank=rank, **seen, **{k: (round(v, 4) if isinstance(v, float) else v)
                                                                         for k, v in (dist_info or {}).items()}))
    return {"per_rank": infos}


def plan_source_of(a, eng):
    return ("autotuned in this process (--autotune)" if a.autotune else
            (f"shipped table {os.path.relpath(eng.tuned_defaults, ROOT)}" if eng.tuned_defaults else
             "cost-model tiles (DF_TUNED_DEFAULTS=0 or no table for this device)"))


def dump_outputs(outputs, path, rank, world):
    """--dump-outputs: the last timed step's results as float32 .npy files, every rank's shard in global sample order."""
    arrays = {k: v.detach().float().cpu().numpy() for k, v in outputs.items()}
    if world > 1:
        shards = [None] * world
        torch.distributed.all_gather_object(shards, arrays)
        arrays = {k: np.concatenate([s[k] for s in shards]) for k in arrays}
    if rank == 0:
        os.makedirs(path, exist_ok=True)
        for k, v in arrays.items():
            np.save(os.path.join(path, k + ".npy"), v.astype(np.float32))


def batch8_block(model, dev, steps, warmup):
    """BASELINE configs[2]'s step shape on the headline engine: sampler batch 8 (UNet batch 16), same loop body as the headline
    (CFG forward with hoisted time embedding + DDIM update).  Reported beside the B = 4 headline: more rows per launch."""
    B = 8
    eng = model.engine
    c = model.get_learned_conditioning(synth.synthetic_cavp(B).to(dev))
    eng.set_context(torch.cat([torch.zeros_like(c), c]))
    tb = DDIMTables(model.alphas_cumprod, 25)
    ts = np.flip(tb.timesteps)
    t_all = torch.tensor(ts.copy(), dtype=torch.float32, device=dev)[:, None].expand(25, B).contiguous()
    eng.set_timesteps([float(v) for v in ts], B, 16, 64, True)
    x = synth.synthetic_xT(B).to(dev)

    def step(i, x):
        i = i % 25
        idx = 25 - i - 1
        e = eng.unet_forward_cfg(x, t_all[i], 4.5, ts_index=i)
        return E.ddim_update(x, e, tb.alphas[idx], tb.alphas_prev[idx], 0.0, tb.sqrt_one_minus_alphas[idx])[0]
    for i in range(warmup):
        x = step(i, x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        x = step(warmup + i, x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = dt / steps * 1e3
    return {"batch": B, "unet_batch": 2 * B, "steps": steps, "steps_per_s": round(steps / dt, 3), "ms_per_step": round(ms, 4),
            "samples_steps_per_s": round(B * steps / dt, 2),
            "step_tflops_algorithmic": round(GFLOP_PER_SAMPLE * 2 * B / ms, 2),
            "frac_of_mfma_peak": round(GFLOP_PER_SAMPLE * 2 * B / ms / PEAK_BF16_TFLOPS, 4)}


def config2_block(model, dev):
    """BASELINE configs[2] as the facade runs it: batch 8, 50-step DPM-Solver++(2M), CFG 4.5 + the double-guidance classifier in the
    loop (sample_log_with_classifier_diff_sampler on the headline model; full-size classifier, procedural weights).  One warm-up
    call, then the better of two timed calls.  `one_stream` = the classifier gradient behind the UNet step on the same stream
    (DF_CLS_OVERLAP=0, the order of rounds 1-5) instead of beside it on a second stream (the product default since round 6)."""
    B, S = 8, 50
    cls = P.AlignmentClassifier(classifier_config=dict(params=dict(synth.CLS_FULL)))
    cls.load_state_dict(synth.make_state_dict(synth.classifier_spec(synth.CLS_FULL), 0))
    cls.attach(model)
    feats = synth.synthetic_cavp(B, 33).to(dev)
    xT = synth.synthetic_xT(B).to(dev)
    c = model.get_learned_conditioning(feats[:, :32])
    uc = torch.zeros_like(c)

    def run():
        best = None
        for it in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            z, _ = model.sample_log_with_classifier_diff_sampler(c, origin_cond=feats, batch_size=B, sampler_name="DPM_Solver", ddim_steps=S,
                                                                 unconditional_guidance_scale=4.5, unconditional_conditioning=uc,
                                                                 classifier=cls, classifier_guide_scale=50.0, x_T=xT)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it and (best is None or dt < best):
                best = dt
        return best, bool(torch.isfinite(z).all())
    keep = os.environ.get("DF_CLS_OVERLAP")
    try:
        os.environ.pop("DF_CLS_OVERLAP", None)
        dt, finite = run()
        os.environ["DF_CLS_OVERLAP"] = "0"
        dt0, _ = run()
    finally:
        if keep is None:
            os.environ.pop("DF_CLS_OVERLAP", None)
        else:
            os.environ["DF_CLS_OVERLAP"] = keep
    return {"batch": B, "sampler": "DPM-Solver++(2M)", "nfe": S, "steps_per_s": round(S / dt, 2), "ms_per_sample_call": round(dt * 1e3, 1),
            "finite": finite, "one_stream": {"steps_per_s": round(S / dt0, 2), "ms_per_sample_call": round(dt0 * 1e3, 1)},
            "what": "LatentDiffusion.sample_log_with_classifier_diff_sampler, classifier gradient on a second HIP stream beside the UNet step"}


def untuned_child(a):
    """`modes.untuned`: the same command in a child process with DF_TUNED_DEFAULTS=0 (the shipped table is imported once per
    process and library, so the cost-model plans need a fresh process): headline loop, instrumented pass and sampler loop."""
    import subprocess
    env = dict(os.environ, DF_TUNED_DEFAULTS="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK", "LOCAL_WORLD_SIZE", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)          # a plain single-process child even when this process was started by torch.distributed.run
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--batch",
           str(a.batch), "--precision", a.precision, "--full", "--no-cpu-baseline", "--no-modes", "--no-vae", "--no-batch8"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
        return {"steps_per_s": d["value"], "ms_per_step": d["ms_per_step"], "plan": d["config"].get("plan_source"),
                "launches_per_step": d["plan"]["launches"], "sampler_loop_steps_per_s": (d.get("sampler_loop") or {}).get("steps_per_s")}
    except Exception as ex:
        return {"error": str(ex)[:200]}


def vae_roofline(model, dev, B):
    """decode_first_stage at batch B (622.2 GFLOP and 0.0989 + 0.6096 B GB of algorithmic traffic)."""
    z = synth.synthetic_xT(B).to(dev)
    for _ in range(6):
        model.decode_first_stage(z)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    n = 5
    for _ in range(n):
        model.decode_first_stage(z)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    gflop, gb = 622.2 * B, 0.0989 + 0.6096 * B
    return {"batch": B, "ms": round(ms, 3), "algorithmic_gflop": gflop, "algorithmic_gb": round(gb, 4),
            "tflops": round(gflop / ms, 1), "frac_of_mfma_peak": round(gflop / ms / PEAK_BF16_TFLOPS, 4),
            "gb_per_s": round(gb / ms * 1e3, 1), "frac_of_hbm_peak": round(gb / ms * 1e3 / 8000.0, 4),
            "bound": "mfma (1005 FLOP/B algorithmic) -- measured far below both ceilings: see profiles/"}


def self_launch(n):
    """Re-executes this script as n ranks of one node: `python -m torch.distributed.run --nnodes=1 --nproc-per-node n
    --master-addr 127.0.0.1 --master-port <free> bench.py <same arguments>` (the form the driver uses for N > 1)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")         # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4, help="samples per GPU (UNet batch is 2x this)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=8)
    ap.add_argument("--autotune", action="store_true", help="re-tune the plans in this process instead of using the shipped table")
    ap.add_argument("--no-autotune", action="store_true", help="(accepted for older command lines; not tuning is the default now)")
    ap.add_argument("--no-batch8", action="store_true", help="skip the configs[2]-shape (B = 8) step block")
    ap.add_argument("--no-modes", action="store_true", help="skip the second operand type and the in-bench golden check")
    ap.add_argument("--no-vae", action="store_true", help="skip the VAE decode roofline block (profiling runs of the step only)")
    ap.add_argument("--precision", default="fp16", choices=["bf16", "fp16"],
                    help="MFMA operand type of the headline value.  fp16 (libdfengine_f16.so) is the default: same MFMA rate and "
                         "the operand type that meets the north-star bound (mel MAE < 1e-3 absolute); bf16 = the literal "
                         "wording of BASELINE configs[1], reported beside it in `modes` (mel MAE 4e-3)")
    ap.add_argument("--dump-ops", default="", help="write a per-op CSV of the instrumented pass (--full)")
    ap.add_argument("--no-time-hoist", action="store_true",
                    help="compute the time embedding inside every step (4 launches) instead of once per sample() call")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the instrumented per-family pass (roofline, kernel times), sampler_loop, "
                         "vae_decode_roofline, batch8, config2_classifier_guided, modes and cpu_baseline (--no-* trim the set)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's latent, pred_x0 and guided eps (every rank's shard) to DIR/<name>.npy, float32")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.dump_ops and not a.full:
        ap.error("--dump-ops writes the per-op CSV of the instrumented pass, which runs under --full")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU, torch.distributed.run on a free
        # local port); rank 0 of that job prints the one JSON line, which passes through this process's stdout
        return self_launch(a.gpus)
    rank, world, local = parallel.init_process_group()
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world} (launcher and flag disagree)")
    dev = torch.device("cuda", local)
    B = a.batch
    G = B * world                                           # weak scaling: fixed per-GPU batch

    # ---- weights: generated on rank 0 only; for N > 1 rank 0 packs them once into the MFMA operand layouts and ONE
    # broadcast of that blob (RCCL over xGMI) feeds every other rank (parallel.broadcast_packed_model)
    spec = synth.state_dict_spec()
    sd = synth.make_state_dict(spec, 0) if rank == 0 else None
    sd_dev = sd

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    lo, hi = parallel.shard_range(G, rank, world)
    main_run = run_mode(a.precision, sd_dev, a, dev, rank, world, lo, hi, barrier, a.dump_ops)
    dt, stats = main_run["dt"], main_run["stats"]
    if a.dump_outputs:
        dump_outputs(main_run["outputs"], a.dump_outputs, rank, world)

    if rank == 0:
        ms_step = dt / a.steps * 1e3
        per_gpu = a.steps / dt
        N = 2 * B
        name = {"bf16": "bf16", "fp16": "f16"}
        out = {
            "metric": "UNet denoise steps/sec (8s audio latent, 25-step DDIM, CFG 4.5), aggregate over GPUs",
            "value": round(per_gpu * world, 3),
            "unit": "denoise_steps/s",
            "per_gpu": round(per_gpu, 3),
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": name[a.precision],
            "data": "synthetic (procedural weights of the full 859.5M-param UNet, unit-norm CAVP-like features, seeded x_T)",
            "config": {"workload": "BASELINE.json configs[1]: single MI355X, batch=4 (UNet batch 8), 25-step DDIM, "
                                   + ("bf16" if a.precision == "bf16" else "fp16 (16-bit MFMA operands at the bf16 rate; the "
                                      "operand type that meets mel MAE < 1e-3 -- the bf16 build is timed in `modes`)")
                                   + " UNet, 32 CAVP context frames, latent 4x16x64, guidance 4.5",
                       "batch_per_gpu": B, "global_batch": G, "parallelism": f"batch-shard x{world}, no step-loop collectives",
                       "time_embedding": ("inside every step" if a.no_time_hoist else
                                          "hoisted: all 25 timesteps by df_unet_set_timesteps before the loop, as DDIMSampler.sample "
                                          "does (depends on t only, like the context operands); a step does one table look-up"),
                       "plan_source": main_run["plan_source"],
                       "weight_distribution": main_run["dist"],
                       "engine_setup_s": round(main_run["t_setup"], 3)},
            "step_tflops_algorithmic": round(GFLOP_PER_SAMPLE * N / ms_step, 2),
        }
        if a.full:
            prof, sub = main_run["prof"], main_run["sub"]
            inst_total = sum(v["ms"] for v in prof.values()) / a.steps            # instrumented: includes event overhead
            norm = ms_step / inst_total                                          # -> family times that sum to ms_per_step
            fam_ms = {k: v["ms"] / a.steps * norm for k, v in prof.items()}
            gemm_ms = fam_ms["gemm"]
            gemm_launches = prof["gemm"]["launches"] // a.steps
            gemm_tflops = GEMM_GFLOP_PER_SAMPLE * N / gemm_ms            # GFLOP / ms = TFLOP/s
            out.update({
                "roofline": {"bound": "mfma", "kernel": "gemm_bf16_kernel / conv3x3_halo_kernel (implicit-GEMM conv3x3/1x1/linear, all tile shapes, incl. split-K reduce)",
                             "achieved": round(gemm_tflops, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(gemm_tflops / PEAK_BF16_TFLOPS, 4),
                             "launches_per_step": int(gemm_launches), "avg_launch_us": round(gemm_ms * 1e3 / max(1, gemm_launches), 2),
                             "algorithmic_gflop_per_step": round(GEMM_GFLOP_PER_SAMPLE * N, 1),
                             "family_ms_per_step": round(gemm_ms, 4),
                             "time_source": "HIP events around every op of the K steps on the launch stream, normalised so that the "
                                            "families sum to the un-instrumented ms_per_step (events add ~2 us per op)",
                             "traffic": pmc_traffic("gemm_bytes_per_step"), "traffic_unit": "HBM-side bytes per STEP of this kernel family (2 x FETCH_SIZE + WRITE_SIZE)",
                             "traffic_per_launch": pmc_traffic("gemm_bytes_per_launch"),
                             "algorithmic_bytes_per_step": round((1.7186 + 0.4478 * B) * 1e9),
                             "traffic_source": "profiles/pmc_traffic.json (rocprofv3 --pmc passes of this command; not measured in this run)",
                             "peak_measured": measured_peak(), "peak_measured_source": "profiles/peaks.json (tools/peaks.py on an MI355X; not measured in this run)",
                             "mfma_busy_pmc": sq_counters(), "mfma_busy_pmc_source": "profiles/sq_counters.json (SQ_VALU_MFMA_BUSY_CYCLES / (32 x SQ_BUSY_CYCLES) per kernel "
                                                                                  "family over 4 denoise steps of this command; includes the matrix pipe's time on padded tiles, "
                                                                                  "so it sits above the algorithmic frac; not measured in this run)"},
                "north_star_families": None if not sub else {
                    "spatial_transformer": {"algorithmic_gflop_per_step": round(73.22 * N, 1), "ms_per_step": round(sub["st_ms"] * norm, 4),
                                            "launches_per_step": sub["st_launches"],
                                            "tflops": round(73.22 * N / (sub["st_ms"] * norm), 1),
                                            "frac_of_mfma_peak": round(73.22 * N / (sub["st_ms"] * norm) / PEAK_BF16_TFLOPS, 4)},
                    "resblock_conv3x3": {"algorithmic_gb_per_step": round(1.0235 + 0.0403 * N, 4), "ms_per_step": round(sub["rc_ms"] * norm, 4),
                                         "gb_per_s": round((1.0235 + 0.0403 * N) / (sub["rc_ms"] * norm) * 1e3, 1),
                                         "frac_of_hbm_peak": round((1.0235 + 0.0403 * N) / (sub["rc_ms"] * norm) * 1e3 / 8000.0, 4),
                                         "tflops": round(81.62 * N / (sub["rc_ms"] * norm), 1)}},
                "sampler_loop": main_run["loop"],
                "kernel_ms_per_step": {k: round(v, 4) for k, v in fam_ms.items()},
                "kernel_ms_per_step_instrumented": {k: round(v["ms"] / a.steps, 4) for k, v in prof.items()},
                "kernel_launches_per_step": {k: int(v["launches"] // a.steps) for k, v in prof.items()},
            })
        out["plan"] = stats
        if a.full and world == 1 and not a.no_vae:
            out["vae_decode_roofline"] = vae_roofline(main_run["model"], dev, B)
        if a.full and world == 1 and not a.no_batch8:
            out["batch8"] = batch8_block(main_run["model"], dev, max(10, a.steps // 2), a.warmup)
            try:
                out["config2_classifier_guided"] = config2_block(main_run["model"], dev)
            except Exception as ex:      # must not hide the headline number
                out["config2_classifier_guided"] = {"error": f"{type(ex).__name__}: {ex}"}
        if a.full and world == 1 and not a.no_modes:
            # both MFMA operand types in ONE driver-run line: steps/s of the same workload + the north-star parity metric
            # (mel MAE of a 25-step DDIM sample against the reference's golden output) measured in this very process
            modes = {}
            par = golden_mel_mae(main_run["model"], dev)
            modes[name[a.precision]] = {"steps_per_s": round(per_gpu, 3), "ms_per_step": round(ms_step, 4), "parity_vs_reference": par}
            other = "fp16" if a.precision == "bf16" else "bf16"
            try:
                o = run_mode(other, sd_dev, a, dev, rank, world, lo, hi, barrier)
                modes[name[other]] = {"steps_per_s": round(a.steps / o["dt"], 3), "ms_per_step": round(o["dt"] / a.steps * 1e3, 4),
                                      "parity_vs_reference": golden_mel_mae(o["model"], dev)}
                del o
            except Exception as ex:      # a missing second build must not hide the headline number
                modes[name[other]] = {"error": str(ex)[:200]}
            modes["untuned"] = untuned_child(a)
            out["modes"] = modes
            out["parity_target"] = "north_star: mel-spec MAE < 1e-3 vs the CPU reference (absolute, mel units); " \
                                   "golden = tests/golden/g5_full_samplers.npz (reference output, B=1, seed 21)"
        del main_run
        if a.full and not a.no_cpu_baseline and world == 1:       # reported at N=1 only (rank 0's host cores)
            out["cpu_baseline"] = cpu_baseline(sd, a.cpu_steps)
        print(json.dumps(out))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
