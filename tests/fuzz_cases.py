"""The cases of the randomised differential tests, in one place: every draw and every seeded input is a function of the seed alone
(and of the ``wide`` flag of the exploratory sweeps), so that three readers see the same case --

  * the GPU fuzz tests (product against the oracle):  test_unet_config_fuzz_gpu.py, test_classifier_config_fuzz_gpu.py,
    test_vae_cond_cavp_fuzz_gpu.py, test_sampler_fuzz_gpu.py;
  * tests/golden/make_golden.py --fuzz, which runs the REFERENCE on them and stores its results (g14_fuzz_<surface>*.npz);
  * test_fuzz_golden_cpu.py, which holds the oracle to those records.

Plain data and functions: no GPU, no fixtures, nothing of the reference.  The second half is the record format the generator writes
and the two tests read.

The generator offsets are part of the cases -- a change to one of them, or to the order of the draws inside a function, changes what
a seed means and needs regenerated records (test_fuzz_golden_cpu.py fails until then)."""
import glob
import json
import os

import numpy as np
import torch

from diff_foley_amd import synth

SURFACES = ("unet", "vae", "cond", "cavp", "classifier", "samplers", "double_guidance")
N_CASES = dict(unet=12, vae=8, cond=6, cavp=6, classifier=10, samplers=16, double_guidance=6)
# classifier: seeds a wider sweep (DF_FUZZ_SEED0=100 DF_FUZZ_CASES=60, round 6) failed on: model_channels 64 with channel_mult [1, 1] --
# the head's conv halves 64 channels to 32, and the backward-data packing refused a Cout that is not a multiple of the 64-channel K step
REGRESSION_SEEDS = dict(unet=[], vae=[], cond=[], cavp=[], classifier=[119, 152], samplers=[], double_guidance=[])


def suite_seeds(surface):
    """The seeds the suite runs, and the records must cover: 0 .. N_CASES - 1 and the regression seeds."""
    return sorted(set(range(N_CASES[surface])) | set(REGRESSION_SEEDS[surface]))


# ----------------------------------------------------------------------------------------------------------------- UNet configurations
# csrc/attention.hip:attention_supported; the suite's draws keep the head dims of the Stage-2 model and the classifier
def _head_dims(wide):
    return (16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 112, 128, 160, 192) if wide else (32, 40, 64, 80, 128, 160)


def unet_draw(seed, wide=False):
    r = np.random.default_rng(4200 + seed)
    head_dims = _head_dims(wide)
    while True:         # channel_mult[0] = 1: the reference's `out` conv takes model_channels inputs (openai_unetmodel.py:682-686)
        mc = int(r.choice([64, 128, 192, 256, 320] if wide else [64, 128, 192]))
        mult = [list(m) for m in ([1, 2], [1, 2, 4], [1, 1, 2], [1, 2, 2, 4], [1, 3], [1, 1], [1, 2, 4, 4])][int(r.integers(0, 7))]
        nrb = int(r.choice([1, 2, 3]))
        levels = len(mult)
        att = sorted(int(2 ** i) for i in range(levels) if r.random() < 0.7)
        # channels of the levels that carry attention (ds = 2^level in attention_resolutions) and of the middle block (always)
        chs = {mc * mult[i] for i in range(levels) if 2 ** i in att} | {mc * mult[-1]}
        heads = [h for h in ((1, 2, 3, 4, 6, 8, 12, 16) if wide else (1, 2, 4, 8)) if all(ch % h == 0 and ch // h in head_dims for ch in chs)]
        if mc * max(mult) <= (1280 if wide else 768) and heads:
            break
    cin, cout = (4, 4) if seed % 2 == 0 else (int(r.choice([1, 3, 8, 9, 16, 64])), int(r.choice([1, 3, 8, 64])))
    cfg = dict(in_channels=cin, out_channels=cout, model_channels=mc, attention_resolutions=att, num_res_blocks=nrb, channel_mult=mult,
               num_heads=int(r.choice(heads)), context_dim=int(r.choice([64, 128, 192, 320])))
    q = 2 ** (levels - 1)
    if wide:
        H = int(r.choice([h for h in (8, 16, 24, 32, 40) if h % q == 0]))
        W = int(r.choice([w for w in (8, 16, 24, 32, 40, 48, 64, 72, 96) if w % q == 0]))
        if mc * max(mult) > 768 and H * W > 512:          # keep the CPU oracle in seconds
            H, W = 8 if 8 % q == 0 else 16, 16
        return cfg, dict(B=int(r.choice([1, 2, 3, 4, 5, 7])), H=H, W=W, T=int(r.choice([1, 2, 9, 31, 32, 33, 40])), seed=seed)
    H = int(r.choice([h for h in (8, 16) if h % q == 0]))
    W = int(r.choice([w for w in (16, 32, 64) if w % q == 0]))
    return cfg, dict(B=int(r.choice([1, 2, 3])), H=H, W=W, T=int(r.choice([1, 9, 32])), seed=seed)


UNET_CFG_SCALE = 3.0      # the guidance scale of the test's classifier-free-guidance call


def unet_case(seed, wide=False):
    """cfg, o, the cond-stage configuration and state dict of the case, and its inputs: x, c, t of the single forward; uc and tt (t[0]
    for every sample) of the classifier-free-guidance call, which runs [uc ; c] on [x ; x] and combines at UNET_CFG_SCALE."""
    cfg, o = unet_draw(seed, wide)
    cond = dict(origin_dim=64, embed_dim=cfg["context_dim"], seq_len=40)
    sd = synth.make_state_dict(synth.state_dict_spec(cfg, synth.VAE_TINY, cond), 100 + seed)
    g = torch.Generator().manual_seed(300 + seed)
    B, H, W, T = o["B"], o["H"], o["W"], o["T"]
    x = torch.randn(B, cfg["in_channels"], H, W, generator=g)
    c = torch.randn(B, T, cfg["context_dim"], generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    uc = 0.3 * torch.randn(B, T, cfg["context_dim"], generator=g)
    tt = torch.full((B,), int(t[0]))
    return dict(cfg=cfg, o=o, cond=cond, sd=sd, x=x, c=c, t=t, uc=uc, tt=tt)


# ----------------------------------------------------------------------------------------------------------- classifier configurations
def classifier_draw(seed, wide=False):
    r = np.random.default_rng(5200 + seed)
    while True:
        mc = int(r.choice([64, 128, 192, 320] if wide else [64, 128]))
        mult = [list(m) for m in ([1, 2], [1, 2, 2], [1, 1, 2], [1, 2, 4], [1, 1])][int(r.integers(0, 5))]
        nrb = int(r.choice([1, 2]))
        levels = len(mult)
        att = sorted(int(2 ** i) for i in range(levels) if r.random() < 0.6)
        chs = {mc * mult[i] for i in range(levels) if 2 ** i in att} | {mc * mult[-1]}
        heads = [h for h in (1, 2, 4, 8, 16) if all(ch % h == 0 and ch // h in (32, 64) for ch in chs)]      # the backward's head dims
        if heads:
            break
    cfg = dict(in_channels=4, out_channels=1, model_channels=mc, attention_resolutions=att, num_res_blocks=nrb, channel_mult=mult,
               num_heads=int(r.choice(heads)), context_dim=int(r.choice([64, 128, 512])))
    q = 2 ** (levels - 1)
    if wide:
        H = int(r.choice([h for h in (8, 16, 24, 32) if h % q == 0]))
        W = int(r.choice([w for w in (8, 16, 24, 32, 40, 64, 96) if w % q == 0]))
        return cfg, dict(B=int(r.choice([1, 2, 3, 4, 5, 8])), H=H, W=W, T=int(r.choice([1, 8, 31, 32, 33, 40])))
    H = int(r.choice([h for h in (8, 16) if h % q == 0]))
    W = int(r.choice([w for w in (16, 32, 64) if w % q == 0]))
    return cfg, dict(B=int(r.choice([1, 2, 3])), H=H, W=W, T=int(r.choice([8, 32, 33])))


def classifier_case(seed, wide=False):
    cfg, o = classifier_draw(seed, wide)
    sd = synth.make_state_dict(synth.classifier_spec(cfg), 500 + seed)
    g = torch.Generator().manual_seed(600 + seed)
    B, H, W, T = o["B"], o["H"], o["W"], o["T"]
    x = torch.randn(B, 4, H, W, generator=g)
    vf = torch.randn(B, T, cfg["context_dim"], generator=g)
    vf = vf / vf.norm(dim=-1, keepdim=True)
    t = torch.randint(0, 1000, (B,), generator=g).float()
    return dict(cfg=cfg, o=o, sd=sd, x=x, vf=vf, t=t)


# ---------------------------------------------------------------------------------------------------------- VAE decoder configurations
def vae_draw(seed, wide=False):
    r = np.random.default_rng(6100 + seed)
    if wide:
        cfg = dict(z_channels=4, embed_dim=4, ch=int(r.choice([64, 128, 192])),
                   ch_mult=[list(m) for m in ([1, 2], [1, 2, 2], [1, 2, 4], [1, 1, 2, 2], [1, 1], [1, 2, 4, 4], [1], [1, 3], [2, 2], [1, 1, 1],
                                              [2, 1])][int(r.integers(0, 11))],
                   num_res_blocks=int(r.choice([1, 2, 3, 4])), out_ch=int(r.choice([1, 2, 3, 4])))
        H, W = [(4, 8), (8, 16), (16, 64), (8, 24), (16, 16), (1, 1), (3, 5), (5, 7), (1, 64), (6, 10), (2, 2), (12, 20)][int(r.integers(0, 12))]
        if cfg["ch"] * max(cfg["ch_mult"]) >= 384 and H * W > 128:
            H, W = 6, 10
        return cfg, dict(B=int(r.choice([1, 2, 3, 5, 9, 17])) if H * W <= 64 else int(r.choice([1, 2, 3])), H=H, W=W)
    cfg = dict(z_channels=4, embed_dim=4, ch=int(r.choice([64, 128])),
               ch_mult=[list(m) for m in ([1, 2], [1, 2, 2], [1, 2, 4], [1, 1, 2, 2], [1, 1], [1, 2, 4, 4])][int(r.integers(0, 6))],
               num_res_blocks=int(r.choice([1, 2, 3])), out_ch=int(r.choice([1, 3])))
    H, W = [(4, 8), (8, 16), (16, 64), (8, 24), (16, 16)][int(r.integers(0, 5))]
    if cfg["ch"] * max(cfg["ch_mult"]) >= 512 and H * W > 256:        # keep the CPU oracle in seconds
        H, W = 8, 16
    return cfg, dict(B=int(r.choice([1, 2, 3, 5])), H=H, W=W)


def vae_case(seed, wide=False):
    cfg, o = vae_draw(seed, wide)
    sd = synth.make_state_dict(synth.state_dict_spec(synth.UNET_TINY, cfg, synth.COND_TINY), 700 + seed)
    z = torch.randn(o["B"], 4, o["H"], o["W"], generator=torch.Generator().manual_seed(800 + seed))
    return dict(cfg=cfg, o=o, sd=sd, z=z)


# ----------------------------------------------------------------------------------------------------------- cond stage configurations
def cond_draw(seed, wide=False):
    """The cond-stage configuration and the (T, B) of the three calls (lengths 1, a random one, seq_len: fewer where they coincide)."""
    r = np.random.default_rng(6300 + seed)
    cond = dict(origin_dim=int(r.choice([64, 128, 512])), embed_dim=int(r.choice([64, 128, 320, 768])), seq_len=int(r.choice([8, 40, 64])))
    if wide:
        cond = dict(origin_dim=int(r.choice([64, 128, 192, 512, 1024])), embed_dim=int(r.choice([64, 128, 192, 320, 768, 1024])),
                    seq_len=int(r.choice([1, 2, 8, 33, 40, 64, 100])))
    lengths = sorted({1, int(r.integers(2, cond["seq_len"] + 1)) if cond["seq_len"] > 1 else 1, cond["seq_len"]})
    calls = [dict(T=T, B=int(r.choice([1, 3, 4]))) for T in lengths]
    return cond, calls


def cond_case(seed, wide=False):
    cond, calls = cond_draw(seed, wide)
    ucfg = dict(synth.UNET_TINY, context_dim=cond["embed_dim"])
    sd = synth.make_state_dict(synth.state_dict_spec(ucfg, synth.VAE_TINY, cond), 900 + seed)
    g = torch.Generator().manual_seed(950 + seed)
    feats = [torch.randn(k["B"], k["T"], cond["origin_dim"], generator=g) for k in calls]
    return dict(cond=cond, calls=calls, ucfg=ucfg, sd=sd, feats=feats)


# ----------------------------------------------------------------------------------------------------------------- CAVP configurations
def cavp_draw(seed, wide=False):
    r = np.random.default_rng(6500 + seed)
    cfg = dict(stage_blocks=[int(v) for v in ([1, 1, 1, 1], [2, 1, 1, 1], [1, 2, 1, 2], [1, 1, 2, 1], [2, 2, 1, 1])[int(r.integers(0, 5))]],
               base_channels=64, embed_dim=int(r.choice([64, 128, 512])))
    n, T, S = int(r.choice([1, 2, 3])), int(r.choice([1, 2, 5, 9])), int(r.choice([64, 96, 160]))
    if wide:
        n, T, S = int(r.choice([1, 2, 3, 5])), int(r.choice([1, 2, 3, 5, 9, 16, 17])), int(r.choice([32, 64, 96, 128, 160, 224]))          # multiples of 32: df_cavp_encode refuses other frame sizes (the path resizes to 224)
        if T * S * S * n > 9 * 160 * 160 * 3:
            n = 1
    return cfg, dict(n=n, T=T, S=S)


def cavp_case(seed, wide=False):
    cfg, o = cavp_draw(seed, wide)
    sd = synth.make_state_dict(synth.cavp_spec(cfg), 1000 + seed)
    v = synth.synthetic_video(o["n"], o["T"], o["S"], seed=1100 + seed)
    return dict(cfg=cfg, o=o, sd=sd, video=v)


# ----------------------------------------------------------------------------------------------------------------------- sampler options
def sampler_draw(seed, wide=False):
    """One option set.  Everything the case needs is a function of the seed."""
    r = np.random.default_rng(7000 + seed)
    name = ["DDIM", "PLMS", "DPM_Solver", "DDPM"][seed % 4]            # every sampler gets its share whatever N_CASES is
    o = dict(name=name, B=int(r.choice([1, 2, 3])), W=int(r.choice([32, 64])), T=int(r.choice([1, 17, 32, 40])))
    if wide:      # exploratory sweeps (DF_FUZZ_WIDE=1): more batches, latent widths (multiples of the UNet's 8 x downsampling) and contexts
        o = dict(name=name, B=int(r.choice([1, 2, 3, 4, 5, 7])), W=int(r.choice([8, 16, 24, 32, 40, 64, 72, 96])),
                 T=int(r.choice([1, 2, 17, 31, 32, 33, 40])))
    o["S"] = int(r.integers(4, 11)) if name != "DPM_Solver" else int(r.choice([2, 3, 7, 12, 16]))
    if name == "DDPM":
        o["S"] = int(r.integers(3, 7))
    if o["S"] == 9 and seed != 0:         # S = 9 is the reference's IndexError case: once is enough
        o["S"] = 8
    o["scale"] = float(r.choice([1.0, 2.5, 4.5, 7.0]))
    o["uc"] = str(r.choice(["zeros", "random", "none"]))
    o["eta"] = float(r.choice([0.0, 0.0, 0.5, 1.0])) if name == "DDIM" else 0.0
    o["temperature"] = float(r.choice([1.0, 0.7, 1.3])) if o["eta"] else 1.0
    o["noise_dropout"] = float(r.choice([0.0, 0.3])) if o["eta"] else 0.0
    o["log_every_t"] = int(r.choice([1, 3, 100]))
    o["inpaint"] = bool(r.random() < 0.35) and name != "DPM_Solver"      # the DPM-Solver sampler's reference drops mask / x0
    o["seed"] = seed
    return o


def sampler_case(seed, wide=False):
    """The option set and its inputs on the tiny configuration (weights: seed 0): unit-norm video features, x_T, the unconditional
    conditioning in cond-stage space (zeros, 0.5 * randn, or None), and x0 / mask when inpainting.  ``q_seed`` seeds the generator that
    q_sample's noise is replayed from, ``noise_seed`` the global generator every other draw of the samplers comes from."""
    o = sampler_draw(seed, wide)
    B, W = o["B"], o["W"]
    g = torch.Generator().manual_seed(9000 + seed)
    feats = torch.randn(B, o["T"], synth.COND_TINY["origin_dim"], generator=g)
    feats = feats / feats.norm(dim=-1, keepdim=True)
    xT = torch.randn(B, 4, 16, W, generator=g)
    cshape = (B, o["T"], synth.COND_TINY["embed_dim"])
    uc_random = 0.5 * torch.randn(cshape, generator=g)        # drawn whichever kind the case uses: the later draws do not move
    uc = {"zeros": torch.zeros(cshape), "random": uc_random, "none": None}[o["uc"]]
    x0 = torch.randn(B, 4, 16, W, generator=g) if o["inpaint"] else None
    mask = (torch.rand(B, 1, 16, W, generator=g) < 0.5).float() if o["inpaint"] else None
    return dict(o=o, feats=feats, xT=xT, uc=uc, x0=x0, mask=mask, q_seed=100 + seed, noise_seed=200 + seed)


def sampler_grid_overruns(o):
    """A step count whose uniform grid runs past the schedule (S = 9: 999 + 1; util.py:48-57): the reference fails with an IndexError
    when it gathers the tables."""
    return o["name"] in ("DDIM", "PLMS") and int((np.arange(0, 1000, 1000 // o["S"]) + 1).max()) >= 1000


def double_guidance_draw(seed, wide=False):
    r = np.random.default_rng(7600 + seed)
    name = ["DDIM", "DPM_Solver"][seed % 2]
    B, W = int(r.choice([1, 2, 3])), int(r.choice([32, 64]))
    S = int(r.choice([4, 6, 8])) if name == "DDIM" else int(r.choice([3, 6, 16]))
    scale, cscale = float(r.choice([2.5, 4.5])), float(r.choice([0.0, 10.0, 50.0]))
    F = int(r.choice([8, 32, 33]))
    if wide:
        B, W, F = int(r.choice([1, 2, 3, 4, 5])), int(r.choice([8, 16, 24, 32, 40, 64, 96])), int(r.choice([1, 8, 31, 32, 33, 40]))
    eta = float(r.choice([0.0, 1.0])) if name == "DDIM" else 0.0
    return dict(name=name, B=B, W=W, S=S, scale=scale, cscale=cscale, F=F, eta=eta)


def double_guidance_case(seed, wide=False):
    """Tiny configuration and tiny classifier (weights: seed 0); the cond stage sees the first 32 frames, the classifier all of them."""
    o = double_guidance_draw(seed, wide)
    g = torch.Generator().manual_seed(9600 + seed)
    vf = torch.randn(o["B"], o["F"], 64, generator=g)
    vf = vf / vf.norm(dim=-1, keepdim=True)
    xT = torch.randn(o["B"], 4, 16, o["W"], generator=g)
    return dict(o=o, vf=vf, xT=xT, noise_seed=300 + seed)


def draw_json(surface, seed):
    """The suite's draw of a seed as canonical JSON text: what a record stores and what a redraw must give again."""
    d = {"unet": lambda: dict(zip(("cfg", "o"), unet_draw(seed))), "vae": lambda: dict(zip(("cfg", "o"), vae_draw(seed))),
         "cond": lambda: dict(zip(("cond", "calls"), cond_draw(seed))), "cavp": lambda: dict(zip(("cfg", "o"), cavp_draw(seed))),
         "classifier": lambda: dict(zip(("cfg", "o"), classifier_draw(seed))), "samplers": lambda: sampler_draw(seed),
         "double_guidance": lambda: double_guidance_draw(seed)}[surface]()
    return json.dumps(d, sort_keys=True, separators=(",", ":"))


# ------------------------------------------------------------------------------------------------------------------------ record format
# A record is a dict: "draw" (canonical JSON), optional "raises" (exception name), optional integer counts ("n_<name>"), and values by
# name.  A value is stored whole as float32 when it has at most FULL_ELEMS elements; otherwise as float64 sums over its last axis and
# SAMPLE_ELEMS elements at positions drawn from default_rng(seed), the positions stored beside them.  Both forms carry the shape and
# the largest magnitude.  In a file the keys are "<seed>/<field>" and "<seed>/<value>/<part>".
FULL_ELEMS = 16384
SAMPLE_ELEMS = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pack_value(t, seed):
    t = t.detach().to(torch.float32).cpu()
    out = dict(shape=np.asarray(t.shape, dtype=np.int64), absmax=np.float64(t.abs().max().item()))
    if t.numel() <= FULL_ELEMS:
        out["full"] = t.numpy()
    else:
        pos = np.sort(np.random.default_rng(seed).choice(t.numel(), SAMPLE_ELEMS, replace=False)).astype(np.int32)
        out["sums"] = t.double().sum(-1).numpy()
        out["pos"] = pos
        out["vals"] = t.flatten()[torch.from_numpy(pos.astype(np.int64))].numpy()
    return out


def flatten_records(records):
    """{seed: record} -> the flat {key: array} of one .npz file."""
    flat = {}
    for seed, rec in records.items():
        for k, v in rec.items():
            if isinstance(v, dict):
                for part, a in v.items():
                    flat[f"{seed}/{k}/{part}"] = a
            else:
                flat[f"{seed}/{k}"] = np.asarray(v)
    return flat


def record_files(surface):
    """g14_fuzz_<surface>.npz and, where a surface is split to keep every file under the size limit, g14_fuzz_<surface>_p<k>.npz."""
    return sorted(glob.glob(os.path.join(GOLDEN, f"g14_fuzz_{surface}.npz")) + glob.glob(os.path.join(GOLDEN, f"g14_fuzz_{surface}_p[0-9]*.npz")))


_records = {}


def load_records(surface):
    """{seed: record} of a surface; an empty dict where no fixture is there."""
    if surface not in _records:
        recs = {}
        for path in record_files(surface):
            with np.load(path) as z:
                for key in z.files:
                    seed, *rest = key.split("/")
                    rec = recs.setdefault(int(seed), {})
                    a = z[key]
                    if len(rest) == 1:
                        rec[rest[0]] = str(a) if a.dtype.kind == "U" else int(a) if a.dtype.kind in "iu" else bool(a) if a.dtype.kind == "b" else a
                    else:
                        rec.setdefault(rest[0], {})[rest[1]] = a
        _records[surface] = recs
    return _records[surface]


def value_pair(stored, t):
    """(reference, computed) tensors of a stored value and a tensor of the same case, for a norm-wise metric: the whole tensors for a
    value stored whole, the elements at the stored positions for a summarised one."""
    assert tuple(t.shape) == tuple(int(v) for v in stored["shape"]), (tuple(t.shape), stored["shape"])
    t = t.detach().to(torch.float32).cpu()
    if "full" in stored:
        return torch.from_numpy(stored["full"]), t
    return torch.from_numpy(stored["vals"]), t.flatten()[torch.from_numpy(stored["pos"].astype(np.int64))]


def check_value(stored, t, tol):
    """The element-wise judgement of test_oracle_golden.py's ``close``: max |t - ref| <= tol * max(1, max |ref|), over the whole tensor
    or over the stored positions; a summarised value's last-axis sums are judged at tol times the axis length."""
    ref, got = value_pair(stored, t)
    scale = max(1.0, float(stored["absmax"]))
    err = (got.double() - ref.double()).abs().max().item() if ref.numel() else 0.0
    assert err <= tol * scale, ("values", err, tol * scale)
    if "sums" in stored:
        s_err = np.abs(t.detach().double().sum(-1).cpu().numpy() - stored["sums"]).max()
        assert s_err <= tol * scale * t.shape[-1], ("last-axis sums", s_err, tol * scale * t.shape[-1])
    return err
