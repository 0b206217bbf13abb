"""Sampler host loops of the MI355X path: DDIM, PLMS, ancestral DDPM -- and the guided evaluation every sampler shares.

Same call surface as the reference sampler classes (``DDIMSampler(model).sample(S, batch_size, shape,
conditioning, ...) -> (samples, intermediates)``), but every tensor operation in the loop is a HIP
kernel behind the C ABI: the CFG UNet evaluation (``df_unet_forward_cfg``: batch duplication, UNet,
guidance combine) and the solver updates (``df_ddim_update`` / ``df_lincomb``).  The cross-attention
context is handed to the engine once per ``sample()`` (it is step-invariant), so the K/V projections
of the 16 SpatialTransformers leave the step loop.  torch is used for RNG (x_T, eta noise) only.

Reference: diff_foley/models/diffusion/ddim.py:58-273, plms.py:60-236, ddpm.py:1083-1268.
"""
import numpy as np
import warnings

import torch

from . import engine as E
from .schedule import DDIMTables, original_step_tables
from .windows import WindowedConditioning

import os as _os
_NO_HOIST = bool(int(_os.environ.get("DF_NO_THOIST", "0")))      # A/B switch: time embedding inside every step


def _warn_batch(conditioning, batch_size):
    if conditioning is not None:
        c = conditioning[list(conditioning.keys())[0]] if isinstance(conditioning, dict) else conditioning
        if isinstance(c, (list, tuple)):
            c = c[0]
        if c.shape[0] != batch_size:
            print(f"Warning: Got {c.shape[0]} conditionings but batch-size is {batch_size}")


# Reference sampler features that are NOT on this path.  The reference classes accept them (ddim.py:58-113, 179-273;
# plms.py:60-110); silently dropping one would return a plausible but wrong sample, so a non-default value raises.  Anything not
# listed is ignored exactly like the reference's own **kwargs.
# (`normals_sequence` is accepted and never read by the reference's samplers -- ddim.py:65,123, plms.py:64 -- so it is ignored here too.)
# (`noise_dropout` IS on the path since round 5: DDIMSampler applies it as ddim.py:270-271 does; with PLMS -- eta = 0, no noise --
# it has nothing to act on and is accepted like the reference.)
_UNSUPPORTED_DEFAULTS = dict(quantize_x0=False)


def reject_unsupported(sampler, kwargs, extra=None):
    checks = dict(_UNSUPPORTED_DEFAULTS)
    checks.update(extra or {})
    for k, default in checks.items():
        if k in kwargs and kwargs[k] is not None and kwargs[k] != default:
            raise NotImplementedError(f"{sampler}: {k}={kwargs[k]!r} is not supported by the MI355X sampling path "
                                      f"(only the default {default!r}); see DESIGN.md section 1")


def _is_table_error(ex):
    """The engine's two messages for a missing / outgrown hoisted timestep table (unet_run in the C ABI unit of csrc)."""
    msg = str(ex)
    return "no timestep table" in msg or "outside the table" in msg or "hoistable" in msg


class _Inpaint:
    """mask / x0 of the reference samplers: the known region is re-noised to the current step and pasted over the sample,
    img <- q_sample(x0, t) * mask + (1 - mask) * img  (ddim.py:206-209, plms.py:147-150, ddpm.py:1239-1241; q_sample ddpm.py:279-282).
    q_noise_fn(shape) -> tensor replaces torch.randn_like(x0) (tests: the reference's noise sequence)."""

    def __init__(self, model, mask, x0, size, q_noise_fn=None):
        self.on = mask is not None
        if not self.on:
            return
        assert x0 is not None                                  # like the reference
        dev = model.device
        B, C, H, W = size
        x0 = x0.to(dev, torch.float32)
        mask = mask.to(dev, torch.float32)
        if mask.dim() == 3:
            mask = mask[:, None]
        if mask.dim() != 4 or x0.dim() != 4 or mask.shape[1] not in (1, C) or tuple(mask.shape[2:]) not in ((H, W), (1, 1)) or \
                mask.shape[0] not in (1, B) or tuple(x0.shape[1:]) != (C, H, W) or x0.shape[0] not in (1, B):
            raise ValueError(f"inpainting: mask {tuple(mask.shape)} / x0 {tuple(x0.shape)} do not broadcast to the latent "
                             f"{(B, C, H, W)} (mask [B][1|C][H][W], x0 [B][C][H][W])")
        mc = C if mask.shape[1] == C and C != 1 else 1
        self.mask = mask.expand(B, mc, H, W).contiguous()      # broadcast copy, no arithmetic
        self.x0 = x0.expand(B, C, H, W).contiguous()
        self.sa = model.sqrt_alphas_cumprod.cpu().numpy()
        self.s1m = model.sqrt_one_minus_alphas_cumprod.cpu().numpy()
        self.noise_fn = q_noise_fn

    def blend(self, img, t):
        noise = self.noise_fn(tuple(self.x0.shape)).to(img.device, torch.float32) if self.noise_fn is not None \
            else torch.randn_like(self.x0)
        return E.q_sample_blend(img, self.x0, noise.contiguous(), self.mask, self.sa[int(t)], self.s1m[int(t)])


class _Guided:
    """eps(x, t) with classifier-free guidance; owns the engine context for the duration of a sample().

    ``timesteps`` (optional): every timestep value the sampler is going to visit, in its own indexing.  The time embedding
    (timestep_embedding -> time_embed MLP -> the emb projection of all 22 ResBlocks; util.py:151-171,
    openai_unetmodel.py:506-511,262) depends on t only, so it is computed for all of them here, before the loop
    (``df_unet_set_timesteps``), and ``eps_fn(x, t, k)`` takes table row ``k`` instead of four launches per step."""

    def __init__(self, model, cond, scale, uc, timesteps=None, size=None):
        self.m = model
        self.eng = model.engine
        self.cfg = not (uc is None or scale == 1.0)
        self.scale = float(scale)
        self.win = None                  # a WindowedConditioning of more than one window: gather -> UNet -> blend per call
        if isinstance(cond, WindowedConditioning):
            cond, uc, size = self._windowed(cond, uc, size)
        else:
            cond = model._cond_tensor(cond)
            uc = model._cond_tensor(uc)
        self._ctx = torch.cat([uc, cond]) if self.cfg else cond
        self.eng.set_context(self._ctx)
        model._ctx_owner = None          # invalidate apply_model's cached context
        self.hoisted = False
        if timesteps is not None and size is not None and not _NO_HOIST:
            B, _, H, W = size
            try:      # an optimisation, never a requirement: a UNet configuration without a hoistable time embedding
                self.eng.set_timesteps([float(v) for v in timesteps], B, H, W, self.cfg)      # keeps the in-step t path
                self.hoisted = True
            except RuntimeError as ex:
                if not _is_table_error(ex):      # anything else (bad shapes, a sticky HIP error) is the caller's to see
                    raise
                self.hoisted = False

    def _windowed(self, cond, uc, size):
        """A WindowedConditioning (windows.py) -> (conditional rows, unconditional rows, the size the UNet sees).  One window is the
        plain call on that window's conditioning: nothing is gathered or blended, the bits are the plain call's.  More than one: the
        context rows of the window batch (row b * K + k), and ``size`` becomes (B * K, C, H, Wc) for the timestep table."""
        if size is None:
            raise ValueError("a windowed conditioning needs the size of the long latent")
        cond.check_latent(size)
        B, Cc, H, W = (int(v) for v in size)
        c = cond.rows(B).to(self.m.device, torch.float32)
        u = cond.uncond_rows(uc, B) if self.cfg else None
        if cond.K > 1:
            self.win = cond
            self._long = (B, Cc, H, W)
            size = (B * cond.K, Cc, H, cond.size_len)
        return c, u, size

    def _window_eval(self, fwd, x, t):
        """eps on the long latent: cut the K windows out, evaluate them as ONE UNet batch (guidance included), blend them back."""
        win = self.win
        if tuple(x.shape) != self._long:
            raise ValueError(f"windowed evaluation of a latent of shape {tuple(x.shape)}, the sample was opened for {self._long}")
        if t.numel() == x.shape[0]:      # one timestep per sample -> one per window row (a broadcast copy; a single t serves all rows)
            t = t.reshape(-1, 1).expand(x.shape[0], win.K).reshape(-1)
        e = fwd(E.window_gather(x, win.col_starts, win.size_len), t)
        return E.window_blend(e, win.col_starts, win.size_len_total)

    def reclaim_context(self):
        """A caller-supplied callback (score_corrector) may have evaluated the model itself -- ``model.apply_model`` and the
        ``model.model`` facades set THEIR context in the engine.  Put the sampler's [uncond ; cond] context back."""
        if self.m._ctx_owner is not None:
            self.eng.set_context(self._ctx)
            self.m._ctx_owner = None

    def __call__(self, x, t, k=None):
        k = k if self.hoisted else None
        unet = (lambda xx, tt, kk: self.eng.unet_forward_cfg(xx, tt, self.scale, ts_index=kk)) if self.cfg else \
               (lambda xx, tt, kk: self.eng.unet_forward(xx, tt, ts_index=kk))
        if self.win is None:
            fwd = lambda kk: unet(x, t, kk)
        else:
            fwd = lambda kk: self._window_eval(lambda xx, tt: unet(xx, tt, kk), x, t)
        if k is None:
            return fwd(None)
        try:
            return fwd(k)
        except RuntimeError as ex:
            # the plan that owned the timestep table was rebuilt in the middle of the sample (plan-cache eviction, a callback that
            # re-finalised the engine): the in-step path computes the same embedding from t, bit-identically.  ONLY that case
            # falls back (the engine names it in its message); every other engine error propagates.
            if not _is_table_error(ex):
                raise
            warnings.warn("diff_foley_amd: the hoisted time-embedding table was dropped in the middle of a sample() call "
                          f"({ex}); the remaining steps compute the embedding inside the step", RuntimeWarning, stacklevel=2)
            self.hoisted = False
            return fwd(None)


def refuse_windowed_classifier(cond, classifier):
    """Double guidance over windows is not defined here: the classifier scores one 32-frame window, and whether its gradient on the
    long latent is taken window by window and blended like eps, or on some other cover, is a modelling decision nobody has made."""
    if classifier is not None and isinstance(cond, WindowedConditioning):
        raise NotImplementedError("classifier guidance with a windowed conditioning is not supported: the alignment classifier scores "
                                  "one 32-frame window, and how its gradient is to be combined over overlapping windows of a long "
                                  "latent has not been decided; sample without the classifier, or one window at a time")


def _classifier_grad(model, classifier, x, t, origin_cond):
    if not hasattr(classifier, "log_prob_grad"):
        raise RuntimeError("classifier guidance needs a diff_foley_amd AlignmentClassifier (log_prob_grad)")
    if classifier.engine is None:        # the notebook passes a freshly loaded classifier (ipynb:288-311)
        classifier.attach(model)
    return classifier.log_prob_grad(x, t, origin_cond)


_side_streams = {}


def _eps_and_classifier_grad(model, classifier, eps_call, x, t, origin_cond):
    """eps(x, t) and the classifier's d log p / d x at the same (x, t) (ddim.py:374-380) do not depend on
    each other, so the gradient's launches go to a second HIP stream beside the UNet step's (round 6).  The gradient plan is ~160
    launches of small grids at the launch floor (1.14 ms per call at B = 8, profiles/r6_classifier_grad_ops.txt); beside the UNet step
    they run on CUs the step's kernels leave idle: configs[2] 152.5 -> 171.1 steps/s, latents bit-equal to the one-stream order
    (tools/cls_overlap_probe.py, profiles/r6_classifier_overlap.txt).  The plans own their workspaces; the only shared inputs are x and
    t, read-only in both.  (Two UNet chains do NOT overlap this way -- every one of their kernels wants the whole chip:
    tools/two_chain_probe.py.)  DF_CLS_OVERLAP=0 restores the one-stream order.  Returns (eps, grad), both ready on the current stream."""
    if _os.environ.get("DF_CLS_OVERLAP", "1") == "0":
        return eps_call(), _classifier_grad(model, classifier, x, t, origin_cond)
    cur = torch.cuda.current_stream(x.device)
    side = _side_streams.get(x.device)
    if side is None:
        side = _side_streams[x.device] = torch.cuda.Stream(x.device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        g = _classifier_grad(model, classifier, x, t, origin_cond)
    x.record_stream(side)
    t.record_stream(side)
    e = eps_call()
    cur.wait_stream(side)
    g.record_stream(cur)
    return e, g


def _classifier_guided_eps(model, classifier, eps_call, x, t, origin_cond, coef):
    """eps - coef * d log p / d x: the classifier's half of double guidance (ddim.py:374-380).  ``coef`` is the caller's own
    sigma_t * classifier_guide_scale, a host scalar."""
    e, g = _eps_and_classifier_grad(model, classifier, eps_call, x, t, origin_cond)
    return E.lincomb([(1.0, e), (-coef, g)])


def _start(model, batch_size, shape, x_T):
    """(the start latent, its size): x_T, or noise from the device generator."""
    C, H, W = shape
    size = (batch_size, C, H, W)
    return (torch.randn(size, device=model.device) if x_T is None else x_T.to(model.device, torch.float32).contiguous()), size


def _ddim_steps(model, img, size, steps, tables, conditioning, unconditional_guidance_scale, unconditional_conditioning, noise_fn=None,
                temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, classifier=None, origin_cond=None,
                classifier_guide_scale=0.0, callback=None, img_callback=None, log_every_t=100, paint=None, combine=None):
    """The step loop of the DDIM family (ddim.py:179-229 with p_sample_ddim :231-273; plms.py:113-236): ``steps`` are the timestep
    values in visiting order, ``tables`` = (alphas, alphas_prev, sigmas, sqrt_one_minus_alphas) indexed by len(steps) - 1 - i at step i.
    DDIMSampler.sample() walks the whole DDIM schedule, decode() a prefix of it (or of the original steps), PLMSSampler.sample() the
    whole schedule with ``combine(e_t, i, eps_at, update) -> eps`` between the evaluation and the update: ``eps_at(x, k)`` is the
    evaluation at step k, ``update(e)`` the step's df_ddim_update from the current latent."""
    dev = model.device
    batch_size = size[0]
    refuse_windowed_classifier(conditioning, classifier)
    alphas, alphas_prev, sigmas, sqrt_one_minus_alphas = tables
    total = steps.shape[0]
    guided = _Guided(model, conditioning, unconditional_guidance_scale, unconditional_conditioning, steps, size)
    t_all = torch.tensor(steps.copy(), dtype=torch.float32, device=dev)[:, None].expand(total, batch_size).contiguous()
    t_long = t_all.long() if score_corrector is not None else None     # the reference hands the callback `ts` (int64, ddim.py:217)

    def eps_at(x, k):
        if classifier is None:
            e = guided(x, t_all[k], k)
        else:                            # ddim.py:374-380: the classifier gradient first ...
            e = _classifier_guided_eps(model, classifier, lambda: guided(x, t_all[k], k), x, t_all[k], origin_cond,
                                       np.sqrt(np.float32(1.0) - alphas[total - k - 1]) * classifier_guide_scale)
        if score_corrector is not None:  # ... then the caller's callback on the guided eps (ddim.py:249-251, 382-384; plms.py:178-190)
            e = E._dev_f32(score_corrector.modify_score(model, e, x, t_long[k], conditioning, **(corrector_kwargs or {})), dev)
            guided.reclaim_context()
        return e

    inter = {"x_inter": [img], "pred_x0": [img]}
    for i in range(total):
        index = total - i - 1
        if paint is not None and paint.on:      # ddim.py:206-209, plms.py:147-150
            img = paint.blend(img, steps[i])
        e_t = eps_at(img, i)
        sigma = sigmas[index]
        noise = None
        if sigma != 0.0:         # ddim.py:269-271: noise * temperature, then dropout of the noise (functional default: training)
            noise = (noise_fn(size) if noise_fn is not None else torch.randn(size, device=dev)) * temperature
            if noise_dropout > 0.0:
                noise = torch.nn.functional.dropout(noise, p=float(noise_dropout))
            noise = noise.to(dev, torch.float32).contiguous()
        update = lambda e: E.ddim_update(img, e, alphas[index], alphas_prev[index], sigma, sqrt_one_minus_alphas[index], noise)
        if combine is not None:
            e_t = combine(e_t, i, eps_at, update)
        img, pred_x0 = update(e_t)
        if callback:
            callback(i)
        if img_callback:
            img_callback(pred_x0, i)
        if index % log_every_t == 0 or index == total - 1:
            inter["x_inter"].append(img)
            inter["pred_x0"].append(pred_x0)
    return img, inter


def sample_with_classifier(self, S, batch_size, shape, conditioning=None, origin_cond=None, callback=None, normals_sequence=None,
                           img_callback=None, quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0,
                           score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
                           unconditional_guidance_scale=1.0, unconditional_conditioning=None, classifier=None,
                           classifier_guide_scale=0.0, **kwargs):
    """The method of that name of the samplers that take a classifier (ddim.py:115-177 and its twin beside the solver): the
    reference's parameter list, forwarded to ``sample``, which takes the three classifier arguments itself."""
    return self.sample(S, batch_size, shape, conditioning, callback=callback, normals_sequence=normals_sequence,
                       img_callback=img_callback, quantize_x0=quantize_x0, eta=eta, mask=mask, x0=x0, temperature=temperature,
                       noise_dropout=noise_dropout, score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                       verbose=verbose, x_T=x_T, log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                       unconditional_conditioning=unconditional_conditioning, classifier=classifier, origin_cond=origin_cond,
                       classifier_guide_scale=classifier_guide_scale, **kwargs)


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        # "uniform" | "quad" (util.py:46-60).  As in the reference, sample() re-makes the schedule with the default ("uniform",
        # ddim.py:90): a "quad" schedule serves callers that drive the step loop from the tables themselves.
        self.tables = DDIMTables(self.model.alphas_cumprod, ddim_num_steps, ddim_eta, ddim_discretize)
        self.ddim_timesteps = self.tables.timesteps
        self.ddim_alphas = self.tables.alphas
        self.ddim_alphas_prev = self.tables.alphas_prev
        self.ddim_sigmas = self.tables.sigmas
        self.ddim_sqrt_one_minus_alphas = self.tables.sqrt_one_minus_alphas
        # the use_original_steps=True tables (ddim.py:34-40, 53-56, 254-257) belong to this schedule too; sample() never reads them,
        # so they are built when stochastic_encode / decode first ask (__getattr__), from the eta given here
        self._original_eta = ddim_eta
        self._original = None
        self._encode_tables = {}      # use_original_steps -> the two device tables of stochastic_encode, uploaded on first use

    # attribute of the reference's sampler after make_schedule -> key of schedule.original_step_tables
    _ORIGINAL = {"alphas_cumprod": "alphas_cumprod", "alphas_cumprod_prev": "alphas_cumprod_prev",
                 "sqrt_alphas_cumprod": "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod": "sampler_sqrt_one_minus_alphas_cumprod",
                 "ddim_sigmas_for_original_num_steps": "ddim_sigmas_for_original_num_steps"}

    def __getattr__(self, name):      # reached only for names that are not set: the original-step tables, built on first use
        if name != "original" and name not in self._ORIGINAL:
            raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")
        d = self.__dict__
        if "_original_eta" not in d:      # no make_schedule yet: the reference's sampler has no such attribute either
            raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}' (call make_schedule first)")
        if d["_original"] is None:
            m = self.model
            d["_original"] = original_step_tables(m.alphas_cumprod, m.alphas_cumprod_prev, m.sqrt_one_minus_alphas_cumprod,
                                                  d["_original_eta"])
        return d["_original"] if name == "original" else d["_original"][self._ORIGINAL[name]]

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """ddim.py:400-413: x0 noised to the DDIM step (or, use_original_steps, the DDPM step) whose TABLE INDEX is t[b] -- one
        df_q_sample.  Fast, but no exact reconstruction (the reference's words).  Needs make_schedule first, like the reference:
        without it the tables are missing attributes, here as there."""
        if use_original_steps:
            tabs = (self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)
        else:
            tabs = (np.sqrt(self.ddim_alphas), self.ddim_sqrt_one_minus_alphas)
        dev = self.model.device
        key = bool(use_original_steps)
        if key not in self._encode_tables:
            self._encode_tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in tabs)
        A, S = self._encode_tables[key]
        x0 = E._dev_f32(x0, dev)
        if noise is None:
            noise = torch.randn_like(x0)
        return E.q_sample(x0, noise, t, A, S)

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False):
        """ddim.py:415-434: denoise x_latent from table index t_start down to 0 under ``cond`` -- the step loop of sample() over
        timesteps[:t_start], flipped.  sigma is the table's, so make_schedule's ddim_eta applies; noise_fn (tests) is not a
        parameter here: set ``self.noise_fn`` to replay a recorded noise sequence."""
        if use_original_steps:
            timesteps = np.arange(self.ddpm_num_timesteps)
            o = self.original
            tables = (o["alphas_cumprod"], o["alphas_cumprod_prev"], o["ddim_sigmas_for_original_num_steps"],
                      o["sqrt_one_minus_alphas_cumprod"])
        else:
            timesteps = self.ddim_timesteps
            tables = (self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sigmas, self.ddim_sqrt_one_minus_alphas)
        timesteps = timesteps[:t_start]
        total_steps = timesteps.shape[0]
        print(f"Running DDIM Sampling with {total_steps} timesteps")
        if total_steps == 0:
            return x_latent
        x = E._dev_f32(x_latent, self.model.device)
        if x.ndim != 4:
            raise ValueError(f"decode: x_latent of shape {tuple(x.shape)}, expected [B][C][H][W]")
        x_dec, _ = _ddim_steps(self.model, x, tuple(x.shape), np.flip(timesteps), tables, cond, unconditional_guidance_scale,
                               unconditional_conditioning, noise_fn=getattr(self, "noise_fn", None))
        return x_dec

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, classifier=None, origin_cond=None, classifier_guide_scale=0.0, **kwargs):
        # the reference's parameters in the reference's order (ddim.py:59-82), so that a positional call means the same; then the
        # three of sample_with_classifier, which is this method
        reject_unsupported("DDIMSampler", dict(kwargs, quantize_x0=quantize_x0))
        noise_fn = kwargs.get("noise_fn")       # tests: replaces the device generator (the reference run's CPU noise sequence)
        _warn_batch(conditioning, batch_size)
        self.make_schedule(S, ddim_eta=eta, verbose=verbose)
        img, size = _start(self.model, batch_size, shape, x_T)
        tb = self.tables
        return _ddim_steps(self.model, img, size, np.flip(tb.timesteps), (tb.alphas, tb.alphas_prev, tb.sigmas, tb.sqrt_one_minus_alphas),
                           conditioning, unconditional_guidance_scale, unconditional_conditioning, noise_fn=noise_fn,
                           temperature=temperature, noise_dropout=noise_dropout, score_corrector=score_corrector,
                           corrector_kwargs=corrector_kwargs, classifier=classifier, origin_cond=origin_cond,
                           classifier_guide_scale=classifier_guide_scale, callback=callback, img_callback=img_callback,
                           log_every_t=log_every_t, paint=_Inpaint(self.model, mask, x0, size, kwargs.get("q_noise_fn")))

    sample_with_classifier = sample_with_classifier


class PLMSSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, **kwargs):
        # the reference's parameters in the reference's order (plms.py:58-81)
        if eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        reject_unsupported("PLMSSampler", dict(kwargs, quantize_x0=quantize_x0, temperature=temperature), dict(temperature=1.0))
        _warn_batch(conditioning, batch_size)
        tb = DDIMTables(self.model.alphas_cumprod, S, 0.0)
        img, size = _start(self.model, batch_size, shape, x_T)
        steps = np.flip(tb.timesteps)
        old_eps = []

        def combine(e_t, i, eps_at, update):      # Adams-Bashforth over the eps history (plms.py:219-236)
            if len(old_eps) == 0:          # pseudo improved Euler (plms.py:219-223)
                x_prev, _ = update(e_t)
                e_next = eps_at(x_prev, min(i + 1, steps.shape[0] - 1))
                e_p = E.lincomb([(0.5, e_t), (0.5, e_next)])
            elif len(old_eps) == 1:
                e_p = E.lincomb([(1.5, e_t), (-0.5, old_eps[-1])])
            elif len(old_eps) == 2:
                e_p = E.lincomb([(23 / 12, e_t), (-16 / 12, old_eps[-1]), (5 / 12, old_eps[-2])])
            else:
                e_p = E.lincomb([(55 / 24, e_t), (-59 / 24, old_eps[-1]), (37 / 24, old_eps[-2]), (-9 / 24, old_eps[-3])])
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
            return e_p
        return _ddim_steps(self.model, img, size, steps, (tb.alphas, tb.alphas_prev, tb.sigmas, tb.sqrt_one_minus_alphas), conditioning,
                           unconditional_guidance_scale, unconditional_conditioning, score_corrector=score_corrector,
                           corrector_kwargs=corrector_kwargs, callback=callback, img_callback=img_callback, log_every_t=log_every_t,
                           paint=_Inpaint(self.model, mask, x0, size, kwargs.get("q_noise_fn")), combine=combine)


@torch.no_grad()
def ancestral_sample(model, cond, shape, x_T=None, timesteps=None, log_every_t=None, return_intermediates=False,
                     noise_fn=None, callback=None, img_callback=None, mask=None, x0=None, q_noise_fn=None):
    """LatentDiffusion.p_sample_loop (ddpm.py:1201-1250): 1000-step ancestral sampling, no CFG, clip_denoised False."""
    dev = model.device
    img = torch.randn(shape, device=dev) if x_T is None else x_T.to(dev, torch.float32).contiguous()
    b = shape[0]
    T = model.num_timesteps if timesteps is None else timesteps
    log_every_t = log_every_t or model.log_every_t
    eps_fn = _Guided(model, cond, 1.0, None, size=tuple(shape))
    tab = {k: getattr(model, k).cpu().numpy() for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                                        "posterior_mean_coef1", "posterior_mean_coef2",
                                                        "posterior_log_variance_clipped")}
    inter = [img]
    paint = _Inpaint(model, mask, x0, tuple(shape), q_noise_fn)
    for i in reversed(range(0, T)):
        ts = torch.full((b,), float(i), device=dev, dtype=torch.float32)
        eps = eps_fn(img, ts)
        # x_recon = c_r x - c_m eps ; mean = c1 x_recon + c2 x   (ddpm.py:221-234)
        cr, cm = tab["sqrt_recip_alphas_cumprod"][i], tab["sqrt_recipm1_alphas_cumprod"][i]
        c1, c2 = tab["posterior_mean_coef1"][i], tab["posterior_mean_coef2"][i]
        terms = [(c1 * cr + c2, img), (-c1 * cm, eps)]
        # noise is drawn at every step (also t == 0, where it is masked) like noise_like() in ddpm.py:1132
        noise = noise_fn(shape).to(dev) if noise_fn is not None else torch.randn(shape, device=dev)
        if i != 0:
            terms.append((np.exp(0.5 * tab["posterior_log_variance_clipped"][i]), noise))
        img = E.lincomb(terms)
        if paint.on:                         # ddpm.py:1239-1241: after the step
            img = paint.blend(img, i)
        if i % log_every_t == 0 or i == T - 1:
            inter.append(img)
        if callback:
            callback(i)
        if img_callback:
            img_callback(img, i)
    return (img, inter) if return_intermediates else img
