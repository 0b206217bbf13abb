"""Drop-in for the reference's ``LatentDiffusion`` on MI355X (the sampling API, and the training objective evaluated without a gradient).

``instantiate_from_config(config.model)`` of the reference notebook (inference/diff_foley_inference.ipynb:80-95,
diff_foley/util.py:176-191) resolves ``target: diff_foley.models.diffusion.ddpm.LatentDiffusion``; pointing that
target at :class:`LatentDiffusion` here keeps the rest of the notebook unchanged:

    model = instantiate_from_config(cfg.model); model.load_state_dict(sd, strict=False); model.cuda(); model.eval()
    c  = model.get_learned_conditioning(video_feat[:, :32])
    z, _ = model.sample_log_diff_sampler(c, batch_size=4, sampler_name="DDIM", ddim_steps=25,
                                         unconditional_guidance_scale=4.5, unconditional_conditioning=zeros_like(c))
    mel = model.decode_first_stage(z)[:, 0]

Method names, kwargs, return shapes/dtypes follow ddpm.py:568 (get_learned_conditioning), :739 (decode_first_stage),
:925 (apply_model), :1252 (sample), :1270-1356 (sample_log*), :279-297 (q_sample, get_loss), :904-913 (forward), :1046-1081
(p_losses).  All compute runs in libdfengine.so (HIP); a missing library or a CPU-only host raises -- there is no fallback path.

Holds LatentDiffusion, its sub-module facades, its encoder's posterior, AlignmentClassifier (it runs on the LatentDiffusion's engine)
and ``instantiate_from_config``; AlignmentClassifierMetric (align_metric.py) and CAVPInference (cavp.py) stay importable from here.
"""
import importlib

import torch

from . import dpm_solver as D
from . import engine as E
from . import samplers as S
from . import windows as W
from .align_metric import (AlignmentClassifierMetric, _MetricBackboneFacade, _MetricCondFacade,  # noqa: F401
                           _MetricFirstStageFacade, align_acc_clip_name, align_acc_frames, align_acc_specs)
from .cavp import CAVPInference
from .model_base import (_EngineModel, _Facade, _check_shapes, _locked, _params, _unet_params, _vae_params,  # noqa: F401
                         _UNET_FIXED, _UNET_KEYS, _VAE_FIXED)
from .schedule import BUFFER_NAMES, register_schedule


def instantiate_from_config(config):
    """diff_foley/util.py:176-191 semantics; reference ``target`` paths of the hot-path classes map to this package."""
    target = config["target"]
    alias = {
        "diff_foley.models.diffusion.ddpm.LatentDiffusion": LatentDiffusion,
        "diff_foley.modules.double_guidance.alignment_classifier.Alignment_Classifier_Double_Guidance": AlignmentClassifier,
    }
    alias["model.cavp_model.CAVP_Inference"] = CAVPInference      # inference/config/Stage1_CAVP.yaml:2
    # evaluation/config/eval_classifier.yaml:3
    alias["diff_foley.modules.double_guidance.alignment_classifier_metric.Alignment_Classifier_metric"] = AlignmentClassifierMetric
    if target in alias:
        return alias[target](**dict(config.get("params", dict())))
    module, cls = target.rsplit(".", 1)
    return getattr(importlib.import_module(module), cls)(**dict(config.get("params", dict())))


class _UNetFacade(_Facade):
    """UNetModel.forward(x, timesteps, context) (openai_unetmodel.py:710-742)."""
    _what = "model.diffusion_model"

    def __call__(self, x, timesteps=None, context=None, y=None, **kwargs):
        if y is not None:
            raise NotImplementedError("class-conditional UNet (y=) is not on the path")
        return self._m.apply_model(x, timesteps, context)


class _DiffusionWrapperFacade(_Facade):
    """DiffusionWrapper (ddpm.py:1545-1571), conditioning_key 'crossattn'."""
    _what = "model"

    def __init__(self, owner):
        super().__init__(owner)
        object.__setattr__(self, "diffusion_model", _UNetFacade(owner))
        object.__setattr__(self, "conditioning_key", "crossattn")

    def __call__(self, x, t, c_concat=None, c_crossattn=None):
        if c_concat:
            raise NotImplementedError("only conditioning_key='crossattn' is on the path")
        cc = c_crossattn[0] if len(c_crossattn) == 1 else torch.cat(list(c_crossattn), 1)
        return self.diffusion_model(x, t, context=cc)


class _FirstStageFacade(_Facade):
    """AutoencoderKL.decode(z) (autoencoder.py: post_quant_conv -> decoder), i.e. decode_first_stage without its 1/scale_factor, and
    AutoencoderKL.encode(x) when the checkpoint's encoder + quant_conv were loaded."""
    _what = "first_stage_model"

    def decode(self, z):
        m = self._m
        zs = E.lincomb([(float(m.scale_factor), E._dev_f32(z, m.device))])      # decode_first_stage(z * s) == decode(z)
        return m.decode_first_stage(zs)

    def encode(self, x):
        """AutoencoderKL.encode (autoencoder.py:324-328): the posterior over the latent of a mel image x [B][in_channels][H][W]."""
        return self._m.encode_first_stage(x)


class DiagonalGaussianDistribution:
    """The posterior ``first_stage_model.encode`` returns (stage1_autoencoder/model.py:34-72): same attributes and methods, the
    tensors live on the engine's device.  ``parameters`` [B][2 zc][h][w] comes from df_vae_encode; ``sample`` runs df_posterior_sample;
    ``kl`` / ``nll`` (training-time losses, not on any hot path) are torch expressions on the device tensors."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.deterministic = deterministic
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)
        else:
            self.std = torch.exp(0.5 * self.logvar)
            self.var = torch.exp(self.logvar)

    def sample(self, scale=1.0):
        """mean + std * randn (model.py:45-47), times ``scale`` (not a reference argument: get_first_stage_encoding folds its
        scale_factor into the same launch).  The noise is drawn like the reference draws it -- torch.randn(shape) from the CPU default
        generator, then uploaded -- so torch.manual_seed(s) gives the reference's sample."""
        if self.deterministic:
            return E.posterior_sample(self.parameters, None, scale)
        noise = torch.randn(self.mean.shape).to(device=self.parameters.device)
        return E.posterior_sample(self.parameters, noise, scale)

    def kl(self, other=None):
        if self.deterministic:
            return torch.Tensor([0.])
        if other is None:
            return 0.5 * torch.sum(torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.sum(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar
                               + other.logvar, dim=[1, 2, 3])

    def nll(self, sample, dims=[1, 2, 3]):
        if self.deterministic:
            return torch.Tensor([0.])
        import math
        return 0.5 * torch.sum(math.log(2.0 * math.pi) + self.logvar + torch.pow(sample - self.mean, 2) / self.var, dim=dims)

    def mode(self):
        return self.mean


class _CondStageFacade(_Facade):
    """cond_stage_model(feats) / .encode(feats) as get_learned_conditioning calls it (ddpm.py:568-579)."""
    _what = "cond_stage_model"

    def __call__(self, c):
        return self._m.get_learned_conditioning(c)

    def encode(self, c):
        return self._m.get_learned_conditioning(c)


class LatentDiffusion(_EngineModel):
    _buffer_names = BUFFER_NAMES + ("lvlb_weights", "logvar")      # the loss tables move to the device with the schedule
    _probe_texts = ("a probe UNet forward (t = 999 / 1)",
                    "  No operand type was requested, so this model now runs on the bf16 build (fp32 exponent range, same speed; "
                    "decoded-mel MAE 4.4e-3 against the fp32 reference instead of 5.8e-4).  LatentDiffusion(..., precision='fp16') keeps "
                    "the fp16 build.",
                    "  Samples would be clamped silently.  Fallback: LatentDiffusion(..., precision='bf16') (fp32 exponent range, same "
                    "speed; decoded-mel MAE 4.4e-3 against the fp32 reference instead of 5.8e-4).")

    def __init__(self, first_stage_config=None, cond_stage_config=None, unet_config=None, linear_start=1e-4,
                 linear_end=2e-2, timesteps=1000, beta_schedule="linear", channels=3, image_size=256,
                 scale_factor=1.0, conditioning_key=None, parameterization="eps", log_every_t=100,
                 v_posterior=0.0, use_ema=True, clip_denoised=True, precision=None, loss_type="l2", l_simple_weight=1.0,
                 original_elbo_weight=0.0, logvar_init=0.0, learn_logvar=False, **ignored):
        # precision: MFMA operand type of the engine.  None -> env DF_PRECISION -> "fp16", the build that meets the north-star
        # tolerance (mel MAE 5.8e-4); "bf16" (BASELINE configs[1]'s wording, same speed) rounds operands 8x coarser and lands at
        # mel MAE 4.5e-3, outside the tolerance -- selectable, never the default.  Not a reference kwarg.
        super().__init__(precision)
        if parameterization != "eps":
            raise NotImplementedError("only eps-parameterisation is on the path")
        if conditioning_key not in (None, "crossattn"):
            raise NotImplementedError("only conditioning_key='crossattn' is on the path (Stage2_LDM.yaml:15)")
        self.unet_cfg = _unet_params(unet_config, "unet_config")
        self.vae_cfg, self._double_z = _vae_params(first_stage_config)
        self._has_encoder = False
        self.cond_cfg = {k: _params(cond_stage_config)[k] for k in ("origin_dim", "embed_dim", "seq_len")}
        self.channels = channels
        self.image_size = image_size
        self.scale_factor = scale_factor
        self.parameterization = parameterization
        self.log_every_t = log_every_t
        self.clip_denoised = False            # LatentDiffusion overrides DDPM's default (ddpm.py:475)
        self.conditioning_key = "crossattn"
        self.num_timesteps = int(timesteps)
        self.linear_start, self.linear_end = linear_start, linear_end
        self._buffers = register_schedule(linear_start, linear_end, timesteps, v_posterior, beta_schedule)
        for k, v in self._buffers.items():
            setattr(self, k, v)
        # the training objective's settings (ddpm.py:102-104, 114-119), read by get_loss / p_losses
        if loss_type not in E.LOSS_TYPES:
            raise NotImplementedError(f"unknown loss type '{loss_type}'")          # ddpm.py:295 raises at the first get_loss
        self.loss_type = loss_type
        self.l_simple_weight = l_simple_weight
        self.original_elbo_weight = original_elbo_weight
        self.learn_logvar = bool(learn_logvar)
        self.logvar = torch.full(fill_value=float(logvar_init), size=(self.num_timesteps,))
        self._ctx_owner = None
        self.first_stage_model = _FirstStageFacade(self)
        self.cond_stage_model = _CondStageFacade(self)
        self.model = _DiffusionWrapperFacade(self)

    # ------------------------------------------------------------------ nn.Module-like plumbing
    def load_state_dict(self, state_dict, strict=False):
        need = ("model.diffusion_model.", "first_stage_model.post_quant_conv.", "first_stage_model.decoder.",
                "cond_stage_model.")
        self._state = {k: v for k, v in state_dict.items() if k.startswith(need)}
        from . import synth
        # The VAE encoder + quant_conv (first_stage_model.encode) are taken only as the COMPLETE key set of the configured
        # architecture; any partial set stays out and is reported as unexpected, as every encoder key was before the encoder existed.
        enc_spec = synth.vae_encoder_spec(self.vae_cfg, "first_stage_model.")
        self._has_encoder = all(k in state_dict for k in enc_spec)
        if self._has_encoder:
            if not self._double_z:
                raise NotImplementedError("first_stage_config.ddconfig: double_z=False is not supported by libdfengine (the posterior "
                                          "needs mean and logvar)")
            self._state.update({k: state_dict[k] for k in enc_spec})
        _check_shapes(self._state, synth.state_dict_spec(self.unet_cfg, self.vae_cfg, self.cond_cfg, with_encoder=self._has_encoder),
                      "LatentDiffusion")
        for k in BUFFER_NAMES + ("logvar",):      # checkpoints carry the schedule buffers too, and logvar (learn_logvar: a parameter)
            if k in state_dict:
                if k == "logvar" and tuple(state_dict[k].shape) != (self.num_timesteps,):
                    raise RuntimeError(f"LatentDiffusion: logvar has shape {tuple(state_dict[k].shape)}, expected ({self.num_timesteps},)")
                setattr(self, k, state_dict[k].detach().float().to(self.device))
        unexpected = [k for k in state_dict if not k.startswith(need) and k not in BUFFER_NAMES + ("logvar",)
                      and not (self._has_encoder and k in enc_spec)]
        if strict and unexpected:
            raise RuntimeError(f"unexpected keys: {unexpected[:5]} ...")
        if self.engine is not None:
            self._upload()
        return [], unexpected

    def _upload(self):
        self._ctx_owner = None            # the engine forgets its cross-attention K/V when weights are (re)loaded
        eng = self._configure()
        for k, v in self._state.items():
            eng.load_tensor(k, v)
        eng.finalize()
        self._range_check()

    def _probe_ready(self):       # a partial (strict=False) load without UNet weights: nothing to probe yet
        return any(k.startswith("model.diffusion_model.") for k in (self._state or {}))

    def _probe(self):
        """The range guard's pass (model_base._EngineModel): one UNet forward at a high and a low timestep (t = 999 and t = 1, one
        N(0, 1) latent of the model's latent shape, one N(0, 1) context).  (openai_unetmodel.py:710-742 runs in fp32: nothing to guard
        there.)"""
        # probe shape = the model's configured latent: (channels, H, W) from image_size (an int or an (H, W) pair; the Stage-2
        # config's 8 s latent is 16 x 64) and the condition stage's sequence length
        isz = self.image_size
        H, W = (int(isz[0]), int(isz[1])) if isinstance(isz, (list, tuple)) and len(isz) == 2 else (16, 64)
        if H % 8 or W % 8:
            H, W = 16, 64
        # context frames: the notebook's window length (truncate_len = 32, ipynb cell 13), never more than the condition stage's
        # positional table holds.  (A longer probe context would also build -- and later export -- the K / V^T cross-attention
        # packings no sampling call of the product shapes uses.)
        T = min(32, int(self.cond_cfg.get("seq_len", 32) or 32))
        g = torch.Generator(device="cpu").manual_seed(999)
        x = torch.randn(2, int(self.unet_cfg["in_channels"]), H, W, generator=g).to(self.device)
        c = torch.randn(2, T, int(self.unet_cfg["context_dim"]), generator=g).to(self.device)
        t = torch.tensor([999.0, 1.0], device=self.device)
        try:
            self.engine.set_context(c)
            self.engine.unet_forward(x, t)
        finally:
            self._ctx_owner = None

    def _configure(self):
        eng = self.engine
        eng.config_unet(self.unet_cfg)
        eng.config_vae(self.vae_cfg, self.scale_factor)
        eng.config_cond(self.cond_cfg)
        eng.config_vae_encoder(dict(in_channels=self.vae_cfg["in_channels"]) if self._has_encoder else None)
        return eng

    # ---- multi-GPU weight distribution: the root rank packs once, the others import the packed operands ----------
    def export_packed(self, batch_size, size_len=64, context_frames=32):
        """(manifest, blob) of this model's packed operands for sampling ``batch_size`` clips (latent 16 x size_len,
        ``context_frames`` CAVP frames): see include/df_engine.h, df_export_packed."""
        return self._require().export_packed(batch_size, 16, size_len, context_frames)

    def load_packed(self, manifest, blob):
        """Counterpart of load_state_dict for non-root ranks: call after .cuda(); no fp32 checkpoint is needed."""
        if self.engine is None:
            raise RuntimeError("load_packed: call .cuda(device) first")
        self._configure()
        self._has_encoder = False         # the packed blob does not carry the VAE encoder: encode raises on an importing rank
        self.engine.config_vae_encoder(None)
        self.engine.import_packed(manifest, blob)
        self.engine.finalize()
        self._state = {}      # (no range probe here: the exporting rank ran it on these very weights)
        return self

    def _cond_tensor(self, cond):
        if isinstance(cond, dict):
            cond = cond["c_crossattn"]
        if isinstance(cond, (list, tuple)):
            cond = torch.cat(list(cond), 1)
        return cond

    # ------------------------------------------------------------------ the path
    @_locked
    @torch.no_grad()
    def get_learned_conditioning(self, c):
        return self._require().cond_encode(c)

    @_locked
    @torch.no_grad()
    def get_windowed_conditioning(self, video_feat, hop=16, size_len=64):
        """The conditioning of a clip of T >= 32 CAVP frames, longer than the one 32-frame window the model was trained on (no
        reference counterpart): K windows of 32 frames at a hop of ``hop`` frames, the last one flush right, each
        encoded on its own with positions 0..31 -- one df_window_gather over the frames and ONE df_cond_encode over the B * K windows.
        ``size_len`` is the latent width of one window.  Hand the result to a sampler with ``size_len=cond.size_len_total``; with
        T == 32 it holds get_learned_conditioning's bits and samples exactly like it."""
        eng = self._require()
        if getattr(video_feat, "ndim", 0) != 3:
            raise ValueError(f"get_windowed_conditioning: video_feat of shape {tuple(getattr(video_feat, 'shape', ()))}, expected (B, T, dim)")
        B, T, D = (int(v) for v in video_feat.shape)
        starts, _ = W.plan_windows(T, hop, size_len)
        feats = E._dev_f32(video_feat, self.device)
        if len(starts) > 1:      # frames are rows of D floats: windows of 32 * D "columns" at starts s_k * D
            feats = E.window_gather(feats.reshape(B, 1, 1, T * D), [s * D for s in starts], W.FRAMES * D).reshape(-1, W.FRAMES, D)
        c = eng.cond_encode(feats)
        return W.WindowedConditioning(c.reshape(B, len(starts), W.FRAMES, c.shape[-1]), starts, hop, T, size_len)

    @_locked
    @torch.no_grad()
    def apply_model(self, x_noisy, t, cond, return_ids=False):
        eng = self._require()
        c = self._cond_tensor(cond)
        # the hoisted K/V projections are reused only for the very same bytes: storage, shape AND torch's version
        # counter (an in-place c.copy_() / c.zero_() bumps it), otherwise they are recomputed like the reference does
        # The cached tensor is held by a STRONG reference: its storage cannot be handed to another tensor while it is the
        # cache key (the caching allocator gives a freed block to the next tensor of the same size -- a data_ptr()-only key
        # would then skip set_context for a different conditioning).
        try:
            ver = c._version
        except RuntimeError:          # tensors made under torch.inference_mode() carry no version counter:
            ver = None                # an in-place edit cannot be seen, so the projections are recomputed every call
        key = (tuple(c.shape), ver)
        if ver is None or self._ctx_owner is None or self._ctx_owner[0] is not c or self._ctx_owner[1] != key:
            eng.set_context(c)
            self._ctx_owner = (c, key)
        return eng.unet_forward(x_noisy, t)

    @_locked
    @torch.no_grad()
    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        if predict_cids:
            raise NotImplementedError("VQ code-book decoding is not on the path (AutoencoderKL first stage)")
        # any batch size: df_vae_decode slices batches above 16 samples itself (2 GiB operand addressing, include/df_engine.h)
        return self._require().vae_decode(z)

    @_locked
    @torch.no_grad()
    def decode_first_stage_windowed(self, z, hop_cols=None, size_len=64):
        """decode_first_stage of a latent wider than one window, by the construction the long latent was sampled with: windows of
        ``size_len`` latent columns at a hop of ``hop_cols`` (default size_len / 2), the last one flush right, each decoded by
        df_vae_decode, and the (B * K, out_ch, f H, f size_len) images blended with the integer tent over their f * size_len columns
        into (B, out_ch, f H, f W).  A latent of exactly ``size_len`` columns is decode_first_stage, bit for bit."""
        eng = self._require()
        z = E._dev_f32(z, self.device)
        if z.ndim != 4:
            raise ValueError(f"decode_first_stage_windowed: z of shape {tuple(z.shape)}, expected [B][C][H][W]")
        Wc = int(size_len)
        starts = W.window_starts(z.shape[3], Wc, Wc // 2 if hop_cols is None else hop_cols)
        if len(starts) == 1:
            return eng.vae_decode(z)
        f = 2 ** (len(self.vae_cfg["ch_mult"]) - 1)
        img = eng.vae_decode(E.window_gather(z, starts, Wc))
        return E.window_blend(img, [f * s for s in starts], f * int(z.shape[3]))

    @_locked
    @torch.no_grad()
    def encode_first_stage(self, x):
        """ddpm.py:860-899 without split_input_params: first_stage_model.encode(x), the posterior of the mel image x
        [B][in_channels][H][W] (H, W multiples of the encoder's downsampling).  Needs the checkpoint's first_stage_model.encoder.* and
        quant_conv.* tensors: without them (a sampling-only state dict, a rank that imported the packed blob) it raises."""
        if not self._has_encoder:
            raise NotImplementedError("the VAE encoder is not loaded: load_state_dict was given no complete set of "
                                      "first_stage_model.encoder.* / first_stage_model.quant_conv.* tensors")
        return DiagonalGaussianDistribution(self._require().vae_encode(x))

    @_locked
    @torch.no_grad()
    def get_first_stage_encoding(self, encoder_posterior):
        """ddpm.py:559-566: scale_factor * posterior.sample() (one launch, the scale folded in), or scale_factor * tensor.  The
        reference's isinstance check names the class of models/distribution.py while its autoencoder returns the one of
        stage1_autoencoder/model.py, so it raises on its own posterior; this facade accepts the posterior its encode returns."""
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            return encoder_posterior.sample(scale=float(self.scale_factor))
        if isinstance(encoder_posterior, torch.Tensor):
            self._require()
            return E.lincomb([(float(self.scale_factor), E._dev_f32(encoder_posterior, self.device))])
        raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")

    @_locked
    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None,
               quantize_denoised=False, mask=None, x0=None, shape=None, **kwargs):
        self._require()
        S.reject_unsupported("LatentDiffusion.sample", dict(quantize_denoised=quantize_denoised), dict(quantize_denoised=False))
        if shape is None:
            shape = (batch_size, self.channels, self.image_size, self.image_size)
        if cond is not None and not isinstance(cond, W.WindowedConditioning):
            cond = self._cond_tensor(cond)[:batch_size]
        # The reference hands p_sample_loop its named parameters only (ddpm.py:1264-1268): log_every_t, callback, img_callback and
        # start_T arriving in **kwargs have no effect there, and none here -- the intermediates follow self.log_every_t.  noise_fn and
        # q_noise_fn are this package's replay hooks (no reference name) and are obeyed.
        return S.ancestral_sample(self, cond, tuple(shape), x_T=x_T, timesteps=timesteps, return_intermediates=return_intermediates,
                                  noise_fn=kwargs.get("noise_fn"), mask=mask, x0=x0, q_noise_fn=kwargs.get("q_noise_fn"))

    # ------------------------------------------------------------------ the training objective, evaluated (no gradient)
    @_locked
    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None):
        """ddpm.py:279-282: sqrt_alphas_cumprod[t] * x_start + sqrt_one_minus_alphas_cumprod[t] * noise with one timestep PER SAMPLE
        (t: (B,) integers; a device tensor is not read on the host) -- one df_q_sample."""
        self._require()
        x_start = E._dev_f32(x_start, self.device)
        if noise is None:
            noise = torch.randn_like(x_start)
        return E.q_sample(x_start, noise, t, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)

    @_locked
    @torch.no_grad()
    def get_loss(self, pred, target, mean=True):
        """ddpm.py:284-297.  mean=True is df_diffusion_loss's first scalar (equal sample sizes: the mean of the per-sample means is the
        mean); mean=False -- the element-wise map, which p_losses never materialises -- is a torch expression on the device tensors."""
        self._require()
        pred, target = E._dev_f32(pred, self.device), E._dev_f32(target, self.device)
        if tuple(pred.shape) != tuple(target.shape):
            raise ValueError(f"get_loss: target of shape {tuple(target.shape)}, expected {tuple(pred.shape)} (the shape of pred)")
        if not mean:
            d = target - pred
            return d.abs() if self.loss_type == "l1" else d * d
        rows = pred.reshape(pred.shape[0], -1) if pred.ndim > 1 else pred.reshape(1, -1)
        t0 = torch.zeros(rows.shape[0], dtype=torch.int64, device=self.device)
        return E.diffusion_loss(rows, target.reshape(rows.shape), t0, self.logvar, self.lvlb_weights, self.loss_type)[1][0]

    @_locked
    @torch.no_grad()
    def p_losses(self, x_start, cond, t, noise=None):
        """ddpm.py:1046-1081 in eval mode: (loss, loss_dict) of the eps-objective at the per-sample timesteps t -- df_q_sample, the
        UNet through apply_model, df_diffusion_loss.  loss is a 0-dim device tensor; the values of loss_dict ('val/loss_simple',
        with learn_logvar 'val/loss_gamma' and 'logvar', 'val/loss_vlb', 'val/loss') are Python floats read with ONE device-to-host
        copy at the end -- nothing else in the call waits for the device."""
        self._require()
        x_start = E._dev_f32(x_start, self.device)
        if x_start.ndim != 4:
            raise ValueError(f"p_losses: x_start of shape {tuple(x_start.shape)}, expected [B][C][H][W]")
        B = int(x_start.shape[0])
        if noise is None:
            noise = torch.randn_like(x_start)
        elif tuple(noise.shape) != tuple(x_start.shape):
            raise ValueError(f"p_losses: noise of shape {tuple(noise.shape)}, expected {tuple(x_start.shape)} (the shape of x_start)")
        noise = E._dev_f32(noise, self.device)
        t = E._timestep_indices(t, B, self.num_timesteps, self.device, "p_losses")
        if x_start.numel() == 0:          # the mean of nothing
            scalars = torch.full((5,), float("nan"), device=self.device)
        else:
            x_noisy = E.q_sample(x_start, noise, t, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)
            model_output = self.apply_model(x_noisy, t, cond)
            _, scalars = E.diffusion_loss(model_output, noise, t, self.logvar, self.lvlb_weights, self.loss_type,
                                          self.l_simple_weight, self.original_elbo_weight)
        simple, gamma, vlb, total, logvar = scalars.tolist()      # the one device-to-host copy
        prefix = "train" if self.training else "val"
        loss_dict = {f"{prefix}/loss_simple": simple}
        if self.learn_logvar:
            loss_dict[f"{prefix}/loss_gamma"] = gamma
            loss_dict["logvar"] = logvar
        loss_dict[f"{prefix}/loss_vlb"] = vlb
        loss_dict[f"{prefix}/loss"] = total
        return scalars[3], loss_dict

    @_locked
    @torch.no_grad()
    def forward(self, x, c, *args, **kwargs):
        """ddpm.py:904-913 for the trainable cond stage of Stage2_LDM.yaml: t ~ randint(0, num_timesteps) per sample, drawn on the
        device, c through get_learned_conditioning, then p_losses.  (shorten_cond_schedule is not on the path.)"""
        self._require()
        t = torch.randint(0, self.num_timesteps, (x.shape[0],), device=self.device).long()
        assert c is not None
        c = self.get_learned_conditioning(c)
        return self.p_losses(x, c, t, *args, **kwargs)

    __call__ = forward

    def _sampler(self, name):
        return {"DDIM": S.DDIMSampler, "DPM_Solver": D.DPMSolverSampler, "PLMS": S.PLMSSampler}[name](self)

    def dpm_solver(self, cond, unconditional_guidance_scale=1.0, unconditional_conditioning=None, classifier=None, origin_cond=None,
                   classifier_guide_scale=0.0, predict_x0=True, thresholding=False, max_val=1.):
        """A dpm_solver.DPM_Solver over this model on the fast route (the guided evaluation of the samplers, time embedding hoisted):
        what dpm_solver/sampler.py:50-80 builds, with the whole family behind ``.sample(x, steps=..., order=..., method=...)``.
        ``classifier`` (an AlignmentClassifier) with ``origin_cond`` selects double guidance."""
        ns = D.NoiseScheduleVP('discrete', alphas_cumprod=self.alphas_cumprod)
        if classifier is None:
            fn = D.model_wrapper(self.apply_model, ns, model_type="noise", guidance_type="classifier-free", condition=cond,
                                 unconditional_condition=unconditional_conditioning, guidance_scale=unconditional_guidance_scale)
        else:
            fn = D.model_wrapper_with_classifier(self.apply_model, ns, model_type="noise", guidance_type="double-guide", condition=cond,
                                                 origin_cond=origin_cond, unconditional_condition=unconditional_conditioning,
                                                 guidance_scale=unconditional_guidance_scale, classifier=classifier,
                                                 classifier_guide_scale=classifier_guide_scale)
        return D.DPM_Solver(fn, ns, predict_x0=predict_x0, thresholding=thresholding, max_val=max_val)

    @_locked
    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, size_len=64, unconditional_guidance_scale=1.0,
                   unconditional_conditioning=None, **kwargs):
        return self.sample_log_diff_sampler(cond, batch_size, "DDIM" if ddim else "DDPM", ddim_steps, size_len,
                                            unconditional_guidance_scale, unconditional_conditioning, **kwargs)

    @_locked
    @torch.no_grad()
    def sample_log_diff_sampler(self, cond, batch_size, sampler_name, ddim_steps, size_len=64,
                                unconditional_guidance_scale=1.0, unconditional_conditioning=None, **kwargs):
        self._require()
        if sampler_name in ("DDIM", "DPM_Solver", "PLMS"):
            shape = (self.channels, 16, size_len)          # hard-coded latent height (ddpm.py:1293)
            return self._sampler(sampler_name).sample(
                ddim_steps, batch_size, shape, cond, verbose=False,
                unconditional_guidance_scale=unconditional_guidance_scale,
                unconditional_conditioning=unconditional_conditioning, **kwargs)
        return self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, **kwargs)

    @_locked
    @torch.no_grad()
    def sample_log_with_classifier(self, embed_cond, origin_cond, batch_size, ddim, ddim_steps, size_len=64,
                                   unconditional_guidance_scale=1.0, unconditional_conditioning=None, classifier=None,
                                   classifier_guide_scale=0.0, **kwargs):
        return self.sample_log_with_classifier_diff_sampler(
            embed_cond, origin_cond, batch_size, "DDIM" if ddim else "DDPM", ddim_steps, size_len,
            unconditional_guidance_scale, unconditional_conditioning, classifier, classifier_guide_scale, **kwargs)

    @_locked
    @torch.no_grad()
    def sample_log_with_classifier_diff_sampler(self, embed_cond, origin_cond, batch_size, sampler_name="DDIM",
                                                ddim_steps=250, size_len=64, unconditional_guidance_scale=1.0,
                                                unconditional_conditioning=None, classifier=None,
                                                classifier_guide_scale=0.0, **kwargs):
        self._require()
        if classifier is not None and getattr(classifier, "engine", 1) is None:
            classifier.attach(self)      # the notebook hands over a freshly loaded classifier (ipynb:288-311)
        if sampler_name in ("DDIM", "DPM_Solver"):
            shape = (self.channels, 16, size_len)
            return self._sampler(sampler_name).sample_with_classifier(
                ddim_steps, batch_size, shape, embed_cond, origin_cond=origin_cond, verbose=False,
                unconditional_guidance_scale=unconditional_guidance_scale,
                unconditional_conditioning=unconditional_conditioning, classifier=classifier,
                classifier_guide_scale=classifier_guide_scale, **kwargs)
        return self.sample(cond=embed_cond, batch_size=batch_size, return_intermediates=True, **kwargs)


class AlignmentClassifier:
    """Alignment_Classifier_Double_Guidance.forward (alignment_classifier.py:269-271): prob = sigmoid(head(backbone)).

    Shares the engine of the LatentDiffusion it guides (``attach``).  ``log_prob_grad`` is the input gradient that
    double guidance needs (ddim.py:333-341): forward + hand-written backward-data pass in libdfengine.so."""

    def __init__(self, classifier_config=None, **ignored):
        self.cfg = _unet_params(classifier_config, "classifier_config")
        self._state = None
        self.engine = None

    def load_state_dict(self, state_dict, strict=False):
        self._state = {k: v for k, v in state_dict.items() if k.startswith("model.")}
        from . import synth
        _check_shapes(self._state, synth.classifier_spec(self.cfg), "AlignmentClassifier")
        return [], []

    def attach(self, ldm):
        with ldm._lock:                       # (re)loading tensors finalises the engine: not under another thread's sample()
            self.engine = ldm._require()
            self.engine.config_classifier(self.cfg)
            for k, v in self._state.items():
                self.engine.load_tensor("classifier." + k, v)
            self.engine.finalize()
        return self

    def cuda(self):
        return self

    def eval(self):
        return self

    @torch.no_grad()
    def forward(self, spec_noisy, video_feat=None, t=None):
        """Same argument order as the reference forward(spec_noisy, video_feat, t) (alignment_classifier.py:269); the
        reference's own callers use keywords (ddim.py:338, dpm_solver.py:1345)."""
        if self.engine is None:
            raise RuntimeError("AlignmentClassifier: not attached to an engine yet -- pass it to "
                               "sample_log_with_classifier_diff_sampler (attaches itself) or call .attach(ldm)")
        if video_feat is None or t is None:
            raise TypeError("AlignmentClassifier.forward needs spec_noisy, video_feat and t")
        return self.engine.classifier_forward(spec_noisy, t, video_feat)

    __call__ = forward

    @torch.no_grad()
    def log_prob_grad(self, x, t, video_feat):
        """d sum(log p) / d x (unscaled), the quantity cal_classifier_loglikelihood_grad differentiates (ddim.py:333-341)."""
        if self.engine is None:
            raise RuntimeError("AlignmentClassifier.attach(ldm) first")
        return self.engine.classifier_grad(x, t, video_feat)
