"""The model of the Align-Acc metric: AlignmentClassifierMetric (the reference's ``Alignment_Classifier_metric``), the facades of its
three sub-modules and the ``align_acc_*`` helpers of the evaluation loop (file names, frame counts, input layouts).  Also importable
from ldm.py, where ``instantiate_from_config`` maps the reference's target path to it."""
import torch

from . import engine as E
from .model_base import _EngineModel, _Facade, _check_shapes, _locked, _params, _unet_params, _vae_params
from .schedule import BUFFER_NAMES, register_schedule


def align_acc_clip_name(file_name):
    """The clip a generated mel file belongs to: its name with the last two ``_`` fields dropped (evaluation/dataset.py:36), the stem
    of the clip's ``<name>.npz`` feature file (:91)."""
    return "_".join(file_name.split("_")[:-2])


def align_acc_frames(fps=4, truncate=131072, sr=16000):
    """Feature rows the evaluation keeps, [0, int(fps * truncate / sr)) (evaluation/dataset.py:95-96): 32 with eval_classifier.yaml."""
    return int(fps * truncate / sr)


def align_acc_specs(specs, channels=3, columns=512):
    """The metric's input images from either layout: (N, channels, H, W) as the reference's dataset yields them pass through;
    one-channel mels (N, n_mels, T), as ``decode_first_stage(z)[:, 0]`` and ``wave_to_mel`` give them, are cut to the first ``columns``
    columns and repeated to ``channels`` channels (evaluation/dataset.py:99-107)."""
    if specs.ndim == 4:
        return specs
    if specs.ndim != 3:
        raise RuntimeError(f"align_acc: specs must be (N, {channels}, H, W) images or (N, n_mels, T) mels, got shape {tuple(specs.shape)}")
    return specs[:, None, :, :columns].expand(-1, channels, -1, -1)


class _MetricBackboneFacade(_Facade):
    """Classifier_Backbone.forward(x, timesteps=None, context=None) (alignment_backbone.py:656): the sigmoid probability, (B, 1)."""
    _what = "model"

    def __call__(self, x, timesteps=None, context=None, y=None, **kwargs):
        if y is not None:
            raise NotImplementedError("class-conditional backbone (y=) is not on the path")
        if timesteps is None or context is None:
            raise TypeError("model(x, timesteps, context): the backbone needs the timesteps and the encoded video features")
        return self._m._classify(x, timesteps, context)


class _MetricCondFacade(_Facade):
    """Video_Feat_Encoder_Posembed.forward(x) (video_feat_encoder.py:12-18)."""
    _what = "cond_model"

    def __call__(self, x):
        return self._m.encode_cond(x)


class _MetricFirstStageFacade(_Facade):
    """AutoencoderKL.encode(x); the metric model holds no decoder."""
    _what = "first_stage_model"

    def encode(self, x):
        return self._m.encode_first_stage(x)

    def decode(self, z):
        raise NotImplementedError("AlignmentClassifierMetric holds the VAE encoder only: the evaluation never decodes")


class AlignmentClassifierMetric(_EngineModel):
    """Mirror of the reference ``Alignment_Classifier_metric`` (alignment_classifier_metric.py:71-288), the model of the Align-Acc
    metric (evaluation/align_acc.py with evaluation/config/eval_classifier.yaml): VAE encoder + quant_conv, cond stage and
    Classifier_Backbone under the checkpoint's prefixes ``first_stage_model.``, ``cond_model.`` and ``model.``, in an engine context of
    its own (as CAVPInference has).  ``model_inference`` (align_acc.py:67-87) runs on it as written:

        z = model.encode_spec_z(spec); c = model.cond_model(video_feat); p = model.model(z, context=c, timesteps=t)

    ``probabilities`` is that chain without a host round trip, ``align_acc`` the dataset loop around it.  The training-side members
    (q_sample, training_step, optimisers) are not part of this class.  All compute runs in libdfengine.so; there is no fallback."""

    _not_ready = ("AlignmentClassifierMetric: call load_state_dict(...) and .cuda() first (the model runs in libdfengine.so on a ROCm "
                  "GPU; there is no CPU fallback)")
    _probe_texts = ("a probe pass of the Align-Acc chain",
                    "  No operand type was requested, so this model now runs on the bf16 build (fp32 exponent range, same speed, 8x the "
                    "operand rounding).  AlignmentClassifierMetric(..., precision='fp16') keeps the fp16 build.",
                    "  Probabilities would come from clamped activations.  Fallback: AlignmentClassifierMetric(..., precision='bf16').")

    def __init__(self, classifier_config, first_stage_config, cond_stage_config, monitor, first_stage_ckpt=None,
                 first_stage_key="spec", scale_factor=1.0, timesteps=2, given_betas=None, beta_schedule="linear",
                 linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3, v_posterior=0., parameterization="eps", *args, **kwargs):
        # precision: not a reference argument; same meaning and the same automatic fp16 -> bf16 move as LatentDiffusion's
        super().__init__(kwargs.pop("precision", None))
        if parameterization not in ("eps", "x0"):
            raise NotImplementedError("mu not supported")
        if given_betas is not None:
            raise NotImplementedError("given_betas is not supported (the schedule is built from linear_start / linear_end)")
        self.cls_cfg = _unet_params(classifier_config, "classifier_config")
        self.vae_cfg, double_z = _vae_params(first_stage_config)
        if not double_z:
            raise NotImplementedError("first_stage_config.ddconfig: double_z=False is not supported by libdfengine (the posterior "
                                      "needs mean and logvar)")
        if not 1 <= self.vae_cfg["in_channels"] <= 4:
            raise NotImplementedError(f"first_stage_config.ddconfig: in_channels={self.vae_cfg['in_channels']} is not supported by "
                                      "libdfengine (the encoder's conv_in is built for 1 .. 4 image channels)")
        self.cond_cfg = {k: int(_params(cond_stage_config)[k]) for k in ("origin_dim", "embed_dim", "seq_len")}
        if self.cond_cfg["embed_dim"] != self.cls_cfg["context_dim"]:
            raise ValueError(f"cond_stage_config.embed_dim={self.cond_cfg['embed_dim']} does not match classifier_config.context_dim="
                             f"{self.cls_cfg['context_dim']}")
        if self.vae_cfg["embed_dim"] != self.cls_cfg["in_channels"]:
            raise ValueError(f"first_stage_config.embed_dim={self.vae_cfg['embed_dim']} does not match classifier_config.in_channels="
                             f"{self.cls_cfg['in_channels']}")
        self.first_stage_key = first_stage_key
        self.monitor = monitor
        self.scale_factor = float(scale_factor)
        self.v_posterior = v_posterior
        self.parameterization = parameterization
        self.num_timesteps = int(timesteps)
        self.linear_start, self.linear_end = linear_start, linear_end
        self._buffers = register_schedule(linear_start, linear_end, timesteps, v_posterior, beta_schedule)
        for k, v in self._buffers.items():
            setattr(self, k, v)
        self.first_stage_model = _MetricFirstStageFacade(self)
        self.cond_model = _MetricCondFacade(self)
        self.model = _MetricBackboneFacade(self)
        self._first_stage_state = {}
        self.first_stage_ckpt = first_stage_ckpt
        if first_stage_ckpt is not None:
            self.init_first_from_ckpt(first_stage_ckpt)

    # ------------------------------------------------------------------ nn.Module-like plumbing
    def _spec(self):
        from . import synth
        return synth.align_metric_spec(self.cls_cfg, self.vae_cfg, self.cond_cfg)

    def init_first_from_ckpt(self, path):
        """alignment_classifier_metric.py:179-193: torch.load, ``state_dict`` unwrapped, ``module.`` stripped; the encoder's and
        quant_conv's tensors are kept for the next upload."""
        model = torch.load(path, map_location="cpu")
        if "state_dict" in list(model.keys()):
            model = model["state_dict"]
        want = self._spec()
        new = {"first_stage_model." + k.replace("module.", ""): v for k, v in model.items()}
        self._first_stage_state = {k: v for k, v in new.items() if k in want}
        _check_shapes(self._first_stage_state, want, "AlignmentClassifierMetric")
        missing = [k for k in want if k.startswith("first_stage_model.") and k not in self._first_stage_state]
        print(f"Restored from {path} with {len(missing)} missing and {len(new) - len(self._first_stage_state)} unexpected keys")

    def load_state_dict(self, state_dict, strict=False):
        """Takes ``first_stage_model.encoder.*``, ``first_stage_model.quant_conv.*``, ``model.*`` and ``cond_model.*``; the decoder's
        tensors, when the checkpoint has them, are not kept and not uploaded.  Every tensor of the three modules must be there (here
        or from ``first_stage_ckpt``): the missing ones are named."""
        want = self._spec()
        state = dict(self._first_stage_state)
        state.update({k: v for k, v in state_dict.items() if k in want})
        _check_shapes(state, want, "AlignmentClassifierMetric")
        missing = [k for k in want if k not in state]
        if missing:
            raise RuntimeError(f"Error(s) in loading state_dict for AlignmentClassifierMetric:\n\tMissing key(s) in state_dict: "
                               + ", ".join(missing[:8]) + (f" ... and {len(missing) - 8} more" if len(missing) > 8 else ""))
        self._state = state
        if "scale_factor" in state_dict:          # a registered buffer of the reference module: the checkpoint's value wins
            self.scale_factor = float(state_dict["scale_factor"])
        for k in BUFFER_NAMES:
            if k in state_dict:
                setattr(self, k, state_dict[k].detach().float().to(self.device))
        unexpected = [k for k in state_dict if k not in want and k not in BUFFER_NAMES and k != "scale_factor"]
        if strict and unexpected:
            raise RuntimeError(f"unexpected keys: {unexpected[:5]} ...")
        if self.engine is not None:
            self._upload()
        return [], unexpected

    def _upload(self):
        eng = self.engine
        eng.config_vae_encoder_only(self.vae_cfg, self.scale_factor)
        eng.config_cond(self.cond_cfg)
        eng.config_classifier(self.cls_cfg)
        for k, v in self._state.items():           # the engine's names: the cond stage as LatentDiffusion loads it, the classifier
            if k.startswith("cond_model."):        # under its "classifier." prefix (include/df_engine.h)
                k = "cond_stage_model." + k[len("cond_model."):]
            elif k.startswith("model."):
                k = "classifier." + k
            eng.load_tensor(k, v)
        eng.finalize()
        self._range_check()

    def _probe(self):
        """The range guard's pass (model_base._EngineModel): the whole chain on a uniform [0, 1] image that gives a 16 x 64 latent,
        N(0, 1) features and a fixed posterior draw, t = 0."""
        f = 2 ** (len(self.vae_cfg["ch_mult"]) - 1)
        g = torch.Generator(device="cpu").manual_seed(999)
        x = torch.rand(1, self.vae_cfg["in_channels"], 16 * f, 64 * f, generator=g).to(self.device)
        feats = torch.randn(1, min(32, self.cond_cfg["seq_len"]), self.cond_cfg["origin_dim"], generator=g).to(self.device)
        noise = torch.randn(1, self.vae_cfg["embed_dim"], 16, 64, generator=g)
        self._chain(x, feats, noise)

    # ------------------------------------------------------------------ the path
    def _classify(self, x, timesteps, context):
        with self._lock, torch.no_grad():
            return self._require().classifier_forward(x, timesteps, context)

    def _chain(self, spec, video_feat, noise):
        """moments -> scale_factor * sample -> cond stage -> backbone at t = 0: the existing plans back to back on the current
        stream, no host synchronisation."""
        eng = self._require()
        moments = eng.vae_encode(spec)
        if noise is None:
            noise = torch.randn((moments.shape[0], moments.shape[1] // 2) + tuple(moments.shape[2:]), device=self.device)
        z = E.posterior_sample(moments, noise, float(self.scale_factor))
        c = eng.cond_encode(video_feat)
        return eng.classifier_forward(z, torch.zeros(z.shape[0], device=self.device), c)

    @_locked
    @torch.no_grad()
    def encode_first_stage(self, x):
        """first_stage_model.encode(x) (:196-199): the posterior of the image x [B][in_channels][H][W]."""
        from .ldm import DiagonalGaussianDistribution       # at call time: ldm.py imports this module for its alias table
        return DiagonalGaussianDistribution(self._require().vae_encode(x))

    @_locked
    @torch.no_grad()
    def get_first_stage_encoding(self, encoder_posterior):
        """scale_factor * posterior.sample() (:201-204), one launch; the noise is drawn as the reference draws it (torch.randn from the
        CPU default generator), so torch.manual_seed(s) gives the reference's sample."""
        self._require()
        return encoder_posterior.sample(scale=float(self.scale_factor))

    @_locked
    @torch.no_grad()
    def encode_spec_z(self, x):
        return self.get_first_stage_encoding(self.encode_first_stage(x))

    @_locked
    @torch.no_grad()
    def encode_cond(self, x):
        return self._require().cond_encode(x)

    @torch.no_grad()
    def forward(self, spec_noisy, video_feat, t):
        """The reference hands its three arguments positionally to the backbone's (x, timesteps, context) (:285-287), which puts the
        video features where the timesteps belong and cannot run; this follows the intent, as AlignmentClassifier.forward does:
        ``video_feat`` is the backbone's context (the cond stage's output), ``t`` its timesteps."""
        return self._classify(spec_noisy, t, video_feat)

    __call__ = forward

    @_locked
    @torch.no_grad()
    def probabilities(self, spec, video_feat, noise=None):
        """(B, 1) fp32 device tensor of p(aligned) for images ``spec`` (B, in_channels, H, W) and raw CAVP features ``video_feat``
        (B, T, origin_dim): model_inference's chain (align_acc.py:81-84) at t = 0 in one pass, without a host synchronisation.
        ``noise`` (B, embed_dim, H / f, W / f) replays a posterior draw; None draws it on the device (torch.randn, the device's
        generator)."""
        return self._chain(spec, video_feat, noise)

    @_locked
    @torch.no_grad()
    def align_acc(self, specs, video_feats, labels=None, batch_size=64, noise=None):
        """The Align-Acc count of a generated set (eval_audio + model_inference, align_acc.py:67-115): (correct, total) as Python ints.
        ``specs``: (N, in_channels, H, W) images, or (N, n_mels, T) one-channel mels (align_acc_specs cuts and repeats them);
        ``video_feats`` (N, T, origin_dim); ``labels`` default to ones (:76).  Runs in slices of ``batch_size``, the last one ragged; the
        two counters stay on the device (df_align_verdict) and only the return value synchronises with the host.  ``noise`` (not in the
        reference) replays the posterior draws of the whole set, (N, embed_dim, H / f, W / f)."""
        self._require()
        specs = align_acc_specs(specs, self.vae_cfg["in_channels"])
        N = int(specs.shape[0])
        if int(video_feats.shape[0]) != N:
            raise RuntimeError(f"align_acc: {N} specs and {int(video_feats.shape[0])} feature sequences")
        if int(batch_size) < 1:
            raise ValueError(f"align_acc: batch_size={batch_size}")
        if labels is not None:
            labels = E._dev_f32(torch.as_tensor(labels), self.device).reshape(-1)
            if labels.numel() != N:
                raise RuntimeError(f"align_acc: {labels.numel()} labels for {N} specs")
        counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        for i in range(0, N, int(batch_size)):
            sl = slice(i, min(i + int(batch_size), N))
            p = self._chain(specs[sl], video_feats[sl], None if noise is None else noise[sl])
            E.align_verdict(p, None if labels is None else labels[sl], counts)
        correct, total = counts.cpu().tolist()
        return int(correct), int(total)
