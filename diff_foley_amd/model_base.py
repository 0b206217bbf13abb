"""What the model classes share: the config readers (``_params``, ``_unet_params``, ``_vae_params``), the state-dict shape check, the
per-model lock, ``_Facade`` (the stand-in for a reference sub-module) and ``_EngineModel``, the base of the models that own an engine
context -- LatentDiffusion (ldm.py), AlignmentClassifierMetric (align_metric.py), CAVPInference (cavp.py): their nn.Module-like
plumbing (``to`` / ``cuda`` / ``eval`` / ``autotune``) and the fp16 range guard behind every upload of weights."""
import functools
import os
import sys
import threading
import warnings

import torch

from . import engine as E
from .schedule import BUFFER_NAMES

_UNET_KEYS = ("in_channels", "out_channels", "model_channels", "attention_resolutions", "num_res_blocks",
              "channel_mult", "num_heads", "context_dim")
# UNetModel constructor arguments (openai_unetmodel.py:451-468) whose non-default values select code that is not built
# here; the value the engine implements is listed, anything else raises instead of producing a different network.
_UNET_FIXED = dict(dims=2, dropout=0, conv_resample=True, num_classes=None, num_head_channels=-1, num_heads_upsample=-1,
                   use_scale_shift_norm=False, resblock_updown=False, use_new_attention_order=False,
                   use_spatial_transformer=True, transformer_depth=1, n_embed=None, legacy=False)


_VAE_FIXED = dict(attn_resolutions=[], dropout=0.0, resamp_with_conv=True, give_pre_end=False, tanh_out=False,
                  use_linear_attn=False, attn_type="vanilla")


def _vae_params(first_stage_config):
    """(the engine's VAE dict, double_z) of an AutoencoderKL ``first_stage_config``."""
    fs = _params(first_stage_config)
    dd = dict(fs["ddconfig"])
    # Decoder constructor arguments (stage1_autoencoder/model.py:557-561) whose non-default values select code that is not built
    # here (attention inside the up levels, conv-less / tanh / pre-end outputs, linear attention): refused, not ignored
    for k, v in _VAE_FIXED.items():
        if k in dd and (list(dd[k]) if isinstance(v, list) else dd[k]) != v and not (k == "dropout" and float(dd[k]) == 0.0):
            raise NotImplementedError(f"first_stage_config.ddconfig: {k}={dd[k]!r} is not supported by libdfengine "
                                      f"(built for {k}={v!r})")
    cfg = dict(z_channels=dd["z_channels"], embed_dim=fs["embed_dim"], ch=dd["ch"],
               ch_mult=[int(v) for v in dd["ch_mult"]], num_res_blocks=dd["num_res_blocks"],
               out_ch=dd["out_ch"], in_channels=int(dd.get("in_channels", 3)))
    return cfg, bool(dd.get("double_z", True))


def _unet_params(cfg, what):
    p = _params(cfg)
    for k, v in _UNET_FIXED.items():
        if k in p and p[k] != v and not (k == "dropout" and float(p[k]) == 0.0):
            raise NotImplementedError(f"{what}: {k}={p[k]!r} is not supported by libdfengine (built for {k}={v!r})")
    out = {k: p[k] for k in _UNET_KEYS}
    for k in ("attention_resolutions", "channel_mult"):
        out[k] = [int(v) for v in out[k]]
    return out


def _params(cfg):
    """Accept {'target':..., 'params': {...}} (YAML form) or the params dict itself."""
    if cfg is None:
        return None
    cfg = dict(cfg)
    return dict(cfg["params"]) if "params" in cfg else cfg


def _check_shapes(state, spec, what):
    """torch's load_state_dict raises on a size mismatch even with strict=False; the engine's packers take a tensor's own shape, so a
    checkpoint of another architecture would load and run as a different network.  ``spec``: name -> shape of the configured modules
    (synth.*_spec: the reference's key layout)."""
    bad = [f"size mismatch for {k}: copying a param with shape {tuple(v.shape)} from checkpoint, the shape in current model is "
           f"{tuple(spec[k])}" for k, v in state.items() if k in spec and tuple(v.shape) != tuple(spec[k])]
    nonfinite = [k for k, v in state.items() if k in spec and v.is_floating_point() and not bool(torch.isfinite(v).all())]
    if nonfinite:       # the reference would sample NaN; the fp16-operand build's saturating stores would hide it
        warnings.warn(f"{what}: {len(nonfinite)} checkpoint tensor(s) hold non-finite values ({nonfinite[0]} ...): the fp32 reference "
                      f"would produce NaN with them", RuntimeWarning, stacklevel=3)
    if bad:
        raise RuntimeError(f"Error(s) in loading state_dict for {what}:\n\t" + "\n\t".join(bad[:8]) +
                           (f"\n\t... and {len(bad) - 8} more" if len(bad) > 8 else ""))


def _locked(fn):
    """One caller at a time per model: a sample() call is a sequence of engine calls that share the model's context operands,
    timestep table and plan workspaces.  (A torch module's forward is re-entrant from several host threads; this keeps the facade so.)"""
    @functools.wraps(fn)
    def run(self, *a, **kw):
        with self._lock:
            return fn(self, *a, **kw)
    return run


class _Facade:
    """Stands where the reference has a sub-module: the forward entry points code outside the samplers calls
    (`model.model.diffusion_model(x, t, context=c)`, `model.first_stage_model.decode(z)`, `model.cond_stage_model(feats)`) run
    on the engine; anything that needs the nn.Module tree itself (parameters, children, weights) raises like before -- the
    weights live in packed HBM buffers owned by libdfengine.so."""
    _what = "module"

    def __init__(self, owner):
        object.__setattr__(self, "_m", owner)

    def __getattr__(self, name):
        raise AttributeError(f"{self._what}.{name}: module tree is not materialised in diff_foley_amd "
                             "(weights live in packed HBM buffers owned by libdfengine.so)")

    def eval(self):
        return self

    def cuda(self, device=None):
        return self


def _warn_caller(message):
    """A RuntimeWarning attributed to the line that called into this package, however deep the load path below it is
    (``cuda`` -> ``to`` -> ``_upload`` -> ``_range_check``, or ``load_state_dict`` -> ``_upload`` -> ...)."""
    level, frame = 1, sys._getframe(0)
    while frame.f_back is not None and frame.f_code.co_filename.startswith(os.path.dirname(__file__) + os.sep):
        level, frame = level + 1, frame.f_back
    warnings.warn(message, RuntimeWarning, stacklevel=level)


class _EngineModel:
    """A model that owns its engine context.  A subclass keeps its tensors in ``_state`` (None until load_state_dict) and writes
    ``_upload``: its ``config_*`` calls, its tensors under the engine's names, ``finalize()`` and, last, ``self._range_check()`` --
    the fp16 range guard.  The default operand type (fp16) clamps at +-65504 where
    the reference (fp32) has no limit, and the tolerance evidence behind that default comes from procedurally generated weights: a
    trained checkpoint whose activations leave the range would clamp and still return a plausible result.  So every (re)load of weights
    is followed by ONE saturation-counted pass of the model on fixed random inputs (``_probe``, with ``_probe_texts`` and, where not
    every load can be probed, ``_probe_ready``); a class without ``_probe`` is not probed."""
    _buffer_names = BUFFER_NAMES      # the schedule buffers that move with the model; () where the class has none
    _not_ready = "call load_state_dict(...) and .cuda() first"
    _probe = None                     # no probe: the class never warns and never changes its precision by itself
    training = False
    _probe_texts = None               # the warning's own words: (what ran, the sentences after a move to bf16, those without one)

    def __init__(self, precision):
        self._lock = threading.RLock()
        self.precision = precision
        # precision=None (and no DF_PRECISION): the operand type is the PRODUCT's choice, so it is also the product's job to keep
        # it safe -- if the range probe behind load_state_dict / .cuda() finds fp16 operands at the saturation point with the loaded
        # weights, the model moves itself to the bf16 build (fp32 exponent range) and says so.  An explicit precision is obeyed.
        self._auto_precision = precision is None and "DF_PRECISION" not in os.environ
        self.device = torch.device("cpu")
        self.engine = None
        self._state = None

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"diff_foley_amd.{type(self).__name__} runs on a ROCm GPU only (no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(device)
        self.device = device
        self.engine = E.Engine(device, precision=self.precision)
        for k in self._buffer_names:
            setattr(self, k, getattr(self, k).to(device))
        if self._state is not None:
            self._upload()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    def autotune(self, enable=True):
        self._require().autotune(enable)
        return self

    def _require(self):
        if self.engine is None or self._state is None:
            raise RuntimeError(self._not_ready)
        return self.engine

    def _probe_ready(self):
        return True

    def _range_check(self):
        """[(op, count)] of the probe's ops that stored operand-type values AT the saturation point (df_debug_saturations).  Any
        count > 0 raises a RuntimeWarning that names the ops; with no operand type requested (``_auto_precision``) the model also
        moves itself to the bf16 build (fp32 exponent range).  DF_RANGE_CHECK=0 skips the probe."""
        eng = self.engine
        if (self._probe is None or eng is None or eng.precision != "fp16" or os.environ.get("DF_RANGE_CHECK", "1") == "0"
                or not self._probe_ready()):
            return []
        tune_was = eng.autotune_on
        if tune_was:
            eng.autotune(False)   # the probe plan must not be tuned: load latency, not a product shape
        bad = []
        eng.debug_saturations(True)
        try:
            self._probe()
            torch.cuda.synchronize(self.device)
            bad = [(lab, n) for lab, n in eng.debug_saturations_read() if n]
        except RuntimeError as ex:      # the guard must never turn a loadable checkpoint into a load-time error
            _warn_caller(f"fp16 range probe skipped: {ex}")
        finally:
            eng.debug_saturations(False)
            eng.finalize()        # drops the probe's plans: a later autotune(True) must meet no ready-made plan of this shape
            if tune_was:
                eng.autotune(True)
        if not bad:
            return bad
        what, moved, explicit = self._probe_texts
        shown = ", ".join(f"{lab}: {n}" for lab, n in bad[:6]) + (" ..." if len(bad) > 6 else "")
        head = f"fp16 operands saturated at +-65504 in {len(bad)} op(s) of {what} with these weights -- {shown}."
        if not self._auto_precision:
            _warn_caller(head + explicit)
            return bad
        _warn_caller(head + moved)
        self.precision = "bf16"
        self._auto_precision = False
        old = self.engine
        self.engine = E.Engine(self.device, precision="bf16")
        if tune_was:
            self.engine.autotune(True)
        old.close()
        self._upload()                # (the bf16 build has no range to probe: _range_check returns at once)
        return bad
