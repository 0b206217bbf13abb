"""The DPM-Solver family of the reference (diff_foley/models/diffusion/dpm_solver/dpm_solver.py) on the MI355X path: NoiseScheduleVP,
model_wrapper / model_wrapper_with_classifier and DPM_Solver with orders 1-3, the singlestep / singlestep_fixed / multistep /
adaptive methods, three step spacings, noise and data prediction, both expansions, t_start / t_end, denoise_to_zero and dynamic
thresholding -- behind the reference's names and parameter lists; and DPMSolverSampler (dpm_solver/sampler.py), the samplers' call
surface over the solver's DPM-Solver++(2M) configuration.

How it runs.  Times and every coefficient are fp32 scalars ON THE HOST (schedule.DPMTables / ContinuousTables); each solver update is
one ``df_lincomb`` of at most four tensors (the D1 / D2 differences of the third-order formulas are expanded into the model values
they are made of), the thresholded data prediction is
``df_dpm_data_prediction`` and the adaptive solver's error estimate ``df_dpm_adaptive_error``.  ``s`` / ``t`` arguments may be floats,
0-d tensors or (B,) tensors with equal entries; a device tensor is read once; unequal entries raise ValueError (the host drives one
time for the whole batch).  ``sample()`` itself waits for the device nowhere -- except ``method='adaptive'``, which reads one float
per attempted step.

Two routes for the model.
  * generic: any callable is called exactly as the reference calls it -- ``model(x, t_input[, cond], **model_kwargs)`` with the
    ``cat`` / ``chunk`` batch of classifier-free guidance -- and the arithmetic around it (guidance combine, the x_start / v / score
    conversions) runs on the engine.
  * fast: when the wrapped model is the bound ``apply_model`` of a diff_foley_amd.LatentDiffusion (``LatentDiffusion.dpm_solver``
    builds exactly that), the guided evaluation is the samplers' ``_Guided`` (``df_unet_forward_cfg``) with the time embedding
    hoisted for every time the call will visit; the singlestep intermediate times are known on the host before the loop.  The
    adaptive solver cannot know its times and computes the embedding inside the step.

Deviations from the reference, all on argument sets the reference cannot run:
  * ``method='singlestep'`` with ``skip_type`` 'time_uniform' / 'time_quadratic' works (the reference calls torch.cumsum without
    ``dim``, dpm_solver.py:495, and raises TypeError on its own recommended call); the cumulative sum is over dim 0.
  * ``method='multistep', order=3, lower_order_final=True, 4 <= steps < 15`` raises ValueError before any launch, with a message that
    names the two ways out (the reference fails with "too many values to unpack", :773, in the middle of the loop).
  * classifier guidance needs a diff_foley_amd AlignmentClassifier (``log_prob_grad``): there is no autograd on this path, so a
    plain ``classifier_fn`` raises NotImplementedError.
  * a NaN error estimate ends the adaptive solver with FloatingPointError (the reference loops forever on it); an unknown
    ``method`` raises ValueError (the reference returns x unchanged).
"""
import numpy as np
import torch

from . import engine as E
from . import samplers
from .schedule import ContinuousTables, DPMTables
from .windows import WindowedConditioning

F = np.float32


def _scalar(t, what="t"):
    """One host fp32 scalar from a float, a 0-d tensor or a vector of equal entries (a device tensor is copied once)."""
    if torch.is_tensor(t):
        t = t.detach().reshape(-1).to("cpu", torch.float32).numpy()
    if isinstance(t, np.ndarray):
        v = t.reshape(-1)
        if v.size == 0:
            raise ValueError(f"{what}: an empty time tensor")
        if not (v == v[0]).all():
            raise ValueError(f"{what}: the entries of a time vector must be equal (one time for the whole batch), got "
                             f"{v[:4].tolist()}{' ...' if v.size > 4 else ''}")
        return F(v[0])
    return F(t)


def _linspace(a, b, n):
    return torch.linspace(a, b, n).numpy().astype(np.float32)      # torch's fp32 formula, on the host


class NoiseScheduleVP:
    """dpm_solver.py:6-174.  The numbers live in ``self.tables`` (host fp32); the five methods take what the reference's take -- a
    tensor of times (any entries) -- and return a tensor on its device, or take a float and return a numpy fp32 scalar."""

    def __init__(self, schedule='discrete', betas=None, alphas_cumprod=None, continuous_beta_0=0.1, continuous_beta_1=20.):
        if schedule not in ['discrete', 'linear', 'cosine']:
            raise ValueError("Unsupported noise schedule {}. The schedule needs to be 'discrete' or 'linear' or 'cosine'".format(schedule))
        self.schedule = schedule
        if schedule == 'discrete':
            self.tables = DPMTables(alphas_cumprod=alphas_cumprod, betas=betas)
            self.total_N = self.tables.N
            self.T = 1.
            self.t_array = torch.from_numpy(self.tables.t_knots.copy()).reshape((1, -1))
            self.log_alpha_array = torch.from_numpy(self.tables.la_knots.copy()).reshape((1, -1))
        else:
            self.tables = ContinuousTables(schedule, continuous_beta_0, continuous_beta_1)
            self.total_N = 1000
            self.beta_0, self.beta_1 = continuous_beta_0, continuous_beta_1
            for k in ("cosine_s", "cosine_beta_max", "cosine_t_max", "cosine_log_alpha_0"):
                setattr(self, k, getattr(self.tables, k))
            self.T = self.tables.T

    def _map(self, fn, t, flat=False):
        if not torch.is_tensor(t):
            return fn(t)
        v = t.detach().to("cpu", torch.float32).numpy()
        out = np.asarray([fn(e) for e in v.reshape(-1)], dtype=np.float32).reshape((-1,) if flat else v.shape)
        return torch.from_numpy(out).to(t.device)

    def marginal_log_mean_coeff(self, t):
        return self._map(self.tables.log_alpha, t, flat=self.schedule == 'discrete')

    def marginal_alpha(self, t):
        return self._map(self.tables.alpha, t, flat=self.schedule == 'discrete')

    def marginal_std(self, t):
        return self._map(self.tables.sigma, t, flat=self.schedule == 'discrete')

    def marginal_lambda(self, t):
        return self._map(self.tables.lam, t, flat=self.schedule == 'discrete')

    def inverse_lambda(self, lamb):
        return self._map(self.tables.inverse_lambda, lamb, flat=self.schedule == 'discrete')


def _ldm_of(model):
    """The LatentDiffusion whose bound apply_model ``model`` is, or None."""
    from .ldm import LatentDiffusion
    owner = getattr(model, "__self__", None)
    if isinstance(owner, LatentDiffusion) and getattr(model, "__func__", None) is LatentDiffusion.apply_model:
        return owner
    return None


class _WrappedModel:
    """What model_wrapper returns: ``fn(x, t_continuous) -> noise`` like the reference's closure, plus what DPM_Solver needs to
    recognise the fast route."""

    def __init__(self, model, noise_schedule, model_type, model_kwargs, guidance_type, condition, unconditional_condition,
                 guidance_scale, classifier_fn, classifier_kwargs, origin_cond=None, classifier=None, classifier_guide_scale=0,
                 guidance_types=("uncond", "classifier", "classifier-free")):
        assert model_type in ["noise", "x_start", "v"]
        assert guidance_type in guidance_types
        if not isinstance(noise_schedule, NoiseScheduleVP):
            raise TypeError("model_wrapper: noise_schedule must be a diff_foley_amd.dpm_solver.NoiseScheduleVP")
        if guidance_type == "classifier" and classifier_fn is not None and not hasattr(classifier_fn, "log_prob_grad"):
            raise NotImplementedError("guidance_type='classifier' needs a diff_foley_amd AlignmentClassifier as classifier_fn (its "
                                      "log_prob_grad is a hand-written backward pass); a plain callable would need autograd, which "
                                      "this path does not have")
        if guidance_type == "double-guide" and classifier is not None and not hasattr(classifier, "log_prob_grad"):
            raise NotImplementedError("guidance_type='double-guide' needs a diff_foley_amd AlignmentClassifier (log_prob_grad): "
                                      "there is no autograd on this path")
        self.model, self.noise_schedule, self.tables = model, noise_schedule, noise_schedule.tables
        self.model_type, self.model_kwargs, self.guidance_type = model_type, dict(model_kwargs or {}), guidance_type
        self.condition, self.unconditional_condition, self.guidance_scale = condition, unconditional_condition, guidance_scale
        self.classifier_fn, self.classifier_kwargs = classifier_fn, dict(classifier_kwargs or {})
        self.origin_cond, self.classifier, self.classifier_guide_scale = origin_cond, classifier, classifier_guide_scale
        self.fast_model = _ldm_of(model)
        self.fast = (self.fast_model is not None and model_type == "noise" and not self.model_kwargs and condition is not None
                     and guidance_type in ("classifier-free", "double-guide"))
        if isinstance(condition, WindowedConditioning):      # a clip longer than one window (windows.py)
            if not self.fast:
                raise NotImplementedError("a windowed conditioning is served by the fast route only (LatentDiffusion.dpm_solver, or "
                                          "model_wrapper around LatentDiffusion.apply_model with model_type='noise' and classifier-free "
                                          "guidance): the generic route hands the condition to a callable that knows nothing of windows")
            samplers.refuse_windowed_classifier(condition, classifier if guidance_type == "double-guide" else None)

    @property
    def cfg(self):
        return not (self.guidance_scale == 1. or self.unconditional_condition is None)

    def _t_input(self, t, n, device):
        return torch.full((n,), float(self.tables.model_time(t)), device=device, dtype=torch.float32)

    def _noise_pred(self, x, t, cond=None):
        t_input = self._t_input(t, x.shape[0], x.device)
        output = self.model(x, t_input, **self.model_kwargs) if cond is None else self.model(x, t_input, cond, **self.model_kwargs)
        output = E._dev_f32(output, x.device)
        if self.model_type == "noise":
            return output
        a, s = self.tables.alpha(t), self.tables.sigma(t)
        if self.model_type == "x_start":
            return E.lincomb([(F(1.0) / s, x), (-a / s, output)])
        if self.model_type == "v":
            return E.lincomb([(a, output), (s, x)])
        return E.lincomb([(-s, output)])          # "score"

    def _grad(self, classifier, x, t, cond):
        t_input = self._t_input(t, x.shape[0], x.device)
        if self.fast_model is not None:
            return samplers._classifier_grad(self.fast_model, classifier, x, t_input, cond)
        return classifier.log_prob_grad(x, t_input, cond)

    def _eval(self, x, t):
        """noise(x, t) at the host time t on the generic route (dpm_solver.py:321-344, 1352-1393)."""
        x = E._dev_f32(x, x.device)
        g = self.guidance_type
        if g == "uncond":
            return self._noise_pred(x, t)
        if g == "classifier":
            assert self.classifier_fn is not None
            if self.classifier_kwargs:
                raise NotImplementedError("classifier_kwargs are not supported: log_prob_grad takes (x, t, cond)")
            grad = self._grad(self.classifier_fn, x, t, self.condition)
            noise = self._noise_pred(x, t)
            return E.lincomb([(1.0, noise), (-F(self.guidance_scale) * self.tables.sigma(t), grad)])
        if not self.cfg:
            return self._noise_pred(x, t, cond=self.condition)
        x_in = torch.cat([x] * 2)
        c_in = torch.cat([self.unconditional_condition, self.condition])
        noise = E.cfg_combine(self._noise_pred(x_in, t, cond=c_in), self.guidance_scale)      # uncond + scale (cond - uncond)
        if g == "double-guide" and self.classifier is not None:
            grad = self._grad(self.classifier, x, t, self.origin_cond)
            noise = E.lincomb([(1.0, noise), (-self.classifier_guide_scale * self.tables.sigma(t), grad)])
        return noise

    def __call__(self, x, t_continuous):
        t = _scalar(t_continuous, "model_fn")
        if self.fast:
            return _FastSession(self, tuple(x.shape))(x, t)
        return self._eval(x, t)


class _FastSession:
    """The guided UNet evaluation of one sample() call on the fast route: the samplers' _Guided over the LatentDiffusion's engine, with
    the time embedding of ``times`` (host fp32, every time the call will visit) hoisted.  A time that is not in the table -- or no
    table at all (adaptive) -- takes the in-step embedding, which gives the same bits."""

    def __init__(self, w, x_shape, times=None):
        self.w, self.m, self.tb = w, w.fast_model, w.tables
        self.B = int(x_shape[0])
        dev = self.m.device
        t_model = None
        self.index, self.t_all = {}, None
        if times:
            uniq = list(dict.fromkeys(float(t) for t in times))
            t_model = [self.tb.model_time(t) for t in uniq]
            self.index = {t: k for k, t in enumerate(uniq)}
            self.t_all = torch.tensor(t_model, dtype=torch.float32, device=dev)[:, None].expand(len(uniq), self.B).contiguous()
        self.double = w.guidance_type == "double-guide" and w.classifier is not None and w.cfg
        if self.double and getattr(w.classifier, "engine", 1) is None:
            w.classifier.attach(self.m)      # loading its tensors re-finalises the engine: before the context and the table are set
        self.eps = samplers._Guided(self.m, w.condition, w.guidance_scale, w.unconditional_condition, t_model, tuple(x_shape))

    def __call__(self, x, t):
        x = E._dev_f32(x, self.m.device)
        k = self.index.get(float(t))
        t_in = self.t_all[k] if k is not None else \
            torch.full((self.B,), float(self.tb.model_time(t)), device=self.m.device, dtype=torch.float32)
        if not self.double:
            return self.eps(x, t_in, k)
        w = self.w                                                 # double guidance (dpm_solver.py:1377-1393)
        return samplers._classifier_guided_eps(self.m, w.classifier, lambda: self.eps(x, t_in, k), x, t_in, w.origin_cond,
                                        w.classifier_guide_scale * self.tb.sigma(t))


def model_wrapper(model, noise_schedule, model_type="noise", model_kwargs={}, guidance_type="uncond", condition=None,
                  unconditional_condition=None, guidance_scale=1., classifier_fn=None, classifier_kwargs={}):
    """dpm_solver.py:177-348: ``model_fn(x, t_continuous) -> noise`` around a model that takes discrete-time (or continuous-time)
    labels, with "uncond" | "classifier" | "classifier-free" guidance and the "noise" | "x_start" | "v" parameterisations."""
    return _WrappedModel(model, noise_schedule, model_type, model_kwargs, guidance_type, condition, unconditional_condition,
                         guidance_scale, classifier_fn, classifier_kwargs)


def model_wrapper_with_classifier(model, noise_schedule, model_type="noise", model_kwargs={}, guidance_type="uncond", condition=None,
                                  origin_cond=None, unconditional_condition=None, guidance_scale=1., classifier_fn=None,
                                  classifier_kwargs={}, classifier=None, classifier_guide_scale=0):
    """dpm_solver.py:1192-1397: model_wrapper plus "double-guide" -- classifier-free guidance and the alignment classifier's gradient
    at ``origin_cond``."""
    return _WrappedModel(model, noise_schedule, model_type, model_kwargs, guidance_type, condition, unconditional_condition,
                         guidance_scale, classifier_fn, classifier_kwargs, origin_cond, classifier, classifier_guide_scale,
                         guidance_types=("uncond", "classifier", "classifier-free", "double-guide"))


def _check_solver_type(solver_type):
    if solver_type not in ['dpm_solver', 'taylor']:
        raise ValueError("'solver_type' must be either 'dpm_solver' or 'taylor', got {}".format(solver_type))


_ORDER3_FINAL = ("method='multistep' with order=3 and lower_order_final=True lowers the order of the last steps when steps < 15, and the "
                 "second-order multistep update cannot take the three-entry history it then meets (the reference fails on the same "
                 "call): pass lower_order_final=False or steps >= 15")


class DPM_Solver:
    def __init__(self, model_fn, noise_schedule, predict_x0=False, thresholding=False, max_val=1.):
        """dpm_solver.py:351-378.  ``model_fn(x, t_continuous) -> noise``: what model_wrapper returns, or any callable."""
        if not isinstance(noise_schedule, NoiseScheduleVP):
            raise TypeError("DPM_Solver: noise_schedule must be a diff_foley_amd.dpm_solver.NoiseScheduleVP")
        self.model = model_fn
        self.noise_schedule = noise_schedule
        self.tables = noise_schedule.tables
        self.predict_x0 = predict_x0
        self.thresholding = thresholding
        self.max_val = max_val
        self.fast = isinstance(model_fn, _WrappedModel) and model_fn.fast
        self._session = None
        self.adaptive_trace = []      # (t tried, E, accepted) of the last adaptive run, host floats

    # ------------------------------------------------------------------ the model
    def _noise(self, x, t):
        if self._session is not None:
            return self._session(x, t)
        if isinstance(self.model, _WrappedModel):
            return self.model(x, t)
        x = E._dev_f32(x, x.device)
        out = self.model(x, torch.full((x.shape[0],), float(t), device=x.device, dtype=torch.float32))
        return E._dev_f32(out, x.device)

    def _data(self, x, t):
        noise = self._noise(x, t)
        x = E._dev_f32(x, noise.device)
        a, s = self.tables.alpha(t), self.tables.sigma(t)
        if self.thresholding:
            return E.dpm_data_prediction(x, noise, a, s, True, self.max_val)
        return E.lincomb([(1.0 / a, x), (-s / a, noise)])

    def _model(self, x, t):
        return self._data(x, t) if self.predict_x0 else self._noise(x, t)

    def noise_prediction_fn(self, x, t):
        return self._noise(x, _scalar(t))

    def data_prediction_fn(self, x, t):
        """x0 = (x - sigma_t noise) / alpha_t, with dynamic thresholding when asked (dpm_solver.py:386-399)."""
        return self._data(x, _scalar(t))

    def model_fn(self, x, t):
        return self._model(x, _scalar(t))

    # ------------------------------------------------------------------ times
    def _time_steps(self, skip_type, t_T, t_0, N):
        tb = self.tables
        if skip_type == 'logSNR':
            lam = _linspace(float(tb.lam(F(t_T))), float(tb.lam(F(t_0))), N + 1)
            return np.asarray([tb.inverse_lambda(v) for v in lam], dtype=np.float32)
        elif skip_type == 'time_uniform':
            return _linspace(t_T, t_0, N + 1)
        elif skip_type == 'time_quadratic':
            t_order = 2
            return _linspace(t_T ** (1. / t_order), t_0 ** (1. / t_order), N + 1) ** t_order
        raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'".format(skip_type))

    def get_time_steps(self, skip_type, t_T, t_0, N, device):
        """dpm_solver.py:410-437: the (N + 1,) time steps as a tensor on ``device`` (computed on the host)."""
        return torch.from_numpy(self._time_steps(skip_type, t_T, t_0, N)).to(device)

    def _orders_and_timesteps(self, steps, order, skip_type, t_T, t_0):
        if order == 3:
            K = steps // 3 + 1
            if steps % 3 == 0:
                orders = [3, ] * (K - 2) + [2, 1]
            elif steps % 3 == 1:
                orders = [3, ] * (K - 1) + [1]
            else:
                orders = [3, ] * (K - 1) + [2]
        elif order == 2:
            if steps % 2 == 0:
                K = steps // 2
                orders = [2, ] * K
            else:
                K = steps // 2 + 1
                orders = [2, ] * (K - 1) + [1]
        elif order == 1:
            K = 1
            orders = [1, ] * steps
        else:
            raise ValueError("'order' must be '1' or '2' or '3'.")
        if skip_type == 'logSNR':      # to reproduce the results of the DPM-Solver paper
            outer = self._time_steps(skip_type, t_T, t_0, K)
        else:                          # the cumulative sum over dim 0 that dpm_solver.py:495 means
            outer = self._time_steps(skip_type, t_T, t_0, steps)[np.cumsum([0, ] + orders)]
        return outer, orders

    def get_orders_and_timesteps_for_singlestep_solver(self, steps, order, skip_type, t_T, t_0, device):
        """dpm_solver.py:439-496 ("DPM-Solver-fast"): (timesteps_outer tensor on ``device``, orders)."""
        outer, orders = self._orders_and_timesteps(steps, order, skip_type, t_T, t_0)
        return torch.from_numpy(np.ascontiguousarray(outer)).to(device), orders

    def _inner_times(self, s, t, r1=None, r2=None):
        """(s1, s2) of a singlestep update from s to t: inverse_lambda(lambda_s + r h) for the given ratios (None: not needed)."""
        tb = self.tables
        lam_s = tb.lam(s)
        h = tb.lam(t) - lam_s
        return tuple(None if r is None else tb.inverse_lambda(lam_s + F(r) * h) for r in (r1, r2))

    def denoise_to_zero_fn(self, x, s):
        return self._data(x, _scalar(s))

    # ------------------------------------------------------------------ updates: each one df_lincomb over host coefficients
    def dpm_solver_first_update(self, x, s, t, model_s=None, return_intermediate=False):
        """DPM-Solver-1 (DDIM) from s to t (dpm_solver.py:504-549)."""
        ns = self.tables
        s, t = _scalar(s, "s"), _scalar(t, "t")
        h = ns.lam(t) - ns.lam(s)
        if model_s is None:
            model_s = self._model(x, s)
        if self.predict_x0:
            x_t = E.lincomb([(ns.sigma(t) / ns.sigma(s), x), (-ns.alpha(t) * np.expm1(-h), model_s)])
        else:
            x_t = E.lincomb([(np.exp(ns.log_alpha(t) - ns.log_alpha(s)), x), (-ns.sigma(t) * np.expm1(h), model_s)])
        return (x_t, {'model_s': model_s}) if return_intermediate else x_t

    def _sides(self, s, u):
        """(coefficient of x, scale of the model terms) of a move from s to u: x_u = cx x - scale * phi * model ..."""
        ns = self.tables
        if self.predict_x0:
            return ns.sigma(u) / ns.sigma(s), ns.alpha(u)
        return np.exp(ns.log_alpha(u) - ns.log_alpha(s)), ns.sigma(u)

    def singlestep_dpm_solver_second_update(self, x, s, t, r1=0.5, model_s=None, return_intermediate=False, solver_type='dpm_solver'):
        """Singlestep DPM-Solver-2 from s to t through s1 = inverse_lambda(lambda_s + r1 h) (dpm_solver.py:551-631)."""
        _check_solver_type(solver_type)
        r1 = F(0.5) if r1 is None else _scalar(r1, "r1")
        ns = self.tables
        s, t = _scalar(s, "s"), _scalar(t, "t")
        h = ns.lam(t) - ns.lam(s)
        s1, _ = self._inner_times(s, t, r1)
        sg = F(-1.0) if self.predict_x0 else F(1.0)          # the exponent's sign: expm1(-h) for data, expm1(h) for noise prediction
        phi_11, phi_1 = np.expm1(sg * r1 * h), np.expm1(sg * h)
        if model_s is None:
            model_s = self._model(x, s)
        cx1, m1 = self._sides(s, s1)
        x_s1 = E.lincomb([(cx1, x), (-m1 * phi_11, model_s)])
        model_s1 = self._model(x_s1, s1)
        cx, m = self._sides(s, t)
        A = m * phi_1
        if solver_type == 'dpm_solver':
            d = -(F(0.5) / r1) * A                                        # coefficient of (model_s1 - model_s)
        elif self.predict_x0:
            d = (F(1.0) / r1) * (m * ((np.exp(-h) - F(1.0)) / h + F(1.0)))
        else:
            d = -(F(1.0) / r1) * (m * ((np.exp(h) - F(1.0)) / h - F(1.0)))
        x_t = E.lincomb([(cx, x), (-A - d, model_s), (d, model_s1)])
        return (x_t, {'model_s': model_s, 'model_s1': model_s1}) if return_intermediate else x_t

    def singlestep_dpm_solver_third_update(self, x, s, t, r1=1. / 3., r2=2. / 3., model_s=None, model_s1=None,
                                           return_intermediate=False, solver_type='dpm_solver'):
        """Singlestep DPM-Solver-3 from s to t through s1, s2 (dpm_solver.py:633-753)."""
        _check_solver_type(solver_type)
        r1 = F(1. / 3.) if r1 is None else _scalar(r1, "r1")
        r2 = F(2. / 3.) if r2 is None else _scalar(r2, "r2")
        ns = self.tables
        s, t = _scalar(s, "s"), _scalar(t, "t")
        h = ns.lam(t) - ns.lam(s)
        s1, s2 = self._inner_times(s, t, r1, r2)
        sg = F(-1.0) if self.predict_x0 else F(1.0)
        phi_11, phi_12, phi_1 = np.expm1(sg * r1 * h), np.expm1(sg * r2 * h), np.expm1(sg * h)
        # data prediction: phi_22 = expm1(-r2 h) / (r2 h) + 1, phi_2 = phi_1 / h + 1; noise prediction: expm1(r2 h) / (r2 h) - 1, phi_1 / h - 1
        phi_22 = np.expm1(sg * r2 * h) / (r2 * h) - sg
        phi_2 = phi_1 / h - sg
        phi_3 = phi_2 / h - F(0.5)
        if model_s is None:
            model_s = self._model(x, s)
        if model_s1 is None:
            cx1, m1 = self._sides(s, s1)
            model_s1 = self._model(E.lincomb([(cx1, x), (-m1 * phi_11, model_s)]), s1)
        cx2, m2 = self._sides(s, s2)
        d2 = -sg * (r2 / r1) * (m2 * phi_22)                              # + for data, - for noise prediction (:690, :729)
        x_s2 = E.lincomb([(cx2, x), (-m2 * phi_12 - d2, model_s), (d2, model_s1)])
        model_s2 = self._model(x_s2, s2)
        cx, m = self._sides(s, t)
        A = m * phi_1
        if solver_type == 'dpm_solver':
            e = -sg * (F(1.0) / r2) * (m * phi_2)                         # coefficient of (model_s2 - model_s)  (:697, :736)
            x_t = E.lincomb([(cx, x), (-A - e, model_s), (e, model_s2)])
        else:
            # D1 = a1 d1 + a2 d2, D2 = b1 d1 + b2 d2 over d1 = model_s1 - model_s, d2 = model_s2 - model_s (:700-703);
            # x_t = cx x - A model_s + cP D1 - Q D2 with cP = +P (data) | -P (noise), P = m phi_2, Q = m phi_3 (:704-709, :743-748)
            den = r2 - r1
            a1, a2 = r2 / (r1 * den), -r1 / (r2 * den)
            b1, b2 = F(-2.0) / (r1 * den), F(2.0) / (r2 * den)
            cP, Q = -sg * (m * phi_2), m * phi_3
            e1, e2 = cP * a1 - Q * b1, cP * a2 - Q * b2
            x_t = E.lincomb([(cx, x), (-A - e1 - e2, model_s), (e1, model_s1), (e2, model_s2)])
        return (x_t, {'model_s': model_s, 'model_s1': model_s1, 'model_s2': model_s2}) if return_intermediate else x_t

    def multistep_dpm_solver_second_update(self, x, model_prev_list, t_prev_list, t, solver_type="dpm_solver"):
        """Multistep DPM-Solver-2 from t_prev_list[-1] to t (dpm_solver.py:755-810)."""
        _check_solver_type(solver_type)
        if len(model_prev_list) != 2 or len(t_prev_list) != 2:
            raise ValueError(f"multistep_dpm_solver_second_update takes a history of two model values, got {len(model_prev_list)}.  "
                             + _ORDER3_FINAL)
        ns = self.tables
        m1, m0 = model_prev_list
        t1, t0, t = _scalar(t_prev_list[0], "t_prev_list[0]"), _scalar(t_prev_list[1], "t_prev_list[1]"), _scalar(t, "t")
        l1, l0, lt = ns.lam(t1), ns.lam(t0), ns.lam(t)
        h0, h = l0 - l1, lt - l0
        r0 = h0 / h
        if self.predict_x0:
            k = ns.alpha(t) * (np.exp(-h) - np.float32(1.0))
            if solver_type == 'dpm_solver':      # x_t = sig_t/sig_0 x - k m0 - 0.5 k (m0 - m1)/r0: the update of DPM-Solver++(2M)
                return E.lincomb([(ns.sigma(t) / ns.sigma(t0), x), (-k - 0.5 * k / r0, m0), (0.5 * k / r0, m1)])
            d = ns.alpha(t) * ((np.exp(-h) - F(1.0)) / h + F(1.0)) / r0
            return E.lincomb([(ns.sigma(t) / ns.sigma(t0), x), (-k + d, m0), (-d, m1)])
        cx = np.exp(ns.log_alpha(t) - ns.log_alpha(t0))
        k = ns.sigma(t) * (np.exp(h) - F(1.0))
        if solver_type == 'dpm_solver':
            d = -F(0.5) * k / r0
        else:
            d = -ns.sigma(t) * ((np.exp(h) - F(1.0)) / h - F(1.0)) / r0
        return E.lincomb([(cx, x), (-k + d, m0), (-d, m1)])

    def multistep_dpm_solver_third_update(self, x, model_prev_list, t_prev_list, t, solver_type='dpm_solver'):
        """Multistep DPM-Solver-3 from t_prev_list[-1] to t (dpm_solver.py:812-857); like the reference, one expansion only."""
        ns = self.tables
        m2, m1, m0 = model_prev_list
        t2, t1, t0 = (_scalar(v, "t_prev_list") for v in t_prev_list)
        t = _scalar(t, "t")
        l2, l1, l0, lt = ns.lam(t2), ns.lam(t1), ns.lam(t0), ns.lam(t)
        h1, h0, h = l1 - l2, l0 - l1, lt - l0
        r0, r1 = h0 / h, h1 / h
        if self.predict_x0:
            cx = ns.sigma(t) / ns.sigma(t0)
            k = ns.alpha(t) * (np.exp(-h) - F(1.0))
            cP = ns.alpha(t) * ((np.exp(-h) - F(1.0)) / h + F(1.0))
            cQ = -ns.alpha(t) * ((np.exp(-h) - F(1.0) + h) / h ** 2 - F(0.5))
        else:
            cx = np.exp(ns.log_alpha(t) - ns.log_alpha(t0))
            k = ns.sigma(t) * (np.exp(h) - F(1.0))
            cP = -ns.sigma(t) * ((np.exp(h) - F(1.0)) / h - F(1.0))
            cQ = -ns.sigma(t) * ((np.exp(h) - F(1.0) - h) / h ** 2 - F(0.5))
        # D1 = (1 + g) D1_0 - g D1_1, D2 = q (D1_0 - D1_1) with D1_0 = (m0 - m1) / r0, D1_1 = (m1 - m2) / r1 (:839-842)
        g, q = r0 / (r0 + r1), F(1.0) / (r0 + r1)
        u, w = cP * (F(1.0) + g) + cQ * q, -cP * g - cQ * q
        return E.lincomb([(cx, x), (-k + u / r0, m0), (-u / r0 + w / r1, m1), (-w / r1, m2)])

    def singlestep_dpm_solver_update(self, x, s, t, order, return_intermediate=False, solver_type='dpm_solver', r1=None, r2=None):
        if order == 1:
            return self.dpm_solver_first_update(x, s, t, return_intermediate=return_intermediate)
        elif order == 2:
            return self.singlestep_dpm_solver_second_update(x, s, t, return_intermediate=return_intermediate, solver_type=solver_type, r1=r1)
        elif order == 3:
            return self.singlestep_dpm_solver_third_update(x, s, t, return_intermediate=return_intermediate, solver_type=solver_type,
                                                           r1=r1, r2=r2)
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))

    def multistep_dpm_solver_update(self, x, model_prev_list, t_prev_list, t, order, solver_type='dpm_solver'):
        if order == 1:
            return self.dpm_solver_first_update(x, t_prev_list[-1], t, model_s=model_prev_list[-1])
        elif order == 2:
            return self.multistep_dpm_solver_second_update(x, model_prev_list, t_prev_list, t, solver_type=solver_type)
        elif order == 3:
            return self.multistep_dpm_solver_third_update(x, model_prev_list, t_prev_list, t, solver_type=solver_type)
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))

    # ------------------------------------------------------------------ the adaptive solver
    def dpm_solver_adaptive(self, x, order, t_T, t_0, h_init=0.05, atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, solver_type='dpm_solver'):
        """DPM-Solver-12 / -23 (dpm_solver.py:909-963).  The step size lives on the host; every attempted step ends with one
        df_dpm_adaptive_error and ONE float read from the device.  self.adaptive_trace keeps (t, E, accepted) per attempt."""
        ns = self.tables
        if order == 2:
            r1 = 0.5
            lower_update = lambda x, s, t: self.dpm_solver_first_update(x, s, t, return_intermediate=True)
            higher_update = lambda x, s, t, **kw: self.singlestep_dpm_solver_second_update(x, s, t, r1=r1, solver_type=solver_type, **kw)
        elif order == 3:
            r1, r2 = 1. / 3., 2. / 3.
            lower_update = lambda x, s, t: self.singlestep_dpm_solver_second_update(x, s, t, r1=r1, return_intermediate=True,
                                                                                  solver_type=solver_type)
            higher_update = lambda x, s, t, **kw: self.singlestep_dpm_solver_third_update(x, s, t, r1=r1, r2=r2,
                                                                                        solver_type=solver_type, **kw)
        else:
            raise ValueError("For adaptive step size solver, order must be 2 or 3, got {}".format(order))
        x = E._dev_f32(x, x.device)
        s, t_0 = F(t_T), F(t_0)
        lambda_s, lambda_0 = ns.lam(s), ns.lam(t_0)
        h = F(h_init)
        x_prev = x
        nfe = 0
        self.adaptive_trace = trace = []
        while abs(s - t_0) > F(t_err):
            t = ns.inverse_lambda(lambda_s + h)
            x_lower, lower_noise_kwargs = lower_update(x, s, t)
            x_higher = higher_update(x, s, t, **lower_noise_kwargs)
            err = F(E.dpm_adaptive_error(x_higher, x_lower, x_prev, atol, rtol)[0].item())      # the one read of this step
            if err != err:
                raise FloatingPointError(f"dpm_solver_adaptive: the error estimate is NaN at t = {float(t):.6g} (step {len(trace)})")
            accepted = bool(err <= 1.)
            trace.append((float(t), float(err), accepted))
            if accepted:
                x = x_higher
                s = t
                x_prev = x_lower
                lambda_s = ns.lam(s)
            with np.errstate(divide="ignore"):
                grow = F(np.float64(err) ** (-1. / order))                # torch.float_power(...).float()
            h = min(F(theta) * h * grow, lambda_0 - lambda_s)
            nfe += order
        print('adaptive solver nfe', nfe)
        return x

    # ------------------------------------------------------------------ sample
    def _singlestep_plan(self, steps, order, skip_type, t_T, t_0, fixed):
        """[(s, t, order, r1, r2)] of method 'singlestep' / 'singlestep_fixed' (dpm_solver.py:1106-1121), all host scalars."""
        ns = self.tables
        if fixed:
            K = steps // order
            orders = [order, ] * K
            outer = self._time_steps(skip_type, t_T, t_0, K)
        else:
            outer, orders = self._orders_and_timesteps(steps, order, skip_type, t_T, t_0)
        plan = []
        for i, o in enumerate(orders):
            s, t = outer[i], outer[i + 1]
            inner = self._time_steps(skip_type, float(s), float(t), o)
            lam = [ns.lam(v) for v in inner]
            h = lam[-1] - lam[0]
            r1 = None if o <= 1 else (lam[1] - lam[0]) / h
            r2 = None if o <= 2 else (lam[2] - lam[0]) / h
            plan.append((s, t, o, r1, r2))
        return plan

    def _open(self, x, times):
        """The evaluation session of one sample(): on the fast route, _Guided with the time embedding of ``times`` hoisted."""
        if self.fast:
            self._session = _FastSession(self.model, tuple(x.shape), times)

    def sample(self, x, steps=20, t_start=None, t_end=None, order=3, skip_type='time_uniform', method='singlestep',
               lower_order_final=True, denoise_to_zero=False, solver_type='dpm_solver', atol=0.0078, rtol=0.05):
        """The sample at t_end from ``x`` at t_start (dpm_solver.py:965-1124); see the module docstring for the two deviations."""
        t_0 = 1. / self.noise_schedule.total_N if t_end is None else t_end
        t_T = self.noise_schedule.T if t_start is None else t_start
        if self.fast:
            with self.model.fast_model._lock, torch.no_grad():
                self.model.fast_model._require()
                return self._sample(E._dev_f32(x, self.model.fast_model.device), steps, t_0, t_T, order, skip_type, method,
                                    lower_order_final, denoise_to_zero, solver_type, atol, rtol)
        with torch.no_grad():
            return self._sample(E._dev_f32(x, x.device), steps, t_0, t_T, order, skip_type, method, lower_order_final,
                                denoise_to_zero, solver_type, atol, rtol)

    def _sample(self, x, steps, t_0, t_T, order, skip_type, method, lower_order_final, denoise_to_zero, solver_type, atol, rtol):
        tail = [F(t_0)] if denoise_to_zero else []
        try:
            if method == 'adaptive':
                self._open(x, None)
                x = self.dpm_solver_adaptive(x, order=order, t_T=t_T, t_0=t_0, atol=atol, rtol=rtol, solver_type=solver_type)
            elif method == 'multistep':
                assert steps >= order
                if order == 3 and lower_order_final and 4 <= steps < 15:
                    raise ValueError(_ORDER3_FINAL)
                ts = self._time_steps(skip_type, t_T, t_0, steps)
                assert ts.shape[0] - 1 == steps
                self._open(x, list(ts[:steps]) + tail)
                model_prev_list = [self._model(x, ts[0])]
                t_prev_list = [ts[0]]
                for init_order in range(1, order):      # the first `order` values by lower-order multistep updates
                    x = self.multistep_dpm_solver_update(x, model_prev_list, t_prev_list, ts[init_order], init_order, solver_type=solver_type)
                    model_prev_list.append(self._model(x, ts[init_order]))
                    t_prev_list.append(ts[init_order])
                for step in range(order, steps + 1):
                    step_order = min(order, steps + 1 - step) if lower_order_final and steps < 15 else order
                    x = self.multistep_dpm_solver_update(x, model_prev_list, t_prev_list, ts[step], step_order, solver_type=solver_type)
                    for i in range(order - 1):
                        t_prev_list[i] = t_prev_list[i + 1]
                        model_prev_list[i] = model_prev_list[i + 1]
                    t_prev_list[-1] = ts[step]
                    if step < steps:                    # the final model value is not needed
                        model_prev_list[-1] = self._model(x, ts[step])
            elif method in ['singlestep', 'singlestep_fixed']:
                plan = self._singlestep_plan(steps, order, skip_type, t_T, t_0, fixed=method == 'singlestep_fixed')
                times = []
                for s, t, o, r1, r2 in plan:
                    times += [v for v in (s,) + self._inner_times(s, t, r1, r2) if v is not None]
                self._open(x, times + tail)
                for s, t, o, r1, r2 in plan:
                    x = self.singlestep_dpm_solver_update(x, s, t, o, solver_type=solver_type, r1=r1, r2=r2)
            else:
                raise ValueError("Unsupported method {}, need to be 'singlestep' or 'singlestep_fixed' or 'multistep' or 'adaptive'".format(method))
            if denoise_to_zero:
                if self._session is None:
                    self._open(x, tail)
                x = self._data(x, F(t_0))
            return x
        finally:
            self._session = None


class DPMSolverSampler(object):
    """dpm_solver/sampler.py:11-156: DPM-Solver++(2M) behind the samplers' call surface -- the model's DPM_Solver (fast route) with
    multistep, order 2, time_uniform, predict_x0 and lower_order_final, which acts only if S < 15."""

    def __init__(self, model, **kwargs):
        self.model = model

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, classifier=None, origin_cond=None, classifier_guide_scale=0.0, **kwargs):
        # the reference's parameters in the reference's order (sampler.py:25-48), then the three of sample_with_classifier.  The
        # reference ignores eta / temperature / noise_dropout, the callbacks and log_every_t here (sampler.py:24-56 passes none of
        # them to DPM_Solver): same
        samplers.reject_unsupported("DPMSolverSampler", dict(kwargs, quantize_x0=quantize_x0, mask=mask, x0=x0, score_corrector=score_corrector),
                                    dict(mask=None, x0=None, score_corrector=None))   # sampler.py:24-56 accepts and drops them
        samplers._warn_batch(conditioning, batch_size)
        x, _ = samplers._start(self.model, batch_size, shape, x_T)
        solver = self.model.dpm_solver(conditioning, unconditional_guidance_scale, unconditional_conditioning, classifier, origin_cond,
                                       classifier_guide_scale)
        return solver.sample(x, steps=S, order=2, skip_type="time_uniform", method="multistep", lower_order_final=True), None

    sample_with_classifier = samplers.sample_with_classifier


# The class lived in samplers.py before it became a client of DPM_Solver; that spelling keeps resolving for callers written against
# it.  Set from here, the one direction the dependency runs: samplers.py knows nothing of this module.
samplers.DPMSolverSampler = DPMSolverSampler
