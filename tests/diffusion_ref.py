"""TEST INFRASTRUCTURE ONLY (never imported by diff_foley_amd/).

Float64 restatement of the two kernels of csrc/diffusion.hip, from the reference's own lines:

    q_sample(x0, noise, t, A, S)[b] = A[t[b]] * x0[b] + S[t[b]] * noise[b]                   ddpm.py:279-282, ddim.py:412-413
    loss_simple[b]  = mean over the sample of (target - pred)^2 | |target - pred|           ddpm.py:284-297, 1061
    simple = mean(loss_simple)                                                               ddpm.py:1062
    gamma  = mean(loss_simple / exp(logvar[t]) + logvar[t])                                  ddpm.py:1066-1070
    vlb    = mean(lvlb_weights[t] * loss_simple)                                             ddpm.py:1075-1077
    loss   = l_simple_weight * gamma + original_elbo_weight * vlb                            ddpm.py:1073, 1078-1079
    logvar = mean(logvar)                                                                    ddpm.py:1071

The inputs are taken as they are (fp32 values widened exactly) and every operation runs in float64, so the distance of a kernel's
fp32 result to this restatement is the kernel's own rounding.  An index outside the table gives NaN for that sample (and the means),
which is what the kernels answer instead of reading out of bounds.  tests/test_diffusion_loss_cpu.py pins this file to the
reference's goldens (g17_q_sample.npz, g17_p_losses.npz) before any GPU test uses it."""
import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)


def _idx(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.int64).reshape(-1)


def q_sample_ref(x0, noise, t, A, S):
    """-> (out float64 of x0's shape, bound float64 of the same shape): the value and the per-element rounding bound of an fp32
    evaluation, 2 u (|A x0| + |S noise|) -- two rounded products and one rounded sum, or one product and one FMA."""
    x0, noise, A, S, t = _f64(x0), _f64(noise), _f64(A), _f64(S), _idx(t)
    out, bound = np.empty_like(x0), np.empty_like(x0)
    for b, tb in enumerate(t):
        if 0 <= tb < len(A):
            p, q = A[tb] * x0[b], S[tb] * noise[b]
            out[b], bound[b] = p + q, 2.0 * U * (np.abs(p) + np.abs(q))
        else:
            out[b], bound[b] = np.nan, np.nan
    return out, bound


def loss_simple_ref(pred, target, loss_type="l2"):
    d = _f64(target) - _f64(pred)
    d = d.reshape(d.shape[0], -1)
    return (d * d if loss_type == "l2" else np.abs(d)).mean(axis=1)


def loss_scalars_ref(loss_simple, t, logvar, lvlb_weights, l_simple_weight=1.0, original_elbo_weight=0.0):
    """-> dict(simple, gamma, vlb, loss, logvar) from per-sample losses (float64)."""
    ls, lv, w, t = _f64(loss_simple).reshape(-1).copy(), _f64(logvar), _f64(lvlb_weights), _idx(t)
    ok = (t >= 0) & (t < len(lv))
    tc = np.where(ok, t, 0)
    lvt, wt = np.where(ok, lv[tc], np.nan), np.where(ok, w[tc], np.nan)
    ls[~ok] = np.nan
    gamma, vlb = (ls / np.exp(lvt) + lvt).mean(), (wt * ls).mean()
    return dict(simple=ls.mean(), gamma=gamma, vlb=vlb, loss=l_simple_weight * gamma + original_elbo_weight * vlb, logvar=lv.mean())


def diffusion_loss_ref(pred, target, t, logvar, lvlb_weights, loss_type="l2", l_simple_weight=1.0, original_elbo_weight=0.0):
    """-> (loss_simple [B] float64 with NaN where t is out of range, dict of the five scalars)."""
    ls = loss_simple_ref(pred, target, loss_type)
    t = _idx(t)
    ls = np.where((t >= 0) & (t < len(_f64(logvar))), ls, np.nan)
    return ls, loss_scalars_ref(ls, t, logvar, lvlb_weights, l_simple_weight, original_elbo_weight)


def loss_dict_ref(scalars, learn_logvar=False, prefix="val"):
    """The reference's loss_dict (ddpm.py:1062-1079) from the five scalars."""
    d = {f"{prefix}/loss_simple": scalars["simple"]}
    if learn_logvar:
        d[f"{prefix}/loss_gamma"] = scalars["gamma"]
        d["logvar"] = scalars["logvar"]
    d[f"{prefix}/loss_vlb"] = scalars["vlb"]
    d[f"{prefix}/loss"] = scalars["loss"]
    return d
