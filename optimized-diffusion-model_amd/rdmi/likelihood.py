"""Likelihood (bits/dim) of a score model by the probability-flow ODE with a Hutchinson divergence estimate.

API counterpart of the `likelihood.py` that score-SDE code bases ship (the reference keeps its `RVESDE.prior_logp` half,
RD/sde_lib.py): integrate d[x ; logp]/dt = [drift(x, t) ; div_x drift(x, t)] from eps to sde.T with scipy's solve_ivp, the
divergence estimated as eps^T (d drift / dx) eps with ONE probe eps per call.  A right-hand side is one forward plus one
vector-Jacobian product: for the native NCSNpp + RVESDE that is NCSNpp.native_vjp (train-mode forward with p = 0 and the VJP-only
backward: no weight gradient is computed) followed by one fused kernel for drift and divergence (rdmi_pf_drift_div).  Host-driven,
like the generic route of sampling.get_ode_sampler.
"""
import numpy as np
import torch

from .models import utils as mutils
from . import _native


def get_likelihood_fn(sde, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45', eps=1e-5, offset=0.0, t_span=None):
    """-> likelihood_fn(model, data, class_labels=None, noise=None) -> (bpd [B], z [B,C,H,W], nfev).

    bpd = -(sde.prior_logp(z).sum + delta_logp) / (D ln 2) + offset, D = C*H*W.  offset: 8 for 8-bit images scaled to [0,1]
    (the density is then per 1/256 bin), 0 reports the bits/dim of the continuous density on the unit cube.
    hutchinson_type: 'Rademacher' or 'Gaussian' probe, drawn once per call from the torch generator; `noise` (like data)
    replaces the draw.  class_labels gives the conditional score (no guidance weight).  t_span=(t0, t1) overrides the interval
    (eps, sde.T): a test hook, like first_step / max_steps of get_ode_sampler.
    No mollifier: the ODE sampler's `bump` factor is not applied here (its derivative would have to enter the divergence), so the
    flow is the plain probability-flow ODE of the reflected SDE.
    Native NCSNpp with RVESDE: native_vjp + rdmi_pf_drift_div.  Any other model or SDE: torch.autograd.grad through whatever the
    model provides."""
    from scipy import integrate
    if hutchinson_type not in ('Rademacher', 'Gaussian'):
        raise NotImplementedError(f'Hutchinson type {hutchinson_type} unknown.')

    def likelihood_fn(model, data, class_labels=None, noise=None):
        shape, B, dev = tuple(data.shape), data.shape[0], data.device
        D = int(np.prod(shape[1:]))
        if noise is not None:
            probe = noise.to(dev).float().contiguous()
        elif hutchinson_type == 'Gaussian':
            probe = torch.randn(shape).to(dev)
        else:
            probe = (torch.randint(0, 2, shape).float() * 2 - 1.).to(dev)
        native, inner = mutils._is_native(model)
        fast = native and hasattr(sde, 'sigma_min')
        if fast:
            model.eval()

        def rhs_native(x, t):
            vec_t = torch.full((B,), float(t), device=dev, dtype=torch.float32)
            sigma = torch.full((B,), float(sde.sigma_min * (sde.sigma_max / sde.sigma_min) ** float(t)), device=dev, dtype=torch.float32)
            score, gx = inner.native_vjp(x, sigma, class_labels, probe)
            return _native.pf_drift_div(score, gx, probe, vec_t, sde.sigma_min, sde.sigma_max)

        def rhs_generic(x, t):
            score_fn = mutils.get_score_fn(sde, model, train=False)
            vec_t = torch.ones(B, device=dev) * t
            with torch.enable_grad():
                x = x.detach().requires_grad_(True)
                rsde = sde.reverse(lambda xx, tt: score_fn(xx, tt, class_labels) if class_labels is not None else score_fn(xx, tt),
                                   probability_flow=True)
                drift = rsde.sde(x, vec_t)[0]
                gx = torch.autograd.grad(torch.sum(drift * probe), x)[0]
            return drift.detach(), torch.sum(gx * probe, dim=tuple(range(1, len(shape))))

        rhs = rhs_native if fast else rhs_generic

        def ode_func(t, y):
            x = mutils.from_flattened_numpy(y[:-B], shape).to(dev).type(torch.float32)
            drift, div = rhs(x, t)
            return np.concatenate([mutils.to_flattened_numpy(drift).astype(np.float64), mutils.to_flattened_numpy(div).astype(np.float64)])

        t0, t1 = (eps, sde.T) if t_span is None else t_span
        init = np.concatenate([mutils.to_flattened_numpy(data).astype(np.float64), np.zeros(B)])
        sol = integrate.solve_ivp(ode_func, (t0, t1), init, rtol=rtol, atol=atol, method=method)
        zp = sol.y[:, -1]
        z = mutils.from_flattened_numpy(zp[:-B], shape).to(dev).type(torch.float32)
        delta_logp = torch.from_numpy(zp[-B:]).to(dev).type(torch.float32)
        prior_logp = sde.prior_logp(z).reshape(B, -1).sum(dim=1)
        bpd = -(prior_logp + delta_logp) / np.log(2) / D + offset
        return bpd, z, sol.nfev

    return likelihood_fn
