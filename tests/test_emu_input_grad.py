"""Input gradients (rdmi_backward_input), the VJP-only backward, rdmi_pf_drift_div and rdmi.likelihood on the CPU emulator: the real HIP
kernels against float64 autograd through the torch oracle (oracle/rd_oracle_torch.ncsnpp_forward with x.requires_grad_()).

The helpers take a device, so tests/test_gpu_input_grad.py runs the same checks on an MI355X."""
import functools
import math
import os

import numpy as np
import pytest
import torch

RGB_ARCH = dict(ch_mult=(1, 2, 2), nrb=1, attn_levels=(False, True, False), scale_by_sigma=True)
GTO_ARCH = {}
CASES = ('layer_f32', 'layer_bf16', 'tiled', 'tiled_wide')
# ||g - g64|| <= BOUND ||g64||: the project's rule for fp32 gradients; the stated bf16 gradient tolerance (check_bf16_train: 4 % of the norm)
BOUND = {'layer_f32': 1e-4, 'layer_bf16': 4e-2, 'tiled': 1e-4, 'tiled_wide': 1e-4}


def small_rgb_model(ge):
    """The 16x16 RGB tiled model of tests/test_emu_tiled_train.py::_small_rgb_model."""
    from oracle.weights import make_params
    from rdmi.models import utils as mutils
    cfg = ge.demo_config(image_size=16, image_width=16)
    m = cfg.model
    m.nf, m.ch_mult, m.num_res_blocks, m.attn_resolutions = 64, [1, 2, 2], 1, [8]
    m.channels, m.scale_by_sigma, m.compute_dtype = 3, True, 'f32'
    cfg.sde.sigma_max = 50
    params = make_params(3, nf=64, ch_mult=(1, 2, 2), num_res_blocks=1, attn_resolutions=(8,), image_size=16, channels=3)
    model = mutils.create_model(cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    return model, cfg, params


def make_case(case, dev, B=None):
    """-> (model, params, arch, (x, sigma, lab, gout) on `dev`, (sigma_min, sigma_max))."""
    import __graft_entry__ as ge
    if case in ('S1', 'S2', 'S3', 'S4'):            # the shape matrix of tests/tiled_shapes.py
        from tests import tiled_shapes
        model, params, arch, args, sig = tiled_shapes.grad_case(case, dev)
        model.eval()
        return model, params, arch, args, sig
    if case.startswith('layer'):
        model, _, params = ge.make_model(dev)
        if case == 'layer_bf16':
            model.train_dtype = 'bf16'
        B = B or 3
        g = torch.Generator().manual_seed(11)
        x = torch.rand(B, 1, 9, 9, generator=g)
        sigma = torch.tensor([0.05, 0.9, 4.0, 0.3][:B])
        lab = torch.rand(B, 1, generator=g)
        gout = torch.randn(B, 1, 9, 9, generator=g)
        arch, sig = GTO_ARCH, (0.01, 5.0)
    else:
        model, _, params = small_rgb_model(ge)
        model = model.to(dev)
        B = B or 2
        g = torch.Generator().manual_seed(21)
        x = torch.rand(B, 3, 16, 16, generator=g)
        sigma = torch.tensor([0.7, 3.0, 12.0, 0.05][:B])
        lab = torch.zeros(B, 1)
        gout = torch.randn(B, 3, 16, 16, generator=g)
        arch, sig = RGB_ARCH, (0.01, 50.0)
    model.eval()
    return model, params, arch, tuple(t.to(dev) for t in (x, sigma, lab, gout)), sig


def oracle_input_grad(params, arch, x, sigma, lab, gout, dtype=torch.float64):
    from oracle import rd_oracle_torch as OT
    p = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in params.items()}
    xr = x.detach().cpu().to(dtype).requires_grad_()
    out = OT.ncsnpp_forward(p, xr, sigma.cpu().to(dtype), lab.cpu().to(dtype), **arch)
    return torch.autograd.grad(out, xr, gout.cpu().to(dtype))[0].double()


def _with_env(case):
    return {'RDMI_TILED_MIN_WGS': '1'} if case == 'tiled_wide' else {}


def run_modes(case, dev, B=None, rounds=1):
    """Train-mode forward (p = 0), then `rounds` x (rdmi_backward, rdmi_backward_input(grads, grad_x), VJP-only) interleaved.
    -> dict(plain, full, gx_full, gx_vjp: lists of tensors per round; stats; info; ref inputs)."""
    env = _with_env(case)
    os.environ.update(env)
    try:
        model, params, arch, (x, sigma, lab, gout), sig = make_case(case, dev, B)
        tctx = model.train_context(x.shape[0], x.shape[2], x.shape[3], x.device)
        out = torch.empty_like(x)
        total = sum(p.numel() for p in model.parameters())
        res = dict(plain=[], full=[], gx_full=[], gx_vjp=[], fwd=[])
        for _ in range(rounds):
            # (a forward per round: the layer plan's recorded forward graph is exercised too; the backward re-reads the same activations)
            tctx.train_forward(x, sigma, lab, out, 0.0, 0)
            res['fwd'].append(out.clone())
            flat = torch.full((total,), float('nan'), device=x.device)
            tctx.backward(gout, flat, x)
            res['plain'].append(flat)
            flat2, gx = torch.full_like(flat, float('nan')), torch.full_like(x, float('nan'))
            tctx.backward(gout, flat2, x, grad_x=gx)
            res['full'].append(flat2); res['gx_full'].append(gx)
            gx2 = torch.full_like(x, float('nan'))
            tctx.backward(gout, None, x, grad_x=gx2)
            res['gx_vjp'].append(gx2)
        res['stats'] = tctx.train_graph_stats()
        res['info'] = tctx.path_info()
        res['names'] = [(n, p.numel()) for n, p in model.named_parameters()]
        res['args'] = (params, arch, x, sigma, lab, gout)
        return res
    finally:
        for k in env:
            os.environ.pop(k, None)


@functools.lru_cache(maxsize=None)
def _emu_modes(case):
    return run_modes(case, 'cpu', rounds=1)


@functools.lru_cache(maxsize=None)
def _ref64(case):
    params, arch, x, sigma, lab, gout = _emu_modes(case)['args']
    return oracle_input_grad(params, arch, x, sigma, lab, gout)


def rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def frame_mask(H, W):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def check_grad_x(g, ref, bound):
    """Whole tensor, every channel, and the one-pixel frame of the image alone, at the same relative bound: a wrong tap validity at
    a border or a swapped channel cannot hide in the norm."""
    g = g.double().cpu()
    assert bool(torch.isfinite(g).all())
    assert rel(g, ref) <= bound, rel(g, ref)
    for c in range(ref.shape[1]):
        assert rel(g[:, c], ref[:, c]) <= bound, (c, rel(g[:, c], ref[:, c]))
    fm = frame_mask(ref.shape[2], ref.shape[3])
    assert rel(g[:, :, fm], ref[:, :, fm]) <= bound, rel(g[:, :, fm], ref[:, :, fm])
    for c in range(ref.shape[1]):
        assert rel(g[:, c][:, fm], ref[:, c][:, fm]) <= bound, (c, 'frame')


# gradients behind embed_backward's `gta`: 17+ res blocks add their Dense_0 data gradients into it with fp32 atomics in whatever order
# the workgroups arrive, so these tensors are not run-to-run identical in rdmi_backward itself (two addends commute, three do not);
# for them the modes are compared at 1e-6 of the norm (reordering a sum of < 64 fp32 terms moves it by a few 6e-8 ulps).  Every other
# parameter gradient at B = 2 has at most two atomic addends per element (layer plan) or none (tiled plan): bit-identical.
UNORDERED = ('time_mlp.', 'label_emb.')


def check_mode_consistency(res, need_replays):
    names = res['names']
    for k in range(len(res['plain'])):
        assert torch.equal(res['gx_vjp'][k], res['gx_full'][0]) and torch.equal(res['gx_full'][k], res['gx_full'][0]), k
        assert torch.equal(res['fwd'][k], res['fwd'][0])
        off = 0
        for n, ne in names:
            a, b, c0 = res['full'][k][off:off + ne], res['plain'][k][off:off + ne], res['plain'][0][off:off + ne]
            off += ne
            if n.startswith(UNORDERED):
                assert float((a - b).norm()) <= 1e-6 * float(b.norm()) + 1e-30, n
                assert float((b - c0).norm()) <= 1e-6 * float(c0.norm()) + 1e-30, n
            else:
                assert torch.equal(a, b) and torch.equal(b, c0), (n, k)
        assert off == res['plain'][k].numel()
    assert bool(torch.isfinite(res['plain'][0]).all())
    rec, rep = res['stats']
    if need_replays:
        assert rec >= 4 and rep >= 4, (rec, rep)      # forward + the three backward modes: recorded on their second call, replayed on the third


@pytest.mark.parametrize('case', CASES)
def test_grad_x_matches_float64_autograd(emu, case):
    """grad_x of the full call and of the VJP-only call against float64 autograd through the oracle, whole / per channel / border frame."""
    res = _emu_modes(case)
    assert res['info'].startswith('tiled' if case.startswith('tiled') else 'layers'), res['info']
    ref = _ref64(case)
    check_grad_x(res['gx_full'][0], ref, BOUND[case])
    check_grad_x(res['gx_vjp'][0], ref, BOUND[case])
    if case == 'layer_bf16':                        # not a silent fp32 run
        assert rel(res['gx_vjp'][0], ref) > 1e-4


@pytest.mark.parametrize('case', ['layer_f32', 'layer_bf16', 'tiled'])
def test_modes_are_consistent(emu, case):
    """Three interleaved rounds of (rdmi_backward, rdmi_backward_input(grads, grad_x), VJP-only) at B = 2: grad_x bit-identical across
    modes and rounds, parameter gradients of the combined call bit-identical to rdmi_backward's (see UNORDERED for the embedding chain).
    The emulator does not capture graphs (hipStreamBeginCapture fails there and the plan falls back to plain launches), so the replay
    count is asserted on the GPU (tests/test_gpu_input_grad.py); here the statistics call must still answer."""
    res = run_modes(case, 'cpu', B=2, rounds=3)
    check_mode_consistency(res, need_replays=False)
    assert 'input-gradient backward calls: 6' in res['info'], res['info']


def test_backward_input_rejects_no_output(emu):
    model, _, _, (x, sigma, lab, gout), _ = make_case('layer_f32', 'cpu', 2)
    tctx = model.train_context(2, 9, 9, 'cpu')
    out = torch.empty_like(x)
    tctx.train_forward(x, sigma, lab, out, 0.0, 0)
    from rdmi import _native
    rc = _native.lib().rdmi_backward_input(tctx._h, gout.data_ptr(), None, 0, None, x.data_ptr(), None)
    assert rc != 0 and b'neither' in _native.lib().rdmi_last_error()


def autograd_surface(case, dev):
    model, _, _, (x, sigma, lab, gout), _ = make_case(case, dev, 2)
    H, W = x.shape[2], x.shape[3]
    key = ('train', str(torch.device(dev)), H, W)
    # (c) x without grad: today's call sequence, no input-gradient launch
    model.train()
    model.dropout, model.cond_drop_prob = 0.0, 0.0
    model.zero_grad(set_to_none=True)
    model(x, sigma, lab).backward(gout)
    assert 'input-gradient backward calls: 0' in model._ctx[key].path_info(), model._ctx[key].path_info()
    pg = {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}
    # (b) trainable parameters and a differentiable input: both kinds of gradient
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_()
    model(xr, sigma, lab).backward(gout)
    assert xr.grad is not None and xr.grad.shape == x.shape
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and p.grad.shape == p.shape, n
            if not n.startswith(UNORDERED):
                assert torch.equal(p.grad, pg[n]), n
    assert 'input-gradient backward calls: 1' in model._ctx[key].path_info()
    # (a) eval mode, frozen parameters: autograd.grad w.r.t. x is the VJP-only backward, the same tensor as native_vjp
    model.eval()
    req = [p.requires_grad for p in model.parameters()]
    for p in model.parameters():
        p.requires_grad_(False)
    try:
        xr2 = x.clone().requires_grad_()
        out = model(xr2, sigma, lab)
        assert out.requires_grad
        (gx,) = torch.autograd.grad(out, xr2, gout)
        out2, gx2 = model.native_vjp(x, sigma, lab, gout)
        assert torch.equal(gx, gx2) and torch.equal(out.detach(), out2)
        assert torch.equal(gx, xr.grad)
        with torch.no_grad():                      # the no-grad path is untouched: the plain eval forward
            assert not model(xr2, sigma, lab).requires_grad
    finally:
        for p, r in zip(model.parameters(), req):
            p.requires_grad_(r)
    return gx


@pytest.mark.parametrize('case', ['layer_f32', 'tiled'])
def test_autograd_surface(emu, case):
    gx = autograd_surface(case, 'cpu')
    _, params, arch, (x, sigma, lab, gout), _ = make_case(case, 'cpu', 2)
    check_grad_x(gx, oracle_input_grad(params, arch, x, sigma, lab, gout), BOUND[case])


def pf_drift_div_check(dev, E):
    from rdmi import _native
    B, smin, smax = 3, 0.01, 50.0
    g = torch.Generator().manual_seed(E)
    score, gx = torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)
    eps = (torch.randint(0, 2, (B, E), generator=g).float() * 2 - 1)
    t = torch.tensor([1e-5, 0.37, 1.0])
    drift, div = _native.pf_drift_div(score.to(dev), gx.to(dev), eps.to(dev), t.to(dev), smin, smax)
    t64 = t.double().numpy()
    g2 = (smin * (smax / smin) ** t64) ** 2 * (2 * math.log(smax / smin))
    rd = -0.5 * g2[:, None] * score.double().numpy()
    rv = -0.5 * g2 * (gx.double().numpy() * eps.double().numpy()).sum(1)
    d, v = drift.cpu().double().numpy(), div.cpu().double().numpy()
    assert drift.shape == (B, E) and div.shape == (B,)
    assert np.all(np.abs(d - rd) <= 1e-6 * np.abs(rd)), float(np.max(np.abs(d - rd) / np.abs(rd)))
    assert np.all(np.abs(v - rv) <= 1e-5 * np.abs(rv)), (v, rv)
    drift2, div2 = _native.pf_drift_div(score.to(dev), gx.to(dev), eps.to(dev), t.to(dev), smin, smax)
    assert torch.equal(drift, drift2) and torch.equal(div, div2)


@pytest.mark.parametrize('E', [81, 3072])
def test_pf_drift_div(emu, E):
    """drift to 1e-6 and div to 1e-5 (relative, per element / per sample) of the float64 numpy formula; run-to-run identical."""
    pf_drift_div_check('cpu', E)


def oracle_likelihood(params, arch, data, lab, noise, t_span, sig, dtype):
    """The same solve_ivp call as rdmi.likelihood, driven by the torch oracle (score + autograd.grad VJP) in `dtype`."""
    from scipy import integrate
    from oracle import rd_oracle_torch as OT
    smin, smax = sig
    p = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in params.items()}
    shape, B = tuple(data.shape), data.shape[0]
    D = int(np.prod(shape[1:]))
    eps_, lab_ = noise.cpu().to(dtype), lab.cpu().to(dtype)

    def f(t, y):
        x = torch.from_numpy(y[:-B].reshape(shape)).to(dtype).requires_grad_()
        sigma = torch.full((B,), smin * (smax / smin) ** t, dtype=dtype)
        score = OT.ncsnpp_forward(p, x, sigma, lab_, **arch)
        gx = torch.autograd.grad((score * eps_).sum(), x)[0]
        c = -0.5 * sigma ** 2 * (2 * math.log(smax / smin))
        drift = c[:, None, None, None] * score.detach()
        div = c * (gx * eps_).reshape(B, -1).sum(1)
        return np.concatenate([drift.double().numpy().ravel(), div.double().numpy()])

    init = np.concatenate([data.cpu().double().numpy().ravel(), np.zeros(B)])
    sol = integrate.solve_ivp(f, t_span, init, rtol=1e-5, atol=1e-5, method='RK45')
    return -(sol.y[-B:, -1]) / math.log(2) / D, sol.nfev


LIK_SPAN = {'layer_f32': (0.3, 0.5), 'tiled': (0.4, 0.45)}


def likelihood_check(case, dev, span=None):
    from rdmi import likelihood, sde_lib
    model, params, arch, (x, _, lab, gout), sig = make_case(case, dev, 2)
    noise = torch.sign(gout) + (gout == 0).float()              # a fixed Rademacher probe
    span = span or LIK_SPAN[case]
    sde = sde_lib.RVESDE(sig[0], sig[1], N=1000)
    fn = likelihood.get_likelihood_fn(sde, t_span=span)
    bpd, z, nfev = fn(model, x, class_labels=lab, noise=noise)
    assert bpd.shape == (2,) and z.shape == x.shape and bool(torch.isfinite(z).all())
    b64, n64 = oracle_likelihood(params, arch, x, lab, noise, span, sig, torch.float64)
    b32, _ = oracle_likelihood(params, arch, x, lab, noise, span, sig, torch.float32)
    mine = bpd.cpu().double().numpy()
    print(f'likelihood {case} on {dev}: bpd {mine}, float64 oracle {b64}, |bpd - bpd64| {np.abs(mine - b64)}, '
          f'fp32 oracle |bpd32 - bpd64| {np.abs(b32 - b64)}, nfev {nfev} / {n64}')
    assert abs(nfev - n64) <= 12, (nfev, n64)
    allow = np.maximum(1e-4 * np.abs(b64), 8 * np.abs(b32 - b64))
    assert np.all(np.abs(mine - b64) <= allow), (mine, b64, b32)
    assert 'input-gradient backward calls: %d' % nfev in model._ctx[('train', str(torch.device(dev)), x.shape[2], x.shape[3])].path_info()


def test_likelihood_matches_oracle(emu):
    """bits/dim of likelihood_fn (9x9 model, B = 2, fixed Rademacher probe, default tolerances) against the same solve_ivp call driven by
    the float64 oracle: |bpd - bpd64| <= max(1e-4 |bpd64|, 8 |bpd32 - bpd64|) with bpd32 the oracle in fp32 on torch CPU; nfev within 12
    of the oracle's.  Through the native route (native_vjp + rdmi_pf_drift_div: one input-gradient backward per right-hand side).
    The spans t in (0.3, 0.5) for this model and (0.4, 0.45) for the RGB tiled model take 200 and 164 right-hand sides at the default
    tolerances -- measured on the MI355X, where tests/test_gpu_input_grad.py runs exactly those (|bpd - bpd64| = 9.6e-6 / 8.9e-6 with
    the fp32 oracle at 9.7e-5 / 2.7e-5 on the 9x9 model; 1.4e-7 / 5.7e-7 with the fp32 oracle at 3.1e-7 / 2.0e-7 on the RGB model; nfev
    equal to the oracle's).  The emulator needs about half a minute per right-hand side, so here the interval is cut to
    (0.3, 0.3002): one accepted step, 8 right-hand sides, same code path, same bound (measured here: |bpd - bpd64| = 1.0e-12 / 1.5e-12
    on bpd64 = 2.1e-6 / 3.7e-6, the fp32 oracle at 5.0e-13 / 2.8e-13, nfev 8 = the oracle's)."""
    likelihood_check('layer_f32', 'cpu', span=(0.3, 0.3002))


def test_likelihood_generic_route_and_probe_types(emu):
    """A model that is not the native NCSNpp takes the torch.autograd route.  For the linear score a(t) (x - 1/2), a = -1 / (1 + sigma^2),
    the Hutchinson estimate is exact for any probe with eps_i^2 = 1 (Rademacher): delta_logp = -0.5 D int g(t)^2 a(t) dt."""
    from rdmi import likelihood, sde_lib

    class Lin(torch.nn.Module):
        def forward(self, x, sigma, class_labels=None):
            return -(x - 0.5) / (1.0 + sigma[:, None, None, None] ** 2)

    sde = sde_lib.RVESDE(0.01, 5, N=1000)
    x = torch.rand(2, 1, 9, 9, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(0)
    bpd, z, nfev = likelihood.get_likelihood_fn(sde, t_span=(0.3, 0.5), offset=8.0)(Lin(), x)
    from scipy import integrate
    k = 2 * math.log(5 / 0.01)
    val, _ = integrate.quad(lambda t: 0.5 * k * (0.01 * 500 ** t) ** 2 / (1 + (0.01 * 500 ** t) ** 2), 0.3, 0.5)
    ref = -(81 * val) / math.log(2) / 81 + 8.0
    assert np.allclose(bpd.numpy(), ref, rtol=1e-4), (bpd, ref)
    with pytest.raises(NotImplementedError):
        likelihood.get_likelihood_fn(sde, hutchinson_type='Sobol')
    gz = likelihood.get_likelihood_fn(sde, hutchinson_type='Gaussian', t_span=(0.3, 0.31))(Lin(), x)
    assert bool(torch.isfinite(gz[0]).all())


def test_dropin_likelihood_reexport():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('dropin_likelihood', os.path.join(root, 'optimized-diffusion-model_amd', 'dropin', 'likelihood.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from rdmi import likelihood
    assert mod.get_likelihood_fn is likelihood.get_likelihood_fn
