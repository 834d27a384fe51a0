"""Training on the TILED plan (csrc/tiled_train.h, csrc/tiled_bwd_kernels.h) on the CPU emulator: the real HIP kernels of the fp32
backward against torch.autograd through the torch oracle, on a small RGB model that the planner tiles like the CIFAR-shape model."""

import numpy as np
import pytest
import torch

ARCH = dict(ch_mult=(1, 2, 2), nrb=1, attn_levels=(False, True, False), scale_by_sigma=True)


def _small_rgb_model(ge):
    """16x16 RGB NCSN++: nf 64, ch_mult [1, 2, 2], one res block per level, attention at 8x8 (C = 128), scale_by_sigma."""
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


def _inputs(B=2, seed=21):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, 16, 16, generator=g)
    sigma = torch.tensor([0.7, 3.0, 12.0, 0.05][:B])
    lab = torch.zeros(B, 1)
    gout = torch.randn(B, 3, 16, 16, generator=g)
    return x, sigma, lab, gout


def _oracle_grads(params, x, sigma, lab, gout, names):
    from oracle import rd_oracle_torch as OT
    p64 = {k: torch.from_numpy(v.copy()).double().requires_grad_(True) for k, v in params.items()}
    out = OT.ncsnpp_forward(p64, x.double(), sigma.double(), lab.double(), **ARCH)
    gr = torch.autograd.grad(out, [p64[n] for n in names], gout.double())
    return {n: g.numpy() for n, g in zip(names, gr)}


def _hip_grads(model, x, sigma, lab, gout):
    model.train()
    model.dropout, model.cond_drop_prob = 0.0, 0.0
    model.zero_grad(set_to_none=True)
    out = model(x, sigma, lab)
    out.backward(gout)
    return {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters() if p.requires_grad}


def _check(hip, ref):
    floor = 1e-6 * max(np.linalg.norm(r) for r in ref.values())
    assert len(hip) == len(ref) and len(hip) > 60
    for n, r in ref.items():
        d = np.linalg.norm(hip[n].astype(np.float64) - r)
        if n.endswith('NIN_1.b'):              # key bias: analytically zero (softmax shift invariance)
            assert d <= floor, (n, d)
        else:
            assert d <= 1e-4 * np.linalg.norm(r), (n, d / np.linalg.norm(r))


@pytest.mark.parametrize('wide', [False, True])
def test_tiled_backward_matches_oracle(emu, wide, monkeypatch):
    """Every parameter gradient of the tiled fp32 backward (dropout off, fixed upstream gradient) against float64 autograd:
    ||g_hip - g_ref|| <= 1e-4 ||g_ref||.  wide: RDMI_TILED_MIN_WGS=1, the forward's widened workgroups (NCT column tiles)."""
    import __graft_entry__ as ge
    if wide:
        monkeypatch.setenv('RDMI_TILED_MIN_WGS', '1')
    model, _, params = _small_rgb_model(ge)
    x, sigma, lab, gout = _inputs()
    hip = _hip_grads(model, x, sigma, lab, gout)
    info = model._ctx[('train', 'cpu', 16, 16)].path_info()
    assert info.startswith('tiled'), info
    _check(hip, _oracle_grads(params, x, sigma, lab, gout, list(hip)))


def test_tiled_train_bf16_not_built(emu):
    import __graft_entry__ as ge
    model, _, _ = _small_rgb_model(ge)
    model.train_dtype = 'bf16'
    model.train()
    x, sigma, lab, _ = _inputs()
    with pytest.raises(NotImplementedError, match='tiled'):
        model(x, sigma, lab)


def test_tiled_step_fn_matches_oracle(emu):
    """One losses.get_step_fn(train=True) step with optimization_manager (clip + Adam + EMA through rdmi_opt_step, warm-up off):
    the loss equals the float64 oracle loss (perturb -> score -> score_hk target, RD/losses.py:68-93), and the parameters and EMA
    after the step match torch Adam + clip_grad_norm_ on the oracle gradients."""
    import __graft_entry__ as ge
    from oracle import rd_oracle as OR
    from oracle import rd_oracle_torch as OT
    from rdmi import losses, sde_lib
    from rdmi.models.ema import ExponentialMovingAverage
    model, cfg, params = _small_rgb_model(ge)
    model.train()
    model.dropout, model.cond_drop_prob = 0.0, 0.0
    cfg.optim.warmup = 0
    sde = sde_lib.RVESDE(0.01, 50, N=1000)
    optimizer = losses.get_optimizer(cfg, model.parameters())
    ema = ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    state = dict(optimizer=optimizer, model=model, ema=ema, step=0, scaler=None)
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=False, likelihood_weighting=False)
    g = torch.Generator().manual_seed(5)
    batch = torch.rand(2, 3, 16, 16, generator=g); labels = torch.zeros(2, 1)
    t = torch.tensor([0.3, 0.8]); z = torch.randn(2, 3, 16, 16, generator=g)
    _r, _n = torch.rand, torch.randn_like
    try:
        torch.rand = lambda *a, **kw: ((t - 1e-5) / (1 - 1e-5)).clone()
        torch.randn_like = lambda x, **kw: z.clone()
        loss = float(step_fn(state, batch, class_labels=labels).detach())
    finally:
        torch.rand, torch.randn_like = _r, _n
    # float64 oracle of the same step
    names = [n for n, p in model.named_parameters()]
    p64 = {k: torch.from_numpy(v.copy()).double().requires_grad_(k != 'time_embed.W') for k, v in params.items()}
    std = OT.sigma_of(t.double(), 0.01, 50.0)
    pert = OT.reflect(batch.double() + std[:, None, None, None] * z.double())
    target = torch.from_numpy(np.asarray(OR.score_hk(pert.float().numpy(), batch.numpy(), std.float().numpy()))).double()
    score = OT.ncsnpp_forward(p64, pert, std, labels.double(), **ARCH)
    ref_loss = (0.5 * ((std ** 2)[:, None, None, None] * (score - target) ** 2).reshape(2, -1).sum(-1)).mean()
    ref_l = float(ref_loss.detach())
    assert abs(loss - ref_l) <= 1e-4 * abs(ref_l), (loss, ref_l)
    ref_loss.backward()
    train = [p64[n] for n in names if p64[n].requires_grad]
    torch.nn.utils.clip_grad_norm_(train, max_norm=cfg.optim.grad_clip)
    opt = torch.optim.Adam(train, lr=cfg.optim.lr, betas=(cfg.optim.beta1, 0.999), eps=cfg.optim.eps)
    opt.step()
    decay = min(cfg.model.ema_rate, 2.0 / 11.0)
    shadow = dict(zip([n for n in names if p64[n].requires_grad], ema.shadow_params))
    for n in names:
        mine = dict(model.named_parameters())[n].detach().double()
        ref = p64[n].detach()
        start = torch.from_numpy(params[n].copy()).double()
        moved = (ref - start).norm()
        if n.endswith('NIN_1.b'):              # key bias: zero gradient up to rounding, so Adam's g / (|g| + eps) is not pinned
            assert float((mine - start).abs().max()) <= 1.01 * cfg.optim.lr, n
            continue
        # one Adam step moves each element by ~lr * g / (|g| + eps): after clipping, elements whose gradient is near eps = 1e-8 carry
        # the gradient's rounding difference almost undamped, hence 1 % of the step rather than the gradient tolerance
        assert float((mine - ref).norm()) <= 1e-2 * float(moved) + 1e-7 * float(ref.norm()), n
        ref_ema = decay * start + (1 - decay) * ref
        if n not in shadow:                    # time_embed.W: not trained, no shadow
            continue
        assert float((shadow[n].double() - ref_ema).norm()) <= 1e-6 * float(ref_ema.norm()) + 1e-2 * float(moved), n
