"""The tiled plan on odd level grids and with attention over L % 16 != 0 positions: shared check functions, run on the CPU emulator by
tests/test_emu_tiled_odd_shapes.py and on an MI355X by tests/test_gpu_tiled_odd_shapes.py.  The reference is
oracle/rd_oracle_torch.ncsnpp_forward with float64 parameters and inputs, as in tests/tiled_shapes.py, whose tolerances and helpers are
imported (that module's make_model fixes 3 image channels: this one builds its own models).

All models are nf 32, ch_mult (1, 2, 2), one res block per level, scale_by_sigma, sigma_max 50, seeded synthetic weights:

O1  10x10, 1 channel, attention at 10x10 (L = 100, C = 32)
      levels 10 / 5 / 2: one nearest resize 4x4 -> 5x5 of h onto the skip grid; the stride-2 Downsample 5 -> 2 never touches its bottom /
      right pad; score rows padded to Lp = 112 (bf16: 128), the softmax and the V transpose write the zero pad; a single image channel
      on the tiled plan.
O2  11x11, 1 channel, attention at the 5x5 level (L = 25, C = 64)
      resizes at two levels (4 -> 5 and 10 -> 11), odd Downsamples 11 -> 5 and 5 -> 2; L = 25 is less than half a 64-tile of the batched
      GEMMs (row and column tails clamped and masked), Lp = 32; three-tile images (11 rows in tiles of 5, 5, 1).
O3  9x9, 3 channels, attention at 9x9 (L = 81)
      the GTO-Halo geometry with RGB input: levels 9 / 4 / 2, one resize 8 -> 9.
O4  10x14 (H x W), 3 channels, no attention
      H != W through the resize (4x6 -> 5x7): a swapped axis cannot cancel.
"""
import functools
import os

import torch

from tests import test_emu_input_grad as IG
from tests import test_emu_tiled_train as TT
from tests import tiled_shapes as S
from tests.tiled_shapes import GRAD_TOL, SMAX, SMIN, STATS_TOL, TAP_TOL, TOL, _p64, oracle_grads, rel_errs

NF, CH_MULT = 32, (1, 2, 2)
SHAPES = {
    'O1': dict(H=10, W=10, ch=1, attn=(10,), resizes=1),
    'O2': dict(H=11, W=11, ch=1, attn=(5,), resizes=2),
    'O3': dict(H=9, W=9, ch=3, attn=(9,), resizes=1),
    'O4': dict(H=10, W=14, ch=3, attn=(), resizes=1),
}


def level_sizes(H):
    """Grid height per level: the stride-2 Downsample with its bottom / right pad floors (10 -> 5 -> 2, 11 -> 5 -> 2, 9 -> 4 -> 2)."""
    return [H // 2 ** i for i in range(len(CH_MULT))]


def oracle_arch(name):
    s = SHAPES[name]
    return dict(ch_mult=CH_MULT, nrb=1, attn_levels=tuple(h in s['attn'] for h in level_sizes(s['H'])), scale_by_sigma=True)


def make_model(name, compute_dtype='f32'):
    """-> (model on the CPU in eval mode, cfg, params), built as tiled_shapes.make_model builds its models, with the shape's channel count."""
    import __graft_entry__ as ge
    from oracle.weights import make_params
    from rdmi.models import utils as mutils
    s = SHAPES[name]
    cfg = ge.demo_config(image_size=s['H'], image_width=s['W'])
    m = cfg.model
    m.nf, m.ch_mult, m.num_res_blocks, m.attn_resolutions = NF, list(CH_MULT), 1, list(s['attn'])
    m.channels, m.scale_by_sigma, m.compute_dtype = s['ch'], True, compute_dtype
    cfg.sde.sigma_max = SMAX
    params = make_params(3, nf=NF, ch_mult=CH_MULT, num_res_blocks=1, attn_resolutions=s['attn'], image_size=s['H'], channels=s['ch'])
    model = mutils.create_model(cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    return model.eval(), cfg, params


def check_path(info, name):
    """The context runs the tiled plan and made the expected number of resize launches."""
    assert info.startswith('tiled'), info
    assert f'resize launches (h onto an odd skip grid): {SHAPES[name]["resizes"]}' in info, info


def _ctx(model, dev, name, train=False):
    s = SHAPES[name]
    key = (str(torch.device(dev)), s['H'], s['W'])
    ctx = model._ctx[('train',) + key if train else key]
    check_path(ctx.path_info(), name)
    return ctx


# ---- forward: classifier-free-guidance score, B = 3, zero labels (tiled_shapes.cf_inputs) ---------------------------------------------
def cf_inputs(name):
    s = SHAPES[name]
    g = torch.Generator().manual_seed(31)
    x = torch.rand(3, s['ch'], s['H'], s['W'], generator=g)
    return x, torch.zeros(3, 1), torch.tensor([0.0, 0.6, 1.5]), torch.tensor([0.15, 0.5, 0.85])


@functools.lru_cache(maxsize=None)
def cf_ref64(name):
    from oracle import rd_oracle_torch as OT
    _, _, params = make_model(name)
    x, lab, w, t = cf_inputs(name)
    with torch.no_grad():
        return OT.cf_score(_p64(params), x.double(), t.double(), lab.double(), w.double(), smax=SMAX, **oracle_arch(name))


@functools.lru_cache(maxsize=None)
def cf_score(name, dtype, dev, wide=False):
    """As tiled_shapes.cf_score (cached: the wide test compares with the narrow run; `wide` must agree with RDMI_TILED_MIN_WGS)."""
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    assert (os.environ.get('RDMI_TILED_MIN_WGS') == '1') == wide
    model, _, _ = make_model(name, dtype)
    model = model.to(dev)
    x, lab, w, t = (a.to(dev) for a in cf_inputs(name))
    with torch.no_grad():
        s = mutils.get_cf_score_fn(sde_lib.RVESDE(SMIN, SMAX, N=1000), model, lab, w)(x, t)
    info = _ctx(model, dev, name).path_info()
    assert ('bf16' in info) == (dtype == 'bf16'), info
    return s.cpu()


def check_forward(name, dtype, dev, wide=False):
    s, ref = cf_score(name, dtype, dev, wide), cf_ref64(name)
    assert s.shape == ref.shape and bool(torch.isfinite(s).all())
    errs = rel_errs(s, ref)
    print(f'tiled odd shapes forward {name} {dtype}{" wide" if wide else ""} on {dev}: max |s - ref64| / max |ref64| per sample '
          + ' '.join(f'{e:.2e}' for e in errs))
    for n, e in enumerate(errs):
        assert e <= TOL[dtype], (name, dtype, n, e)
    return s


# ---- short-tile GroupNorm statistics: every conv bias + 40 (tiled_shapes.check_shifted_statistics) ------------------------------------
def check_shifted_statistics(name, dev, monkeypatch):
    from oracle import rd_oracle_torch as OT
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    s = SHAPES[name]
    g = torch.Generator().manual_seed(12)
    x = torch.rand(2, s['ch'], s['H'], s['W'], generator=g); lab = torch.zeros(2, 1); t = torch.tensor([0.6, 0.3])

    def run():
        model, _, _ = make_model(name)
        sd = model.state_dict()
        model.load_state_dict({**sd, **{k: v + 40.0 for k, v in sd.items()
                                        if k.endswith('Conv_0.bias') or k.endswith('Conv_1.bias') or k == 'input_conv.bias'}})
        model = model.to(dev)
        with torch.no_grad():
            out = mutils.get_score_fn(sde_lib.RVESDE(SMIN, SMAX, N=1000), model)(x.to(dev), t.to(dev), class_labels=lab.to(dev))
        _ctx(model, dev, name)
        return out.cpu(), model.state_dict()
    out, sd = run()
    monkeypatch.setenv('RDMI_TILED_STATS_PASS', '1')
    out2, _ = run()
    monkeypatch.delenv('RDMI_TILED_STATS_PASS')
    with torch.no_grad():
        ref = OT.ncsnpp_forward(_p64(sd), x.double(), OT.sigma_of(t.double(), SMIN, SMAX), lab.double(), **oracle_arch(name))
    e1, e2 = rel_errs(out, ref), rel_errs(out, out2.double())
    print(f'tiled odd shapes shifted statistics {name} on {dev}: vs float64 oracle ' + ' '.join(f'{e:.2e}' for e in e1)
          + ', vs the two-pass statistics ' + ' '.join(f'{e:.2e}' for e in e2))
    for n in range(2):
        amp = float(ref[n].abs().max())
        assert float((out[n].double() - ref[n]).abs().max()) <= STATS_TOL * amp, (name, n, e1[n])
        assert float((out[n] - out2[n]).abs().max()) <= STATS_TOL * amp, (name, n, e2[n])


# ---- localising taps (tiled_shapes.check_taps) ----------------------------------------------------------------------------------------
def check_taps(name, dev, tap_names):
    from oracle import rd_oracle_torch as OT
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    s = SHAPES[name]
    g = torch.Generator().manual_seed(13)
    x = torch.rand(2, s['ch'], s['H'], s['W'], generator=g); lab = torch.zeros(2, 1); t = torch.tensor([0.7, 0.2])
    model, _, params = make_model(name)
    model = model.to(dev)
    xd = x.to(dev)
    with torch.no_grad():
        mutils.get_score_fn(sde_lib.RVESDE(SMIN, SMAX, N=1000), model)(xd, t.to(dev), class_labels=lab.to(dev))
    ctx = _ctx(model, dev, name)
    taps = {}
    with torch.no_grad():
        OT.ncsnpp_forward(_p64(params), x.double(), OT.sigma_of(t.double(), SMIN, SMAX), lab.double(), taps=taps, **oracle_arch(name))
    for k in tap_names:
        a, r = ctx.get_tap(k, xd, 2).cpu().double(), taps[k]
        assert a.shape == r.shape, (k, a.shape, r.shape)
        err, amp = float((a - r).abs().max()), float(r.abs().max())
        print(f'tiled odd shapes tap {name} {k} on {dev}: max |a - ref64| {err:.2e}, max |ref64| {amp:.2e}')
        assert err <= TAP_TOL * max(1.0, amp), (k, err, amp)


# ---- backward, fp32 (tiled_shapes.check_backward; the rounds of test_emu_input_grad.run_modes) ----------------------------------------
def grad_case(name, dev):
    s = SHAPES[name]
    model, _, params = make_model(name)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(2, s['ch'], s['H'], s['W'], generator=g)
    sigma = torch.tensor([0.7, 3.0])
    lab = torch.zeros(2, 1)
    gout = torch.randn(2, s['ch'], s['H'], s['W'], generator=g)
    return model.to(dev), params, oracle_arch(name), tuple(a.to(dev) for a in (x, sigma, lab, gout))


def run_backward(name, dev, rounds=2):
    """Train-mode forward (p = 0), then `rounds` x (rdmi_backward, rdmi_backward_input(grads, grad_x), VJP-only), as IG.run_modes does
    for its own cases (which are looked up by name there)."""
    model, params, arch, (x, sigma, lab, gout) = grad_case(name, dev)
    tctx = model.train_context(x.shape[0], x.shape[2], x.shape[3], x.device)
    out = torch.empty_like(x)
    total = sum(p.numel() for p in model.parameters())
    res = dict(plain=[], full=[], gx_full=[], gx_vjp=[])
    tctx.train_forward(x, sigma, lab, out, 0.0, 0)
    for _ in range(rounds):
        flat = torch.full((total,), float('nan'), device=x.device)
        tctx.backward(gout, flat, x)
        res['plain'].append(flat)
        flat2, gx = torch.full_like(flat, float('nan')), torch.full_like(x, float('nan'))
        tctx.backward(gout, flat2, x, grad_x=gx)
        res['full'].append(flat2); res['gx_full'].append(gx)
        gx2 = torch.full_like(x, float('nan'))
        tctx.backward(gout, None, x, grad_x=gx2)
        res['gx_vjp'].append(gx2)
    res['info'] = tctx.path_info()
    res['names'] = [(n, p.numel()) for n, p in model.named_parameters()]
    res['args'] = (params, arch, x, sigma, lab, gout)
    return res


def check_backward(name, dev):
    res = run_backward(name, dev)
    check_path(res['info'], name)
    flat, off, hip = res['plain'][0].cpu(), 0, {}
    for n, ne in res['names']:
        if n != 'time_embed.W':                    # fixed Fourier frequencies: not trained
            hip[n] = flat[off:off + ne].numpy()
        off += ne
    assert off == flat.numel()
    ref, gx = oracle_grads(*res['args'], names=list(hip))
    ref = {n: v.reshape(-1) for n, v in ref.items()}
    print(f'tiled odd shapes backward {name} on {dev}: worst parameter gradient ||g - g64|| / ||g64|| '
          f'{max(IG.rel(torch.from_numpy(hip[n]), torch.from_numpy(ref[n])) for n in hip if not n.endswith("NIN_1.b")):.2e}, '
          f'grad_x full {IG.rel(res["gx_full"][0], gx):.2e}, VJP-only {IG.rel(res["gx_vjp"][0], gx):.2e}')
    TT._check(hip, ref)
    IG.check_grad_x(res['gx_full'][0], gx, GRAD_TOL)
    IG.check_grad_x(res['gx_vjp'][0], gx, GRAD_TOL)
    # two backward calls on the same inputs: bit-identical grad_x (both modes) and parameter gradients; the embedding chain behind `gta`
    # takes fp32 atomics in arrival order (IG.UNORDERED, documented there) and is compared at 1e-6 of the norm
    assert torch.equal(res['gx_full'][1], res['gx_full'][0]) and torch.equal(res['gx_vjp'][1], res['gx_vjp'][0])
    assert torch.equal(res['gx_vjp'][0], res['gx_full'][0])
    off = 0
    for n, ne in res['names']:
        for key in ('plain', 'full'):
            a, b = res[key][1][off:off + ne], res['plain'][0][off:off + ne]
            if n.startswith(IG.UNORDERED):
                assert float((a - b).norm()) <= 1e-6 * float(b.norm()) + 1e-30, (n, key)
            else:
                assert torch.equal(a, b), (n, key)
        off += ne


# ---- the fused sampler loop: three teacher-forced updates against a chain of oracle updates fed the same draws ------------------------
def check_sampler(name, dev, corrector):
    """get_pc_sampler(fused=True), N = 4 scales, injected noise: the trace after each of the 3 updates against OT.pc_update fed the same
    draws, with the tolerance of tests/test_gpu_cifar.py::test_cifar_cfg_score_and_pc_update_vs_oracle for its teacher-forced tiled
    updates (an expression in that test's body, restated here: 2e-5 + 1e-4 g(t)^2 / N max |score|)."""
    from oracle import rd_oracle as O
    from oracle import rd_oracle_torch as OT
    from rdmi import sampling, sde_lib
    s = SHAPES[name]
    shape = (2, s['ch'], s['H'], s['W'])
    B, E, Ns = 2, s['ch'] * s['H'] * s['W'], 4
    langevin = corrector == 'langevin'
    per = 2 if langevin else 1
    model, _, params = make_model(name)
    model = model.to(dev)
    p64 = _p64(params)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(*shape, generator=g); lab = torch.zeros(B, 1); w = torch.tensor([0.0, 0.7])
    noise = torch.randn((Ns - 1) * per, B, E, generator=g)
    teacher = torch.rand(Ns - 1, B, E, generator=g)
    sde = sde_lib.RVESDE(SMIN, SMAX, N=Ns)
    ts = O.torch_linspace(1, 1e-5, Ns)
    trace = torch.zeros(Ns - 1, B, E, device=dev)
    fn = sampling.get_pc_sampler(sde, shape, sampling.get_predictor('euler_maruyama'), sampling.get_corrector(corrector),
                                 sampling.get_denoiser('none'), 0.01, 1, 1e-5, dev, noise=noise.to(dev), trace=trace,
                                 teacher=teacher.to(dev), fused=True)
    _rand = torch.rand
    torch.rand = lambda *a, **k: x.clone()
    try:
        xs, nfe = fn(model, weight=w.to(dev), class_labels=lab.to(dev))
    finally:
        torch.rand = _rand
    assert nfe == Ns * 2
    _ctx(model, dev, name)
    trace = trace.cpu()
    for i in range(Ns - 1):
        x_prev = (x if i == 0 else teacher[i - 1].reshape(shape)).double()
        tv = torch.full((B,), float(ts[i]), dtype=torch.float64)
        with torch.no_grad():
            r = OT.pc_update(p64, x_prev, tv, lab.double(), w.double(), noise[per * i + per - 1].reshape(shape).double(), Ns,
                             z_corr=noise[per * i].reshape(shape).double() if langevin else None, smax=SMAX, **oracle_arch(name))
            sc = float(OT.cf_score(p64, x_prev, tv, lab.double(), w.double(), smax=SMAX, **oracle_arch(name)).abs().max())
        gg = float(OT.g_of(torch.tensor([float(ts[i])]), smax=SMAX)[0]) ** 2 / Ns
        err = float((trace[i].reshape(shape).double() - r).abs().max())
        print(f'tiled odd shapes sampler {name} corrector {corrector} on {dev}: update {i} max |x - ref64| {err:.2e} (bound {2e-5 + 1e-4 * gg * sc:.2e})')
        assert err <= 2e-5 + 1e-4 * gg * sc, (i, err, gg, sc)
    assert float(xs.min()) >= 0 and float(xs.max()) <= 1
