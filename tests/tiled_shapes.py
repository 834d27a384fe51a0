"""Shape matrix of the spatially TILED plan (csrc/tiled_kernels.h, tiled_bwd_kernels.h, tiled_train.h; planned by TiledBuilder in
csrc/rdmi.hip) off the power-of-two grids: shared check functions, run on the CPU emulator by tests/test_emu_tiled_shapes.py and on an
MI355X by tests/test_gpu_tiled_shapes.py.  The reference is oracle/rd_oracle_torch.ncsnpp_forward (architecture-generic, pinned to the
reference by the 9x9 and CIFAR fixtures) with float64 parameters and inputs.

All models are RGB, one res block per level, scale_by_sigma, sigma_max 50, seeded synthetic weights (oracle/weights.py).  Each shape is
there for the edges named beside it:

S1  24x24, nf 64, ch_mult (1,2,2), attention at 12x12
      24-wide level: TR = 2, tiles of 48 pixels (rows 48..63 of the MFMA row tiles are masked); 12x12 level: TR = 5, three tiles per
      image, the last with 2 rows (24 of 60 pixels: the short-tile path of the channel records and their Chan merge); 6x6 level: one
      36-pixel tile; stride-2 and x2-upsample windows on tiles that are not 64 pixels; attention over L = 144, C = 128: bgemm_nt with
      M = N = 144 (two 64-tiles and 16), softmax rows of 144, the generic transpose_lc_kernel, and in bf16 the route that is not the
      fused core (P V contracts K = 144 = 4 x 32 + 16).
S2  16x24 (H x W), nf 64, ch_mult (1,2), no attention
      H != W everywhere (a swapped H / W in window, stride or upsample indexing cannot cancel); 8x12 level: TR = 5, two tiles, the last
      with 3 rows.
S3  8x8, nf 32, ch_mult (1,2,2), attention at 4x4
      Cout_pad = 32 < 64 (waves whose column tiles lie beyond the padded width); a whole-image 4x4 tile (one MFMA row tile) and a 2x2
      bottleneck (4 pixels, the window larger than the image on every side); attention over L = 16 (less than one bgemm tile; the bf16
      P V contracts K = 16); concatenations of 96 channels (24 groups).
S4  16x16, nf 96, ch_mult (1,2), no attention
      channel counts 96 / 192 / 288 / 384: GroupNorm groups of 9 channels at C = 288 (odd, straddling the float4 quads: the Cg & 3 != 0
      branch of tconv_commit, and groups that cross gn_act_fin's 64-channel slices), of 6 and of 12; Cout_pad = 96 (one and a half
      64-column workgroups); bf16 convs with Cin % 64 != 0 (96, 288) stay on tconv_kernel<bf16> while their neighbours (192, 384) take
      gn_act + tconv_pre, with the column interleave on some convs only.
"""
import functools
import os

import torch

from tests import test_emu_input_grad as IG
from tests import test_emu_tiled_train as TT

SHAPES = {
    'S1': dict(H=24, W=24, nf=64, ch_mult=(1, 2, 2), attn=(12,)),
    'S2': dict(H=16, W=24, nf=64, ch_mult=(1, 2), attn=()),
    'S3': dict(H=8, W=8, nf=32, ch_mult=(1, 2, 2), attn=(4,)),
    'S4': dict(H=16, W=16, nf=96, ch_mult=(1, 2), attn=()),
}
SMIN, SMAX = 0.01, 50.0
TOL = {'f32': 2e-5, 'bf16': 3e-2}          # of each sample's largest |score|: the project's stated tolerances (test_tiled_plan_small_rgb_model, test_gpu_cifar.py)
STATS_TOL = 1e-4                           # test_tiled_plan_groupnorm_statistics_with_large_group_means
TAP_TOL = 1e-4                             # x max(1, max |tap|): test_cifar_forward_golden_and_taps
GRAD_TOL = IG.BOUND['tiled']               # ||g - g64|| <= 1e-4 ||g64||


def oracle_arch(name):
    s = SHAPES[name]
    return dict(ch_mult=s['ch_mult'], nrb=1, attn_levels=tuple(s['H'] // 2 ** i in s['attn'] for i in range(len(s['ch_mult']))),
                scale_by_sigma=True)


def make_model(name, compute_dtype='f32'):
    """-> (model on the CPU in eval mode, cfg, params): built as test_emu_parity._small_rgb_model builds the 16x16 model."""
    import __graft_entry__ as ge
    from oracle.weights import make_params
    from rdmi.models import utils as mutils
    s = SHAPES[name]
    cfg = ge.demo_config(image_size=s['H'], image_width=s['W'])
    m = cfg.model
    m.nf, m.ch_mult, m.num_res_blocks, m.attn_resolutions = s['nf'], list(s['ch_mult']), 1, list(s['attn'])
    m.channels, m.scale_by_sigma, m.compute_dtype = 3, True, compute_dtype
    cfg.sde.sigma_max = SMAX
    params = make_params(3, nf=s['nf'], ch_mult=s['ch_mult'], num_res_blocks=1, attn_resolutions=s['attn'], image_size=s['H'], channels=3)
    model = mutils.create_model(cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    return model.eval(), cfg, params


def _p64(sd):
    return {k: (v if torch.is_tensor(v) else torch.from_numpy(v.copy())).detach().cpu().double() for k, v in sd.items()}


def _ctx(model, dev, name, train=False):
    s = SHAPES[name]
    key = (str(torch.device(dev)), s['H'], s['W'])
    ctx = model._ctx[('train',) + key if train else key]
    info = ctx.path_info()
    assert info.startswith('tiled'), info
    return ctx


# ---- forward: classifier-free-guidance score, B = 3 (odd batch, 6 forwards), distinct times across the schedule ----------------------
def cf_inputs(name):
    s = SHAPES[name]
    g = torch.Generator().manual_seed(31)
    x = torch.rand(3, 3, s['H'], s['W'], generator=g)
    # zero labels, as the RGB configuration feeds them (test_gpu_cifar.py): both halves of the guidance batch then are the same network
    # evaluation, and (1 + w) s - w s carries one forward's error, which is what the per-sample tolerance is stated for
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
    """The score of the tiled plan (cached: the wide tests compare with the narrow run).  `wide` must agree with RDMI_TILED_MIN_WGS in the
    environment, which the calling test sets with monkeypatch: contexts read it at creation."""
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


def rel_errs(s, ref):
    return [float((s[n].double() - ref[n]).abs().max() / ref[n].abs().max()) for n in range(ref.shape[0])]


def check_forward(name, dtype, dev, wide=False):
    s, ref = cf_score(name, dtype, dev, wide), cf_ref64(name)
    assert s.shape == ref.shape and bool(torch.isfinite(s).all())
    errs = rel_errs(s, ref)
    print(f'tiled shapes forward {name} {dtype}{" wide" if wide else ""} on {dev}: max |s - ref64| / max |ref64| per sample '
          + ' '.join(f'{e:.2e}' for e in errs))
    for n, e in enumerate(errs):
        assert e <= TOL[dtype], (name, dtype, n, e)
    return s


# ---- short-tile GroupNorm statistics: every conv bias + 40 ----------------------------------------------------------------------
def check_shifted_statistics(name, dev, monkeypatch):
    from oracle import rd_oracle_torch as OT
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    s = SHAPES[name]
    g = torch.Generator().manual_seed(12)
    x = torch.rand(2, 3, s['H'], s['W'], generator=g); lab = torch.zeros(2, 1); t = torch.tensor([0.6, 0.3])

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
    print(f'tiled shapes shifted statistics {name} on {dev}: vs float64 oracle ' + ' '.join(f'{e:.2e}' for e in e1)
          + ', vs the two-pass statistics ' + ' '.join(f'{e:.2e}' for e in e2))
    for n in range(2):
        amp = float(ref[n].abs().max())
        assert float((out[n].double() - ref[n]).abs().max()) <= STATS_TOL * amp, (name, n, e1[n])
        assert float((out[n] - out2[n]).abs().max()) <= STATS_TOL * amp, (name, n, e2[n])


# ---- localising taps -----------------------------------------------------------------------------------------------------------
def check_taps(name, dev, tap_names):
    from oracle import rd_oracle_torch as OT
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    s = SHAPES[name]
    g = torch.Generator().manual_seed(13)
    x = torch.rand(2, 3, s['H'], s['W'], generator=g); lab = torch.zeros(2, 1); t = torch.tensor([0.7, 0.2])
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
        print(f'tiled shapes tap {name} {k} on {dev}: max |a - ref64| {err:.2e}, max |ref64| {amp:.2e}')
        assert err <= TAP_TOL * max(1.0, amp), (k, err, amp)


# ---- backward, fp32: parameter gradients and grad_x (full and VJP-only call) against float64 autograd -----------------------------
def grad_case(name, dev):
    """make_case of tests/test_emu_input_grad.py for a shape of this matrix (B = 2, dropout off, a fixed random upstream gradient)."""
    s = SHAPES[name]
    model, _, params = make_model(name)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(2, 3, s['H'], s['W'], generator=g)
    sigma = torch.tensor([0.7, 3.0])
    lab = torch.zeros(2, 1)
    gout = torch.randn(2, 3, s['H'], s['W'], generator=g)
    return model.to(dev), params, oracle_arch(name), tuple(a.to(dev) for a in (x, sigma, lab, gout)), (SMIN, SMAX)


def oracle_grads(params, arch, x, sigma, lab, gout, names):
    """float64 autograd through the oracle -> ({name: parameter gradient}, grad_x)."""
    from oracle import rd_oracle_torch as OT
    p = {k: v.requires_grad_(k in names) for k, v in _p64(params).items()}
    xr = x.detach().cpu().double().requires_grad_()
    out = OT.ncsnpp_forward(p, xr, sigma.cpu().double(), lab.cpu().double(), **arch)
    gr = torch.autograd.grad(out, [xr] + [p[n] for n in names], gout.cpu().double())
    return {n: v.numpy() for n, v in zip(names, gr[1:])}, gr[0]


def check_backward(name, dev):
    res = IG.run_modes(name, dev, rounds=1)
    assert res['info'].startswith('tiled'), res['info']
    flat, off, hip = res['plain'][0].cpu(), 0, {}
    for n, ne in res['names']:
        if n != 'time_embed.W':                    # fixed Fourier frequencies: not trained
            hip[n] = flat[off:off + ne].numpy()
        off += ne
    assert off == flat.numel()
    ref, gx = oracle_grads(*res['args'], names=list(hip))
    ref = {n: v.reshape(-1) for n, v in ref.items()}
    TT._check(hip, ref)
    print(f'tiled shapes backward {name} on {dev}: worst parameter gradient ||g - g64|| / ||g64|| '
          f'{max(IG.rel(torch.from_numpy(hip[n]), torch.from_numpy(ref[n])) for n in hip if not n.endswith("NIN_1.b")):.2e}, '
          f'grad_x full {IG.rel(res["gx_full"][0], gx):.2e}, VJP-only {IG.rel(res["gx_vjp"][0], gx):.2e}')
    IG.check_grad_x(res['gx_full'][0], gx, GRAD_TOL)
    IG.check_grad_x(res['gx_vjp'][0], gx, GRAD_TOL)
