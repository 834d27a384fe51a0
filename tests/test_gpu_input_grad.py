"""Input gradients, the VJP-only backward, the autograd surface and rdmi.likelihood on an MI355X: the checks of
tests/test_emu_input_grad.py on the device (9x9 model fp32 / bf16, 16x16 RGB tiled model), plus grad_x of the CIFAR-shape model."""
import pytest
import torch

from tests import test_emu_input_grad as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _device_library():
    from rdmi import _native
    if _native._lib is not None and _native.is_emulator():
        pytest.fail('the emulator build is bound: GPU tests need librdmi.so')


@pytest.mark.parametrize('case', ['layer_f32', 'layer_bf16', 'tiled'])
def test_grad_x_and_modes(case):
    """Tests 1-3 on the device: grad_x (full and VJP-only call) against float64 autograd, whole / per channel / border frame; then three
    interleaved rounds of the three modes at B = 2, bit-identical grad_x and parameter gradients, and -- on the layer plan, whose
    launches are recorded graphs -- replays of every mode's graph."""
    res = T.run_modes(case, DEV, rounds=1)
    params, arch, x, sigma, lab, gout = res['args']
    ref = T.oracle_input_grad(params, arch, x, sigma, lab, gout)
    T.check_grad_x(res['gx_full'][0], ref, T.BOUND[case])
    T.check_grad_x(res['gx_vjp'][0], ref, T.BOUND[case])
    res2 = T.run_modes(case, DEV, B=2, rounds=3)
    T.check_mode_consistency(res2, need_replays=case.startswith('layer'))
    assert 'input-gradient backward calls: 6' in res2['info'], res2['info']


@pytest.mark.parametrize('case', ['layer_f32', 'layer_bf16', 'tiled'])
def test_autograd_surface(case):
    gx = T.autograd_surface(case, DEV)
    _, params, arch, (x, sigma, lab, gout), _ = T.make_case(case, 'cpu', 2)
    T.check_grad_x(gx, T.oracle_input_grad(params, arch, x, sigma, lab, gout), T.BOUND[case])


@pytest.mark.parametrize('E', [81, 3072])
def test_pf_drift_div(E):
    T.pf_drift_div_check(DEV, E)


@pytest.mark.parametrize('case', ['layer_f32', 'tiled'])
def test_likelihood_matches_oracle(case):
    """As tests/test_emu_input_grad.py::test_likelihood_matches_oracle, on the device."""
    T.likelihood_check(case, DEV)


def test_cifar_grad_x_matches_oracle():
    """CIFAR-shape model, B = 2: grad_x of the VJP-only backward against float64 autograd through the oracle on the CPU,
    ||g - g64|| <= max(1e-4 ||g64||, 8 ||g32 - g64||) with g32 the same oracle in fp32 (the rule of test_cifar_gradients_match_oracle),
    whole tensor, per channel and on the border frame."""
    import __graft_entry__ as ge
    from oracle import rd_oracle_torch as OT
    model, _, params = ge.make_cifar_model(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 32, 32, generator=g)
    sigma = torch.tensor([0.3, 7.0])
    lab = torch.zeros(2, 1)
    gout = torch.randn(2, 3, 32, 32, generator=g)
    out, gx = model.native_vjp(x.to(DEV), sigma.to(DEV), lab.to(DEV), gout.to(DEV))
    assert model._ctx[('train', DEV, 32, 32)].path_info().startswith('tiled')
    g64 = T.oracle_input_grad(params, OT.CIFAR_ARCH, x, sigma, lab, gout)
    g32 = T.oracle_input_grad(params, OT.CIFAR_ARCH, x, sigma, lab, gout, dtype=torch.float32)
    gx = gx.cpu().double()
    fm = T.frame_mask(32, 32)
    views = [lambda t: t, lambda t: t[:, :, fm]] + [lambda t, c=c: t[:, c] for c in range(3)] + [lambda t, c=c: t[:, c][:, fm] for c in range(3)]
    for i, v in enumerate(views):
        d, d32, n = float((v(gx) - v(g64)).norm()), float((v(g32) - v(g64)).norm()), float(v(g64).norm())
        print(f'cifar grad_x view {i}: rel {d / n:.3e}, fp32 oracle {d32 / n:.3e}')
        assert d <= max(1e-4 * n, 8 * d32), (i, d / n, d32 / n)
