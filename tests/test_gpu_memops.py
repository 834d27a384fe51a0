"""The data-movement ops of the fused U-Net (one-pass GroupNorm, batched gather: DESIGN 4.2h) on an MI355X: the cases of
tests/test_emu_memops.py on the device.  Every case is one guided score of B <= 3 samples, run twice on one context.

Bound: 2e-4 * max |ref64| on every element (float64 torch oracle); the second call returns the same bits."""
import numpy as np
import pytest
import torch

from tests import test_emu_memops as M

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def genv():
    """The device library bound, the shipped parameters in float32 and float64 (what test_emu_fold9.env holds for the emulator)."""
    import __graft_entry__ as ge
    from rdmi import _native
    if _native._lib is not None and _native.is_emulator():
        pytest.fail('the emulator build is bound: GPU tests need librdmi.so')
    ge.build()
    assert not _native.is_emulator()
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    _, _, params = ge.make_model('cpu')
    return dict(ge=ge, params=params, p64={k: torch.from_numpy(v).double() for k, v in params.items()})


def gpu_tol(ref):
    return 2e-4 * float(np.abs(ref).max())


@pytest.mark.parametrize('B,H,W,prog,extra', [c[1:] for c in M.SHIP_CASES], ids=[c[0] for c in M.SHIP_CASES])
def test_shipped_model(genv, B, H, W, prog, extra):
    M.check_ship(genv, DEV, gpu_tol, B, H, W, prog, extra)


@pytest.mark.parametrize('name,prog,B', M.MATRIX_CASES, ids=[f'{n}-{p}-B{B}' for n, p, B in M.MATRIX_CASES])
def test_shape_matrix(genv, name, prog, B):
    M.check_matrix(DEV, gpu_tol, name, prog, B)
