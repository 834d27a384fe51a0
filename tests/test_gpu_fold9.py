"""The attention k projection folded into q on the GPU, through the C ABI: k-folded inference programs (two
projections, K = the GroupNorm_0 output) against three projections
(RDMI_NO_K_FOLD=1 RDMI_NO_DENSE_IO=1) and against the float64 torch oracle.

Tolerance: the one the project uses for this forward on the GPU, 2e-4 * max|score| (max|score| of a
sample's oracle output), on every element of the (guided) score."""
import os

import numpy as np
import pytest
import torch

from tests.test_emu_fold9 import ATTN, CASES, IDS, OFF, _inputs, _oracle, check_pack, check_shapes

pytestmark = pytest.mark.gpu

TOL = 2e-4


@pytest.fixture(scope='module')
def env():
    import __graft_entry__ as ge
    ge.build()
    from rdmi import _native
    assert not _native.is_emulator()
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    _, _, params = ge.make_model('cpu')
    for a in ATTN:          # the dropped score terms vanish trivially with zero q / k biases: the fixture's are not
        assert np.abs(params[a + '.NIN_0.b']).min() > 0 and np.abs(params[a + '.NIN_1.b']).min() > 0
    p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
    return dict(ge=ge, dev=torch.device('cuda:0'), params=params, p64=p64)


def _run(env, B, H, W, seed, envvars, guided=True):
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    dev = env['dev']
    x, t, lab, w = _inputs(B, H, W, seed)
    os.environ.update(envvars)
    try:
        model, _, _ = env['ge'].make_model(dev)
        sde = sde_lib.RVESDE(0.01, 5, N=1000)
        with torch.no_grad():
            if guided:
                s = mutils.get_cf_score_fn(sde, model, lab.to(dev), w.to(dev))(x.to(dev), t.to(dev))
            else:
                s = mutils.get_score_fn(sde, model)(x.to(dev), t.to(dev), class_labels=lab.to(dev))
        ctx = model._ctx[(str(dev), H, W)]
        assert not ctx.coop_gave_up()                 # rdmi_coop_status == 0
        return s.cpu().numpy(), ctx.programs(), ctx.path_info()
    finally:
        for k in envvars:
            os.environ.pop(k, None)


@pytest.mark.parametrize('B,H,W,base,guided', CASES, ids=IDS)
def test_folded_matches_three_projections_and_oracle(env, B, H, W, base, guided):
    seed = 60 + B + H
    a, progs, info = _run(env, B, H, W, seed, base, guided)
    b, progs_off, info_off = _run(env, B, H, W, seed, dict(base, **OFF), guided)
    assert info == info_off, (info, info_off)
    if 'RDMI_S' in base:
        assert 'S=2 samples/workgroup from batch 2' in info, info
    else:
        assert ('co-operative groups' in info) == ('RDMI_COOP' not in base), info
    check_shapes(progs, progs_off, H * W)
    ref = _oracle(env, B, H, W, seed, guided)
    bound = (TOL * np.abs(ref).reshape(ref.shape[0], -1).max(1))[:, None, None, None]
    d_ref, d_off, d_fold = np.abs(a - ref), np.abs(b - ref), np.abs(a - b)
    print(f'folded vs oracle {d_ref.max():.3e} ({(d_ref / bound).max():.3f} of the bound), three projections vs oracle {d_off.max():.3e} '
          f'({(d_off / bound).max():.3f}), folded vs three projections {d_fold.max():.3e} ({(d_fold / bound).max():.3f} of the bound), '
          f'bit-equal: {np.array_equal(a, b)}')
    assert (d_ref <= bound).all(), float((d_ref / bound).max())
    assert (d_off <= bound).all(), float((d_off / bound).max())
    assert (d_fold <= bound).all(), float((d_fold / bound).max())


def test_packed_products(env):
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    dev = env['dev']
    model, _, _ = env['ge'].make_model(dev)
    ctx = model.native_context(2, 9, 9, str(dev))
    with torch.no_grad():          # any forward repacks
        mutils.get_score_fn(sde_lib.RVESDE(0.01, 5, N=1000), model)(torch.rand(1, 1, 9, 9, device=dev), torch.tensor([0.5], device=dev),
                                                                      class_labels=torch.rand(1, 1, device=dev))
    check_pack(ctx, env['params'])
