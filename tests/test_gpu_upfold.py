"""The nearest-x2 upsample folded into its 3x3 conv on the GPU, through the C ABI: folded inference
programs against the nine-tap op (RDMI_NO_UP_FOLD=1) and against the float64 torch oracle.

Tolerance: the one the project uses for this forward on the GPU, 2e-4 * max|score| (max|score| of a
sample's oracle output), on every element of the (guided) score."""
import os

import numpy as np
import pytest
import torch

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
    p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
    return dict(ge=ge, dev=torch.device('cuda:0'), p64=p64)


def _inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 1, H, W, generator=g)
    t = torch.rand(B, generator=g) * 0.99 + 0.01
    lab = torch.rand(B, 1, generator=g)
    w = torch.tensor([0.0, 0.5, 0.25][:B])
    return x, t, lab, w


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


def _up_taps(prog):
    """K description of the level-0 upsample conv ops of a program (the only 64-row CONV ops of the demo model)."""
    return [d.split()[3] for d in prog['ops'] if d.startswith('CONV rows=64 ')]


def _check(a, b, ref):
    """a: folded, b: nine taps, ref: float64 oracle."""
    bound = (TOL * np.abs(ref).reshape(ref.shape[0], -1).max(1))[:, None, None, None]
    d_ref, d_fold = np.abs(a - ref), np.abs(a - b)
    print(f'folded vs oracle {d_ref.max():.3e} ({(d_ref / bound).max():.3f} of the bound), folded vs nine taps {d_fold.max():.3e}')
    assert (d_ref <= bound).all(), float((d_ref / bound).max())
    assert (np.abs(b - ref) <= bound).all()
    assert (d_fold <= bound).all(), float((d_fold / bound).max())       # fp32 re-association only


@pytest.mark.parametrize('B,H,W,coop', [(2, 9, 9, True), (2, 8, 9, True), (3, 9, 9, True), (2, 9, 9, False)],
                         ids=['9x9-coop-group', '8x9-coop-group', '9x9-ragged-group', '9x9-single-sample'])
def test_folded_matches_nine_taps_and_oracle(env, B, H, W, coop):
    from oracle import rd_oracle_torch as OT
    base = {} if coop else {'RDMI_COOP': '0'}
    seed = 40 + B + H
    a, progs, info = _run(env, B, H, W, seed, base)
    b, progs_b, _ = _run(env, B, H, W, seed, dict(base, RDMI_NO_UP_FOLD='1'))
    assert ('co-operative groups' in info) == coop, info
    assert all(_up_taps(q) and set(_up_taps(q)) == {'K=4x128(+0)'} for q in progs), [q['ops'] for q in progs]
    assert all(_up_taps(q) and set(_up_taps(q)) == {'K=9x128(+0)'} for q in progs_b)
    x, t, lab, w = _inputs(B, H, W, seed)
    with torch.no_grad():
        ref = OT.cf_score(env['p64'], x.double(), t.double(), lab.double(), w.double()).numpy()
    _check(a, b, ref)


def test_two_samples_per_workgroup(env):
    """The S = 2 program at a small batch (RDMI_S_MIN_WG=1, co-operative program off: two plain forwards = one workgroup of two
    sample slots, each with its own folded upsample op)."""
    from oracle import rd_oracle_torch as OT
    base = {'RDMI_S_MIN_WG': '1', 'RDMI_COOP': '0', 'RDMI_S': '2'}
    a, progs, info = _run(env, 2, 9, 9, 51, base, guided=False)
    b, _, _ = _run(env, 2, 9, 9, 51, dict(base, RDMI_NO_UP_FOLD='1'), guided=False)
    assert 'S=2 samples/workgroup from batch 2' in info, info
    s2 = [q for q in progs if q['S'] == 2]
    assert len(s2) == 1 and _up_taps(s2[0]) == ['K=4x128(+0)'] * 2, s2
    x, t, lab, _ = _inputs(2, 9, 9, 51)
    with torch.no_grad():
        ref = OT.ncsnpp_forward(env['p64'], x.double(), OT.sigma_of(t.double()), lab.double()).numpy()
    _check(a, b, ref)
