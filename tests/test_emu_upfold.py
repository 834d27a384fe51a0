"""The nearest-x2 upsample folded into its 3x3 conv, on the CPU emulator: the inference programs run
`upsample.<nlev-2>.Conv_0` as four 2x2 phase convs over the 4x4 source with pre-summed tap weights, the training
forward keeps the nine-tap op.  Folded against unfolded (RDMI_NO_UP_FOLD=1) and against the float64 torch oracle.

Tolerance: the one the project uses for this forward on the emulator, 5e-5 absolute (tests/test_emu_parity.py), on
every element of the guided score."""
import os

import numpy as np
import pytest
import torch

TOL = 5e-5
UP = 'upsample.1.Conv_0'          # the upsample onto level 0 of the three-level demo model


@pytest.fixture(scope='module')
def env(emu):
    import __graft_entry__ as ge
    _, _, params = ge.make_model('cpu')
    p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
    return dict(ge=ge, params=params, p64=p64)


def _inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 1, H, W, generator=g)
    t = torch.rand(B, generator=g) * 0.99 + 0.01
    lab = torch.rand(B, 1, generator=g)
    w = torch.tensor([0.0, 0.5, 0.25][:B])
    return x, t, lab, w


_ref_cache = {}


def _oracle(env, B, H, W, seed):
    """float64 guided score of the case's inputs, computed once per case."""
    key = (B, H, W, seed)
    if key not in _ref_cache:
        from oracle import rd_oracle_torch as OT
        x, t, lab, w = _inputs(B, H, W, seed)
        with torch.no_grad():
            _ref_cache[key] = OT.cf_score(env['p64'], x.double(), t.double(), lab.double(), w.double()).numpy()
    return _ref_cache[key]


def _run(env, B, H, W, seed, envvars):
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    x, t, lab, w = _inputs(B, H, W, seed)
    os.environ.update(envvars)
    try:
        model, _, _ = env['ge'].make_model('cpu')
        with torch.no_grad():
            s = mutils.get_cf_score_fn(sde_lib.RVESDE(0.01, 5, N=1000), model, lab, w)(x, t).numpy()
        ctx = model._ctx[('cpu', H, W)]
        assert not ctx.coop_gave_up()
        return s, ctx.programs(), ctx.path_info()
    finally:
        for k in envvars:
            os.environ.pop(k, None)


def _up_ops(prog):
    """Descriptions of the level-0 upsample conv ops of a program: the only 64-row CONV ops of the demo model."""
    return [d for d in prog['ops'] if d.startswith('CONV rows=64 ')]


@pytest.mark.parametrize('B,H,W,coop', [(2, 9, 9, True), (2, 8, 9, True), (3, 9, 9, True), (2, 9, 9, False)],
                         ids=['9x9-coop-group', '8x9-coop-group', '9x9-ragged-group', '9x9-single-sample'])
def test_folded_matches_unfolded_and_oracle(env, B, H, W, coop):
    """B = 2 with guidance is four forwards = one co-operative group; B = 3 is six = a full and a ragged group;
    RDMI_COOP=0 runs the S = 1 program."""
    base = {} if coop else {'RDMI_COOP': '0'}
    seed = 40 + B + H
    a, progs, info = _run(env, B, H, W, seed, base)
    b, progs_b, _ = _run(env, B, H, W, seed, dict(base, RDMI_NO_UP_FOLD='1'))
    assert ('co-operative groups' in info) == coop, info
    for q in progs:
        assert [('K=4x128' in d) for d in _up_ops(q)] == [True] * (1 if q['coop'] else q['S']), q['ops']
    for q in progs_b:
        assert all('K=9x128' in d for d in _up_ops(q)) and _up_ops(q), q['ops']
    ref = _oracle(env, B, H, W, seed)
    d_ref, d_fold = np.abs(a - ref), np.abs(a - b)
    print(f'folded vs oracle {d_ref.max():.3e}, folded vs unfolded {d_fold.max():.3e}')
    assert d_ref.max() <= TOL, float(d_ref.max())
    assert np.abs(b - ref).max() <= TOL
    assert d_fold.max() <= TOL, float(d_fold.max())      # fp32 re-association only: far below the oracle tolerance


def test_phase_weights_are_the_tap_sums(env):
    """All 16 packed matrices (4 phases x 4 taps) against numpy sums of the reference-layout weight, summed in the same fixed
    order (ky ascending, then kx) in float32: the difference must be ZERO."""
    model, _, _ = env['ge'].make_model('cpu')
    ctx = model.native_context(2, 9, 9, 'cpu')
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    with torch.no_grad():          # any forward repacks
        mutils.get_score_fn(sde_lib.RVESDE(0.01, 5, N=1000), model)(torch.rand(1, 1, 9, 9), torch.tensor([0.5]), class_labels=torch.rand(1, 1))
    Wt = env['params'][UP + '.weight']                    # [Cout][Cin][3][3]
    Cout, Cin = Wt.shape[:2]
    assert (Cout, Cin) == (128, 128)
    got = ctx.packed(UP + '.up4', 16 * Cin * Cout).numpy().reshape(4, 4, Cin // 16, Cout, 16)      # [phase][tap][K/16][N][16]
    taps = {0: ([0], [1, 2]), 1: ([0, 1], [2])}           # phase bit -> 3x3 taps read at source offsets (phase - 1, phase)
    for p in range(4):
        for t in range(4):
            acc = None
            for ky in taps[p >> 1][t >> 1]:
                for kx in taps[p & 1][t & 1]:
                    acc = Wt[:, :, ky, kx].copy() if acc is None else (acc + Wt[:, :, ky, kx]).astype(np.float32)
            want = acc.T.reshape(Cin // 16, 16, Cout).transpose(0, 2, 1)      # [ci][co] -> [K/16][N][16]
            assert np.array_equal(got[p, t], want), (p, t, float(np.abs(got[p, t] - want).max()))


def test_training_program_keeps_nine_taps(env):
    model, _, _ = env['ge'].make_model('cpu')
    progs = model.train_context(2, 9, 9, 'cpu').programs()
    tr = [q for q in progs if q['train']]
    assert len(tr) == 1
    assert [('K=9x128' in d) for d in _up_ops(tr[0])] == [True], tr[0]['ops']
    inf = [q for q in progs if not q['train']]
    assert inf and all(_up_ops(q) and all('K=4x128' in d for d in _up_ops(q)) for q in inf)
