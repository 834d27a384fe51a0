"""The attention k projection folded into q, on the CPU emulator: the inference programs of the fused plan
compute q' = xn (Wq Wk^T) + bq Wk^T and the NIN_3-folded v' only and read the GroupNorm_0 output xn itself as K -- the score
terms that depend on the query row alone cancel in the softmax over keys.  Folded against three projections (RDMI_NO_K_FOLD=1;
RDMI_NO_DENSE_IO=1 belongs to the comparison configuration and switches nothing yet) and against the float64 torch oracle.

Tolerance: the one the project uses for this forward on the emulator, 5e-5 absolute (tests/test_emu_parity.py), on every
element of the guided score."""
import os

import numpy as np
import pytest
import torch

TOL = 5e-5
OFF = {'RDMI_NO_K_FOLD': '1', 'RDMI_NO_DENSE_IO': '1'}
ATTN = ['down_attn.0', 'down_attn.1', 'up_attn.6', 'up_attn.7', 'up_attn.8']      # the five attention blocks of the demo model


@pytest.fixture(scope='module')
def env(emu):
    import __graft_entry__ as ge
    _, _, params = ge.make_model('cpu')
    # the dropped score terms vanish trivially with zero q / k biases: the fixture's are not
    for a in ATTN:
        assert np.abs(params[a + '.NIN_0.b']).min() > 0 and np.abs(params[a + '.NIN_1.b']).min() > 0
    p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
    return dict(ge=ge, params=params, p64=p64)


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
    x, t, lab, w = _inputs(B, H, W, seed)
    os.environ.update(envvars)
    try:
        model, _, _ = env['ge'].make_model('cpu')
        sde = sde_lib.RVESDE(0.01, 5, N=1000)
        with torch.no_grad():
            if guided:
                s = mutils.get_cf_score_fn(sde, model, lab, w)(x, t).numpy()
            else:
                s = mutils.get_score_fn(sde, model)(x, t, class_labels=lab).numpy()
        ctx = model._ctx[('cpu', H, W)]
        assert not ctx.coop_gave_up()
        return s, ctx.programs(), ctx.path_info()
    finally:
        for k in envvars:
            os.environ.pop(k, None)


def _oracle(env, B, H, W, seed, guided=True):
    from oracle import rd_oracle_torch as OT
    x, t, lab, w = _inputs(B, H, W, seed)
    with torch.no_grad():
        if guided:
            return OT.cf_score(env['p64'], x.double(), t.double(), lab.double(), w.double()).numpy()
        return OT.ncsnpp_forward(env['p64'], x.double(), OT.sigma_of(t.double()), lab.double()).numpy()


def _proj(prog):
    """The attention projection ops of a program (the only dst_kind 3 convs)."""
    return [d for d in prog['ops'] if d.startswith('CONV ') and ' dst=3' in d]


def check_shapes(progs, progs_off, rows):
    """Folded inference programs hold one two-projection conv per attention block and sample slot and no Cout=192 conv; with the
    switches set the projections are the three-projection ops again and NOTHING else in the op list differs."""
    for q, q_off in zip(progs, progs_off):
        assert not q['train'] and (q['S'], q['coop']) == (q_off['S'], q_off['coop'])
        slots = 1 if q['coop'] else q['S']
        assert not any('Cout=192' in d for d in q['ops']), q['ops']
        assert len(_proj(q)) == len(ATTN) * slots, q['ops']
        assert all(d.startswith(f'CONV rows={rows} ') and ' K=1x64(+0) Cout=128 dst=3' in d for d in _proj(q)), _proj(q)
        assert len(_proj(q_off)) == len(ATTN) * slots and all(' K=1x64(+0) Cout=192 dst=3' in d for d in _proj(q_off)), _proj(q_off)
        assert [d.replace(' Cout=128 dst=3', ' Cout=192 dst=3') for d in q['ops']] == q_off['ops']
    assert len(progs) == len(progs_off) and progs


CASES = [(2, 9, 9, {}, True), (2, 8, 9, {}, True), (3, 9, 9, {}, True), (2, 9, 9, {'RDMI_COOP': '0'}, True),
         (2, 9, 9, {'RDMI_S_MIN_WG': '1', 'RDMI_COOP': '0', 'RDMI_S': '2'}, False)]
IDS = ['9x9-coop-group', '8x9-coop-group', '9x9-ragged-group', '9x9-single-sample', '9x9-two-per-workgroup']


@pytest.mark.parametrize('B,H,W,base,guided', CASES, ids=IDS)
def test_folded_matches_unfolded_and_oracle(env, B, H, W, base, guided):
    """B = 2 with guidance is four forwards = one co-operative group; B = 3 is six = a full and a ragged group; RDMI_COOP=0 runs
    the S = 1 program; the last case two plain forwards as one workgroup of the S = 2 program."""
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
    d_ref, d_off, d_fold = np.abs(a - ref), np.abs(b - ref), np.abs(a - b)
    print(f'folded vs oracle {d_ref.max():.3e} ({d_ref.max() / TOL:.3f} of the bound), three projections vs oracle {d_off.max():.3e}, '
          f'folded vs three projections {d_fold.max():.3e} ({d_fold.max() / TOL:.3f} of the bound), bit-equal: {np.array_equal(a, b)}')
    assert d_ref.max() <= TOL, float(d_ref.max())
    assert d_off.max() <= TOL, float(d_off.max())
    assert d_fold.max() <= TOL, float(d_fold.max())


def gamma(n):
    u = n * 2.0 ** -24
    return u / (1 - u)


def check_pack(ctx, params):
    """The device-packed q' | v' blocks, read back, against float64 numpy: per element within gamma_64 * sum|a||b| of the exact
    product (64-term fma chains), the v' half identical to the three-projection packing's."""
    C = 64
    for a in ATTN:
        Wq, Wk, bq = (params[a + s].astype(np.float64) for s in ('.NIN_0.W', '.NIN_1.W', '.NIN_0.b'))       # NIN weights are [in][out]
        Wv, W3, bv = (params[a + s].astype(np.float64) for s in ('.NIN_2.W', '.NIN_3.W', '.NIN_2.b'))
        got = ctx.packed(a + '.qv2f', 2 * C * C).cpu().numpy().reshape(C // 16, 2 * C, 16)                  # [K/16][N][16]
        mat = got.transpose(0, 2, 1).reshape(C, 2 * C)                                                        # [ci][co]
        bias = ctx.packed(a + '.bqvf', 2 * C).cpu().numpy()
        worst = 0.0
        for have, want, bound in ((mat[:, :C], Wq @ Wk.T, np.abs(Wq) @ np.abs(Wk).T), (bias[:C], bq @ Wk.T, np.abs(bq) @ np.abs(Wk).T),
                                  (mat[:, C:], Wv @ W3, np.abs(Wv) @ np.abs(W3)), (bias[C:], bv @ W3, np.abs(bv) @ np.abs(W3))):
            err = np.abs(have.astype(np.float64) - want)
            assert (err <= gamma(C) * bound).all(), (a, float((err / (gamma(C) * bound)).max()))
            worst = max(worst, float((err / (gamma(C) * bound)).max()))
        old = ctx.packed(a + '.qkv3f', 3 * C * C).cpu().numpy().reshape(C // 16, 3 * C, 16)
        assert np.array_equal(got[:, C:, :], old[:, 2 * C:, :])
        assert np.array_equal(bias[C:], ctx.packed(a + '.bqkvf', 3 * C).cpu().numpy()[2 * C:])
        print(f'{a}: largest packed-product error {worst:.3f} of gamma_64 * sum|a||b|')


def test_packed_products(env):
    model, _, _ = env['ge'].make_model('cpu')
    ctx = model.native_context(2, 9, 9, 'cpu')
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    with torch.no_grad():          # any forward repacks
        mutils.get_score_fn(sde_lib.RVESDE(0.01, 5, N=1000), model)(torch.rand(1, 1, 9, 9), torch.tensor([0.5]), class_labels=torch.rand(1, 1))
    check_pack(ctx, env['params'])


def test_unfolded_context_carries_no_folded_block(env):
    """Only contexts that build a k-folded program pack q' | v'."""
    os.environ.update(OFF)
    try:
        model, _, _ = env['ge'].make_model('cpu')
        ctx = model.native_context(2, 9, 9, 'cpu')
        with pytest.raises(Exception):
            ctx.packed(ATTN[0] + '.qv2f', 16)
    finally:
        for k in OFF:
            os.environ.pop(k, None)


def test_training_program_keeps_three_projections(env):
    """The training forward's op list does not depend on the switches: Cout=192 projections, the nine-tap input conv, the
    one-column output conv."""
    lists = []
    for envvars in ({}, OFF):
        os.environ.update(envvars)
        try:
            model, _, _ = env['ge'].make_model('cpu')
            progs = model.train_context(2, 9, 9, 'cpu').programs()
        finally:
            for k in envvars:
                os.environ.pop(k, None)
        tr = [q for q in progs if q['train']]
        assert len(tr) == 1
        ops = tr[0]['ops']
        assert len(_proj(tr[0])) == len(ATTN) and all(' K=1x64(+0) Cout=192 dst=3' in d for d in _proj(tr[0])), ops
        assert any(' K=9x16(+0) Cout=64 ' in d for d in ops) and any(' K=9x64(+0) Cout=1 dst=2' in d for d in ops), ops
        assert not any('Cout=128 dst=3' in d for d in ops)
        lists.append(ops)
        inf = [q for q in progs if not q['train']]
        assert inf and all(len(_proj(q)) and all((' Cout=192 ' in d) == bool(envvars) for d in _proj(q)) for q in inf)
    assert lists[0] == lists[1]
