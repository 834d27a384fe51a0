"""The data-movement ops of the fused U-Net (csrc/unet_kernel.h) on the CPU emulator: the one-pass stand-alone GroupNorm (fop_gn:
every lane normalises the values it read for the statistics), the batched concat / resize gather (fop_gather) and the skip spill
(fop_store) whose tensors the gathers read back.  DESIGN 4.2h.  Every case is one guided score of B <= 3 samples (2B network evaluations) against the float64
torch oracle, on the program the case names; tests/test_gpu_memops.py runs the same cases on the device.

Shipped model (9x9, nf 64, ch_mult (1,2,2)):
  * B = 2 (one co-operative group of four evaluations) and B = 3 (a full and a ragged group) on the co-operative, the S = 1
    (RDMI_COOP=0) and the S = 2 program, selected as tests/test_emu_fold9.py selects them;
  * 8x9, B = 2: 72 rows -- lanes of a 16-lane group whose rows are clamped copies, masked out of the sums and not written;
  * RDMI_NO_GNFUSE=1, B = 2: all 40 GroupNorms of a forward are stand-alone ops, with 4-, 6- and 8-channel groups.
Shape matrix (tests/fused_shapes.py): F2 (4x8, nf 32), F5 (4x4, nf 128: un-fused 8-channel groups on a 16-row level, multi-sample
and co-operative programs), F4 (9x9, ch_mult (1,2)), every program the planner builds for them.

Bound: 5e-5 absolute on every element (the project's bound for this forward on the emulator, tests/test_emu_parity.py); on the device
2e-4 * max |score| on every element.  A second call on the same context returns the same bits."""
import numpy as np
import pytest
import torch

from tests import fused_shapes as FS
from tests import test_emu_fold9 as F9
from tests.test_emu_fold9 import env  # noqa: F401  (module-scoped fixture: emulator bound, shipped parameters in float32 and float64)

# program -> (what FusedPlan::pick must report, the environment that makes it the pick), as test_emu_fold9.CASES
SHIP_PROGRAMS = {
    'coop': ((4, True), {}),
    's1': ((1, False), {'RDMI_COOP': '0'}),
    's2': ((2, False), {'RDMI_S_MIN_WG': '1', 'RDMI_COOP': '0', 'RDMI_S': '2'}),
}
# (id, B, H, W, program, extra switches)
SHIP_CASES = ([(f'9x9-{p}-B{B}', B, 9, 9, p, {}) for p in SHIP_PROGRAMS for B in (2, 3)]
              + [('8x9-coop-B2', 2, 8, 9, 'coop', {}), ('9x9-coop-B2-nogn', 2, 9, 9, 'coop', {'RDMI_NO_GNFUSE': '1'})])
MATRIX_CASES = [(n, p, B) for n in ('F2', 'F5', 'F4') for p, B in FS.FORWARD[n]]


def ship_inputs(B, H, W):
    return F9._inputs(B, H, W, 60 + B + H)


def ship_score(ge, dev, B, H, W, prog, extra):
    """Two guided scores of the case on one fresh context of the shipped model, with the asserts on the program taken."""
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    x, t, lab, w = (a.to(dev) for a in ship_inputs(B, H, W))
    want, envvars = SHIP_PROGRAMS[prog]
    with FS.environment(dict(envvars, **extra)):
        model, _, _ = ge.make_model(dev)
        fn = mutils.get_cf_score_fn(sde_lib.RVESDE(0.01, 5, N=1000), model, lab, w)
        with torch.no_grad():
            a = fn(x, t).cpu().numpy()
            b = fn(x, t).cpu().numpy()
    ctx = model._ctx[(str(torch.device(dev)), H, W)]
    assert not ctx.coop_gave_up()
    info = ctx.path_info()
    assert FS.picked(info, 2 * B) == want, (prog, info)
    if prog == 's2':
        assert 'S=2 samples/workgroup from batch 2' in info, info
    else:
        assert ('co-operative groups' in info and 'disabled' not in info) == (prog == 'coop'), info
    if extra.get('RDMI_NO_GNFUSE'):
        ops = [q for q in ctx.programs() if not q['train'] and (q['S'], q['coop']) == want][0]['ops']
        gn = [d for d in ops if d.startswith('GN ')]
        assert not any('+GN' in d for d in ops) and len(gn) == 40, ops
        C = {int(d.split('C=')[1]) for d in gn}
        assert {c // min(c // 4, 32) for c in C} == {4, 6, 8}, C          # channels per group of the stand-alone ops
    return a, b


def ship_oracle(env, B, H, W):  # noqa: F811
    return F9._oracle(env, B, H, W, 60 + B + H)


_REF = {}


def ship_ref(env, B, H, W):  # noqa: F811
    """float64 oracle, once per input."""
    if (B, H, W) not in _REF:
        _REF[(B, H, W)] = ship_oracle(env, B, H, W)
    return _REF[(B, H, W)]


def check_ship(env, dev, tol_of, B, H, W, prog, extra):  # noqa: F811
    a, b = ship_score(env['ge'], dev, B, H, W, prog, extra)
    ref = ship_ref(env, B, H, W)
    tol = tol_of(ref)
    d = np.abs(a - ref)
    print(f'memops shipped {H}x{W} {prog} B={B} {extra} on {dev}: max |s - ref64| {d.max():.3e} (bound {tol:.3e}, max |ref64| {np.abs(ref).max():.3f}), '
          f'second call bit-equal: {np.array_equal(a, b)}')
    assert np.isfinite(a).all()
    assert d.max() <= tol, float(d.max())
    assert np.array_equal(a, b)


def check_matrix(dev, tol_of, name, prog, B):
    """A shape of the matrix through program `prog` (FS._score asserts the program exists, was picked and did not give up)."""
    with FS.environment(FS.PROGRAMS[prog][1]):
        model = FS.make_model(name, dev)
        a = FS._score(model, name, prog, B, dev).numpy()
        b = FS._score(model, name, prog, B, dev).numpy()
    ref = FS.cf_ref64(name, B).numpy()
    tol = tol_of(ref)
    d = np.abs(a - ref)
    print(f'memops matrix {name} {prog} B={B} on {dev}: max |s - ref64| {d.max():.3e} (bound {tol:.3e}, max |ref64| {np.abs(ref).max():.3f}), '
          f'second call bit-equal: {np.array_equal(a, b)}')
    assert np.isfinite(a).all()
    assert d.max() <= tol, float(d.max())
    assert np.array_equal(a, b)


def emu_tol(ref):
    return 5e-5


@pytest.mark.parametrize('B,H,W,prog,extra', [c[1:] for c in SHIP_CASES], ids=[c[0] for c in SHIP_CASES])
def test_shipped_model(env, B, H, W, prog, extra):  # noqa: F811
    check_ship(env, 'cpu', emu_tol, B, H, W, prog, extra)


@pytest.mark.parametrize('name,prog,B', MATRIX_CASES, ids=[f'{n}-{p}-B{B}' for n, p, B in MATRIX_CASES])
def test_shape_matrix(emu, name, prog, B):
    check_matrix('cpu', emu_tol, name, prog, B)
