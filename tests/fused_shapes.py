"""Shape and architecture matrix of the workgroup-resident ("fused") U-Net (kernel csrc/unet_kernel.h, planned by csrc/fused_plan.h)
off the shipped GTO-Halo model: shared check functions, run on the CPU emulator by tests/test_emu_fused_shapes.py and on an MI355X by
tests/test_gpu_fused_shapes.py.  tests/fused_programs.py pins the op lists of such architectures; this module RUNS them, every
inference program the planner builds, against oracle/rd_oracle_torch.cf_score with float64 parameters and inputs.

All models have one image channel and are conditional; seeded synthetic weights (oracle/weights.py).  Each shape is the smallest that
reaches the edges named beside it:

F1  9x9, nf 64, ch_mult (1,1,2), two res blocks, attention at 4x4
      a single-sample C = 64 conv with a fused GroupNorm on 16 rows (one row tile for WM = 2 waves along M: the wave without a tile parks
      no partial sums); attention over 16 positions inside a per-sample section; S = 2 and S = 4 refused, the co-operative program built.
F2  4x8 (H x W), nf 32, ch_mult (1,1), two res blocks, no attention
      32-channel convs and 8-group GroupNorms (WN = 2, WM = 4 over two row tiles); H != W; no level of 4 pixels: no co-operative program.
F3  8x8, nf 64, ch_mult (1,1,2), one res block, no attention
      the co-operative program's per-sample 4x4 level at C = 64.
F4  9x9, nf 64, ch_mult (1,2), two res blocks, attention at 9x9
      two levels: the S = 2 and S = 4 programs' multi-sample section is the bottleneck level alone; no co-operative program.
F5  4x4, nf 128, ch_mult (1,1), one res block, no attention
      Cout 128 and 256 (16 column tiles), unfused GroupNorms with 8-channel groups, multi-sample and co-operative programs on a 16-row
      top level.
F6  8x8, nf 64, ch_mult (1,1,1), one res block, attention at 8x8
      attention over 64 positions; C = 64 on the multi-sample 4x4 and 2x2 levels; the co-operative program refused by its conv shape.
F7  8x8, the shipped channels (nf 64, ch_mult (1,2,2), attention at level 0) with three res blocks
      117 ops: the LDS arena and the spill-slot replay over more blocks than the shipped model has.
SHIP  the shipped model at 9x9: the planner switches only (RDMI_NO_GNFUSE, RDMI_NO_ATTN_FOLD, RDMI_NO_QKV1).

Programs are chosen as tests/test_emu_fold9.py and tests/test_gpu_upfold.py choose them: RDMI_S_MIN_WG=1 lets the S = 2 / S = 4 programs
exist at max_batch 16, RDMI_S caps S, RDMI_COOP=0 leaves the co-operative program out; the batch decides between what is left
(FusedPlan::pick, restated by `picked` over rdmi_path_info).  A guided score of B samples is 2B network evaluations.

Bounds: the ones the project states for this forward -- 5e-5 absolute on the emulator (tests/test_emu_upfold.py, test_emu_parity.py),
2e-4 on the card (tests/test_gpu_upfold.py) -- times max(1, max |ref64|) of the sample (as TAP_TOL in tests/tiled_shapes.py: these
models' scores reach about 4).  The switch comparisons use the same bound; the repeated-context comparison is exact equality."""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import torch

from tests.fused_programs import MAX_PROGRAMS, SWITCHES

SHAPES = {
    'F1': dict(H=9, W=9, nf=64, ch_mult=(1, 1, 2), nrb=2, attn=(4,)),
    'F2': dict(H=4, W=8, nf=32, ch_mult=(1, 1), nrb=2, attn=()),
    'F3': dict(H=8, W=8, nf=64, ch_mult=(1, 1, 2), nrb=1, attn=()),
    'F4': dict(H=9, W=9, nf=64, ch_mult=(1, 2), nrb=2, attn=(9,)),
    'F5': dict(H=4, W=4, nf=128, ch_mult=(1, 1), nrb=1, attn=()),
    'F6': dict(H=8, W=8, nf=64, ch_mult=(1, 1, 1), nrb=1, attn=(8,)),
    'F7': dict(H=8, W=8, nf=64, ch_mult=(1, 2, 2), nrb=3, attn=(8,)),
    'SHIP': dict(H=9, W=9, nf=64, ch_mult=(1, 2, 2), nrb=2, attn=(9,)),
}
SMIN, SMAX = 0.01, 5.0
TOL = {'cpu': 5e-5, 'cuda': 2e-4}

# ---- programs: (S, co-operative) and the environment that makes FusedPlan::pick take it -----------------------------------------
PROGRAMS = {
    's1': ((1, False), {'RDMI_S_MIN_WG': '1', 'RDMI_S': '1'}),
    's2': ((2, False), {'RDMI_S_MIN_WG': '1', 'RDMI_S': '2', 'RDMI_COOP': '0'}),
    's4': ((4, False), {'RDMI_S_MIN_WG': '1', 'RDMI_S': '4', 'RDMI_COOP': '0'}),
    'coop': ((4, True), {'RDMI_S_MIN_WG': '1'}),
}
# What the planner builds per shape with every program asked for (RDMI_S_MIN_WG=1 alone), and the reason it gives for each one it
# refuses.  A planner change that drops or adds a program fails check_plan; it does not just shrink the forward coverage.
S_LOW_ATTN = 'attention inside the multi-sample (low-resolution) section is not built'
S_ODD_GRID = 'multi-sample ops need a power-of-two pixel count'
COOP_NO_LEVEL = 'no level of exactly 4 pixels per sample: nothing to share'
PLAN = {
    'F1': dict(built=('s1', 'coop'), refused={'s2': S_LOW_ATTN, 's4': S_LOW_ATTN}),
    'F2': dict(built=('s1', 's2', 's4'), refused={'coop': COOP_NO_LEVEL}),
    'F3': dict(built=('s1', 's2', 's4', 'coop'), refused={}),
    'F4': dict(built=('s1', 's2', 's4'), refused={'coop': COOP_NO_LEVEL}),
    'F5': dict(built=('s1', 's2', 's4', 'coop'), refused={}),
    'F6': dict(built=('s1', 's2', 's4'), refused={'coop': 'co-operative conv shape (Cout 64, 1 row tiles, 4 chunks)'}),
    'F7': dict(built=('s1', 's2', 's4', 'coop'), refused={}),
    'SHIP': dict(built=('s1', 's2', 's4', 'coop'), refused={}),
}
N_OPS = {'F7': 117}          # ops of the S = 1 program where the shape is there for its length

# The forward cases: (program, B).  Every program of PLAN[...]['built'] runs; B = 3 (six evaluations) is the ragged batch of each shape:
# a full group of four and a remainder of two under S = 4 or under the co-operative program.
FORWARD = {
    'F1': (('s1', 1), ('coop', 3)),
    'F2': (('s1', 2), ('s2', 2), ('s4', 3)),
    'F3': (('s1', 1), ('s2', 1), ('s4', 2), ('coop', 3)),
    'F4': (('s1', 1), ('s2', 2), ('s4', 3)),
    'F5': (('s1', 2), ('s2', 2), ('s4', 3), ('coop', 3)),
    'F6': (('s1', 1), ('s2', 2), ('s4', 3)),
    'F7': (('s1', 1), ('s2', 1), ('s4', 2), ('coop', 3)),
}
FORWARD_CASES = [(n, p, B) for n, cs in FORWARD.items() for p, B in cs]
# The switch runs: RDMI_NO_GNFUSE at every shape, the attention switches where there is attention off the shipped model, all three at
# the shipped model; each against the oracle AND against the run without the switch, on the (program, B) named here.
SWITCH_BASE = {'F1': ('s1', 1), 'F2': ('s2', 2), 'F3': ('coop', 3), 'F4': ('s2', 2), 'F5': ('coop', 3), 'F6': ('s2', 2), 'F7': ('s1', 1),
               'SHIP': ('coop', 2)}
SWITCH_CASES = ([(n, 'RDMI_NO_GNFUSE') for n in SWITCH_BASE]
                + [(n, sw) for n in ('F1', 'F6', 'SHIP') for sw in ('RDMI_NO_ATTN_FOLD', 'RDMI_NO_QKV1')])
# The repeated-context cases: the single-sample fused GroupNorm read partial-sum slots that no wave of a short conv wrote, i.e. whatever
# earlier work left in LDS -- a run can then pass by luck.  Same context, other preceding work, the same bits.
REPEAT_CASES = [('F1', 's1', 1), ('F2', 's2', 2), ('F3', 'coop', 3)]


def attn_levels(name):
    s = SHAPES[name]
    return tuple(s['H'] // 2 ** i in s['attn'] for i in range(len(s['ch_mult'])))


@functools.lru_cache(maxsize=None)
def params_of(name):
    from oracle.weights import make_params
    s = SHAPES[name]
    return make_params(7, nf=s['nf'], ch_mult=s['ch_mult'], num_res_blocks=s['nrb'], attn_resolutions=s['attn'], image_size=s['H'], channels=1)


def make_model(name, dev):
    """The model of shape `name` on `dev`, eval mode: built as tiled_shapes.make_model builds its models."""
    import __graft_entry__ as ge
    from rdmi.models import utils as mutils
    s = SHAPES[name]
    cfg = ge.demo_config(image_size=s['H'], image_width=s['W'])
    m = cfg.model
    m.nf, m.ch_mult, m.num_res_blocks, m.attn_resolutions = s['nf'], list(s['ch_mult']), s['nrb'], list(s['attn'])
    assert m.channels == 1 and m.conditional and not m.scale_by_sigma and cfg.sde.sigma_max == SMAX
    model = mutils.create_model(cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params_of(name).items()}, strict=True)
    return model.to(dev).eval()


@contextlib.contextmanager
def environment(env):
    """Every switch the planners read at create cleared, then `env` (contexts read them when they are created)."""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def programs(ctx):
    """(S, co-operative) of every INFERENCE program the context holds.  (Context.programs() stops at the first index the library
    answers -1 for, which is a refused program as well as the end of the list: F1's co-operative program sits behind two refused ones.)"""
    from rdmi import _native
    out = []
    for i in range(MAX_PROGRAMS + 1):
        S, coop, train = C.c_int(), C.c_int(), C.c_int()
        n = _native.lib().rdmi_debug_program(ctx._h, i, C.byref(S), C.byref(coop), C.byref(train), None, 0)
        if n >= 0 and not train.value:
            out.append((S.value, bool(coop.value), n))
    return out


def picked(info, NB):
    """FusedPlan::pick over what rdmi_path_info reports: the co-operative program up to its batch limit unless disabled, otherwise
    the program with the most samples per workgroup whose first batch NB reaches."""
    assert info.startswith('fused: workgroup-resident U-Net'), info
    m = re.search(r'co-operative groups of 4 workgroups up to batch (\d+) \(([^)]*)\)', info)
    if m and 'disabled' not in m.group(2) and NB <= int(m.group(1)):
        return (4, True)
    return (max([1] + [int(S) for S, frm in re.findall(r'S=(\d+) samples/workgroup from batch (\d+)', info) if NB >= int(frm)]), False)


def check_plan(name, dev):
    """The programs the planner builds for the shape and the reason it states for each one it refuses."""
    from rdmi import _native
    s, want = SHAPES[name], PLAN[name]
    with environment({'RDMI_S_MIN_WG': '1'}):
        model = make_model(name, dev)
        ctx = model.native_context(2, s['H'], s['W'], dev)
    assert ctx.max_batch == 16
    info, progs = ctx.path_info(), programs(ctx)
    print(f'fused shapes plan {name} on {dev}: {info}')
    assert sorted(p[:2] for p in progs) == sorted(PROGRAMS[p][0] for p in want['built']), (name, progs, info)
    for p, why in want['refused'].items():
        S = PROGRAMS[p][0][0]         # (a refused co-operative program is reported as its S = 4: the text tests/golden/fused_programs.json pins)
        assert f'; S={S} unavailable ({why})' in info, (name, p, info)
    assert info.count('unavailable') == len(want['refused']), info
    if name in N_OPS:
        assert [n for S, coop, n in progs if (S, coop) == (1, False)] == [N_OPS[name]], progs
    assert not _native.is_emulator() or str(dev) == 'cpu'


# ---- the guided score ----------------------------------------------------------------------------------------------------------
def cf_inputs(name, B):
    """Distinct times across the schedule, random labels, guidance weights including 0 from B = 2 on."""
    s = SHAPES[name]
    g = torch.Generator().manual_seed(100 + B)
    x = torch.rand(B, 1, s['H'], s['W'], generator=g)
    lab = torch.rand(B, 1, generator=g)
    return x, lab, torch.tensor([0.6, 0.0, 1.5, 0.3][:B]), torch.tensor([0.15, 0.85, 0.5, 0.97][:B])


@functools.lru_cache(maxsize=None)
def cf_ref64(name, B):
    """float64 oracle, once per shape and input."""
    from oracle import rd_oracle_torch as OT
    s = SHAPES[name]
    p64 = {k: torch.from_numpy(v.copy()).double() for k, v in params_of(name).items()}
    x, lab, w, t = cf_inputs(name, B)
    with torch.no_grad():
        return OT.cf_score(p64, x.double(), t.double(), lab.double(), w.double(), smax=SMAX, ch_mult=s['ch_mult'], nrb=s['nrb'],
                           attn_levels=attn_levels(name))


def _score(model, name, prog, B, dev, scale=1.0):
    """One guided score of the case's inputs (x scaled by `scale`) on `model`, with the asserts that `prog` exists and was taken."""
    from rdmi import sde_lib
    from rdmi.models import utils as mutils
    s = SHAPES[name]
    x, lab, w, t = (a.to(dev) for a in cf_inputs(name, B))
    with torch.no_grad():
        out = mutils.get_cf_score_fn(sde_lib.RVESDE(SMIN, SMAX, N=1000), model, lab, w)(x * scale, t)
    ctx = model._ctx[(str(torch.device(dev)), s['H'], s['W'])]
    assert not ctx.coop_gave_up()
    info, want = ctx.path_info(), PROGRAMS[prog][0]
    assert want in [p[:2] for p in programs(ctx)], (name, prog, info)
    assert picked(info, 2 * B) == want, (name, prog, B, info)
    return out.cpu()


@functools.lru_cache(maxsize=None)
def cf_score(name, prog, B, dev, switch=None):
    """The guided score of a fresh context through program `prog` (cached: the switch and repeated-context checks compare with it)."""
    with environment(dict(PROGRAMS[prog][1], **({switch: '1'} if switch else {}))):
        return _score(make_model(name, dev), name, prog, B, dev)


def errs(a, ref):
    """max |a - ref| per sample, in units of the sample's bound max(1, max |ref|)."""
    return [float((a[n].double() - ref[n].double()).abs().max() / max(1.0, float(ref[n].abs().max()))) for n in range(ref.shape[0])]


def check_forward(name, prog, B, dev, switch=None):
    s, ref = cf_score(name, prog, B, dev, switch), cf_ref64(name, B)
    assert s.shape == ref.shape
    tol = TOL[torch.device(dev).type]
    e = errs(s, ref)
    print(f'fused shapes forward {name} {prog} B={B}{" " + switch if switch else ""} on {dev}: max |ref64| {float(ref.abs().max()):.2f}, '
          f'max |s - ref64| / max(1, max |ref64|) per sample ' + ' '.join(f'{v:.2e}' for v in e) + f' (bound {tol:.0e})')
    assert bool(torch.isfinite(s).all()), (name, prog, B, switch)
    assert max(e) <= tol, (name, prog, B, switch, e)
    return s


def check_switch(name, switch, dev):
    """The run with the planner switch set: against the oracle, and against the run without it under the same bound."""
    prog, B = SWITCH_BASE[name]
    a = check_forward(name, prog, B, dev, switch)
    b = check_forward(name, prog, B, dev)
    ref = cf_ref64(name, B)
    e = [float((a[n].double() - b[n].double()).abs().max() / max(1.0, float(ref[n].abs().max()))) for n in range(B)]
    print(f'fused shapes switch {name} {switch} on {dev}: against the run without it ' + ' '.join(f'{v:.2e}' for v in e)
          + f', bit-equal: {bool(torch.equal(a, b))}')
    assert max(e) <= TOL[torch.device(dev).type], (name, switch, e)


def check_repeat(name, prog, B, dev):
    """One context, two launches: a batch with inputs scaled by 50, then the test batch.  The second result equals a fresh context's
    bit for bit -- nothing a launch reads may be left over from the work before it."""
    fresh = check_forward(name, prog, B, dev)
    with environment(PROGRAMS[prog][1]):
        model = make_model(name, dev)
        big = _score(model, name, prog, B, dev, scale=50.0)
        again = _score(model, name, prog, B, dev)
    assert not torch.equal(big, fresh)
    d = float((again.double() - fresh.double()).abs().max())
    print(f'fused shapes repeated context {name} {prog} B={B} on {dev}: max |second launch - fresh context| {d:.2e}')
    assert torch.equal(again, fresh), (name, prog, d)


# ---- training forward at F3 -----------------------------------------------------------------------------------------------------
def train_inputs(name):
    s = SHAPES[name]
    g = torch.Generator().manual_seed(23)
    x = torch.rand(2, 1, s['H'], s['W'], generator=g)
    return x, torch.tensor([0.7, 3.0]), torch.rand(2, 1, generator=g), torch.randn(2, 1, s['H'], s['W'], generator=g)


def check_training_forward(name, dev):
    """The fused training program (S = 1 ops + a stash of every layer output) against the layer plan's forward (RDMI_TRAIN_FUSED=0) as
    test_training_forward_fused_equals_layer_plan does at the shipped model, and output and parameter gradients against float64
    autograd through the oracle under the bound of tests/test_emu_tiled_train.py."""
    from oracle import rd_oracle_torch as OT
    from tests import test_emu_tiled_train as TT
    s = SHAPES[name]
    x, sigma, lab, gout = train_inputs(name)

    def run(env):
        with environment(env):
            model = make_model(name, dev).train()
            model.dropout, model.cond_drop_prob = 0.0, 0.0
            out = model(x.to(dev), sigma.to(dev), lab.to(dev))
            out.backward(gout.to(dev))
            info = model._ctx[('train', str(torch.device(dev)), s['H'], s['W'])].path_info()
        return out.detach().cpu(), {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters() if p.requires_grad}, info
    oa, ga, ia = run({})
    ob, gb, ib = run({'RDMI_TRAIN_FUSED': '0'})
    assert 'training forward: fused program' in ia and 'training forward' not in ib, (ia, ib)
    p64 = {k: torch.from_numpy(v.copy()).double().requires_grad_(k in ga) for k, v in params_of(name).items()}
    ref = OT.ncsnpp_forward(p64, x.double(), sigma.double(), lab.double(), ch_mult=s['ch_mult'], nrb=s['nrb'], attn_levels=attn_levels(name))
    gr = torch.autograd.grad(ref, [p64[n] for n in ga], gout.double())
    gref = {n: g.numpy() for n, g in zip(ga, gr)}
    ref = ref.detach()
    tol = TOL[torch.device(dev).type]
    ea, eb = errs(oa, ref), errs(ob, ref)
    worst = max(np.linalg.norm(ga[n].astype(np.float64) - gref[n]) / np.linalg.norm(gref[n]) for n in ga if not n.endswith('NIN_1.b'))
    print(f'fused shapes training forward {name} on {dev}: fused program vs float64 ' + ' '.join(f'{v:.2e}' for v in ea)
          + ', layer plan vs float64 ' + ' '.join(f'{v:.2e}' for v in eb) + f'; worst parameter gradient ||g - g64|| / ||g64|| {worst:.2e}')
    assert max(ea) <= tol and max(eb) <= tol, (ea, eb)
    for n in ga:                     # fused program against the layer plan: the bound of test_training_forward_fused_equals_layer_plan
        assert np.abs(ga[n] - gb[n]).max() <= 2e-4 * np.abs(gb[n]).max() + 1e-7, n
    TT._check(ga, gref)
