"""The op lists of the workgroup-resident ("fused") programs (csrc/fused_plan.h) are the observable plan: this module pins them.  Shared
by tests/test_emu_fused_programs.py (CPU emulator) and tests/test_gpu_fused_programs.py (MI355X).  Contexts are created (and given a
training plan where a training program is asked for); nothing is run.

The fixture tests/golden/fused_programs.json was recorded from the commit BEFORE the planner moved into csrc/fused_plan.h, with the
emulator library of that commit:

    python tests/fused_programs.py --record

Per configuration it holds the rdmi_path_info string (which carries the `why` text of every program the planner refused) and, per
program that was built, its index, S, coop, train, op count and the SHA-256 of its op descriptions joined by newlines; for the shipped
configurations also the op lists themselves, so that a mismatch names the first differing op.

Every context has max_batch = 16 under RDMI_S_MIN_WG=1: the S = 2, S = 4 and co-operative programs all exist, and the co-operative
batch limit (min(max_batch, resident workgroups)) reads 16 on the emulator and on the card alike."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'fused_programs.json')
MAX_BATCH = 16
MAX_PROGRAMS = 5          # S = 1, 2, 4, co-operative, training: the builder makes no more (describe() asserts that no sixth exists)

# every switch the planners read at rdmi_create: a configuration sets the ones it names and clears the others
SWITCHES = ('RDMI_NO_GNFUSE', 'RDMI_NO_UP_FOLD', 'RDMI_NO_K_FOLD', 'RDMI_NO_ATTN_FOLD', 'RDMI_NO_QKV1', 'RDMI_COOP', 'RDMI_S',
            'RDMI_S_MIN_WG', 'RDMI_COOP_STRIDE', 'RDMI_STAMPS', 'RDMI_UDBG', 'RDMI_PATH', 'RDMI_DEBUG_TAPS', 'RDMI_TRAIN_FUSED',
            'RDMI_COOP_TEST_BREAK')

SHIPPED = dict(nf=64, ch_mult=(1, 2, 2), nrb=2, attn_levels=0b001, conditional=1, dtype=0, H=9, W=9, train=False, env={})


def _cfg(**kw):
    return {**SHIPPED, **kw}


CONFIGS = {
    'shipped_9x9': _cfg(),
    'shipped_8x9': _cfg(H=8),
    'train_f32_9x9': _cfg(train=True),
    'train_f32_8x9': _cfg(train=True, H=8),
    'train_bf16_9x9': _cfg(train=True, dtype=1),
    'train_bf16_8x9': _cfg(train=True, dtype=1, H=8),
    'no_gnfuse': _cfg(env={'RDMI_NO_GNFUSE': '1'}),
    'no_up_fold': _cfg(env={'RDMI_NO_UP_FOLD': '1'}),
    'no_k_fold': _cfg(env={'RDMI_NO_K_FOLD': '1'}),
    'no_attn_fold': _cfg(env={'RDMI_NO_ATTN_FOLD': '1'}),
    'no_qkv1': _cfg(env={'RDMI_NO_QKV1': '1'}),
    'coop_0': _cfg(env={'RDMI_COOP': '0'}),
    's_1': _cfg(env={'RDMI_S': '1'}),
    # architectures off the shipped one (the plan only)
    'levels_1': _cfg(ch_mult=(1,)),
    'levels_2': _cfg(ch_mult=(1, 2)),
    'nf_32': _cfg(nf=32, ch_mult=(1, 1), attn_levels=0, H=4, W=8),      # 32-channel convs and GroupNorms (8 groups), S = 1 / 2 / 4; no level of 4 pixels: the co-operative `why`
    'nf_32_9x9': _cfg(nf=32, attn_levels=0),                    # the layer plan refuses it (32 output columns over 81 pixels): the error text is recorded
    'no_attention': _cfg(attn_levels=0),
    'attention_low_level': _cfg(ch_mult=(1, 1, 2), attn_levels=0b010),      # C = 64 at the 4x4 level: the multi-sample programs refuse it
    'unconditional': _cfg(conditional=0),
}
FULL_LISTS = ('shipped_9x9', 'shipped_8x9')


@contextlib.contextmanager
def _environment(env):
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ['RDMI_S_MIN_WG'] = '1'
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def describe(name, dev):
    """Create the context of configuration `name` on `dev` and return what the fixture records for it."""
    from rdmi import _native
    cfg = CONFIGS[name]
    a = _native.Arch()
    a.nf, a.n_levels, a.num_res_blocks, a.attn_levels = cfg['nf'], len(cfg['ch_mult']), cfg['nrb'], cfg['attn_levels']
    for i, v in enumerate(cfg['ch_mult']):
        a.ch_mult[i] = v
    a.channels, a.num_classes, a.conditional, a.scale_by_sigma, a.compute_dtype = 1, 1, cfg['conditional'], 0, cfg['dtype']
    rec = dict(error=None, path_info=None, programs=[])
    ctx = None
    try:
        with _environment(cfg['env']):
            try:
                ctx = _native.Context(a, MAX_BATCH, cfg['H'], cfg['W'], dev)
                if cfg['train']:
                    ctx.enable_training()
            except RuntimeError as e:
                rec['error'] = str(e)
                return rec
        rec['path_info'] = ctx.path_info()
        lib = _native.lib()
        for i in range(MAX_PROGRAMS + 1):      # rdmi_debug_program answers -1 for a program that was refused as for one past the end
            S, coop, train = C.c_int(), C.c_int(), C.c_int()
            desc = (C.c_char_p * 512)()
            n = lib.rdmi_debug_program(ctx._h, i, C.byref(S), C.byref(coop), C.byref(train), desc, 512)
            if n < 0:
                continue
            assert i < MAX_PROGRAMS, f'{name}: a program at index {i}: raise MAX_PROGRAMS'
            assert n <= 512, n
            ops = [desc[k].decode() for k in range(n)]
            p = dict(index=i, S=S.value, coop=bool(coop.value), train=bool(train.value), n_ops=n,
                     sha256=hashlib.sha256('\n'.join(ops).encode()).hexdigest())
            if name in FULL_LISTS:
                p['ops'] = ops
            rec['programs'].append(p)
    finally:
        if ctx is not None:
            ctx.close()
    return rec


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def check(name, dev):
    got, want = describe(name, dev), fixture()[name]
    assert got['error'] == want['error'], (name, got['error'], want['error'])
    assert got['path_info'] == want['path_info'], f'{name}: rdmi_path_info\n  now:      {got["path_info"]}\n  recorded: {want["path_info"]}'
    head = lambda ps: [(p['index'], p['S'], p['coop'], p['train']) for p in ps]
    assert head(got['programs']) == head(want['programs']), (name, head(got['programs']), head(want['programs']))
    for g, w in zip(got['programs'], want['programs']):
        tag = f'{name} program {g["index"]} (S={g["S"]} coop={g["coop"]} train={g["train"]})'
        if 'ops' in w:
            for k, (x, y) in enumerate(zip(g['ops'], w['ops'])):
                assert x == y, f'{tag}: first differing op {k}: now {x!r}, recorded {y!r}'
        assert g['n_ops'] == w['n_ops'], f'{tag}: {g["n_ops"]} ops, recorded {w["n_ops"]}'
        assert g['sha256'] == w['sha256'], f'{tag}: op descriptions differ from the recorded ones'


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: python tests/fused_programs.py --record     (with the tree of the commit to record from)')
    for p in (ROOT, os.path.join(ROOT, 'optimized-diffusion-model_amd')):
        sys.path.insert(0, p)
    from rdmi import _native
    from tests.emu.build_emu import build
    _native.use_library(build())
    out = {name: describe(name, 'cpu') for name in CONFIGS}
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    for name, r in out.items():
        print(name, r['error'] or [(p['index'], p['S'], p['coop'], p['train'], p['n_ops']) for p in r['programs']])
