"""Ownership of device memory, on the CPU emulator (tests/emu): the emulator counts live hipMalloc / hipHostMalloc blocks and can
make the k-th allocation fail.  Every block a context, its training plan and its fused programs allocate is released by
rdmi_destroy, also when rdmi_create or rdmi_enable_training fails part-way."""
import ctypes as C
import gc

import pytest
import torch


@pytest.fixture(scope='module')
def shim(emu):
    lib = emu.lib()
    lib.rdmi_emu_live_blocks.argtypes, lib.rdmi_emu_live_blocks.restype = [], C.c_long
    lib.rdmi_emu_fail_alloc.argtypes, lib.rdmi_emu_fail_alloc.restype = [C.c_long], None
    gc.collect()
    gc.disable()                 # no context of another test may be collected while blocks are counted
    yield lib
    gc.enable()


@pytest.fixture(scope='module')
def models():
    import __graft_entry__ as ge
    from tests.test_emu_tiled_train import _small_rgb_model
    m9, _, _ = ge.make_model('cpu')
    rgb, _, _ = _small_rgb_model(ge)
    return {'9x9': (m9, 9, 9), 'tiled': (rgb, 16, 16)}


def _context(emu, model, H, W):
    ctx = emu.Context(model._arch(), 2, H, W, 'cpu')
    ctx.bind(model._named_tensors())
    return ctx


def _train_step(ctx, model, H, W):
    x = torch.rand(1, model.channels, H, W)
    out = torch.empty_like(x)
    ctx.train_forward(x, torch.tensor([0.4]), torch.zeros(1, 1), out, 0.1, 5)
    grads = torch.empty(sum(p.numel() for p in model.parameters()))
    ctx.backward(torch.randn_like(x), grads, x)
    assert torch.isfinite(out).all() and torch.isfinite(grads).all()


def _failing(shim, k, fn):
    """fn() with the k-th allocation it makes failing."""
    shim.rdmi_emu_fail_alloc(k)
    try:
        return fn()
    finally:
        shim.rdmi_emu_fail_alloc(-1)


def _fail_each_allocation(call):
    """call(k) for k = 0, 1, 2, ... until a call succeeds (it makes fewer than k + 1 allocations).  -> that k"""
    k = 0
    while call(k) != 0:
        k += 1
    return k


def test_destroy_releases_every_block(emu, shim, models):
    base = shim.rdmi_emu_live_blocks()
    m, H, W = models['9x9']
    ctx = _context(emu, m, H, W)
    assert shim.rdmi_emu_live_blocks() > base
    o = emu.PcOpts()
    o.N, o.eps, o.sigma_min, o.sigma_max, o.seed = 2, 1e-5, 0.01, 5.0, 7
    ctx.pc_sample(torch.rand(1, 1, H, W), torch.zeros(1, 1), None, None, None, None, o)     # the sampler's resizable buffers
    ctx.close()
    assert shim.rdmi_emu_live_blocks() == base
    m, H, W = models['tiled']
    ctx = _context(emu, m, H, W)
    ctx.enable_training()
    _train_step(ctx, m, H, W)
    ctx.close()
    assert shim.rdmi_emu_live_blocks() == base


def test_create_failing_at_every_allocation(emu, shim, models):
    base = shim.rdmi_emu_live_blocks()
    m, H, W = models['9x9']
    arch = m._arch()

    def create(k):
        h = C.c_void_p()
        rc = _failing(shim, k, lambda: shim.rdmi_create(C.byref(arch), 2, H, W, C.byref(h)))
        if rc == 0:
            shim.rdmi_destroy(h)
        else:
            assert not h.value and shim.rdmi_last_error(), k
        assert shim.rdmi_emu_live_blocks() == base, k
        return rc
    assert _fail_each_allocation(create) > 10


@pytest.mark.parametrize('name', ['9x9', 'tiled'])
def test_enable_training_failing_at_every_allocation(emu, shim, models, name):
    base = shim.rdmi_emu_live_blocks()
    m, H, W = models[name]

    def enable(k):
        ctx = _context(emu, m, H, W)
        rc = _failing(shim, k, lambda: shim.rdmi_enable_training(ctx._h))
        assert rc == 0 or shim.rdmi_last_error(), k
        ctx.close()
        assert shim.rdmi_emu_live_blocks() == base, k
        return rc
    assert _fail_each_allocation(enable) > 10


def test_enable_training_again_after_a_failure(emu, shim, models):
    """A 9x9 (fp32 layer plan) context whose rdmi_enable_training failed half-way enables training on the next call and runs a
    training step; rdmi_destroy then releases every block."""
    base = shim.rdmi_emu_live_blocks()
    m, H, W = models['9x9']
    ctx = _context(emu, m, H, W)
    assert _failing(shim, 20, lambda: shim.rdmi_enable_training(ctx._h)) != 0
    ctx.enable_training()
    _train_step(ctx, m, H, W)
    ctx.close()
    assert shim.rdmi_emu_live_blocks() == base
