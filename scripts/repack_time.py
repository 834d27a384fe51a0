"""Host-side plan cost on the GPU, one JSON line: rdmi_create + bind + first rdmi_repack of the shipped 9x9 model (5 contexts, max_batch 256),
rdmi_repack after rebinding one parameter (out_conv.bias, 10 times per context), and create + rdmi_enable_training + first repack.

    python scripts/repack_time.py [ROOT]      ROOT: the checkout to measure (default: this one); an A/B alternates two checkouts,
                                              one process per line (profiles/fused_plan_bench_ab.json)"""
import ctypes as C, json, os, statistics, sys, time
tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
os.chdir(tree)
sys.path.insert(0, tree)
import torch
import __graft_entry__ as ge
ge.build()
from rdmi import _native
dev = torch.device('cuda:0')
model, cfg, _ = ge.make_model(dev)
named = model._named_tensors()
torch.cuda.synchronize()
lib = _native.lib()
def create(train):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    ctx = _native.Context(model._arch(), 256, 9, 9, dev)
    if train:
        ctx.enable_training()
    ctx.bind(named)
    _native.check(lib.rdmi_repack(ctx._h, None))
    torch.cuda.synchronize()
    return ctx, (time.perf_counter() - t0) * 1e3
ctx, _ = create(False); ctx.close()          # first use of the device and of the library
first, rebind = [], []
for _ in range(5):
    ctx, ms = create(False); first.append(ms)
    name, t = next((n, t) for n, t in named if n == 'out_conv.bias')
    for _ in range(10):
        t2 = t.detach().clone()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ctx.bind([(name, t2)])
        _native.check(lib.rdmi_repack(ctx._h, None))
        torch.cuda.synchronize()
        rebind.append((time.perf_counter() - t0) * 1e3)
    ctx.bind(named)
    ctx.close()
tctx, train_ms = create(True); tctx.close()
print(json.dumps({'create_first_repack_ms': first, 'create_first_repack_median_ms': statistics.median(first),
                  'rebind_repack_ms_median': statistics.median(rebind), 'rebind_repack_ms_min_max': [min(rebind), max(rebind)],
                  'create_train_first_repack_ms': train_ms}))
