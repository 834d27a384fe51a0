"""Secondary measurement: forward + backward of the CIFAR-shape NCSN++ (tiled plan, fp32) at B = 64 on one GPU, with and without the
parameter gradients -- the right-hand side of a likelihood evaluation is one forward plus one vector-Jacobian product.
usage: bench_vjp_cifar.py [--mode full|vjp] [--steps K] [--warmup W].  Not the driver's bench.py; prints one JSON line.
  full  rdmi_train_forward + rdmi_backward (every parameter gradient; what a checkout without rdmi_backward_input can run: timing (a))
  vjp   rdmi_train_forward + the VJP-only rdmi_backward_input (grad_x only: timing (b)), and the input data-gradient kernel alone from
        rdmi_get_profile (timing (c))
Each step is timed on its own between device synchronisations; median and min / max over the timed steps are reported."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'optimized-diffusion-model_amd'))
import torch
import __graft_entry__ as ge

args = sys.argv[1:]
def opt(name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default
mode, K, W, B = opt('--mode', 'vjp'), opt('--steps', 12), opt('--warmup', 3), opt('--batch', 64)
dev = torch.device('cuda:0')
model, cfg, _ = ge.make_cifar_model(dev)
g = torch.Generator(device=dev).manual_seed(B)
x = torch.rand(B, 3, 32, 32, device=dev, generator=g)
sigma = torch.exp(torch.rand(B, device=dev, generator=g) * 8.5 - 4.6)
lab = torch.zeros(B, 1, device=dev)
gout = torch.randn(B, 3, 32, 32, device=dev, generator=g)
tctx = model.train_context(B, 32, 32, dev)
out, gx = torch.empty_like(x), torch.empty_like(x)
flat = torch.empty(sum(p.numel() for p in model.parameters()), device=dev)

def step():
    tctx.train_forward(x, sigma, lab, out, 0.0, 0)
    if mode == 'full':
        tctx.backward(gout, flat, x)
    else:
        tctx.backward(gout, None, x, grad_x=gx)

for _ in range(W):
    step()
ts = []
for _ in range(K):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    step()
    torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
res = {'metric': f'CIFAR-shape NCSN++ fp32 train_forward + backward ({mode}), B = {B}', 'mode': mode, 'steps': K, 'warmup': W,
       'ms_median': statistics.median(ts), 'ms_min': min(ts), 'ms_max': max(ts), 'ms_all': [round(t, 3) for t in ts]}
if mode == 'vjp':
    tctx.set_profiling(True)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    prof = tctx.get_profile()
    tctx.set_profiling(False)
    k = [p for p in prof if p['kernel'] == 'input_dgrad_kernel']
    res['input_dgrad_kernel_us'] = 1e3 * k[0]['ms'] / k[0]['launches'] if k else None
    res['profiled_kernels'] = sorted({p['kernel'] for p in prof})
print(json.dumps(res))
