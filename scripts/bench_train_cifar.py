"""Secondary measurement (BASELINE config #5 shape): fp32 score-matching training steps of the CIFAR-shape NCSN++ (tiled plan,
csrc/tiled_train.h) on one GPU -- dropout 0.1, label drop 0.5, clip + Adam + EMA -- at B = 64 and 128.
usage: bench_train_cifar.py [B ...] [--steps K].  Not the driver's bench.py; prints one JSON line.
FLOPs are counted from the launch shapes (the profile's per-launch FLOP counts of one step: forward convs and attention GEMMs,
backward weight- and data-gradient contractions) against the fp32 matrix peak of 157.3 TFLOP/s."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'optimized-diffusion-model_amd'))
import torch
import __graft_entry__ as ge
from rdmi import losses, sde_lib
from rdmi.models.ema import ExponentialMovingAverage

PEAK = 157.3e12
args = [a for a in sys.argv[1:]]
K = 5
if '--steps' in args:
    i = args.index('--steps'); K = int(args[i + 1]); del args[i:i + 2]
batches = [int(a) for a in args] or [64, 128]
dev = torch.device('cuda:0')
model, cfg, _ = ge.make_cifar_model(dev)
model.train()
sde = sde_lib.RVESDE(0.01, 50, N=1000)
opt = losses.get_optimizer(cfg, model.parameters())
ema = ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
state = dict(optimizer=opt, model=model, ema=ema, step=0, scaler=None)
step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=False, likelihood_weighting=False)
res = {'metric': 'CIFAR-shape NCSN++ fp32 training step (tiled plan; dropout 0.1, label drop 0.5, clip + Adam + EMA)', 'steps': K,
       'peak_tflops': PEAK / 1e12, 'batches': {}}
for B in batches:
    g = torch.Generator(device=dev).manual_seed(B)
    batch = torch.rand(B, 3, 32, 32, device=dev, generator=g); labels = torch.zeros(B, 1, device=dev)
    for _ in range(2):
        l = step_fn(state, batch, class_labels=labels)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(K):
        l = step_fn(state, batch, class_labels=labels)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / K
    ctx = model._ctx[('train', str(dev), 32, 32)]
    ctx.set_profiling(True)
    step_fn(state, batch, class_labels=labels)
    torch.cuda.synchronize()
    prof = ctx.get_profile()
    ctx.set_profiling(False)
    flops = sum(p['flops'] for p in prof)
    top = sorted(prof, key=lambda p: -p['ms'])[:8]
    res['batches'][str(B)] = {'ms_per_step': dt * 1e3, 'samples_per_s': B / dt, 'loss': float(l.detach()),
                              'profiled_launches_per_step': sum(p['launches'] for p in prof), 'gflop_per_step': flops / 1e9,
                              'tflops': flops / dt / 1e12, 'peak_fraction': flops / dt / PEAK,
                              'top_kernels_ms': {p['kernel']: round(p['ms'], 2) for p in top}}
print(json.dumps(res))
