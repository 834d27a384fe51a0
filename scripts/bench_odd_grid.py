"""Secondary measurement: the fused PC sampler loop of the shipped GTO-Halo architecture (nf 64, ch_mult [1, 2, 2], 2 res blocks per level,
attention at full resolution, conditional with classifier-free guidance) on a square single-channel grid beyond 9x9, which the tiled
plan runs: 10x10 and 11x11 take the nearest resize of h onto the odd skip grids and attention rows padded to Lp (L = 100 -> 112,
121 -> 128); 12x12 (no resize, L = 144) is the neighbouring grid that needs neither.  fp32, B = 128 (256 forwards per score).
usage: bench_odd_grid.py [--size S] [--batch B] [--updates U] [--steps K] [--warmup W] [--lib PATH].  Not the driver's bench.py; prints
one JSON line.  An iteration is one rdmi_pc_sample call of U reflected Euler-Maruyama updates (N = U + 1 scales, in-kernel noise), timed
on its own between device synchronisations; ms per update = iteration time / U, median and min / max over the timed iterations.  The
share of the resize launches and of the attention core (scores, softmax, V transpose, P V) comes from a separate profiled call
(rdmi_set_profiling).  --lib binds another build of the library (the parent commit's, for the 12x12 comparison)."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'optimized-diffusion-model_amd'))
import torch
import __graft_entry__ as ge

args = sys.argv[1:]
def opt(name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default
S, B, U, K, W, lib = opt('--size', 10), opt('--batch', 128), opt('--updates', 8), opt('--steps', 12), opt('--warmup', 3), opt('--lib', '')
from rdmi import _native, sampling, sde_lib
from rdmi.models import utils as mutils
from oracle.weights import make_params
if lib:
    _native.use_library(lib)
dev = torch.device('cuda:0')
cfg = ge.demo_config(num_scales=U + 1, image_size=S, image_width=S)
cfg.model.attn_resolutions = [S]
model = mutils.create_model(cfg)
params = make_params(0, image_size=S, attn_resolutions=(S,))
model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
model = model.to(dev).eval()
sde = sde_lib.RVESDE(0.01, 5, N=U + 1)
lab = torch.rand(B, 1, device=dev)
fn = sampling.get_pc_sampler(sde, (B, 1, S, S), sampling.get_predictor('euler_maruyama'), sampling.get_corrector('none'),
                             sampling.get_denoiser('none'), 0.01, 1, 1e-5, dev, seed=7)

def step():
    return fn(model, weight=0.5, class_labels=lab)[0]

for _ in range(W):
    step()
ts = []
for _ in range(K):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    x = step()
    torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3 / U)
assert bool(torch.isfinite(x).all()) and float(x.min()) >= 0 and float(x.max()) <= 1
ctx = model._ctx[(str(dev), S, S)]
ctx.set_profiling(True)
step()
torch.cuda.synchronize()
prof = ctx.get_profile()
ctx.set_profiling(False)
total = sum(p['ms'] for p in prof)
def share(names):
    return sum(p['ms'] for p in prof if p['kernel'] in names) / total if total else None
res = {'metric': f'GTO-Halo architecture, {S}x{S}x1, fused PC loop (EM, guidance on), fp32, B = {B}: ms per update', 'size': S, 'batch': B,
       'updates': U, 'steps': K, 'warmup': W, 'library': _native.library_path(), 'path_info': ctx.path_info(),
       'ms_per_update_median': statistics.median(ts), 'ms_per_update_min': min(ts), 'ms_per_update_max': max(ts),
       'ms_per_update_all': [round(t, 4) for t in ts],
       'share_resize': share({'nearest_resize_kernel'}),
       'share_attention_core': share({'bgemm_nt_kernel', 'softmax_rows_kernel', 'transpose_lc_kernel'}),
       'profile_ms': {p['kernel']: round(p['ms'], 4) for p in prof}}
print(json.dumps(res))
