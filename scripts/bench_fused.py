"""bench.py --gpus 1 --steps 3 --warmup 1 --full --no-cpu-baseline of a checkout, with the two CIFAR-shape (tiled plan) variants left out:
the headline, the fused-path variants and the training steps, one JSON line.

    python scripts/bench_fused.py [ROOT]      ROOT: the checkout to measure (default: this one)"""
import os, sys
tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
os.chdir(tree)
sys.path.insert(0, tree)
import bench
bench.cifar_variant = lambda *a, **k: {'skipped': 'tiled plan: not part of this A/B'}
sys.argv = ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--full', '--no-cpu-baseline']
bench.main()
