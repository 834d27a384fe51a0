set -x
cd $GRAFT_REPO_ROOT
O=${O:-out}; mkdir -p $O
timeout -k 10 300 python -m pytest tests -m gpu -x -q 2>&1 | tail -4
timeout -k 10 500 python bench.py --steps 2 --warmup 1 --full 2>&1 | tail -1 | tee $O/bench_none.json
