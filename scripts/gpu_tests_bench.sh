#!/bin/bash
O=${O:-out/tests_bench}; mkdir -p $O
python -m pytest tests -x -q -m gpu > $O/tests.log 2>&1 && tail -3 $O/tests.log && python bench.py --steps 3 --warmup 1 --full > $O/bench.json 2> $O/bench.err && cat $O/bench.json
