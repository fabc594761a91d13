#!/bin/bash
cd $GRAFT_REPO_ROOT
OUT_DIR=${OUT_DIR:-out}; mkdir -p $OUT_DIR
python -u -m pytest tests/test_gpu_kernels.py -m gpu -q -x > $OUT_DIR/t7.log 2>&1; echo "exit $?" >> $OUT_DIR/t7.log
tail -3 $OUT_DIR/t7.log
timeout -k 10 120 python tools/diag/mb_conv.py f3 20 2>&1 | grep conv
python bench.py --full --no-cpu-baseline --no-dropin --steps 10 --warmup 2 > $OUT_DIR/b_x.json 2>/dev/null
python - <<PY
import json
d=json.loads(open('$OUT_DIR/b_x.json').read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'])
print('bench', {k:(v['ms'],v['frac']) for k,v in d['hbm_layers'].items()})
PY
