#!/bin/bash
# full GPU test suite, then the four bench lines
cd $GRAFT_REPO_ROOT
OUT_DIR=${OUT_DIR:-out}; mkdir -p $OUT_DIR
python -u -m pytest tests -m gpu -q > $OUT_DIR/t_full.log 2>&1; echo "exit $?" >> $OUT_DIR/t_full.log
tail -4 $OUT_DIR/t_full.log
python -u bench.py --full --no-cpu-baseline > $OUT_DIR/b_c2.json 2> $OUT_DIR/b_c2.err; echo "bench c2 $?"
python -u bench.py --full --no-cpu-baseline --sp 4 --fp 64 --steps 10 --warmup 2 > $OUT_DIR/b_c4.json 2> $OUT_DIR/b_c4.err; echo "bench c4 $?"
