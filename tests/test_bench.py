"""bench.py's own options: `--dump-outputs` (what the timed path computed, for comparing two builds output for output)
and the plain run (the headline line only; the extra passes are behind `--full`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 1000)
    g = torch.Generator().manual_seed(5)
    arrays = {'big': torch.randn(3, 700, generator=g).bfloat16(), 'small': torch.randn(2, 5, generator=g),
              'count': torch.tensor(7, dtype=torch.int64)}
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    big, small, count = (np.load(str(tmp_path / 'a' / (n + '.npy'))) for n in ('big', 'small', 'count'))
    assert big.dtype == np.float32 and big.shape == (1000,)
    flat = arrays['big'].float().reshape(-1).numpy()
    assert np.isin(big, flat).all()                     # values of the array, not of a copy made elsewhere
    assert np.array_equal(big, np.load(str(tmp_path / 'b' / 'big.npy')))   # the same positions every time
    assert small.dtype == np.float32 and np.array_equal(small, arrays['small'].numpy())
    assert count.dtype == np.float64 and count == 7


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 100)
    with pytest.raises(RuntimeError, match='exceed'):
        bench.dump_outputs(str(tmp_path / 'x'), {'a': torch.zeros(26)})
    assert not (tmp_path / 'x').exists()


@pytest.mark.gpu
def test_plain_bench_run_times_the_given_steps_and_dumps_the_last_one(tmp_path):
    """A plain run: the headline line with `steps` as given and no --full passes; --dump-outputs writes the last
    timed step's loss, fused maps, state and gradient as float arrays within 64 MB."""
    import bench
    out = tmp_path / 'dump'
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '2', '--dump-outputs', str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 2 and line['warmup'] == 2 and line['ms_per_step'] > 0
    assert line['unit'] == 'clips/s' and line['higher_is_better'] is True and line['dtype'] == 'bf16'
    assert abs(line['value'] - 1e3 / line['ms_per_step']) < 1e-2 * line['value']
    assert line['cpu_baseline'] is None and line['dropin_api_ms_per_step'] is None
    assert line['kernel_events']['layer_table_steps'] is None
    files = {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    assert files['loss'].shape == () and files['loss'] > 0
    assert files['out.0'].shape == (bench.DUMP_SAMPLE,) and files['out.pool'].shape == (1, 256, 12, 21)
    assert files['state.fast_conv1.weight'].ndim == 5 and 'state.bn_s1.running_var' in files and 'grad' in files
