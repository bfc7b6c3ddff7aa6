"""bench.py end to end on the GPU: a plain run (the smallest workload, C2, two
timed steps) prints the headline line without the figures that belong to
--full, and --dump-outputs leaves the last step's parameters and statistics as
float .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_outputs(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', 'c2',
                          '--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path)],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(line) for line in out.stdout.splitlines() if line.startswith('{')]
    assert len(lines) == 1
    r = lines[0]
    assert r['steps'] == 2 and r['warmup'] == 1 and r['n_gpus'] == 1
    assert r['unit'] == 'env-steps/s' and r['higher_is_better'] is True and r['dtype'] == 'f32'
    assert r['ms_per_step'] > 0
    # value = env steps of the timed region / its wall time (C2: 64 segments x 50 steps)
    assert abs(r['value'] - 64 * 50 / (r['ms_per_step'] * 1e-3)) <= 1e-3 * r['value']
    for k in ('roofline', 'kernels', 'phase_ms_per_step', 'cpu_baseline', 'host_fed', 'calib'):
        assert k not in r, f'{k} belongs to --full'
    files = sorted(os.listdir(tmp_path))
    assert 'stats.npy' in files
    assert any(f.startswith('ppo.actor.') for f in files) and any(f.startswith('ppo.critic.') for f in files)
    total = 0
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    # the two timed steps updated the model: the statistics of the last one are set
    assert np.abs(np.load(tmp_path / 'stats.npy')).max() > 0
