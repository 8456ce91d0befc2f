"""bench.py's command line: a plain run times the headline steps only, `--full` adds the other legs, `--dump-outputs DIR` writes what
the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def test_dump_kernels_needs_full():
    """The per-kernel table comes from the roofline leg, which only a --full run has: refused before anything is set up."""
    r = subprocess.run([sys.executable, BENCH, '--dump-kernels', os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 2 and b'--full' in r.stdout, r.stdout.decode()[-2000:]


def _plain_run(out_dir, steps, warmup):
    cmd = [sys.executable, BENCH, '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup), '--size', '32', '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    lines = [l for l in out.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, out[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    from van_gan_amd import RESULT_KEYS
    d = _plain_run(tmp_path / 'a', 10, 2)
    assert d['steps'] == 10 and d['warmup'] == 2 and d['unit'] == 'Mvoxels/s' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
    assert d['ms_per_step'] > 0 and abs(d['value'] - 32 ** 3 / d['ms_per_step'] / 1e3) <= 1e-6 * d['value']
    for k in ('roofline', 'cpu_baseline', 'configs', 'inference', 'ddp_path', 'ms_per_step_synced', 'replay_ms_per_step'):
        assert d[k] is None, k                              # the --full legs did not run
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(k + '.npy' for k in RESULT_KEYS)
    for k in RESULT_KEYS:
        a = np.load(tmp_path / 'a' / (k + '.npy'))
        assert a.dtype == np.float64 and a.shape == (1,) and a[0] == d['losses'][k], k
    # the same arguments again: the last step runs from the seeded initial state, so only the rounding of the float atomics differs
    # (measured <= 4e-3 relative, in the cycle losses; 10 steps of training from run-dependent states drift further)
    e = _plain_run(tmp_path / 'b', 10, 2)
    for k in RESULT_KEYS:
        a, b = np.load(tmp_path / 'a' / (k + '.npy'))[0], np.load(tmp_path / 'b' / (k + '.npy'))[0]
        assert abs(a - b) <= 2e-2 * abs(a) + 1e-6, (k, a, b)
        assert b == e['losses'][k], k
