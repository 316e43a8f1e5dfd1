"""bench.py --dump-outputs: the poses of the last timed step, on seeded inputs, so two builds can be compared output for output;
--steps is the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_steps_below_one_is_refused(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse_args()


def test_dump_outputs_is_parsed(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '3', '--dump-outputs', 'out/x'])
    a = bench.parse_args()
    assert a.steps == 3 and a.dump_outputs == 'out/x'
    monkeypatch.setattr(sys, 'argv', ['bench.py'])
    assert bench.parse_args().dump_outputs is None


def _bench(tmp_path, tag, steps, warmup):
    d = tmp_path / tag
    r = subprocess.run([sys.executable, 'bench.py', '--batch', '2', '--steps', str(steps), '--warmup', str(warmup),
                        '--no-extras', '--cpu-seconds', '0', '--dump-outputs', str(d)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(line) == 1, r.stdout[-4000:]
    assert sorted(os.listdir(d)) == ['poses.npy']
    return json.loads(line[0]), np.load(d / 'poses.npy')


@pytest.mark.gpu
def test_dump_is_the_same_poses_whatever_the_step_count(cuda, tmp_path):
    out1, p1 = _bench(tmp_path, 'a', 1, 0)
    out3, p3 = _bench(tmp_path, 'b', 3, 1)
    assert out1['steps'] == 1 and out3['steps'] == 3
    assert p1.dtype == np.float32 and p1.shape == (2, 17, 3) and np.isfinite(p1).all()
    # the same seeded weights and crops, and a forward with no cross-step state: the last step's poses match bit for bit
    assert np.array_equal(p1, p3)
