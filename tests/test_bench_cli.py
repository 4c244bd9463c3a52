"""bench.py's command line on the harness stub (CPU, no HIP library): --steps sets the timed folds and the line
carries ms_per_step; --dump-outputs writes the last timed fold, the same from run to run; the CPU baseline is
behind --full; dump_outputs keeps its files under the size limit with a fixed subset."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    env = dict(os.environ, DM_DIST_BACKEND='gloo', MASTER_ADDR='127.0.0.1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'stub'] + args, env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    return lines[0]


@pytest.fixture(scope='module')
def dumped(tmp_path_factory):
    """One stub run of 3 timed folds after 2 warm-up folds, dumped: (result line, samples)."""
    d = tmp_path_factory.mktemp('dump')
    line = _bench(['--gpus', '1', '--steps', '3', '--warmup', '2', '--dump-outputs', str(d)])
    assert sorted(os.listdir(d)) == ['samples.npy']
    return line, np.load(os.path.join(d, 'samples.npy'))


def test_line_fields_of_a_plain_run(dumped):
    line, _ = dumped
    assert line['steps'] == 3 and line['warmup'] == 2 and line['n_gpus'] == 1
    assert line['unit'] == 'images/sec' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['ms_per_step'] >= 0 and line['value'] > 0
    assert line['cpu_baseline'] is None and 'gpu_over_cpu' not in line


def test_dump_is_the_last_timed_fold(dumped):
    """The stub's fold is the clamped draw of a generator seeded 2022: with W = 2 and K = 3 the dumped fold is
    the fifth draw, so --steps and --warmup really set how many folds ran."""
    _, got = dumped
    assert got.dtype == np.float32 and got.shape == (4, 3, 8, 8)
    gen = torch.Generator().manual_seed(2022)
    for _ in range(5):
        want = torch.randn((4, 3, 8, 8), generator=gen).clamp(-1, 1)
    assert np.array_equal(got, want.numpy())


def test_dump_repeats_and_full_is_accepted(dumped, tmp_path):
    _, first = dumped
    line = _bench(['--gpus', '1', '--steps', '3', '--warmup', '2', '--full', '--dump-outputs', str(tmp_path)])
    assert np.array_equal(np.load(os.path.join(tmp_path, 'samples.npy')), first)
    assert line['steps'] == 3 and line['cpu_baseline'] is None   # the stub has no model to run on the CPU


def test_dump_outputs_stays_under_the_limit(tmp_path):
    import bench
    x = torch.arange(10 * 6, dtype=torch.float64).view(10, 2, 3)
    kept = bench.dump_outputs(str(tmp_path), dict(a=x, b=x[:2]), limit=2 * 4 * 24)   # 4 images of 24 bytes per file
    a, b = np.load(os.path.join(tmp_path, 'a.npy')), np.load(os.path.join(tmp_path, 'b.npy'))
    assert a.dtype == np.float32 and a.shape == (4, 2, 3) and a.nbytes + b.nbytes <= 2 * 4 * 24
    assert kept['b'] is None and np.array_equal(b, x[:2].numpy())
    assert kept['a'] == sorted(kept['a']) and len(set(kept['a'])) == 4
    assert np.array_equal(a, x[kept['a']].numpy())
    again = bench.dump_outputs(str(tmp_path / 'again'), dict(a=x, b=x[:2]), limit=2 * 4 * 24)
    assert again == kept
