"""bench.py's plain run on the GPU: the line carries the contract's keys and no --full extras, --steps is the number of timed steps, and
--dump-outputs writes what the last timed step returned (outputs, losses, updated parameters, gradients) as float32 / float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / 'outputs'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--rays', '1024', '--dump-outputs', str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res['metric'] == 'train_rays_per_sec' and res['unit'] == 'rays/s' and res['higher_is_better'] is True and res['dtype'] == 'f32'
    assert res['steps'] == 3 and res['warmup'] == 1 and res['ms_per_step'] > 0
    assert abs(res['value'] - 1024 * 1e3 / res['ms_per_step']) <= 1e-3 * res['value']
    for k in ('roofline', 'cpu_baseline', 'full_report', 'value_bf16', 'render_ms_per_frame'):
        assert k not in res, k
    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 10 ** 6
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    assert files['out.rgb_fine'].shape == (1024, 3) and files['loss.TotalLoss'].shape == ()
    params = [k for k in files if k.startswith('param.')]
    assert len(params) > 0 and len([k for k in files if k.startswith('grad.')]) == len(params)
    assert files['param.fine_model.pts_linears.0.weight'].shape == (256, 63)
