"""bench.py as the driver runs it: the plain one-GPU line carries the headline and nothing that needs runs of its own, and --dump-outputs writes the
last timed step; the --full line carries the contract's fields (`roofline`, `cpu_baseline`), and the N > 1 launch line
(`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`) works end to end -- here with two ranks sharing the one test GPU over gloo
(INTEL_SINGLE_DEVICE / INTEL_DIST_BACKEND: RCCL refuses two ranks on one device; the RCCL collectives themselves run in tests/test_dp_gpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import ROOT

pytestmark = pytest.mark.gpu


def _line(out):
    lines = [l for l in out.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out[-2000:]            # rank 0 prints ONE JSON line
    return json.loads(lines[0])


def test_default_line_has_the_contract_fields():
    # (--cpu_budget: the CPU baseline's bounded sample, 24 s by default -- thread sweep, B = 512 and B = 4096 -- is 6 s at one thread count and B = 512 here and the four short lines of the other workloads, the bf16-mode line and the feed measurement are left out -- the
    # line's contract fields are what is checked)
    r = subprocess.run([sys.executable, 'bench.py', '--full', '--steps', '4', '--warmup', '2', '--cpu_budget', '6', '--no_workloads', '--no_bf16_line', '--no_feed'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _line(r.stdout)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in j, k
    assert j['n_gpus'] == 1 and j['steps'] == 4 and j['warmup'] == 2 and j['unit'] == 'sessions/s' and j['value'] > 0 and j['vs_baseline'] is None
    assert j['dtype'] == 'f32' and j['data'] == 'synthetic' and 'workload' in j['config'] and 'model' not in j['config']
    ro = j['roofline']
    assert ro['bound'] in ('hbm', 'mfma') and ro['unit'] in ('GB/s', 'TFLOP/s') and abs(ro['frac'] - ro['achieved'] / ro['peak']) < 1e-3 and 0 < ro['frac'] < 1
    assert ro['traffic'] is None or ro['traffic'] > 0
    cb = j['cpu_baseline']
    assert cb['kind'] == 'port' and cb['value'] > 0 and cb['cores'] >= 1 and cb['sample']
    assert j['value'] > 50 * cb['value']           # a sanity bound, not a target


def test_two_rank_launch_line_runs_end_to_end():
    # plain `python bench.py --gpus 2`: bench.py starts its own two ranks (torch.distributed.run as a child process), relays rank 0's line and checks
    # that the process group really spans two ranks (`rccl_ranks`)
    env = dict(os.environ, INTEL_SINGLE_DEVICE='1', INTEL_DIST_BACKEND='gloo')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, 'bench.py', '--gpus', '2', '--full', '--steps', '3', '--warmup', '1', '--no_cpu_baseline', '--no_feed', '--no_bf16_line']
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _line(r.stdout)
    assert j['n_gpus'] == 2 and j['rccl_ranks'] == 2 and j['backend'] == 'gloo' and j['scaling'] == 'weak' and j['config']['global_batch'] == 2 * j['config']['per_gpu_batch'] and j['config']['parallelism'] == 'dp2'
    assert j['value'] > 0 and abs(j['value'] - j['config']['global_batch'] / (j['ms_per_step'] * 1e-3)) <= 1e-3 * j['value']
    # data parallel: the line says which exchange form ran and what it cost / how much of it stayed exposed (HIP events around every collective)
    ex = j['exchange']
    assert ex['form'] in ('dense', 'touched_rows', 'sharded') and ex['steps'] == 5
    assert ex['table_exchange_ms'] > 0 and ex['table_branch_ms'] >= ex['table_exchange_ms'] and ex['dense_buckets_allreduce_ms'] > 0
    assert 0 <= ex['exposed_ms'] <= 10 * j['ms_per_step']


def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    # what a plain run measures and prints: set-up, warm-up, the --steps timed steps, the line; whatever needs runs of its own waits for --full.
    # Two runs with the same arguments start from the same seeded inputs, so their dumped outputs are the same computation -- up to the order of
    # the atomically accumulated gradient sums: the losses agree to 1e-8 and the parameters by 1e-8 on average (measured), while other inputs move
    # every parameter by about one Adam step (lr = 1e-3); a near-zero gradient whose sign flips may move one element by a few steps
    runs = []
    for tag in ('a', 'b'):
        d = tmp_path / tag
        r = subprocess.run([sys.executable, 'bench.py', '--steps', '3', '--warmup', '1', '--dump-outputs', str(d)], cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        runs.append((_line(r.stdout), d))
    j, d = runs[0]
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in j, k
    assert j['steps'] == 3 and j['warmup'] == 1 and j['unit'] == 'sessions/s' and j['higher_is_better'] is True and j['dtype'] == 'f32'
    assert j['value'] > 0 and abs(j['value'] - j['config']['global_batch'] / (j['ms_per_step'] * 1e-3)) <= 1e-3 * j['value']
    for k in ('value_spread', 'eval_sessions_per_s', 'roofline', 'kernel_ms_per_step', 'feed', 'gather_roofline', 'bf16_mode', 'workloads', 'cpu_baseline'):
        assert k not in j, k
    files = sorted(os.listdir(d))
    assert files == sorted(os.listdir(runs[1][1]))
    assert {'loss.npy', 'ensemble_loss.npy', 'intent_loss.npy', 'param.iid_embeddings.weight.npy'} <= set(files)
    total, diff_sum, n = 0, 0.0, 0
    for f in files:
        x, y = np.load(d / f), np.load(runs[1][1] / f)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.isfinite(x).all(), f
        if f.startswith('param.'):
            diff = np.abs(x.astype(np.float64) - y)
            assert diff.max() <= 1e-2, (f, diff.max())
            diff_sum, n = diff_sum + diff.sum(), n + diff.size
        else:
            np.testing.assert_allclose(x, y, rtol=1e-6, err_msg=f)
        total += x.nbytes
    assert n > 0 and diff_sum / n <= 1e-6, diff_sum / n
    assert total <= 64 << 20
    assert abs(float(np.load(d / 'loss.npy')[0]) - j['loss_last_step']) <= 1e-6 * max(1.0, abs(j['loss_last_step']))
