"""Launch order of the backward's three schedules (csrc/model.cpp: backward_impl) against a recorded one.

The library's built-in profiler records every launch in host enqueue order with its stream (tests/helpers.KernelTrace).  One
training forward and one backward on a constant upstream gradient are run per case, only the backward call(s) are traced, the
streams are renumbered by first appearance inside the trace (the profiler's indices are process-global) and the whole sequence of
(record name, stream) is compared with tests/golden/bwd_launch_order.json (tests/golden/make_launch_order_golden.py writes it from
trace_case below).  A change that is meant to leave the schedules alone must pass against the JSON of the commit before it.

    four streams + chains            default, gru_bpr   phase 0 (cross attention on, <= 1024 sessions)
    four streams, kernel-per-op head noxatt             phase 0 (cross_attention = 0: no chains, the towers' gate arm)
                                     default            phase 0 in a child process with INTEL_HEAD_FUSED=0 (read once per process)
    two calls                        default, noxatt    phase 1 then phase 2, traced together
    one stream                       default            phase 0 with intel_set_concurrency(ctx, 0)
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.helpers import GOLDEN, ROOT, Fixture, KernelTrace, build_model

pytestmark = pytest.mark.gpu
GOLDEN_JSON = os.path.join(GOLDEN, 'bwd_launch_order.json')

# id -> (fixture, mode, environment of the process that runs it)
CASES = {
    'chains-default': ('default', 'one_call', {}),
    'chains-gru_bpr': ('gru_bpr', 'one_call', {}),
    'per_op-noxatt': ('noxatt', 'one_call', {}),
    'per_op-default': ('default', 'one_call', {'INTEL_HEAD_FUSED': '0'}),
    'two_calls-default': ('default', 'two_calls', {}),
    'two_calls-noxatt': ('noxatt', 'two_calls', {}),
    'one_stream-default': ('default', 'one_stream', {}),
}
FOUR_STREAMS = ('chains-default', 'chains-gru_bpr', 'per_op-noxatt', 'per_op-default')


def backward_trace(fixture, mode):
    """[[record name, stream], ...] of the backward call(s) of one training step, streams numbered by first appearance."""
    from intel_sigir2023_amd import _lib
    dev = torch.device('cuda:0')
    fx = Fixture(fixture)
    model, _ = build_model(fx, dev)
    batch, keep = model.prepare_batch(fx.batch(dev))
    params = [p.detach() for _, _, p in model.slot_items()]
    lib, ctx = _lib.lib(), model._context()
    if mode == 'one_stream':
        lib.intel_set_concurrency(ctx, 0)
    try:
        weights, ens, intents = model.run_forward(batch, keep, params, train=True)
        d_out = [torch.full_like(t, 0.01) for t in (weights, ens, intents)]
        torch.cuda.synchronize()
        with KernelTrace() as kt:
            grads = None
            for phase in ((1, 2) if mode == 'two_calls' else (0,)):
                grads = model.run_backward(batch, keep, params, *d_out, grad_tensors=grads, phase=phase)
    finally:
        if mode == 'one_stream':
            lib.intel_set_concurrency(ctx, 1)
    order = {}
    return [[r['name'], order.setdefault(r['stream'], len(order))] for r in kt.records]


def trace_case(case):
    """The trace of one of CASES; a case with switches runs in a child process that has them set (they are read once per process)."""
    fixture, mode, env = CASES[case]
    if all(os.environ.get(k) == v for k, v in env.items()):
        return backward_trace(fixture, mode)
    r = subprocess.run([sys.executable, '-m', 'tests.test_bwd_schedule_gpu', case], cwd=ROOT, env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN_JSON) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('case', list(CASES))
def test_backward_launch_order_matches_the_recorded_one(case, recorded):
    got, want = trace_case(case), recorded[case]
    streams = len({s for _, s in got})
    if case in FOUR_STREAMS:
        assert streams == 4, 'the one-call schedule ran on %d streams' % streams
    if CASES[case][1] == 'one_stream':
        assert streams == 1, 'concurrency is off, yet the backward ran on %d streams' % streams
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, 'launch %d of %d (recorded %d): got %s, recorded %s' % (
        first, len(got), len(want), got[first] if first < len(got) else None, want[first] if first < len(want) else None)


if __name__ == '__main__':      # the child of trace_case: the trace as one JSON line
    print(json.dumps(backward_trace(*CASES[sys.argv[1]][:2])))
