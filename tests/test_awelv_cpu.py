"""CPU-side checks of the aWELv baseline (intel_sigir2023_amd/awelv.py): registry and parser, the reference's initial state_dict from the
same seed, no CPU path, the exported C-ABI entries -- and the float64 restatement the GPU tests use as their yardstick at other shapes
(tests/awelv_ref.py), validated here against the arrays the unmodified reference produced (tests/golden/awelv_base.npz)."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import awelv_ref as R
from tests.helpers import ROOT, make_args, make_corpus

NEW_SYMBOLS = ('intel_awelv_forward', 'intel_awelv_backward_workspace_bytes', 'intel_awelv_backward')


def test_registry_and_parser():
    from intel_sigir2023_amd.main import build_parser, MODELS
    from intel_sigir2023_amd import awelv
    assert MODELS['aWELv'] is awelv.aWELv and awelv.aWELv.ENGINE is awelv.aWELvEngine
    assert (awelv.aWELv.reader, awelv.aWELv.runner) == ('BaseReader', 'BaseRunner')
    _, parser = build_parser(['--model_name', 'aWELv', '--loss_name', 'Listloss'])
    a, _ = parser.parse_known_args(['--model_name', 'aWELv', '--loss_name', 'Listloss'])
    assert (a.hidden_size, a.model_num, a.model_path, a.buffer) == (32, 2, '', 1)          # aWELv.py:17, BaseModel.py:21-25
    a, _ = parser.parse_known_args(['--hidden_size', '64', '--model_num', '3'])
    assert (a.hidden_size, a.model_num) == (64, 3)


@pytest.mark.parametrize('argv', [['--model_name', 'aWELv'], ['--model_name', 'aWELv', '--loss_name', 'IntListloss'],
                                  ['--model_name', 'aWELv', '--loss_name', 'IntMSEloss']])
def test_intent_losses_are_rejected_with_the_plain_ones_named(argv):
    from intel_sigir2023_amd.main import build_parser
    with pytest.raises(SystemExit) as e:          # the CLI default is IntBPRloss
        build_parser(argv)
    for name in ('Listloss', 'BPRloss', 'MSEloss'):
        assert name in str(e.value)


def test_engine_rejects_intent_losses_before_touching_the_model():
    from intel_sigir2023_amd import awelv
    with pytest.raises(ValueError) as e:
        awelv.aWELvEngine(None, 'IntBPRloss')
    for name in ('Listloss', 'BPRloss', 'MSEloss'):
        assert name in str(e.value)


def test_same_seed_gives_the_reference_initial_state_bit_for_bit():
    from intel_sigir2023_amd import awelv
    z, cfg = R.load()
    torch.manual_seed(cfg['seed'])
    model = awelv.aWELv(make_args(cfg['args'], torch.device('cpu')), make_corpus(cfg['shape']))
    sd = model.state_dict()
    assert list(sd) == ['uid_embeddings.weight', 'model_embeddings.weight']
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), z['sd_raw/' + k]), k
    assert model.count_variables() == (cfg['shape']['users'] + 3) * 32
    groups = model.customize_parameters()
    assert len(groups[0]['params']) == 2 and groups[1] == {'params': [], 'weight_decay': 0}
    assert (model.model_num, model.intent_num, model.max_his, model.optimizer) == (3, cfg['shape']['I'], 20, None)
    model.load_state_dict(R.state(z, 'sd'), strict=True)
    assert np.array_equal(model.uid_embeddings.weight.detach().numpy(), z['sd/uid_embeddings.weight'])


def test_forward_on_cpu_tensors_raises():
    from intel_sigir2023_amd import _lib, awelv
    z, cfg = R.load()
    model = awelv.aWELv(make_args(cfg['args'], torch.device('cpu')), make_corpus(cfg['shape']))
    with pytest.raises(_lib.IntelHipError):
        model(R.batch(z, 'in/'))
    with pytest.raises(_lib.IntelHipError):
        awelv.awelv_forward(torch.zeros(4, 8), torch.zeros(3, 8), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 5, 3))


def test_header_exports_and_library_carry_the_awelv_symbols():
    from intel_sigir2023_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'intel_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, txt), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.intel_abi_version() == 5
    # the backward's workspace does not grow with B beyond the workgroup cap
    small, big, huge = (lib.intel_awelv_backward_workspace_bytes(b, 3, 32) for b in (4, 4096, 1 << 20))
    assert 3 * 32 * 4 <= small < big == huge
    assert lib.intel_awelv_backward_workspace_bytes(0, 3, 32) == 0


@pytest.mark.parametrize('state', ['raw', 'scaled'])
def test_float64_restatement_reproduces_the_reference_outputs_and_gradients(state):
    """The yardstick of tests/test_awelv_gpu.py at other shapes: float64 forward + restated Listloss / MSEloss through autograd against
    what the reference computed in fp32.  Outputs to 3e-5 * max(1, max|ref|), losses to 1e-5, gradients to 1e-6 + 2e-4 * max|ref|."""
    z, cfg = R.load()
    b = R.batch(z, 'in/')
    sd = R.state(z, 'sd_raw' if state == 'raw' else 'sd')
    E = sd['uid_embeddings.weight'].double().requires_grad_(True)
    M = sd['model_embeddings.weight'].double().requires_grad_(True)
    weights, ens = R.forward64(E, M, b['u_id_c'], b['scores'])
    prefix = 'out_raw/' if state == 'raw' else 'out/'
    for got, key in ((weights, 'weights'), (ens, 'ens_score')):
        ref = z[prefix + key]
        assert got.shape == ref.shape
        assert np.abs(got.detach().numpy() - ref).max() <= 3e-5 * max(1.0, np.abs(ref).max()), key
    assert np.abs(weights.detach().numpy().sum(-1) - 1.0).max() < 1e-12
    a = cfg['args']
    for lname, fn in (('list', R.listloss64), ('mse', R.mseloss64)):
        E.grad = M.grad = None
        weights, ens = R.forward64(E, M, b['u_id_c'], b['scores'])
        loss = fn(weights, ens, b, a['cal_diversity'], a['diversity_alpha'])
        loss.backward()
        assert abs(float(loss.detach()) - float(z['%s/%s/loss' % (state, lname)])) <= 1e-5, lname
        for pn, p in (('uid_embeddings.weight', E), ('model_embeddings.weight', M)):
            ref = z['%s/%s/grad/%s' % (state, lname, pn)]
            err = np.abs(p.grad.numpy() - ref).max()
            assert err <= 1e-6 + 2e-4 * np.abs(ref).max(), (lname, pn, err)


def test_analytic_backward_of_the_restatement_equals_autograd():
    """R.backward64 (the closed form the kernel tests compare with) against autograd of R.forward64, with gradients in the pad slots."""
    g = torch.Generator().manual_seed(3)
    B, Lm, K, H, users = 5, 7, 3, 8, 6
    E = torch.randn(users, H, generator=g, dtype=torch.float64, requires_grad=True)
    M = torch.randn(K, H, generator=g, dtype=torch.float64, requires_grad=True)
    u = torch.tensor([0, 3, 3, 5, 0])
    sc = torch.rand(B, Lm, K, generator=g, dtype=torch.float64)
    d_ens = torch.randn(B, Lm, generator=g, dtype=torch.float64)
    d_w = torch.randn(B, Lm, K, generator=g, dtype=torch.float64)
    weights, ens = R.forward64(E, M, u, sc)
    ((weights * d_w).sum() + (ens * d_ens).sum()).backward()
    dE, dM = R.backward64(E.detach(), M.detach(), u, sc, d_ens, d_w)
    assert float((dE - E.grad).abs().max()) < 1e-12 and float((dM - M.grad).abs().max()) < 1e-12
    assert float(dE[[1, 2, 4]].abs().max()) == 0.0
