"""The aWELv baseline on the GPU (intel_sigir2023_amd/awelv.py, csrc/awelv.hip).

Yardsticks: the arrays the unmodified reference produced (tests/golden/awelv_base.npz, written by tests/golden/make_awelv_base_golden.py) and,
at shapes the fixture does not have, the float64 restatement of tests/awelv_ref.py, which tests/test_awelv_cpu.py holds to that fixture.

Tolerances are the project's own: outputs 3e-5 * max(1, max|ref|); |sum_k w - 1| < 1e-5; losses 1e-5; gradients 1e-6 + 2e-4 * max|ref|
(tests/test_variant_gpu.py); one optimizer step 4 ulp + 2e-5 * lr and a trajectory 2e-3 * move + 1e-7 per element (tests/test_trajectory_gpu.py).
"""
import argparse

import numpy as np
import pytest
import torch

from tests import awelv_ref as R
from tests.helpers import make_args, make_corpus

pytestmark = pytest.mark.gpu

PARAMS = ('uid_embeddings.weight', 'model_embeddings.weight')


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _out_tol(ref):
    return 3e-5 * max(1.0, float(ref.abs().max()))


def _grad_tol(ref):
    return 1e-6 + 2e-4 * float(ref.abs().max())


def _case(B, Lm, K, H, users, seed, scale=0.3, user_ids=None):
    """Seeded inputs on the host (float32 values, so that the float64 reference starts from the very numbers the kernel reads): scores and
    upstream gradients are non-zero in EVERY slot of the padded list, and only every other user occurs."""
    g = torch.Generator().manual_seed(seed)
    c = dict(E=torch.randn(users, H, generator=g) * scale, M=torch.randn(K, H, generator=g) * scale,
             scores=torch.rand(B, Lm, K, generator=g) + 0.05,
             d_ens=torch.randn(B, Lm, generator=g), d_w=torch.randn(B, Lm, K, generator=g) * 0.5)
    c['u'] = (torch.randint(0, (users + 1) // 2, (B,), generator=g) * 2).int() if user_ids is None else user_ids.int()
    return c


def _run_backward(c, dev, d_w, prefill):
    from intel_sigir2023_amd import awelv
    users, H = c['E'].shape
    K = c['M'].shape[0]
    d_uid = prefill.clone().to(dev)
    d_model = torch.full((K, H), float('nan'), device=dev)
    flags = torch.zeros(users, dtype=torch.uint8, device=dev)
    awelv.awelv_backward(c['E'].to(dev), c['M'].to(dev), c['u'].to(dev), c['scores'].to(dev), c['w_dev'], c['d_ens'].to(dev),
                         None if d_w is None else d_w.to(dev), d_uid, d_model, row_flags=flags)
    torch.cuda.synchronize()
    return d_uid.cpu(), d_model.cpu(), flags.cpu()


# every B in {1, 4, 5, 257} (waves of a workgroup, one round past the backward's 64-workgroup cap), L in {1, 63, 64, 65, 130} (lane stride
# over the list), K in {1, 2, 3, 16} (both register bounds of the k loops), H in {4, 32, 60, 64, 68, 256} (float4 lanes of the h loop)
KERNEL_CASES = [(1, 1, 1, 4), (4, 63, 2, 32), (5, 64, 3, 60), (257, 65, 3, 32), (5, 130, 16, 256), (4, 50, 16, 68), (257, 1, 2, 64),
                (5, 65, 1, 32), (1, 130, 3, 4), (257, 63, 16, 60), (4, 64, 4, 256), (5, 1, 5, 68)]


@pytest.mark.parametrize('B,Lm,K,H', KERNEL_CASES)
def test_kernels_against_float64(B, Lm, K, H):
    from intel_sigir2023_amd import awelv
    dev = _dev()
    users = 50
    c = _case(B, Lm, K, H, users, seed=B * 1000 + Lm * 10 + K + H)
    w, weights, ens = awelv.awelv_forward(c['E'].to(dev), c['M'].to(dev), c['u'].to(dev), c['scores'].to(dev))
    c['w_dev'] = w
    E64, M64 = c['E'].double(), c['M'].double()
    rweights, rens = R.forward64(E64, M64, c['u'], c['scores'])
    assert weights.shape == (B, Lm, K) and ens.shape == (B, Lm) and w.shape == (B, K)
    for got, ref, what in ((weights, rweights, 'weights'), (ens, rens, 'ens_score'), (w, rweights[:, 0, :], 'w')):
        err = float((got.cpu().double() - ref).abs().max())
        print('%s: max error %.3g (bound %.3g)' % (what, err, _out_tol(ref)))
        assert err <= _out_tol(ref), what
    assert float((weights.cpu().double().sum(-1) - 1.0).abs().max()) < 1e-5
    # backward: d_uid_table is ADDED into (a known pattern of exactly representable values), d_model_table WRITTEN (pre-filled with NaN)
    pattern = ((torch.arange(users * H) % 7).float() * 0.25).reshape(users, H)
    rdE, rdM = R.backward64(E64, M64, c['u'], c['scores'], c['d_ens'], c['d_w'])
    d_uid, d_model, flags = _run_backward(c, dev, c['d_w'], pattern)
    present = torch.zeros(users, dtype=torch.bool)
    present[c['u'].long()] = True
    for got, ref, what in ((d_uid.double() - pattern.double(), rdE, 'd_uid_table'), (d_model.double(), rdM, 'd_model_table')):
        assert bool(torch.isfinite(got).all()), what
        err = float((got - ref).abs().max())
        print('%s: max error %.3g (bound %.3g)' % (what, err, _grad_tol(ref)))
        assert err <= _grad_tol(ref), what
    assert torch.equal(d_uid[~present], pattern[~present])                    # rows of absent users untouched ...
    assert torch.equal(flags, present.to(torch.uint8))                         # ... their flags 0, the flags of present users 1
    # d_weights = NULL is d_weights = 0
    rdE0, rdM0 = R.backward64(E64, M64, c['u'], c['scores'], c['d_ens'], None)
    zero = torch.zeros(users, H)
    d_uid0, d_model0, _ = _run_backward(c, dev, None, zero)
    d_uidz, d_modelz, _ = _run_backward(c, dev, torch.zeros_like(c['d_w']), zero)
    assert float((d_uid0.double() - rdE0).abs().max()) <= _grad_tol(rdE0) and float((d_model0.double() - rdM0).abs().max()) <= _grad_tol(rdM0)
    assert float((d_uidz.double() - rdE0).abs().max()) <= _grad_tol(rdE0)
    assert torch.equal(d_model0, d_modelz)


def test_arguments_outside_the_limits_are_refused():
    from intel_sigir2023_amd import awelv, _lib
    dev = _dev()
    for K, H in ((17, 32), (3, 30), (3, 260), (3, 0)):
        with pytest.raises(_lib.IntelHipError):
            awelv.awelv_forward(torch.zeros(8, H, device=dev), torch.zeros(K, H, device=dev), torch.zeros(2, dtype=torch.int32, device=dev),
                                torch.zeros(2, 5, K, device=dev))


def test_softmax_is_stable_at_saturated_logits():
    """Embeddings of +-2.5 at H = 32: logits up to +-200 (exp(200) overflows fp32: a softmax without the max subtraction returns NaN)."""
    from intel_sigir2023_amd import awelv
    dev = _dev()
    B, Lm, K, H, users = 8, 50, 3, 32, 8
    c = _case(B, Lm, K, H, users, seed=5, user_ids=torch.arange(B))
    g = torch.Generator().manual_seed(6)
    c['E'] = (torch.randint(0, 2, (users, H), generator=g).float() * 2 - 1) * 2.5
    c['M'] = (torch.randint(0, 2, (K, H), generator=g).float() * 2 - 1) * 2.5
    c['M'][0], c['M'][1] = c['E'][0], -c['E'][0]                 # session 0: logits +200 and -200
    w, weights, ens = awelv.awelv_forward(c['E'].to(dev), c['M'].to(dev), c['u'].to(dev), c['scores'].to(dev))
    c['w_dev'] = w
    E64, M64 = c['E'].double(), c['M'].double()
    z = E64 @ M64.t()
    assert float(z.max()) == 200.0 and float(z.min()) == -200.0
    rweights, rens = R.forward64(E64, M64, c['u'], c['scores'])
    for got, ref in ((weights, rweights), (ens, rens)):
        assert bool(torch.isfinite(got).all())
        assert float((got.cpu().double() - ref).abs().max()) <= _out_tol(ref)
    assert float((weights.cpu().double().sum(-1) - 1.0).abs().max()) < 1e-5
    rdE, rdM = R.backward64(E64, M64, c['u'], c['scores'], c['d_ens'], c['d_w'])
    d_uid, d_model, _ = _run_backward(c, dev, c['d_w'], torch.zeros(users, H))
    for got, ref in ((d_uid, rdE), (d_model, rdM)):
        assert bool(torch.isfinite(got).all())
        assert float((got.double() - ref).abs().max()) <= _grad_tol(ref)


@pytest.mark.parametrize('shared', [True, False], ids=['one_user_64_times', 'distinct_users'])
def test_duplicate_users_and_reproducibility(shared):
    from intel_sigir2023_amd import awelv
    dev = _dev()
    B, Lm, K, H, users = 64, 50, 3, 32, 80
    ids = torch.full((B,), 7) if shared else torch.randperm(users, generator=torch.Generator().manual_seed(2))[:B]
    c = _case(B, Lm, K, H, users, seed=9, user_ids=ids)
    c['w_dev'] = awelv.awelv_forward(c['E'].to(dev), c['M'].to(dev), c['u'].to(dev), c['scores'].to(dev))[0]
    rdE, rdM = R.backward64(c['E'].double(), c['M'].double(), c['u'], c['scores'], c['d_ens'], c['d_w'])
    zero = torch.zeros(users, H)
    a_uid, a_model, _ = _run_backward(c, dev, c['d_w'], zero)
    b_uid, b_model, _ = _run_backward(c, dev, c['d_w'], zero)
    assert float((a_uid.double() - rdE).abs().max()) <= _grad_tol(rdE)          # shared: row 7 is the sum of 64 sessions' rows
    assert float((a_model.double() - rdM).abs().max()) <= _grad_tol(rdM)
    assert torch.equal(a_model, b_model)                                         # fixed-order sum: bit-identical in both cases
    if shared:
        assert float(a_uid[7].abs().max()) > 0.0 and float(a_uid[torch.arange(users) != 7].abs().max()) == 0.0
    else:
        assert torch.equal(a_uid, b_uid)                                         # one addend per row: the atomics' order cannot matter


# ---- the reference's arrays -------------------------------------------------------------------------------------------------------------
def _model(cfg, sd, dev):
    from intel_sigir2023_amd import awelv
    args = make_args(cfg['args'], dev)
    model = awelv.aWELv(args, make_corpus(cfg['shape']))
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.to(dev).train(), args


def _noise(z, cfg, B, Lm):
    torch.manual_seed(cfg['noise_seed'])
    noise = torch.rand(B, Lm, Lm)            # the reference's draw (loss/BPRloss.py: torch.rand on the CPU generator), re-drawn with its seed
    assert np.array_equal(noise[0, 0, :8].numpy(), z['bpr_noise_head']), 'the CPU generator does not reproduce the fixture\'s noise draw'
    return noise


def _criterion(lname, args):
    from intel_sigir2023_amd import loss as loss_mod
    return {'list': loss_mod.Listloss, 'mse': loss_mod.MSEloss, 'bpr': loss_mod.BPRloss}[lname](args)


LOSS_CLASS = {'list': 'Listloss', 'mse': 'MSEloss', 'bpr': 'BPRloss'}


@pytest.mark.parametrize('lname', ['list', 'mse', 'bpr'])
@pytest.mark.parametrize('state', ['raw', 'scaled'])
def test_fixture_parity(state, lname):
    dev = _dev()
    z, cfg = R.load()
    model, args = _model(cfg, R.state(z, 'sd_raw' if state == 'raw' else 'sd'), dev)
    b = R.batch(z, 'in/', dev)
    B, Lm = b['ranking'].shape
    b['bpr_noise'] = _noise(z, cfg, B, Lm).to(dev)
    with torch.no_grad():
        o = model(b)
    assert sorted(o) == ['ens_score', 'weights']
    prefix = 'out_raw/' if state == 'raw' else 'out/'
    for key in ('weights', 'ens_score'):
        ref = torch.from_numpy(z[prefix + key])
        assert float((o[key].cpu() - ref).abs().max()) <= _out_tol(ref), key
    model.zero_grad()
    loss, l2_, l3_ = _criterion(lname, args)(model(b), b)
    loss.backward()
    ref_loss = float(z['%s/%s/loss' % (state, lname)])
    print('%s %s: loss %.7f, reference %.7f' % (state, lname, float(loss.detach()), ref_loss))
    assert abs(float(loss.detach()) - ref_loss) <= 1e-5
    for pn, p in model.named_parameters():
        ref = torch.from_numpy(z['%s/%s/grad/%s' % (state, lname, pn)])
        err = float((p.grad.cpu() - ref).abs().max())
        print('  grad %s: max error %.3g (bound %.3g)' % (pn, err, _grad_tol(ref)))
        assert err <= _grad_tol(ref), pn


@pytest.mark.parametrize('lname', ['list', 'mse', 'bpr'])
def test_engine_step_equals_the_autograd_path(lname):
    """One aWELvEngine.train_step from sd against zero_grad / forward / criterion / backward / torch.optim.Adam.step over the same kernels."""
    from intel_sigir2023_amd import awelv
    dev = _dev()
    z, cfg = R.load()
    lr, l2 = cfg['lr'], cfg['l2']
    b = R.batch(z, 'in/', dev)
    B, Lm = b['ranking'].shape
    b['bpr_noise'] = _noise(z, cfg, B, Lm).to(dev)
    fused, args = _model(cfg, R.state(z, 'sd'), dev)
    plain, _ = _model(cfg, R.state(z, 'sd'), dev)
    eng = awelv.aWELvEngine(fused, LOSS_CLASS[lname], args, lr=lr, l2=l2)
    loss_e, _, _ = eng.train_step(b)
    opt = torch.optim.Adam(plain.customize_parameters(), lr=lr, weight_decay=l2)
    opt.zero_grad()
    loss_a, _, _ = _criterion(lname, args)(plain(b), b)
    loss_a.backward()
    opt.step()
    torch.cuda.synchronize()
    assert abs(float(loss_e) - float(loss_a.detach())) <= 1e-5
    for pn in PARAMS:
        got, want = fused.state_dict()[pn].cpu(), plain.state_dict()[pn].cpu()
        init = R.state(z, 'sd')[pn]
        assert float((want - init).abs().max()) > 0.5 * lr                     # the step moved the parameters
        bound = 4.0 * torch.from_numpy(np.spacing(want.abs().numpy())) + 2e-5 * lr
        over = (got - want).abs() - bound
        print('%s %s: worst |engine - autograd| %.3g' % (lname, pn, float((got - want).abs().max())))
        assert float(over.max()) <= 0.0, (pn, float(over.max()))
    assert int(eng._flags.max()) == 0 and float(eng.grad['uid'].abs().max()) == 0.0      # the rows sweep consumed flags and gradient


def _traj_batches(z, cfg, dev):
    return [R.batch(z, 'traj/in%d/' % i, dev) for i in range(cfg['steps'])]


def _check_final(z, model):
    init = R.state(z, 'sd')
    for pn in PARAMS:
        got, want = model.state_dict()[pn].cpu().double(), torch.from_numpy(z['traj/final/' + pn]).double()
        move = (want - init[pn].double()).abs()
        err = (got - want).abs()
        outside = int((err > 2e-3 * move + 1e-7).sum())
        print('trajectory %s: worst error %.3g, largest move %.3g, %d elements outside the bound' % (pn, float(err.max()), float(move.max()), outside))
        assert outside == 0, pn


def test_ten_reference_steps_through_the_engine():
    from intel_sigir2023_amd import awelv
    dev = _dev()
    z, cfg = R.load()
    model, args = _model(cfg, R.state(z, 'sd'), dev)
    eng = awelv.aWELvEngine(model, 'Listloss', args, lr=cfg['lr'], l2=cfg['l2'])
    losses = [eng.train_step(b)[0] for b in _traj_batches(z, cfg, dev)]
    torch.cuda.synchronize()
    for step, (got, want) in enumerate(zip(losses, z['traj/losses'])):
        print('step %d: loss %.7f, reference %.7f' % (step, float(got), float(want)))
        assert abs(float(got) - float(want)) <= 1e-5, step
    _check_final(z, model)


def test_ten_reference_steps_through_the_runner():
    from intel_sigir2023_amd import awelv
    from intel_sigir2023_amd.runner import BaseRunner
    dev = _dev()
    z, cfg = R.load()
    model, args = _model(cfg, R.state(z, 'sd'), dev)
    rargs = BaseRunner.parse_runner_args(argparse.ArgumentParser()).parse_args([])
    for k, v in vars(args).items():
        setattr(rargs, k, v)
    rargs.lr, rargs.l2 = cfg['lr'], cfg['l2']
    runner = BaseRunner(rargs, use_engine=True)
    mean = runner.fit(model, _traj_batches(z, cfg, dev), _criterion('list', args), 'Listloss')
    assert type(runner.engine) is awelv.aWELvEngine                           # picked through aWELv.ENGINE
    assert abs(mean - float(np.mean(z['traj/losses']))) <= 1e-5
    _check_final(z, model)


# ---- runner end to end ------------------------------------------------------------------------------------------------------------------
def _float64_two_epochs(dev, seed, batch_size, train_batches, lr):
    """The run main() makes on the `tiny` workload, restated in float64 on the host: the same seeded initial state (the model is the first
    consumer of torch's CPU generator after main's torch.manual_seed), the same device-generated batches, torch.optim.Adam."""
    from intel_sigir2023_amd import synth
    torch.manual_seed(seed)
    E = torch.nn.Embedding(synth.WORKLOADS['tiny']['corpus']['users'], 32).weight.detach().double().requires_grad_(True)
    M = torch.nn.Embedding(3, 32).weight.detach().double().requires_grad_(True)
    opt = torch.optim.Adam([E, M], lr=lr)
    means = []
    for ep in range(2):
        ls = []
        for i in range(train_batches):
            b = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in synth.make_batch('tiny', batch_size, dev, seed=ep * 1000 + i, ragged=True).items()}
            opt.zero_grad()
            weights, ens = R.forward64(E, M, b['u_id_c'], b['scores'])
            loss = R.listloss64(weights, ens, b, 0, 0.01)
            loss.backward()
            opt.step()
            ls.append(float(loss.detach()))
        means.append(float(np.mean(ls)))
    return means


def test_main_trains_and_evaluates_on_the_tiny_workload():
    """main() with the CLI defaults (lr 1e-3, batch 256, 8 batches per epoch, N(0, 1) initialisation).  The training loss falls from epoch 1
    to epoch 2, and both epoch means equal the float64 restatement of the same run to 1e-4: the single-step loss bound of 1e-5 with room for
    16 steps of fp32 drift (the batches of the two epochs differ, so a fall alone could be the data's).  --use_engine 0 runs the same first
    epoch through autograd + torch.optim.Adam."""
    from intel_sigir2023_amd.main import main
    dev = _dev()
    argv = ['--model_name', 'aWELv', '--loss_name', 'Listloss', '--workload', 'tiny', '--epoch', '2', '--verbose', '30']
    res = main(argv)
    run = dict(main.last_run)
    assert 'NDCG@1' in res and 'pay_HR@1' in res and not [k for k in res if k.startswith('Int-')]
    assert all(np.isfinite(v) for v in res.values())
    first, second = run['train_losses']
    want = _float64_two_epochs(dev, 0, 256, 8, 1e-3)
    print('train losses %.7f -> %.7f; float64 restatement %.7f -> %.7f' % (first, second, want[0], want[1]))
    assert second < first
    assert abs(first - want[0]) <= 1e-4 and abs(second - want[1]) <= 1e-4
    res0 = main(argv[:-4] + ['--epoch', '1', '--verbose', '30', '--use_engine', '0'])
    assert 'NDCG@1' in res0 and not [k for k in res0 if k.startswith('Int-')]
    assert abs(main.last_run['train_losses'][0] - first) <= 1e-5
