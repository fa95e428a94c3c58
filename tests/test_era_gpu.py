"""GPU tests of the ERA baseline (csrc/era.hip) through `intel_era_features` / `intel_era_fitness`, and of era.ERARunner.

The yardstick is a float64 numpy restatement, written below, of the formulae in include/intel_hip.h (ERA.py:31-65 and the "All"
NDCG@1 of ERARunner.evaluate_method, :43-57 and :87-97 of the reference).

Tolerances
  * features: bit-equal (ranks are integers, psc is the float32 rounding of a float64 quotient);
  * predictions: |pred - f64| <= 1e-5 * (1 + |f64|);
  * fitness: a (solution, session) pair is AMBIGUOUS when, in float64, a candidate with a different label lies within
    1e-4 * (1 + |best|) of the best prediction -- fp32 rounding may then pick another winner, which moves that pair's gain by at
    most 1.  Per solution: |fit_gpu - fit_f64| <= ambiguous_p / N + 1e-9, on inputs whose share of ambiguous pairs is at most 1 %.
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRED_TOL = 1e-5
AMB_TOL = 1e-4


# ======================================================================================================================
# float64 restatement
# ======================================================================================================================
def ref_features(scores, slen, window):
    """scores [B, L, K] float32 -> feat [B, L, 2 + K] float32 = [p10, mAgr, psc_0 ..]; zeros from slen on."""
    B, L, K = scores.shape
    feat = np.zeros((B, L, K + 2), dtype=np.float32)
    for b in range(B):
        n = int(slen[b])
        if n == 0:
            continue
        idx = np.arange(n)
        ranks = np.empty((K, n), dtype=np.int64)
        for m in range(K):
            x = scores[b, :n, m]
            better = (x[None, :] > x[:, None]) | ((x[None, :] == x[:, None]) & (idx[None, :] > idx[:, None]))      # [l, j]
            ranks[m] = 1 + better.sum(1)
            feat[b, :n, 2 + m] = (1.0 - (ranks[m] - 1).astype(np.float64) / n).astype(np.float32)
        feat[b, :n, 0] = (ranks <= 10).sum(0)
        feat[b, :n, 1] = 0.5 * (np.abs(ranks[1] - ranks[0]) <= window)
    return feat


def ref_pred(pop, feat, hidden):
    """pop [P, G], feat [B, L, F] -> float64 predictions [P, B, L] of the MLP (Linear + ReLU per hidden width, linear output)."""
    pop = np.asarray(pop, dtype=np.float64)
    h = np.broadcast_to(np.asarray(feat, dtype=np.float64)[None], (pop.shape[0],) + feat.shape)
    at, fan_in = 0, feat.shape[2]
    for i, out in enumerate(list(hidden) + [1]):
        W = pop[:, at:at + out * fan_in].reshape(-1, out, fan_in)
        at += out * fan_in
        bias = pop[:, at:at + out]
        at += out
        h = np.einsum('pblf,pof->pblo', h, W) + bias[:, None, None, :]
        if i < len(hidden):
            h = np.maximum(h, 0.0)
        fan_in = out
    assert at == pop.shape[1]
    return h[..., 0]


def genes(F, hidden):
    g, fan_in = 0, F
    for h in hidden:
        g += h * fan_in + h
        fan_in = h
    return g + fan_in + 1


def ref_gain(pred, ranking, slen, width):
    """pred [P, B, L] float64 -> (gain [P, B], ambiguous [P, B] bool)."""
    P, B, _ = pred.shape
    gain = np.zeros((P, B))
    amb = np.zeros((P, B), dtype=bool)
    for b in range(B):
        n = int(slen[b])
        cand = pred[:, b, :n]
        lab = np.maximum(ranking[b, :n], 0).astype(np.int64)
        if n < width:                                  # one pad candidate: prediction 0, label 0
            cand = np.concatenate([cand, np.zeros((P, 1))], axis=1)
            lab = np.concatenate([lab, [0]])
        if cand.shape[1] == 0:
            continue
        best = cand.max(1)
        win = np.where(cand == best[:, None], lab[None, :], np.iinfo(np.int64).max).min(1)      # equal predictions: smallest label
        gain[:, b] = win / max(1, int(lab.max()))
        near = cand >= (best - AMB_TOL * (1.0 + np.abs(best)))[:, None]
        amb[:, b] = (near & (lab[None, :] != win[:, None])).any(1)
    return gain, amb


# ======================================================================================================================
# C ABI
# ======================================================================================================================
def _dev():
    return torch.device('cuda:0')


def _lib():
    from intel_sigir2023_amd import _lib as L
    return L, L.lib()


def gpu_features(scores, slen, window, expect_rc=0):
    L, lib = _lib()
    dev = _dev()
    B, Lm, K = scores.shape
    s = torch.from_numpy(np.array(scores, dtype=np.float32)).to(dev)
    sl = torch.from_numpy(np.array(slen, dtype=np.int32)).to(dev)
    feat = torch.full((B, Lm, K + 2), -777.0, dtype=torch.float32, device=dev)
    rc = lib.intel_era_features(B, Lm, K, L.ptr(s), L.ptr(sl), int(window), L.ptr(feat), L.stream_ptr(dev))
    torch.cuda.synchronize()
    assert (rc == 0) == (expect_rc == 0), lib.intel_last_error()
    return feat.cpu().numpy(), rc


def gpu_fitness(pop, feat, ranking, slen, width, hidden, gain=None, want_pred=False, F=None, L_=None):
    """-> (rc, gain_sum [P] float64 numpy, pred [P, B, L] numpy or None)."""
    L, lib = _lib()
    dev = _dev()
    P = pop.shape[0]
    B, Lm, Ff = feat.shape
    F = Ff if F is None else F
    Lm = Lm if L_ is None else L_
    pop_d = torch.from_numpy(np.array(pop, dtype=np.float32)).to(dev)
    feat_d = torch.from_numpy(np.array(feat, dtype=np.float32)).to(dev)
    rk = torch.from_numpy(np.array(ranking, dtype=np.int32)).to(dev)
    sl = torch.from_numpy(np.array(slen, dtype=np.int32)).to(dev)
    g = torch.zeros(P, dtype=torch.float64, device=dev) if gain is None else gain
    pred = torch.full((P, B, Lm), -777.0, dtype=torch.float32, device=dev) if want_pred else None
    nbytes = int(lib.intel_era_fitness_workspace_bytes(P, B))
    ws = torch.full((max(nbytes, 8),), 0xFF, dtype=torch.uint8, device=dev)          # NaN bit patterns: a partial nobody wrote shows
    hid = (C.c_int * len(hidden))(*hidden)
    rc = lib.intel_era_fitness(P, B, Lm, F, len(hidden), hid, L.ptr(pop_d), L.ptr(feat_d), L.ptr(rk), L.ptr(sl), int(width), L.ptr(g),
                               L.ptr(pred), L.ptr(ws), L.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, g, (pred.cpu().numpy() if want_pred else None)


# ======================================================================================================================
# inputs
# ======================================================================================================================
def distinct_scores(rng, B, L, K):
    """Scores that are pairwise distinct in fp32 within every (session, ranker): a permutation of an arithmetic grid."""
    s = np.empty((B, L, K), dtype=np.float32)
    for b in range(B):
        for m in range(K):
            s[b, :, m] = (rng.permutation(L).astype(np.float32) + 0.25) / np.float32(L + 1)
    return s


def ragged_lengths(rng, B, L):
    """Lengths that include 1, 10, 11 (the p10 threshold) and L wherever they fit."""
    slen = rng.integers(1, L + 1, size=B)
    must = [v for v in (L, 1, 10, 11) if v <= L]
    for i, v in enumerate(must[:B]):
        slen[i] = v
    if B == 1:
        slen[0] = L
    return slen.astype(np.int32)


@functools.lru_cache(maxsize=None)
def fitness_case(hidden=(16,), N=257, L=13, P=33, K=3, seed=0):
    """Shared, read-only: features from the restatement, U(-1, 1) weights, labels in {-1 .. 3}, ragged lengths incl. 1 and L."""
    rng = np.random.default_rng(seed)
    scores = distinct_scores(rng, N, L, K)
    slen = rng.integers(1, L + 1, size=N).astype(np.int32)
    slen[0], slen[1] = L, 1
    feat = ref_features(scores, slen, 3)
    ranking = rng.integers(-1, 4, size=(N, L)).astype(np.int32)
    pop = rng.uniform(-1.0, 1.0, size=(P, genes(K + 2, hidden))).astype(np.float32)
    pred = ref_pred(pop, feat, hidden)
    for a in (feat, ranking, pop, pred, slen):
        a.setflags(write=False)
    return dict(feat=feat, ranking=ranking, slen=slen, pop=pop, pred=pred, hidden=list(hidden), N=N, L=L, P=P)


# ======================================================================================================================
# features
# ======================================================================================================================
@pytest.mark.parametrize('window', [0, 3])
@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('L', [1, 11, 63, 64, 65, 130])
@pytest.mark.parametrize('B', [1, 5, 9])
def test_features_bit_equal(B, L, K, window):
    rng = np.random.default_rng(1000 * B + 10 * L + K)
    scores = distinct_scores(rng, B, L, K)
    slen = ragged_lengths(rng, B, L)
    got, _ = gpu_features(scores, slen, window)
    ref = ref_features(scores, slen, window)
    assert got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.argwhere(got != ref)[:5]


def test_features_tie_rule():
    """Equal scores: the LATER slot ranks better (np.argsort(x)[::-1] in its stable form)."""
    scores = np.zeros((2, 12, 2), dtype=np.float32)
    scores[0, :4, 0] = [0.5, 0.5, 0.5, 0.5]          # ranks 4, 3, 2, 1
    scores[0, :4, 1] = [0.9, 0.1, 0.9, 0.1]          # ranks 2, 4, 1, 3
    scores[1, :, 0] = 0.25                           # twelve equal scores: ranks 12 .. 1, so p10 counts slots 2 .. 11 only
    scores[1, :, 1] = np.arange(12) / 12.0           # ranks 12 .. 1 as well
    slen = np.array([4, 12], dtype=np.int32)
    got, _ = gpu_features(scores, slen, 1)
    ref = ref_features(scores, slen, 1)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert got[0, :4, 2].tolist() == [0.25, 0.5, 0.75, 1.0]                      # psc_0 = 1 - (rank - 1) / 4
    assert got[0, :4, 1].tolist() == [0.0, 0.5, 0.5, 0.0]                        # |rank_1 - rank_0| = 2, 1, 1, 2 against window 1
    assert got[1, :, 0].tolist() == [0.0, 0.0] + [2.0] * 10
    assert not got[0, 4:].any()


# ======================================================================================================================
# predictions
# ======================================================================================================================
@pytest.mark.parametrize('P', [1, 33])
@pytest.mark.parametrize('hidden', [(16,), (5,), (64,), (16, 8)], ids=lambda h: 'h' + 'x'.join(map(str, h)))
def test_predictions_against_float64(hidden, P):
    c = fitness_case(hidden=hidden, N=37, L=13, P=P, seed=7)
    rc, _, pred = gpu_fitness(c['pop'], c['feat'], c['ranking'], c['slen'], c['L'], c['hidden'], want_pred=True)
    assert rc == 0
    valid = np.arange(c['L'])[None, :] < c['slen'][:, None]
    ref = c['pred']
    err = np.abs(pred - ref) / (1.0 + np.abs(ref))
    print('max scaled prediction error %.3g' % err[:, valid].max())
    assert err[:, valid].max() <= PRED_TOL
    assert (pred[:, ~valid] == 0.0).all()                       # pad slots are exactly 0


@pytest.mark.parametrize('L', [70, 200])
def test_predictions_long_lists(L):
    """More than one item per lane (two and four)."""
    c = fitness_case(hidden=(16,), N=6, L=L, P=3, seed=11)
    rc, g, pred = gpu_fitness(c['pop'], c['feat'], c['ranking'], c['slen'], L, c['hidden'], want_pred=True)
    assert rc == 0
    valid = np.arange(L)[None, :] < c['slen'][:, None]
    err = np.abs(pred - c['pred']) / (1.0 + np.abs(c['pred']))
    assert err[:, valid].max() <= PRED_TOL and (pred[:, ~valid] == 0.0).all()
    gain, amb = ref_gain(c['pred'], c['ranking'], c['slen'], L)
    assert (np.abs(g.cpu().numpy() - gain.sum(1)) <= amb.sum(1) + 1e-9).all()


# ======================================================================================================================
# fitness
# ======================================================================================================================
@pytest.mark.parametrize('pad', ['longest', 'L+2'])
def test_fitness_against_float64(pad):
    c = fitness_case()
    N, L = c['N'], c['L']
    width = int(c['slen'].max()) if pad == 'longest' else L + 2
    gain, amb = ref_gain(c['pred'], c['ranking'], c['slen'], width)
    share = amb.mean()
    print('ambiguous pairs: %d of %d (%.3f %%)' % (amb.sum(), amb.size, 100 * share))
    assert share <= 0.01                                        # a condition on the inputs
    rc, g, _ = gpu_fitness(c['pop'], c['feat'], c['ranking'], c['slen'], width, c['hidden'])
    assert rc == 0
    fit_gpu, fit_ref = g.cpu().numpy() / N, gain.sum(1) / N
    print('max |fit_gpu - fit_f64| = %.3g' % np.abs(fit_gpu - fit_ref).max())
    assert (np.abs(fit_gpu - fit_ref) <= amb.sum(1) / N + 1e-9).all()


def _zero_pop(b2, F=5, H=16):
    pop = np.zeros((1, genes(F, [H])), dtype=np.float32)
    pop[0, -1] = b2
    return pop


def test_fitness_exact_cases():
    """All-zero weights make every prediction equal the output bias: fp32 and float64 agree bit for bit."""
    L = 6
    ranking = np.array([[2, 1, 3, 0, 0, 0],        # len 3: lowest label 1 of max 3
                        [0, 3, 0, 0, 0, 0],        # len 2: lowest label 0
                        [-1, 0, -1, 0, 0, 0],      # len 4: all labels <= 0 -> gain 0, never NaN
                        [2, 9, 9, 9, 9, 9],        # len 1: the one item wins
                        [3, 2, 2, 3, 2, 3]],       # len 6 == L: lowest label 2 of max 3
                       dtype=np.int32)
    slen = np.array([3, 2, 4, 1, 6], dtype=np.int32)
    feat = ref_features(distinct_scores(np.random.default_rng(3), 5, L, 3), slen, 3)
    # b2 = 0.5 beats the pad (0): the lowest label of every session wins
    rc, g, _ = gpu_fitness(_zero_pop(0.5), feat, ranking, slen, L + 2, [16])
    assert rc == 0 and abs(g.item() - (1 / 3 + 0.0 + 0.0 + 1.0 + 2 / 3)) <= 1e-12          # 1e-12: the order of five double adds
    # b2 = -0.5 where every session owns a pad: the pad wins, every gain is 0
    rc, g, _ = gpu_fitness(_zero_pop(-0.5), feat, ranking, slen, L + 2, [16])
    assert rc == 0 and g.item() == 0.0
    # the same weights with len == width: the full list owns no pad and its lowest label wins again
    rc, g, _ = gpu_fitness(_zero_pop(-0.5), feat, ranking, slen, L, [16])
    assert rc == 0 and abs(g.item() - 2 / 3) <= 1e-12
    # one session at a time: all labels <= 0, and the one-item session
    for b, want in ((2, 0.0), (3, 1.0)):
        rc, g, _ = gpu_fitness(_zero_pop(0.5), feat[b:b + 1], ranking[b:b + 1], slen[b:b + 1], L, [16])
        assert rc == 0 and g.item() == want and np.isfinite(g.item())


def test_fitness_accumulates_and_is_reproducible():
    c = fitness_case()
    width = c['L'] + 2
    args = lambda lo, hi: (c['pop'], c['feat'][lo:hi], c['ranking'][lo:hi], c['slen'][lo:hi], width, c['hidden'])
    _, whole, _ = gpu_fitness(*args(0, c['N']))
    _, again, _ = gpu_fitness(*args(0, c['N']))
    assert torch.equal(whole, again)                            # bit-identical
    _, part, _ = gpu_fitness(*args(0, 100))
    _, part, _ = gpu_fitness(*args(100, c['N']), gain=part)     # chained into the same sums
    a, b = whole.cpu().numpy(), part.cpu().numpy()
    assert (np.abs(a - b) <= 1e-12 * np.abs(a)).all()
    _, twice, _ = gpu_fitness(*args(0, c['N']), gain=whole.clone())
    assert np.allclose(twice.cpu().numpy(), 2 * a, rtol=1e-12)  # never reset


def test_fitness_many_sessions_per_wave():
    """B >= 65 536: a wave owns two consecutive sessions (the shape-dependent split of era.hip)."""
    c = fitness_case(hidden=(5,), N=257, L=13, P=3, seed=5)
    reps = 256
    B = 257 * reps
    feat, ranking, slen = (np.tile(c[k], (reps,) + (1,) * (c[k].ndim - 1)) for k in ('feat', 'ranking', 'slen'))
    gain, amb = ref_gain(c['pred'], c['ranking'], c['slen'], 13)
    rc, g, _ = gpu_fitness(c['pop'], feat, ranking, slen, 13, c['hidden'])
    assert rc == 0
    assert (np.abs(g.cpu().numpy() / B - gain.sum(1) / 257) <= amb.sum(1) / 257 + 1e-9).all()


def test_argument_checks_launch_nothing():
    L, lib = _lib()
    c = fitness_case(hidden=(16,), N=37, L=13, P=1, seed=7)
    lib.intel_prof_timeline()
    lib.intel_prof_enable(1)
    try:
        # K = 1
        _, rc = gpu_features(np.zeros((2, 4, 1), dtype=np.float32), [4, 4], 3, expect_rc=-1)
        assert rc != 0 and b'K=1' in lib.intel_last_error()
        # L = 257
        _, rc = gpu_features(np.zeros((1, 257, 2), dtype=np.float32), [4], 3, expect_rc=-1)
        assert rc != 0 and b'257' in lib.intel_last_error()
        rc, g, _ = gpu_fitness(c['pop'], c['feat'], c['ranking'], c['slen'], 13, [16], L_=257)
        assert rc != 0 and b'257' in lib.intel_last_error() and g.item() == 0.0
        # three hidden layers
        rc, g, _ = gpu_fitness(c['pop'], c['feat'], c['ranking'], c['slen'], 13, [4, 4, 4])
        assert rc != 0 and b'hidden layers' in lib.intel_last_error() and g.item() == 0.0
        # a hidden width of 65
        rc, g, _ = gpu_fitness(c['pop'], c['feat'], c['ranking'], c['slen'], 13, [65])
        assert rc != 0 and b'65' in lib.intel_last_error() and g.item() == 0.0
        torch.cuda.synchronize()
        recs = json.loads(lib.intel_prof_timeline().decode())
    finally:
        lib.intel_prof_enable(0)
    assert [r['name'] for r in recs if 'era' in r['name']] == []


# ======================================================================================================================
# runner
# ======================================================================================================================
@functools.lru_cache(maxsize=None)
def runner_case():
    """One seeded GA run on the tiny workload (12 solutions, 5 generations, two dev batches of 32 sessions), shared by the tests."""
    from intel_sigir2023_amd import era, synth
    from intel_sigir2023_amd.main import build_parser
    dev = _dev()
    argv = ['--model_name', 'ERA', '--runner_name', 'ERARunner', '--num_solutions', '12', '--num_generations', '5', '--random_seed', '3']
    _, parser = build_parser(argv)
    parser.set_defaults(**synth.WORKLOADS['tiny']['flags'])
    args, _ = parser.parse_known_args(argv)
    args.device = dev
    corpus, _ = synth.make_corpus('tiny')
    dev_batches = [synth.make_batch('tiny', 32, dev, seed=10_000 + i, ragged=True) for i in range(2)]
    data = {'dev': dev_batches, 'test': dev_batches}

    def run():
        torch.manual_seed(0)
        model = era.ERA(args, corpus).to(dev)
        runner = era.ERARunner(args)
        return model, runner, runner.train(model, data)
    model, runner, curve = run()
    _, _, curve2 = run()
    return dict(model=model, runner=runner, curve=curve, curve2=curve2, data=data, args=args)


def test_runner_curve_is_monotone_and_seeded():
    r = runner_case()
    assert len(r['curve']) == 5
    assert all(b >= a for a, b in zip(r['curve'], r['curve'][1:]))
    assert r['curve'] == r['curve2']
    assert r['runner'].best_fitness == r['curve'][-1]


def test_runner_best_fitness_is_the_loaded_models():
    from intel_sigir2023_amd import era
    r = runner_case()
    model, runner = r['model'], r['runner']
    sol = era.solution_from_model(model).cpu().numpy()
    assert np.array_equal(sol, runner.best_solution)
    prepared = runner.prepare(model, r['data']['dev'])
    fresh = runner.fitness(model, sol[None, :], prepared)
    assert fresh.shape == (1,) and fresh[0] == runner.best_fitness
    # ... and the float64 restatement's value of that solution, within the ambiguity bound
    gains, ambs, n = 0.0, 0, 0
    for b, (feat_d, _, _) in zip(r['data']['dev'], prepared['sets']):
        scores = b['scores'].float().cpu().numpy()
        slen = b['session_len'].cpu().numpy()
        feat = ref_features(scores, slen, model.window_size)
        assert np.array_equal(feat.view(np.uint32), feat_d.cpu().numpy().view(np.uint32))
        gain, amb = ref_gain(ref_pred(sol[None, :], feat, model.hidden), b['ranking'].cpu().numpy(), slen, prepared['width'])
        gains, ambs, n = gains + gain.sum(), ambs + int(amb.sum()), n + len(slen)
    assert n == 64 and abs(runner.best_fitness - gains / n) <= ambs / n + 1e-9


def test_runner_evaluate_keys():
    from intel_sigir2023_amd.runner import BaseRunner
    r = runner_case()
    runner = r['runner']
    loss, res = runner.evaluate(r['model'], r['data']['test'], runner.topk, runner.metrics)
    # the keys of BaseRunner.evaluate's evaluate_method part for the same topk / metrics (ERA predicts no intents)
    want = BaseRunner.reduce_device_metrics(np.zeros(7 * len(runner.topk)), np.ones(3), 1.0, runner.topk, runner.metrics)
    assert sorted(res) == sorted(want) and 'NDCG@1' in res
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in res.values())
    ens = r['model'](r['data']['test'][0])
    assert ens.shape == r['data']['test'][0]['ranking'].shape and ens.dtype == torch.float32
