"""CPU-side checks of the ERA baseline (intel_sigir2023_amd/era.py): the three C-ABI entries exist, the CLI carries the reference's
defaults (models/supervise/ERA.py:19-22, ERARunner.py:101-136), the solution vector has pygad.torchga's layout, the host GA step
keeps its elites, its shape and its seed, and the model refuses to run off-GPU."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import ROOT

NEW_SYMBOLS = ('intel_era_features', 'intel_era_fitness_workspace_bytes', 'intel_era_fitness')


def _args(**over):
    d = dict(model_num=3, window_size=10, hidden_sizes='16', model_path='')
    d.update(over)
    return argparse.Namespace(**d)


def _model(**over):
    from intel_sigir2023_amd import era
    torch.manual_seed(0)
    return era.ERA(_args(**over), argparse.Namespace(zero_int=np.zeros(30)))


def test_header_exports_and_library_carry_the_era_symbols():
    from intel_sigir2023_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'intel_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, txt), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.intel_era_fitness_workspace_bytes(100, 65536) >= 100 * 8
    assert lib.intel_era_fitness_workspace_bytes(100, 0) == 0


def test_cli_defaults_match_the_reference():
    from intel_sigir2023_amd.main import build_parser, MODELS, RUNNERS
    assert 'ERA' in MODELS and 'ERARunner' in RUNNERS
    _, parser = build_parser(['--model_name', 'ERA', '--runner_name', 'ERARunner'])
    a, _ = parser.parse_known_args([])
    expect = dict(window_size=10, hidden_sizes='16', model_num=2, num_solutions=100, num_generations=200, num_parents_mating=5,
                  crossover_prob=0.65, mutation_prob=0.25, reproduction_prob=0.1, elitism=2, topk='1,3,5', metrics='NDCG,HR',
                  main_metric='NDCG@1', batch_size=256, eval_batch_size=100)
    for k, v in expect.items():
        assert getattr(a, k) == v, k


@pytest.mark.parametrize('hidden_sizes', ['16', '16,8'])
def test_solution_vector_round_trip_and_order(hidden_sizes):
    from intel_sigir2023_amd import era
    model = _model(hidden_sizes=hidden_sizes)
    n = len(hidden_sizes.split(','))
    assert list(model.state_dict()) == [k for i in range(n + 1) for k in ('mlp.Linear-%d.weight' % i, 'mlp.Linear-%d.bias' % i)]
    vec = era.solution_from_model(model)
    assert torch.equal(vec, torch.cat([v.flatten() for v in model.state_dict().values()]))
    assert vec.numel() == model.count_variables() == (113 if n == 1 else 5 * 16 + 16 + 16 * 8 + 8 + 8 + 1)
    new = torch.arange(vec.numel(), dtype=torch.float32) / 7
    era.load_solution(model, new.numpy())
    assert torch.equal(era.solution_from_model(model), new)
    assert torch.equal(model.mlp[0].weight, new[:5 * 16].reshape(16, 5))          # weight [out, in] row-major, then the bias
    assert torch.equal(model.mlp[0].bias, new[80:96])
    with pytest.raises(ValueError):
        era.load_solution(model, new[:-1])


def _stand_in_fitness(pop):
    return -np.abs(pop.astype(np.float64) - 0.5).sum(1)


def _step(seed, pop, **kw):
    from intel_sigir2023_amd import era
    return era.ga_step(pop, _stand_in_fitness(pop), np.random.default_rng(seed), **kw)


def test_ga_step_elites_shape_and_seed():
    from intel_sigir2023_amd import era
    rng = np.random.default_rng(0)
    pop = era.initial_population(np.linspace(-1, 1, 113), 20, rng)
    assert pop.shape == (20, 113) and pop.dtype == np.float32
    assert np.array_equal(pop[0], np.linspace(-1, 1, 113).astype(np.float32))      # row 0 = the model's weights
    assert (np.abs(pop[1:] - pop[0]) <= 1.0 + 1e-6).all() and (pop[1:] != pop[0]).any(1).all()
    fit = _stand_in_fitness(pop)
    new = _step(1, pop)
    assert new.shape == pop.shape and new.dtype == pop.dtype
    order = np.argsort(-fit, kind='stable')
    assert np.array_equal(new[:2], pop[order[:2]])                                 # the two elites, bit-identical, best first
    assert np.array_equal(new, _step(1, pop))                                      # same seed, same population
    assert not np.array_equal(new[2:], _step(2, pop)[2:])                          # another seed, other offspring
    assert np.array_equal(_step(2, pop)[:2], new[:2])
    four = _step(1, pop, elitism=4)
    assert np.array_equal(four[:4], pop[order[:4]])


def test_ga_step_elite_ties_go_to_the_lower_index_and_best_never_drops():
    from intel_sigir2023_amd import era
    pop = np.arange(6 * 4, dtype=np.float32).reshape(6, 4)
    fit = np.array([1.0, 3.0, 3.0, 0.0, 3.0, 2.0])
    new = era.ga_step(pop, fit, np.random.default_rng(0))
    assert np.array_equal(new[0], pop[1]) and np.array_equal(new[1], pop[2])
    # with the elites carried over, the best stand-in fitness is non-decreasing over generations
    rng = np.random.default_rng(5)
    pop = era.initial_population(np.zeros(30), 12, rng)
    best = []
    for _ in range(6):
        fit = _stand_in_fitness(pop)
        best.append(fit.max())
        pop = era.ga_step(pop, fit, rng)
    assert all(b >= a for a, b in zip(best, best[1:]))
    # without crossover or mutation every offspring is a copy of a tournament winner
    kids = era.ga_step(pop, _stand_in_fitness(pop), np.random.default_rng(1), crossover_prob=0.0, mutation_prob=0.0)
    assert all(any(np.array_equal(k, p) for p in pop) for k in kids)


def test_forward_on_cpu_tensors_raises():
    from intel_sigir2023_amd import _lib
    model = _model()
    batch = {'scores': torch.rand(2, 7, 3), 'session_len': torch.tensor([7, 3], dtype=torch.int32)}
    with pytest.raises(_lib.IntelHipError):
        model(batch)
