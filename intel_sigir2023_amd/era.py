"""ERA (Evolutionary Rank Aggregation) -- the reference's genetic-algorithm baseline (``models/supervise/ERA.py`` and
``ERARunner.py``; Oliveira et al., CEC 2016) on the HIP path.

ERA is a genetic algorithm over the weights of a tiny MLP that scores every item from rank features of the base rankers
(``p10``, ``mAgr``, ``psc_m``).  The reference scores one solution at a time through ``pygad.torchga.predict`` and the numpy
``evaluate_method``; here the features of the dev set are computed once on the device (``intel_era_features``) and one launch per
dev batch scores the WHOLE population (``intel_era_fitness``).  The GA operators touch ``num_solutions x genes`` floats (100 x 113 by
default) and stay on the host, driven by a seeded ``np.random.Generator``: they are the operators the reference configures in
``pygad.GA`` (ERARunner.py:163-176), not a reproduction of pygad's random stream.  There is no CPU path.
"""
import ctypes as C
import logging

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import parallel
from .runner import BaseRunner, format_metric

K_TOURNAMENT = 7          # ERARunner.py:168


def _one_rank(what):
    if parallel.world_size() > 1:
        raise RuntimeError('%s runs on one rank only (data-parallel ERA is not implemented): start it without torchrun' % what)


# ---- kernels ----------------------------------------------------------------------------------------------------------
def era_features(scores, session_len, window):
    """ERA.Dataset._get_feed_dict (ERA.py:54-65) for a padded batch: scores [B, L, K] -> feat [B, L, 2 + K] fp32
    = [p10, mAgr, psc_0 .. psc_{K-1}], zeros from session_len on.  Ranks do not change under the feed's per-list min-max
    normalisation, so this runs on ``batch['scores']`` as the model receives them (cast to fp32 as the model does)."""
    L.require_gpu(scores)
    scores = scores.float().contiguous()
    sl = session_len.to(device=scores.device, dtype=torch.int32).contiguous()
    B, Lm, K = scores.shape
    feat = torch.empty(B, Lm, K + 2, dtype=torch.float32, device=scores.device)
    L.check(L.lib().intel_era_features(B, Lm, K, L.ptr(scores), L.ptr(sl), int(window), L.ptr(feat), L.stream_ptr(scores.device)),
            'intel_era_features')
    return feat


def era_fitness(pop, feat, ranking, session_len, width, hidden, gain_sum=None, want_pred=False):
    """gain_sum[p] += sum over the batch's sessions of solution p's NDCG@1 (intel_era_fitness); returns (gain_sum, pred or None).
    pop [P, G] fp32, feat [B, L, F] fp32, ranking [B, L] / session_len [B] int32, hidden: host list of hidden widths."""
    L.require_gpu(feat)
    dev = feat.device
    P = int(pop.shape[0])
    B, Lm, F = feat.shape
    if gain_sum is None:
        gain_sum = torch.zeros(P, dtype=torch.float64, device=dev)
    pred = torch.empty(P, B, Lm, dtype=torch.float32, device=dev) if want_pred else None
    lib = L.lib()
    ws = torch.empty(max(int(lib.intel_era_fitness_workspace_bytes(P, B)), 8), dtype=torch.uint8, device=dev)
    hid = (C.c_int * len(hidden))(*[int(h) for h in hidden])
    L.check(lib.intel_era_fitness(P, B, Lm, F, len(hidden), hid, L.ptr(pop), L.ptr(feat), L.ptr(ranking), L.ptr(session_len), int(width),
                                  L.ptr(gain_sum), L.ptr(pred), L.ptr(ws), L.stream_ptr(dev)), 'intel_era_fitness')
    return gain_sum, pred


# ---- model ------------------------------------------------------------------------------------------------------------
class ERA(nn.Module):
    reader, runner = 'BaseReader', 'ERARunner'
    extra_log_args = ['hidden_sizes']

    @staticmethod
    def parse_model_args(parser):
        """ERA.py:19-22 + BaseModel.py:20-27."""
        parser.add_argument('--window_size', type=int, default=10, help='mAgr Window size.')
        parser.add_argument('--hidden_sizes', type=str, default='16')
        parser.add_argument('--model_path', type=str, default='', help='Model save path.')
        parser.add_argument('--buffer', type=int, default=1, help='Whether to buffer feed dicts for dev/test')
        parser.add_argument('--model_num', type=int, default=2, help='Number of base models.')
        return parser

    def __init__(self, args, corpus):
        super().__init__()
        _one_rank('ERA')
        self.device = getattr(args, 'device', torch.device('cpu'))
        self.model_path = getattr(args, 'model_path', '')
        self.model_num = int(args.model_num)
        self.window_size = int(args.window_size)
        self.intent_num = len(getattr(corpus, 'zero_int', ()))           # what main.py's columnar feed asks of a model
        self.max_his = int(getattr(args, 'history_max', 20))
        # the reference hard-codes n_features = 5 = 2 + its three base rankers (ERA.py:28); here 2 + --model_num
        n_features = 2 + self.model_num
        self.hidden = [int(x) for x in str(args.hidden_sizes).split(',')]
        self.hidden_sizes = [n_features] + self.hidden
        self.mlp = nn.Sequential()                                      # ERA.py:31-37: same module names, same state_dict keys
        for i in range(len(self.hidden_sizes) - 1):
            self.mlp.add_module('Linear-%d' % i, nn.Linear(self.hidden_sizes[i], self.hidden_sizes[i + 1]))
            self.mlp.add_module('Activate-%d' % i, nn.ReLU())
        self.mlp.add_module('Linear-%d' % (len(self.hidden_sizes) - 1), nn.Linear(self.hidden_sizes[-1], 1))

    def count_variables(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def to(self, *a, **k):
        m = super().to(*a, **k)
        self.device = next(self.parameters()).device
        return m

    def save_model(self, model_path=None):
        torch.save(self.state_dict(), model_path or self.model_path)

    def load_model(self, model_path=None):
        self.load_state_dict(torch.load(model_path or self.model_path, map_location=self.device))

    @torch.no_grad()
    def forward(self, batch):
        """ERA.forward (ERA.py:39-45) -> ens_score [B, L] fp32 (pad slots 0): the features kernel, then the fitness kernel with a
        population of one and its predictions kept."""
        scores = batch['scores']
        L.require_gpu(scores)
        L.require_gpu(self.mlp[0].weight)
        feat = era_features(scores, batch['session_len'], self.window_size)
        B, Lm, _ = feat.shape
        sl = batch['session_len'].to(device=feat.device, dtype=torch.int32).contiguous()
        labels = torch.zeros(B, Lm, dtype=torch.int32, device=feat.device)       # the predictions do not depend on the labels
        pop = solution_from_model(self).reshape(1, -1).contiguous()
        _, pred = era_fitness(pop, feat, labels, sl, Lm, self.hidden, want_pred=True)
        return pred[0]


def solution_from_model(model):
    """The model's weights as one fp32 vector in pygad.torchga's layout (model_weights_as_vector): the state_dict order, per Linear
    weight [out, in] row-major then bias [out]."""
    return torch.cat([v.detach().reshape(-1) for v in model.state_dict().values()]).float()


@torch.no_grad()
def load_solution(model, vec):
    """Inverse of solution_from_model (pygad.torchga.model_weights_as_dict + load_state_dict)."""
    vec = torch.as_tensor(np.asarray(vec) if not torch.is_tensor(vec) else vec).reshape(-1)
    sd = model.state_dict()
    total = sum(v.numel() for v in sd.values())
    if vec.numel() != total:
        raise ValueError('solution has %d genes, the model %d' % (vec.numel(), total))
    at = 0
    for v in sd.values():
        v.copy_(vec[at:at + v.numel()].reshape(v.shape).to(device=v.device, dtype=v.dtype))
        at += v.numel()
    return model


# ---- genetic operators (host) -----------------------------------------------------------------------------------------
def initial_population(base, num_solutions, rng):
    """pygad.torchga.TorchGA.create_population: row 0 = the model's weights, rows 1.. = those weights + U(-1, 1)."""
    base = np.asarray(base, dtype=np.float32).reshape(-1)
    pop = np.tile(base, (int(num_solutions), 1))
    pop[1:] += rng.uniform(-1.0, 1.0, size=pop[1:].shape).astype(np.float32)
    return pop


def ga_step(pop, fitness, rng, num_parents_mating=5, elitism=2, crossover_prob=0.65, mutation_prob=0.25):
    """One generation with the operators of ERARunner.py:163-176: the `elitism` best solutions unchanged (ties -> lower index);
    `num_parents_mating` parents by tournament (K_TOURNAMENT draws with replacement, best fitness wins, ties -> lower index);
    offspring i from parents i mod n and (i + 1) mod n -- single-point crossover with probability crossover_prob, else a copy of the
    first; then every gene of an offspring, with probability mutation_prob, gets U(-1, 1) ADDED (mutation_by_replacement=False)."""
    pop = np.asarray(pop, dtype=np.float32)
    fitness = np.asarray(fitness, dtype=np.float64)
    S, G = pop.shape
    elitism = max(0, min(int(elitism), S))
    order = np.argsort(-fitness, kind='stable')
    out = np.empty_like(pop)
    out[:elitism] = pop[order[:elitism]]
    n = int(num_parents_mating)
    parents = np.empty((n, G), dtype=np.float32)
    for k in range(n):
        draws = rng.integers(0, S, size=K_TOURNAMENT)
        best = fitness[draws].max()
        parents[k] = pop[int(draws[fitness[draws] == best].min())]
    for i in range(S - elitism):
        a, b = parents[i % n], parents[(i + 1) % n]
        child = a.copy()
        if rng.random() < crossover_prob:
            cut = int(rng.integers(0, G))
            child[cut:] = b[cut:]
        mask = rng.random(G) < mutation_prob
        child[mask] += rng.uniform(-1.0, 1.0, size=int(mask.sum())).astype(np.float32)
        out[elitism + i] = child
    return out


# ---- runner -----------------------------------------------------------------------------------------------------------
class ERARunner(BaseRunner):
    @staticmethod
    def parse_runner_args(parser):
        """ERARunner.py:101-136 (the flags main.py's global parser already owns are not repeated)."""
        parser.add_argument('--epoch', type=int, default=200, help='Number of epochs.')
        parser.add_argument('--topk', type=str, default='1,3,5', help='The number of items recommended to each user.')
        parser.add_argument('--metrics', type=str, default='NDCG,HR', help='metrics: NDCG, HR')
        parser.add_argument('--main_metric', type=str, default='NDCG@1', help='main metric')
        parser.add_argument('--num_solutions', type=int, default=100)
        parser.add_argument('--num_generations', type=int, default=200)
        parser.add_argument('--num_parents_mating', type=int, default=5)
        parser.add_argument('--crossover_prob', type=float, default=0.65)
        parser.add_argument('--mutation_prob', type=float, default=0.25)
        parser.add_argument('--reproduction_prob', type=float, default=0.1, help='Parsed and never read, like the reference.')
        parser.add_argument('--elitism', type=int, default=2)
        parser.add_argument('--batch_size', type=int, default=256, help='Batch size during training.')
        parser.add_argument('--eval_batch_size', type=int, default=100, help='Batch size during testing.')
        parser.add_argument('--pin_memory', type=int, default=0, help='pin_memory in DataLoader')
        return parser

    def __init__(self, args, use_engine=True):
        _one_rank('ERARunner')
        self.args = args
        self.topk = [int(x) for x in args.topk.split(',')]
        self.metrics = [m.strip().upper() for m in args.metrics.split(',')]
        self.main_metric = args.main_metric
        self.num_solutions = int(args.num_solutions)
        self.num_generations = int(args.num_generations)
        self.num_parents_mating = int(args.num_parents_mating)
        self.crossover_prob = float(args.crossover_prob)
        self.mutation_prob = float(args.mutation_prob)
        self.elitism = int(args.elitism)
        self.random_seed = int(getattr(args, 'random_seed', 0))
        self.test_ensemble = 1
        self.device_metrics = True
        self._eval_sets = {}
        self.best_solution, self.best_fitness = None, None

    # ---- fitness of a population over an evaluation set ------------------------------------------------------------
    @staticmethod
    def prepare(model, batches):
        """The features of every batch, computed once and kept on the device (ERARunner.py:182-202 builds val_inputs once too);
        width = the reference's max_len = max(longest list of the whole set, the cutoff 1) (ERARunner.py:43 with topk = [1])."""
        sets, longest, n = [], 0, 0
        for b in batches:
            feat = era_features(b['scores'], b['session_len'], model.window_size)
            sl = b['session_len'].to(device=feat.device, dtype=torch.int32).contiguous()
            rk = b['ranking'].to(device=feat.device, dtype=torch.int32).contiguous()
            sets.append((feat, rk, sl))
            longest = max(longest, int(sl.max()))
            n += int(sl.shape[0])
        return {'sets': sets, 'width': max(longest, 1), 'n': n}

    @staticmethod
    def fitness(model, pop, prepared):
        """NDCG@1 of every row of pop [S, G] over the prepared set: one launch per batch into the same sums, S doubles back."""
        dev = prepared['sets'][0][0].device
        pop_d = torch.as_tensor(np.ascontiguousarray(pop, dtype=np.float32)).to(dev)
        gain = torch.zeros(pop_d.shape[0], dtype=torch.float64, device=dev)
        for feat, rk, sl in prepared['sets']:
            era_fitness(pop_d, feat, rk, sl, prepared['width'], model.hidden, gain_sum=gain)
        return gain.cpu().numpy() / float(prepared['n'])

    def train(self, model, data, criterion=None, loss_name=None):
        """ERARunner.train (:154-210).  Returns the best fitness of every generation's population; the best solution is loaded
        into the model."""
        _one_rank('ERARunner')
        prepared = self.prepare(model, data['dev'])
        rng = np.random.default_rng(self.random_seed)
        pop = initial_population(solution_from_model(model).cpu().numpy(), self.num_solutions, rng)
        fit = self.fitness(model, pop, prepared)
        curve = []
        best_i = int(np.argmax(fit))
        self.best_solution, self.best_fitness = pop[best_i].copy(), float(fit[best_i])
        for gen in range(self.num_generations):
            pop = ga_step(pop, fit, rng, self.num_parents_mating, self.elitism, self.crossover_prob, self.mutation_prob)
            fit = self.fitness(model, pop, prepared)
            best_i = int(np.argmax(fit))
            if fit[best_i] > self.best_fitness:
                self.best_solution, self.best_fitness = pop[best_i].copy(), float(fit[best_i])
            curve.append(float(fit[best_i]))
            logging.info('Generation = %d\tFitness = %.6f' % (gen + 1, fit[best_i]))
        load_solution(model, self.best_solution)
        logging.info('Fitness value of the best solution = %.6f' % self.best_fitness)
        return curve

    @torch.no_grad()
    def evaluate(self, model, batches, topk, metrics, criterion=None, **_):
        """ERARunner.evaluate (:212-242) over ALL batches of the set -> (0.0, the evaluate_method dict); ERA has no loss.  The
        reference's final evaluation keeps each batch with probability one half (:227); that is a defect and is not reproduced."""
        model.eval()
        if not isinstance(batches, list):
            batches = list(batches)
        width, lps = self._eval_set(batches, topk)
        dev = batches[0]['session_len'].device
        nk = len(topk)
        sums = torch.zeros(7 * nk, dtype=torch.float64, device=dev)
        counts = torch.zeros(4, dtype=torch.float64, device=dev)
        for batch, lp in zip(batches, lps):
            ens = model(batch)
            rk = batch['ranking'].to(torch.int32)
            sl = batch['session_len'].to(torch.int32)
            vals, valid = self.evaluate_method_device(ens, rk, sl, topk, metrics, width=width, label_pos=lp)
            w = torch.ones_like(vals)
            for t in range(3):
                w[:, t * nk * 2:(t + 1) * nk * 2] *= valid[:, t:t + 1].double()
            sums += torch.where(w > 0, vals, torch.zeros_like(vals)).sum(0)
            counts[:3] += valid.double().sum(0)
            counts[3] += vals.shape[0]
        c = counts.cpu().numpy()
        res = self.reduce_device_metrics(sums.cpu().numpy(), c[:3], float(c[3]), topk, metrics)
        logging.info('metrics: %s' % format_metric(res))
        return 0.0, res
