"""aWELv -- the reference's per-user fusion-weight baseline (``models/supervise/aWELv.py``; Liu, Du, Wu, JMLR 23 (2022)) on the HIP path:
the method ``aWELv_IntEL`` extends and the first line of the reference's comparison table (``script/baselines.sh:33``).

A user embedding table E [users, H] and a base-ranker embedding table M [K, H]; a session of user u fuses its K base scores with
``w = softmax_k(E[u] . M[k])``.  Forward and backward are one launch each (csrc/awelv.hip: ``intel_awelv_forward`` /
``intel_awelv_backward``); ``aWELv.forward`` goes through a ``torch.autograd.Function`` over the two, so the loss classes of loss.py and
``torch.optim.Adam`` train it unchanged, and ``aWELvEngine`` is the fused step (forward, one loss launch with gradients, backward with
row flags, the Adam launches; no host synchronisation in between).  There is no CPU path.
"""
import ctypes as C
import logging
import os

import torch
import torch.nn as nn

from . import _lib as L
from . import parallel

PLAIN_LOSSES = ('Listloss', 'BPRloss', 'MSEloss')
ADAM_ROWS_D = (16, 32, 64, 128, 256)          # row widths of intel_adam_step_rows


def _one_rank(what):
    if parallel.world_size() > 1:
        raise RuntimeError('%s runs on one rank only (data-parallel aWELv is not implemented): start it without torchrun' % what)


def plain_loss_message(loss_name):
    return ('aWELv predicts no intent: --loss_name %s is not available for it, use one of %s' % (loss_name, ', '.join(PLAIN_LOSSES)))


# ---- kernels ----------------------------------------------------------------------------------------------------------
def _f32(t):
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _i32(t, device):
    return t if (t.dtype == torch.int32 and t.is_contiguous() and t.device == device) else t.to(device=device, dtype=torch.int32).contiguous()


def awelv_forward(uid_table, model_table, u_id, scores):
    """aWELv.forward (aWELv.py:26-40): uid_table [users, H], model_table [K, H], u_id [B], scores [B, L, K] ->
    (w [B, K], weights [B, L, K], ens_score [B, L]) fp32; every l < L is computed, pads included (the reference does not mask)."""
    L.require_gpu(scores)
    L.require_gpu(uid_table)
    L.require_gpu(model_table)
    dev = scores.device
    # temporaries stay referenced until the launch is enqueued
    E, M, u, sc = _f32(uid_table.detach()), _f32(model_table.detach()), _i32(u_id, dev), _f32(scores.detach())
    B, Lm, K = sc.shape
    users, H = E.shape
    if M.shape != (K, H):
        raise L.IntelHipError('aWELv: model table %s does not fit scores [.., %d] and hidden size %d' % (tuple(M.shape), K, H))
    w = torch.empty(B, K, dtype=torch.float32, device=dev)
    weights = torch.empty(B, Lm, K, dtype=torch.float32, device=dev)
    ens = torch.empty(B, Lm, dtype=torch.float32, device=dev)
    L.check(L.lib().intel_awelv_forward(B, Lm, K, H, L.ptr(E), users, L.ptr(M), L.ptr(u), L.ptr(sc), L.ptr(w), L.ptr(weights), L.ptr(ens),
                                        L.stream_ptr(dev)), 'intel_awelv_forward')
    return w, weights, ens


def awelv_backward(uid_table, model_table, u_id, scores, w, d_ens, d_weights, d_uid_table, d_model_table, row_flags=None):
    """The autograd backward of aWELv.forward: d_uid_table [users, H] is ADDED into (and row_flags[u_b] set when given),
    d_model_table [K, H] is WRITTEN; d_weights may be None (= zeros).  Returns (d_uid_table, d_model_table)."""
    L.require_gpu(scores)
    L.require_gpu(d_uid_table)
    dev = scores.device
    E, M, u, sc = _f32(uid_table.detach()), _f32(model_table.detach()), _i32(u_id, dev), _f32(scores.detach())
    wc, de = _f32(w), _f32(d_ens)
    dw = None if d_weights is None else _f32(d_weights)
    B, Lm, K = sc.shape
    users, H = E.shape
    for t, shape, what in ((d_uid_table, (users, H), 'd_uid_table'), (d_model_table, (K, H), 'd_model_table'), (wc, (B, K), 'w'), (de, (B, Lm), 'd_ens')):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise L.IntelHipError('aWELv backward: %s must be a contiguous fp32 tensor of shape %s' % (what, shape))
    lib = L.lib()
    workspace = torch.empty(max(int(lib.intel_awelv_backward_workspace_bytes(B, K, H)), 8), dtype=torch.uint8, device=dev)
    L.check(lib.intel_awelv_backward(B, Lm, K, H, L.ptr(E), users, L.ptr(M), L.ptr(u), L.ptr(sc), L.ptr(wc), L.ptr(de), L.ptr(dw),
                                     L.ptr(d_uid_table), L.ptr(row_flags), L.ptr(d_model_table), L.ptr(workspace), L.stream_ptr(dev)),
            'intel_awelv_backward')
    return d_uid_table, d_model_table


class _aWELvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, uid_table, model_table, u_id, scores):
        u, sc = _i32(u_id, scores.device), _f32(scores.detach())
        w, weights, ens = awelv_forward(uid_table, model_table, u, sc)
        ctx.save_for_backward(uid_table, model_table, u, sc, w)
        return weights, ens

    @staticmethod
    def backward(ctx, d_weights, d_ens):
        uid_table, model_table, u, sc, w = ctx.saved_tensors
        d_uid = torch.zeros(uid_table.shape, dtype=torch.float32, device=sc.device)       # dense, like nn.Embedding(sparse=False)
        d_model = torch.empty(model_table.shape, dtype=torch.float32, device=sc.device)
        awelv_backward(uid_table, model_table, u, sc, w, d_ens, d_weights, d_uid, d_model)
        return d_uid.to(uid_table.dtype), d_model.to(model_table.dtype), None, None


# ---- model ------------------------------------------------------------------------------------------------------------
class aWELv(nn.Module):
    reader, runner = 'BaseReader', 'BaseRunner'
    extra_log_args = []

    @staticmethod
    def parse_model_args(parser):
        """aWELv.py:16-18 + BaseModel.py:20-27."""
        parser.add_argument('--hidden_size', type=int, default=32)
        parser.add_argument('--model_path', type=str, default='', help='Model save path.')
        parser.add_argument('--buffer', type=int, default=1, help='Whether to buffer feed dicts for dev/test')
        parser.add_argument('--model_num', type=int, default=2, help='Number of base models.')
        return parser

    def __init__(self, args, corpus):
        super().__init__()
        _one_rank('aWELv')
        self.device = getattr(args, 'device', torch.device('cpu'))
        self.model_path = getattr(args, 'model_path', '')
        self.buffer = getattr(args, 'buffer', 1)
        self.optimizer = None
        self.model_num = int(args.model_num)
        self.hidden_size = int(args.hidden_size)
        self.intent_num = len(getattr(corpus, 'zero_int', ()))           # what main.py's columnar feed asks of a model
        self.max_his = int(getattr(args, 'history_max', 20))
        self.user_num = int(corpus.max_uid + 1)
        # aWELv.py:23-24: this order and torch's default N(0, 1) initialisation, so the same torch.manual_seed gives the reference's state_dict
        self.uid_embeddings = nn.Embedding(self.user_num, self.hidden_size)
        self.model_embeddings = nn.Embedding(self.model_num, self.hidden_size)

    # ---- reference auxiliary API (BaseModel.py:53-78) -------------------------------------------
    def customize_parameters(self, define_dict={}):
        weight_p, bias_p = [], []
        for name, p in filter(lambda x: x[1].requires_grad, self.named_parameters()):
            (bias_p if 'bias' in name else weight_p).append(p)
        return [{'params': weight_p}, {'params': bias_p, 'weight_decay': 0}]

    def count_variables(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def save_model(self, model_path=None):
        model_path = model_path or self.model_path
        d = os.path.dirname(model_path)
        if d and not os.path.exists(d):
            os.makedirs(d)
        torch.save(self.state_dict(), model_path)

    def load_model(self, model_path=None):
        model_path = model_path or self.model_path
        self.load_state_dict(torch.load(model_path, map_location=self.device))
        logging.info('Load model from ' + model_path)

    def to(self, *a, **k):
        m = super().to(*a, **k)
        self.device = next(self.parameters()).device
        return m

    def forward(self, batch):
        """aWELv.forward (aWELv.py:26-40) -> {'weights' [B, L, K], 'ens_score' [B, L]}; no 'intents' key, like the reference."""
        scores = batch['scores']
        L.require_gpu(scores)
        L.require_gpu(self.uid_embeddings.weight)
        if scores.shape[2] != self.model_num:
            raise L.IntelHipError('aWELv: the batch carries %d base scores, --model_num is %d' % (scores.shape[2], self.model_num))
        weights, ens = _aWELvFunction.apply(self.uid_embeddings.weight, self.model_embeddings.weight, batch['u_id_c'], scores)
        return {'weights': weights, 'ens_score': ens}


# ---- fused training step ----------------------------------------------------------------------------------------------
class aWELvEngine(object):
    """What BaseRunner.fit uses of an engine (train_step, set_lr, flush, defer_table_wait) for aWELv: forward -> loss with gradients ->
    backward with row flags -> Adam on both tables (torch.optim.Adam as BaseRunner._build_optimizer configures it: coupled L2 = --l2 on
    both tables, neither is a bias), all enqueued on the current stream.  Gradients and moments are fp32 buffers owned by the engine; the
    parameters are updated in place."""

    def __init__(self, model, loss_name='Listloss', args=None, lr=1e-3, l2=0.0, betas=(0.9, 0.999), eps=1e-8):
        _one_rank('aWELvEngine')
        if loss_name not in PLAIN_LOSSES:
            raise ValueError(plain_loss_message(loss_name))
        self.model = model
        self.loss_name = loss_name
        self.kind = 'bpr' if 'BPR' in loss_name else ('mse' if 'MSE' in loss_name else 'list')
        g = lambda k, d: getattr(args, k, d) if args is not None else d
        self.cal_diversity, self.alpha = int(g('cal_diversity', 0)), float(g('diversity_alpha', 0.01))
        self.lr, self.l2, self.betas, self.eps = float(lr), float(l2), betas, float(eps)
        self.defer_table_wait = False          # accepted, unused: nothing of a step is left running on another stream
        self.step_count = 0
        # BPR tie-breaking noise (BPRloss.py:26) drawn inside the loss kernel, seeded the way IntELEngine seeds it: one generator per
        # engine, seeded from torch's CPU generator (reproducible under torch.manual_seed)
        self._noise_gen = torch.Generator()
        self._noise_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()))
        E, M = model.uid_embeddings.weight, model.model_embeddings.weight
        L.require_gpu(E)
        L.require_gpu(M)
        for p in (E, M):
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise L.IntelHipError('aWELvEngine: the embedding tables must be contiguous fp32 tensors')
        self.device = E.device
        self.grad = {'uid': torch.zeros_like(E.data), 'model': torch.zeros_like(M.data)}       # 'uid' is re-zeroed by the Adam sweep that consumes it
        self.m = {k: torch.zeros_like(v) for k, v in self.grad.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.grad.items()}
        # one byte per user row: the backward marks the rows it adds into, intel_adam_step_rows reads and clears the gradient only there
        self._flags = torch.zeros(E.shape[0], dtype=torch.uint8, device=self.device) if E.shape[1] in ADAM_ROWS_D else None
        self._bufs = {}

    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._bufs[name] = t
        return t

    def set_lr(self, lr):
        """StepLR counterpart of the engine path (helpers/BaseRunner.py:238-241)."""
        self.lr = float(lr)

    def flush(self):
        """Nothing is ever pending: every launch of a step is on the caller's stream."""

    def train_step(self, batch):
        """forward + loss + backward + Adam on one batch.  Returns (loss, loss, loss) like the plain criteria, a device tensor (no host
        sync).  batch['bpr_noise']: optional [B, L, L] tie-breaking noise of the BPR loss (pins the draw through intel_bpr_loss, as loss.py does);
        without it the noise is drawn inside the kernel from the engine's generator."""
        model, lib, dev = self.model, L.lib(), self.device
        E, M = model.uid_embeddings.weight.data, model.model_embeddings.weight.data
        scores = batch['scores']
        L.require_gpu(scores)
        sc32 = _f32(scores)
        sc64 = scores.contiguous() if scores.dtype == torch.float64 else None       # the diversity term reads the float64 scores, as loss.py does
        u = _i32(batch['u_id_c'], dev)
        ranking, slen = _i32(batch['ranking'], dev), _i32(batch['session_len'], dev)
        B, Lm, K = sc32.shape
        users, H = E.shape
        st = L.stream_ptr(dev)
        w = self._buf('w', (B, K), torch.float32)
        weights = self._buf('weights', (B, Lm, K), torch.float32)
        ens = self._buf('ens', (B, Lm), torch.float32)
        L.check(lib.intel_awelv_forward(B, Lm, K, H, L.ptr(E), users, L.ptr(M), L.ptr(u), L.ptr(sc32), L.ptr(w), L.ptr(weights), L.ptr(ens), st),
                'intel_awelv_forward')
        nb = lib.intel_loss_workspace_bytes(B, Lm, K)
        ws = self._buf('loss_ws', (int(nb),), torch.uint8)
        loss = torch.empty(1, dtype=torch.float32, device=dev)       # fresh: the caller may keep every step's value (runner.fit)
        d_ens = self._buf('d_ens', (B, Lm), torch.float32)
        d_w = self._buf('d_w', (B, Lm, K), torch.float32)
        if self.kind == 'bpr':
            select = self._buf('select', (B, Lm), torch.int32)
            noise = batch.get('bpr_noise')
            if noise is None:
                seed = int(torch.randint(0, 2 ** 62, (1,), generator=self._noise_gen).item())
                L.check(lib.intel_bpr_loss_seeded(B, Lm, K, L.ptr(ens), L.ptr(ranking), L.ptr(slen), C.c_ulonglong(seed), C.c_ulonglong(0),
                                                  L.ptr(sc64), L.ptr(sc32), L.ptr(weights), self.cal_diversity, self.alpha, 1.0, L.ptr(loss),
                                                  L.ptr(select), L.ptr(d_ens), L.ptr(d_w), L.ptr(ws), nb, st), 'intel_bpr_loss_seeded')
            else:
                noise = noise.to(dev).float().contiguous()
                L.check(lib.intel_bpr_loss(B, Lm, K, L.ptr(ens), L.ptr(ranking), L.ptr(slen), L.ptr(noise), L.ptr(sc64), L.ptr(sc32),
                                           L.ptr(weights), self.cal_diversity, self.alpha, 1.0, L.ptr(loss), L.ptr(select), L.ptr(d_ens),
                                           L.ptr(d_w), L.ptr(ws), nb, st), 'intel_bpr_loss')
        elif self.kind == 'mse':
            L.check(lib.intel_mse_loss(B, Lm, K, L.ptr(ens), L.ptr(ranking), L.ptr(slen), L.ptr(sc64), L.ptr(sc32), L.ptr(weights),
                                       self.cal_diversity, self.alpha, 1.0, L.ptr(loss), L.ptr(d_ens), L.ptr(d_w), L.ptr(ws), nb, st),
                    'intel_mse_loss')
        else:
            L.check(lib.intel_list_loss(B, Lm, K, L.ptr(ens), L.ptr(ranking), L.ptr(slen), L.ptr(sc64), L.ptr(sc32), L.ptr(weights),
                                        self.cal_diversity, self.alpha, 1.0, L.ptr(loss), L.ptr(d_ens), L.ptr(d_w), L.ptr(ws), nb, st),
                    'intel_list_loss')
        bws = self._buf('bwd_ws', (max(int(lib.intel_awelv_backward_workspace_bytes(B, K, H)), 8),), torch.uint8)
        gu, gm = self.grad['uid'], self.grad['model']
        L.check(lib.intel_awelv_backward(B, Lm, K, H, L.ptr(E), users, L.ptr(M), L.ptr(u), L.ptr(sc32), L.ptr(w), L.ptr(d_ens), L.ptr(d_w),
                                         L.ptr(gu), L.ptr(self._flags), L.ptr(gm), L.ptr(bws), st), 'intel_awelv_backward')
        self.step_count += 1
        b1, b2 = self.betas
        if self._flags is not None:
            L.check(lib.intel_adam_step_rows(L.ptr(E), L.ptr(gu), L.ptr(self.m['uid']), L.ptr(self.v['uid']), users, H, L.ptr(self._flags),
                                             self.lr, b1, b2, self.eps, self.l2, self.step_count, 1.0, st), 'intel_adam_step_rows')
        else:
            L.check(lib.intel_adam_step(L.ptr(E), L.ptr(gu), L.ptr(self.m['uid']), L.ptr(self.v['uid']), E.numel(), self.lr, b1, b2, self.eps,
                                        self.l2, self.step_count, 1.0, 1, st), 'intel_adam_step')
        L.check(lib.intel_adam_step(L.ptr(M), L.ptr(gm), L.ptr(self.m['model']), L.ptr(self.v['model']), M.numel(), self.lr, b1, b2, self.eps,
                                    self.l2, self.step_count, 1.0, 0, st), 'intel_adam_step')
        out = loss.reshape(())
        return out, out, out


aWELv.ENGINE = aWELvEngine
