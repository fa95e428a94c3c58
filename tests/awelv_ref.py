"""float64 restatement of the aWELv baseline (models/supervise/aWELv.py:26-40 of the reference) and of its list-wise and MSE losses,
shared by tests/test_awelv_cpu.py (which validates it against the reference's own arrays, tests/golden/awelv_base.npz) and
tests/test_awelv_gpu.py (which uses it as the yardstick at shapes the fixture does not have)."""
import json
import os

import numpy as np
import torch

from tests.helpers import GOLDEN

_CACHE = {}


def load():
    """(npz, cfg) of tests/golden/awelv_base.npz, read once."""
    if 'z' not in _CACHE:
        z = np.load(os.path.join(GOLDEN, 'awelv_base.npz'))
        _CACHE['z'] = ({k: z[k] for k in z.files}, json.loads(str(z['cfg'])))
    return _CACHE['z']


def state(z, prefix):
    return {k[len(prefix) + 1:]: torch.from_numpy(v.copy()) for k, v in z.items() if k.startswith(prefix + '/')}


def batch(z, prefix, device='cpu'):
    b = {k[len(prefix):]: torch.from_numpy(v.copy()).to(device) for k, v in z.items() if k.startswith(prefix)}
    b['batch_size'] = int(b['u_id_c'].shape[0])
    b['phase'] = 'train'
    return b


def forward64(E, M, u_id, scores):
    """w = softmax_k(E[u] . M[k]) repeated over the WHOLE padded list, ens = sum_k w_k score_k; float64 in, float64 out."""
    w = torch.softmax(E[u_id.long()] @ M.t(), dim=-1)
    sc = scores.double()
    weights = w[:, None, :].expand(-1, sc.shape[1], -1)
    return weights, (weights * sc).sum(-1)


def backward64(E, M, u_id, scores, d_ens, d_weights=None):
    """Closed form of what autograd returns for forward64: (dE [users, H] dense, dM [K, H])."""
    u = u_id.long()
    e = E[u]
    w = torch.softmax(e @ M.t(), dim=-1)
    gw = (d_ens.double()[:, :, None] * scores.double()).sum(1)
    if d_weights is not None:
        gw = gw + d_weights.double().sum(1)
    dz = w * (gw - (w * gw).sum(-1, keepdim=True))
    dE = torch.zeros_like(E)
    dE.index_add_(0, u, dz @ M)
    return dE, dz.t() @ e


def _masks(ens, b):
    valid = torch.arange(ens.shape[1], device=ens.device)[None, :] < b['session_len'].long()[:, None]
    return valid, b['ranking'].long().clamp(min=0)


def listloss64(weights, ens, b, cal_diversity, alpha):
    """List-wise loss: for every positive item, log(1 + sum over the lower-labelled valid items of exp(-(ens_i - ens_j))), averaged over
    a list's positives, then over lists; the diversity term is subtracted with weight alpha."""
    valid, r = _masks(ens, b)
    pair = (r[:, :, None] > r[:, None, :]) & valid[:, :, None] & valid[:, None, :]
    diff = ens[:, :, None] - ens[:, None, :]
    ex = torch.exp(-diff)
    pos = r > 0
    npos = pos.sum(1)
    denom = (ex * pair).sum(2) + 1.0
    loss = (torch.log((denom * pos).clamp(min=1.0)).sum(1) / npos).mean()
    if cal_diversity:
        sc = b['scores'].double()
        bd = sc[:, :, None, :] - sc[:, None, :, :]
        up = ((ex[..., None] * (bd - diff[..., None]) * pair[..., None]).sum(2)) ** 2
        loss = loss - alpha * (((weights * up).sum(-1) / (2.0 * denom ** 2) * pos).sum(1) / npos).mean()
    return loss


def mseloss64(weights, ens, b, cal_diversity, alpha):
    """Per-list mean of (ens - max(label, 0))^2 over the valid slots, averaged over lists; minus alpha times the weighted spread of the
    base scores around the ensemble score."""
    valid, r = _masks(ens, b)
    n = valid.sum(1)
    loss = (((ens - r) ** 2 * valid).sum(1) / n).mean()
    if cal_diversity:
        spread = weights * (b['scores'].double() - ens[:, :, None]) ** 2
        loss = loss - alpha * ((spread * valid[:, :, None]).sum((1, 2)) / n).mean()
    return loss
