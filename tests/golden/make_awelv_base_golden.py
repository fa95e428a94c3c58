#!/usr/bin/env python3
"""Generates tests/golden/awelv_base.npz by running the reference's aWELv model (models/supervise/aWELv.py) and its Listloss,
MSEloss and BPRloss, all imported unmodified (build container only), on a small seeded batch in collate_batch's layout.
Arrays plus a JSON cfg; nothing of the reference's source is stored.

    python tests/golden/make_awelv_base_golden.py

Contents
  sd_raw/*                 the seeded state_dict: torch's default N(0, 1) embeddings, as the reference leaves them
  sd/*                     the same state x 0.1 (see "conditioning")
  in/*                     the batch
  out_raw/*, out/*         weights, ens_score of the forward from sd_raw / sd
  <state>/<loss>/loss, <state>/<loss>/grad/<parameter>     state in (raw, scaled), loss in (list, mse, bpr), cal_diversity 1
  bpr_noise_head           the first values of the BPR tie-breaking draw, torch.rand(B, L, L) under cfg['noise_seed']
  traj/in<i>/*, traj/losses, traj/final/*                  10 Adam steps (lr 1e-3, weight_decay 1e-4) of Listloss from sd

Conditioning.  At N(0, 1) the logits E[u] . M[k] have a standard deviation of about sqrt(H), the softmax saturates, its backward
cancels in fp32 and Adam divides that noise by its own magnitude: the reference's own fp32 trajectory then leaves the bound the
trajectory tests use (2e-3 * move + 1e-7 per element) against a float64 run of the same steps.  At 0.1 x it does not.  Before the
file is written the 10 steps are repeated in float64 with the restatement below and the fp32 result is ASSERTED to have no element
outside that bound: the condition under which the fixture is a fair yardstick.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (shims, synthetic batch, helpers)

SHAPE = dict(B=6, L=50, lens=[50, 50, 37, 12, 5, 23], I=30, H=20, items=3000, users=40, classes=60, ctx=100)
OVER = dict(model_num=3, hidden_size=32, cal_diversity=1, diversity_alpha=1e-2)
SEED, STEPS, LR, L2 = 11, 10, 1e-3, 1e-4
TRAJ_KEYS = ('u_id_c', 'session_len', 'ranking', 'scores', 'intents')


def forward64(E, M, batch):
    """float64 restatement of the model: w = softmax_k(E[u] . M[k]) repeated over the list, ens = sum_k w_k score_k."""
    z = E[batch['u_id_c']] @ M.t()
    w = torch.softmax(z, dim=-1)
    sc = batch['scores'].double()
    weights = w[:, None, :].expand(-1, sc.shape[1], -1)
    return weights, (weights * sc).sum(-1)


def listloss64(weights, ens, batch, cal_diversity, alpha):
    """float64 restatement of the list-wise loss with its diversity term."""
    Lm = ens.shape[1]
    valid = torch.arange(Lm)[None, :] < batch['session_len'][:, None]
    r = batch['ranking'].clamp(min=0)
    pair = (r[:, :, None] > r[:, None, :]) & valid[:, :, None] & valid[:, None, :]
    diff = ens[:, :, None] - ens[:, None, :]
    ex = torch.exp(-diff)
    pos = r > 0
    npos = pos.sum(1)
    denom = (ex * pair).sum(2) + 1.0
    loss = (torch.log((denom * pos).clamp(min=1.0)).sum(1) / npos).mean()
    if cal_diversity:
        sc = batch['scores'].double()
        bd = sc[:, :, None, :] - sc[:, None, :, :]
        up = ((ex[..., None] * (bd - diff[..., None]) * pair[..., None]).sum(2)) ** 2
        div = (((weights * up).sum(-1) / (2.0 * denom ** 2) * pos).sum(1) / npos).mean()
        loss = loss - alpha * div
    return loss


def main():
    G.install_shims()
    from models.supervise.aWELv import aWELv
    from loss.Listloss import Listloss
    from loss.MSEloss import MSEloss
    from loss.BPRloss import BPRloss
    torch.set_num_threads(4)
    args = G.make_args(OVER)
    corpus = G.make_corpus(SHAPE)
    torch.manual_seed(SEED)
    model = aWELv(args, corpus)
    rng = np.random.default_rng(SEED)
    batch = G.make_batch(SHAPE, args.model_num, rng, args.history_max)
    B, Lm = batch['i_id_s'].shape
    noise_seed = 1000 + SEED
    out = {}
    a = {k: v for k, v in vars(args).items() if k != 'device'}
    a['model_name'] = 'aWELv'
    out['cfg'] = np.array(json.dumps(dict(args=a, shape=SHAPE, seed=SEED, noise_seed=noise_seed, lr=LR, l2=L2, steps=STEPS)))
    sd_raw = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd = {k: v * np.float32(0.1) for k, v in sd_raw.items()}
    for k in sd_raw:
        out['sd_raw/' + k] = sd_raw[k].numpy().copy()
        out['sd/' + k] = sd[k].numpy().copy()
    for k, v in batch.items():
        out['in/' + k] = v
    tb = G.to_torch(batch)
    torch.manual_seed(noise_seed)
    noise = torch.rand(B, Lm, Lm)
    out['bpr_noise_head'] = noise[0, 0, :8].numpy().copy()
    for tag, state in (('raw', sd_raw), ('scaled', sd)):
        model.load_state_dict(state)
        with torch.no_grad():
            o = model(tb)
        prefix = 'out_raw/' if tag == 'raw' else 'out/'
        out[prefix + 'weights'], out[prefix + 'ens_score'] = o['weights'].numpy().copy(), o['ens_score'].numpy().copy()
        for lname, cls in (('list', Listloss), ('mse', MSEloss), ('bpr', BPRloss)):
            model.zero_grad()
            torch.manual_seed(noise_seed)          # BPRloss draws torch.rand_like of a [B, L, L] mask: the draw above
            loss, _, _ = cls(args)(model(tb), tb)
            loss.backward()
            out['%s/%s/loss' % (tag, lname)] = loss.detach().numpy().copy()
            for pn, p in model.named_parameters():
                out['%s/%s/grad/%s' % (tag, lname, pn)] = p.grad.numpy().copy()

    # ---- 10 Adam steps of Listloss from sd, fp32 reference against float64 restatement
    batches = [G.make_batch(SHAPE, args.model_num, np.random.default_rng(SEED * 100 + i), args.history_max) for i in range(STEPS)]
    model.load_state_dict(sd)
    model.train()
    opt = torch.optim.Adam(model.customize_parameters(), lr=LR, weight_decay=L2)
    crit = Listloss(args)
    losses = []
    for b in batches:
        t = G.to_torch(b)
        opt.zero_grad()
        loss, _, _ = crit(model(t), t)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    E = sd['uid_embeddings.weight'].double().clone().requires_grad_(True)
    M = sd['model_embeddings.weight'].double().clone().requires_grad_(True)
    opt64 = torch.optim.Adam([E, M], lr=LR, weight_decay=L2)
    losses64 = []
    for b in batches:
        t = G.to_torch(b)
        opt64.zero_grad()
        weights, ens = forward64(E, M, t)
        loss = listloss64(weights, ens, t, args.cal_diversity, args.diversity_alpha)
        loss.backward()
        opt64.step()
        losses64.append(float(loss.detach()))
    final = {k: v.detach().clone() for k, v in model.state_dict().items()}
    worst = 0.0
    for k, v64 in (('uid_embeddings.weight', E), ('model_embeddings.weight', M)):
        move = (v64.detach() - sd[k].double()).abs()
        err = (final[k].double() - v64.detach()).abs()
        outside = int((err > 2e-3 * move + 1e-7).sum())
        worst = max(worst, float(err.max()))
        assert outside == 0, 'the reference\'s fp32 trajectory leaves 2e-3 * move + 1e-7 in %d elements of %s: not a fair yardstick' % (outside, k)
    dl = float(np.abs(np.array(losses) - np.array(losses64)).max())
    assert dl < 1e-5, dl
    print('trajectory: fp32 reference against float64, worst parameter error %.3g, worst loss difference %.3g' % (worst, dl))
    for i, b in enumerate(batches):
        for k in TRAJ_KEYS:
            out['traj/in%d/%s' % (i, k)] = b[k]
    out['traj/losses'] = np.array(losses)
    for k, v in final.items():
        out['traj/final/' + k] = v.numpy().copy()
    path = os.path.join(HERE, 'awelv_base.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, '%.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
