"""Standalone timing of the aWELv training step (intel_sigir2023_amd/awelv.py, csrc/awelv.hip) at the Tmall shape of the reference's
comparison table (script/baselines.sh:33): 100 000 users, L = 50, K = 3, H = 32, Listloss with the diversity term.
usage: python tools/awelv_bench.py [--batches 512,4096] [--users 100000] [--L 50] [--K 3] [--H 32] [--steps 200] [--warmup 20]
For every batch size it times, with HIP events on the current stream after a warm-up (median of --steps steps, each step between its own
pair of events):
  fused      aWELvEngine.train_step: forward, one loss launch with gradients, backward with row flags, two Adam launches
  autograd   the same module through its autograd Function + loss.Listloss + torch.optim.Adam (the --use_engine 0 path)
  eager      a torch-eager restatement of the reference's step on the same GPU: nn.Embedding lookups, softmax, the list-wise loss with
             its diversity term from [B, L, L(, K)] tensors, loss.backward(), torch.optim.Adam
and prints the fused step's algorithmic bytes and the bandwidth they amount to.  Needs an MI355X."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from intel_sigir2023_amd import awelv, loss as loss_mod


def make_batch(B, Lm, K, users, dev, seed):
    """Scores min-max normalised per list and base ranker, float64 like collate_batch delivers them; labels 3, 2, 1, 1, 1 and zeros."""
    g = torch.Generator(device=dev).manual_seed(seed)
    slen = torch.randint(Lm // 4, Lm + 1, (B,), generator=g, device=dev)
    slen[0] = Lm
    valid = torch.arange(Lm, device=dev)[None, :] < slen[:, None]
    scores = torch.rand(B, Lm, K, generator=g, device=dev, dtype=torch.float64) * valid[:, :, None]
    order = (torch.rand(B, Lm, generator=g, device=dev) + (~valid) * 2.0).argsort(dim=1)
    ranking = torch.zeros(B, Lm, dtype=torch.int64, device=dev)
    ranking.scatter_(1, order[:, :5], torch.tensor([3, 2, 1, 1, 1], device=dev)[None, :].expand(B, 5))
    return {'u_id_c': torch.randint(0, users, (B,), generator=g, device=dev).int(), 'scores': scores, 'ranking': (ranking * valid).int(),
            'session_len': slen.int(), 'batch_size': B, 'phase': 'train'}


def eager_step(E, M, opt, b, alpha):
    """The reference's step restated with torch operators (fp32 model, float64 base scores in the diversity term)."""
    opt.zero_grad()
    sc = b['scores']
    w = torch.softmax(E(b['u_id_c'].long()) @ M.weight.t(), dim=-1)[:, None, :].expand(-1, sc.shape[1], -1)
    ens = (w * sc.float()).sum(-1)
    valid = torch.arange(ens.shape[1], device=ens.device)[None, :] < b['session_len'][:, None]
    r = b['ranking'].clamp(min=0)
    pair = (r[:, :, None] > r[:, None, :]) & valid[:, :, None] & valid[:, None, :]
    diff = ens[:, :, None] - ens[:, None, :]
    ex = torch.exp(-diff)
    pos = r > 0
    npos = pos.sum(1)
    denom = (ex * pair).sum(2) + 1.0
    loss = (torch.log((denom * pos).clamp(min=1.0)).sum(1) / npos).mean()
    bd = sc[:, :, None, :] - sc[:, None, :, :]
    up = ((ex[..., None] * (bd - diff[..., None]) * pair[..., None]).sum(2)) ** 2
    loss = loss - alpha * (((w * up).sum(-1) / (2.0 * denom ** 2) * pos).sum(1) / npos).mean()
    loss.backward()
    opt.step()
    return loss


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def step_bytes(B, Lm, K, H, users):
    """Algorithmic bytes of one fused step: what each launch must read and write once."""
    fwd = 4 * (B * Lm * K + B * H + K * H + B) + 4 * (B * Lm * K + B * Lm + B * K)                       # scores, E rows, M, ids -> weights, ens, w
    loss = B * Lm * (8 * K + 4 * K + 4 + 4) + 4 * B + 4 * (B * Lm + B * Lm * K)                           # float64 scores, weights, ens, labels, lengths -> d_ens, d_weights
    bwd = 4 * (B * Lm * (2 * K + 1) + B * (K + 1) + B * H + K * H) + 4 * (2 * B * H + K * H)              # scores, d_weights, d_ens, w, ids, E rows, M -> row adds, dM
    table = 6 * 4 * users * H + users + 2 * 4 * B * H                                                     # p, m, v read and written; flags; the flagged gradient rows
    small = 7 * 4 * K * H
    return dict(forward=fwd, loss=loss, backward=bwd, table_sweep=table, model_table_adam=small, total=fwd + loss + bwd + table + small)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=str, default='512,4096')
    ap.add_argument('--users', type=int, default=100000)
    ap.add_argument('--L', type=int, default=50)
    ap.add_argument('--K', type=int, default=3)
    ap.add_argument('--H', type=int, default=32)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--l2', type=float, default=1e-4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/awelv_bench.py needs an MI355X')
    dev = torch.device('cuda:0')
    args = argparse.Namespace(model_num=a.K, hidden_size=a.H, model_path='', buffer=1, device=dev, cal_diversity=1, diversity_alpha=1e-2,
                              intent_weight=0.1, ensemble_weight=1, kl_weight=0.5, kl_temp=2)
    corpus = argparse.Namespace(max_uid=a.users - 1, zero_int=np.zeros(30))
    for B in [int(x) for x in a.batches.split(',')]:
        batches = [make_batch(B, a.L, a.K, a.users, dev, seed=s) for s in range(4)]
        it = {'i': 0}

        def nxt():
            it['i'] += 1
            return batches[it['i'] % len(batches)]
        torch.manual_seed(0)
        fused = awelv.aWELv(args, corpus).to(dev).train()
        eng = awelv.aWELvEngine(fused, 'Listloss', args, lr=a.lr, l2=a.l2)
        t_fused = timed(lambda: eng.train_step(nxt()), a.steps, a.warmup)
        torch.manual_seed(0)
        plain = awelv.aWELv(args, corpus).to(dev).train()
        opt = torch.optim.Adam(plain.customize_parameters(), lr=a.lr, weight_decay=a.l2)
        crit = loss_mod.Listloss(args)

        def autograd_step():
            b = nxt()
            opt.zero_grad()
            loss, _, _ = crit(plain(b), b)
            loss.backward()
            opt.step()
        t_auto = timed(autograd_step, a.steps, a.warmup)
        torch.manual_seed(0)
        E, M = torch.nn.Embedding(a.users, a.H).to(dev), torch.nn.Embedding(a.K, a.H).to(dev)
        eopt = torch.optim.Adam([E.weight, M.weight], lr=a.lr, weight_decay=a.l2)
        t_eager = timed(lambda: eager_step(E, M, eopt, nxt(), args.diversity_alpha), max(20, a.steps // 4), max(5, a.warmup // 4))
        nb = step_bytes(B, a.L, a.K, a.H, a.users)
        print('aWELv step, %d sessions, users=%d L=%d K=%d H=%d, Listloss + diversity: median ms (min ... max)' % (B, a.users, a.L, a.K, a.H))
        for name, t in (('fused', t_fused), ('autograd', t_auto), ('eager', t_eager)):
            print('  %-9s %.4f ms (%.4f ... %.4f)  %.0f sessions/s' % (name, t[0], t[1], t[2], B / (t[0] * 1e-3)))
        print('  fused against autograd %.2fx, against torch-eager %.2fx' % (t_auto[0] / t_fused[0], t_eager[0] / t_fused[0]))
        print('  algorithmic bytes per fused step: %.2f MB (%s) -> %.3f TB/s' % (
            nb['total'] / 1e6, ', '.join('%s %.2f' % (k, v / 1e6) for k, v in nb.items() if k != 'total'), nb['total'] / (t_fused[0] * 1e-3) / 1e12))


if __name__ == '__main__':
    main()
