#!/usr/bin/env python3
"""Toy-Tmall fixture (BASELINE.json configs[0] plumbing): a slice of the reference's bundled toy Tmall sample (data/Tmall_toy) and what the
REFERENCE's SeqReader + IntEL.Dataset produce from it (the first six training feed dicts under np.random.seed(11), the deterministic stand-in for
the sample's missing intents_multi.json next to it), written to tests/golden/tmall_toy.npz.  The slice keeps every session (train / dev / test
lines, verbatim) of the first USERS users, one session with the largest item id and one with the latest c_time_i, the metadata of every item and user
those sessions name, and one item / user for every value of each metadata feature the reader reads -- so the reader derives the same corpus figures
(max_iid, contextfnum, itemfnum, userfnum, intent width) as from the whole sample, which main() checks.  Build container only (needs the reference
tree); tests/test_data_cpu.py replays it."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF_SRC, install_shims  # noqa: E402

TOY = os.path.join(os.path.dirname(REF_SRC), 'data', 'Tmall_toy')
FILES = ('train.csv', 'dev.csv', 'test.csv', 'item_metadata.json', 'user_metadata.json')
CFG = dict(dataset='Tmall_toy', sep='\t', intent_note='_multi', max_session_len=100, model_num=3,
           history_max=20, model_path='', buffer=1, encoder='BERT4Rec', context_emb_size=16, i_emb_size=16, u_emb_size=32,
           s_emb_size=32, im_emb_size=16, intent_emb_size=16, cross_attn_qsize=32, num_heads=1, dropout=0, num_layers=1,
           cross_attention=1, intent_weight=0.1, ensemble_weight=1, kl_temp=2, kl_weight=0.5, cal_diversity=1,
           diversity_alpha=0.01)
N_FEED, NP_SEED = 6, 11
USERS = 2


def _literal(v):
    import ast
    return ast.literal_eval(v) if isinstance(v, str) else v


def write_slice(root):
    """The slice of the toy sample described above, written to root; returns {file name: bytes}."""
    import pandas as pd
    frames, lines = {}, {}
    for p in ('train', 'dev', 'test'):
        raw = open(os.path.join(TOY, p + '.csv'), 'rb').read().decode()
        lines[p] = raw.splitlines(keepends=True)
        frames[p] = pd.read_csv(os.path.join(TOY, p + '.csv'), sep=CFG['sep'])
        assert len(frames[p]) == len(lines[p]) - 1
    users = set(sorted(set().union(*[set(f['u_id_c']) for f in frames.values()]))[:USERS])
    max_iid = max(max(_literal(s)) for f in frames.values() for s in f['i_id_s'])
    max_time = max(int(f['c_time_i'].max()) for f in frames.values())
    anchors = {}           # the first session (phase, row) that holds the largest item id / the latest c_time_i
    for p, f in frames.items():
        for i in range(len(f)):
            if max_iid in _literal(f['i_id_s'][i]):
                anchors.setdefault('iid', (p, i))
            if f['c_time_i'][i] == max_time:
                anchors.setdefault('time', (p, i))
    out, keep_items, keep_users = {}, set(), set()
    for p, f in frames.items():
        rows = [i for i in range(len(f)) if f['u_id_c'][i] in users or (p, i) in anchors.values()]
        for i in rows:
            keep_items |= set(_literal(f['i_id_s'][i]))
            keep_users.add(int(f['u_id_c'][i]))
        out[p + '.csv'] = ''.join([lines[p][0]] + [lines[p][i + 1] for i in rows]).encode()
    from intel_sigir2023_amd.data import SeqReader
    for name, keep, feats in (('item_metadata.json', keep_items, SeqReader.ifeatures), ('user_metadata.json', keep_users, SeqReader.ufeatures)):
        meta = json.load(open(os.path.join(TOY, name)))
        keys = {str(k) for k in keep if str(k) in meta}
        for feat in feats:                 # one entry per value of every feature the reader reads (it counts them)
            first = {}
            for k in sorted(meta, key=int):
                first.setdefault(meta[k][feat], k)
            keys |= set(first.values())
        out[name] = json.dumps({k: meta[k] for k in meta if k in keys}).encode()
    os.makedirs(root)
    for name, raw in out.items():
        with open(os.path.join(root, name), 'wb') as fh:
            fh.write(raw)
    return out


def read_corpus(tmp, SeqReader, torch):
    args = argparse.Namespace(datapath=tmp, **CFG)
    args.device = torch.device('cpu')
    return args, SeqReader(args)


def figures(c):
    return (c.max_iid, len(c.zero_int), list(c.contextfnum), list(c.itemfnum), list(c.userfnum))


def main(tmp):
    install_shims()
    sys.path.insert(0, REF_SRC)
    import torch
    from helpers.SeqReader import SeqReader
    from models.IntEL.IntEL import IntEL
    from intel_sigir2023_amd.data import standin_intents
    whole = os.path.join(tmp, 'whole')
    os.makedirs(os.path.join(whole, 'Tmall_toy'))
    for f in FILES:
        os.symlink(os.path.join(TOY, f), os.path.join(whole, 'Tmall_toy', f))
    json.dump(standin_intents(os.path.join(whole, 'Tmall_toy')), open(os.path.join(whole, 'Tmall_toy', 'intents_multi.json'), 'w'))
    want = figures(read_corpus(whole, SeqReader, torch)[1])
    root = os.path.join(tmp, 'Tmall_toy')
    out = {'cfg': np.array(json.dumps(CFG)), 'n_feed': np.array(N_FEED), 'np_seed': np.array(NP_SEED)}
    for f, raw in write_slice(root).items():
        out['file/' + f] = np.frombuffer(raw, dtype=np.uint8)
    json.dump(standin_intents(root), open(os.path.join(root, 'intents_multi.json'), 'w'))
    args, corpus = read_corpus(tmp, SeqReader, torch)
    assert figures(corpus) == want, (figures(corpus), want)
    print('corpus figures of the slice = of the whole sample:', want)
    torch.manual_seed(0)
    model = IntEL(args, corpus)
    np.random.seed(NP_SEED)
    ds = IntEL.Dataset(model, corpus, 'train')
    for i in range(N_FEED):
        for k, v in ds[i].items():
            out['ref/%d/%s' % (i, k)] = np.asarray(v)
    path = os.path.join(HERE, 'tmall_toy.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, '%.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        main(d)
