"""GPU parity of the session, row and LayerNorm-backward kernels (csrc/session.hip, csrc/rowops.hip) through their
`intel_op_*` entry points, against float64 torch on the CPU.

Every reference is written here from the reference model's formulas (modules/attention.py:55-62, IntEL.py:212-215,
GeneralSeq.py:100-105, torch.nn.LayerNorm / Embedding / softmax under autograd); backward references are torch autograd of the
float64 forward.  Tolerances are those of tests/test_ops_gpu.py: 2e-5 for forward outputs, 5e-5 for gradients, relative to
max(1, |ref|max) -- the kernels only re-associate fp32 sums.

The shapes sit where the kernels change path: four sessions per 256-thread workgroup (B = 1 / 5 / 9: a partial last workgroup,
more than one slab), the register forms of the pooling (L = 20|21, 52|53, 100|101), 16- and 64-row LayerNorm blocks
(M = 16 384|16 385), 16-pair chunks and workgroup spans of the sorted scatter.

Alignment: every pointer handed to the pooling kernels is 16-byte aligned and `ldxb` is a multiple of 4, as in the model.  A
misaligned base would send their 16-byte loads to unaligned addresses; that path is deliberately NOT exercised here.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 2e-5, 5e-5
SENT = -12345.0


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _close(got, ref, tol=FWD_TOL, name=''):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, '%s: shape %s vs %s' % (name, tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    assert err <= tol * scale, '%s: max err %.3e (scale %.3e)' % (name, err, scale)


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k) + 1
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _len_vectors(B, specials, hi, g):
    """Session-length vectors of B entries that together contain every value of `specials`; the rest is random in [0, hi].
    B >= len(specials): one vector (shuffled); smaller B: as many vectors as it takes."""
    out = []
    for i in range(0, len(specials), B):
        v = list(specials[i:i + B]) if B < len(specials) else list(specials)
        while len(v) < B:
            v.append(int(torch.randint(0, hi + 1, (1,), generator=g)))
        perm = torch.randperm(B, generator=g)
        out.append(torch.tensor(v, dtype=torch.int32)[perm])
        if B >= len(specials):
            break
    return out


def _i32(t, dev):
    return t.to(torch.int32).contiguous().to(dev)


# ======================================================================================================================
# cross-attention pooling
# ======================================================================================================================
def _pool_ref(x, qk, slen, scale):
    """modules/attention.py:55-62 with one query row: scores over ALL L rows, minus their max, rows l >= len masked to -inf,
    softmax, NaN -> 0, weighted sum."""
    L = x.shape[1]
    att = torch.einsum('bld,bd->bl', x, qk) * scale
    att = att - att.max(dim=-1, keepdim=True)[0]
    valid = torch.arange(L)[None, :] < slen[:, None].long()
    att = att.masked_fill(~valid, float('-inf'))
    w = att.softmax(dim=-1)
    w = w.masked_fill(torch.isnan(w), 0)
    return torch.einsum('bl,bld->bd', w, x), w


def _pool_ref_diff(x, qk, slen, scale):
    """The same function without a NaN on the way (autograd through softmax of an all -inf row gives NaN gradients where the
    reference's are zero): e = exp(att - max) on the valid rows, w = e / sum e, 0 for an empty sum."""
    L = x.shape[1]
    att = torch.einsum('bld,bd->bl', x, qk) * scale
    att = att - att.max(dim=-1, keepdim=True)[0].detach()
    valid = (torch.arange(L)[None, :] < slen[:, None].long()).double()
    e = torch.exp(att) * valid
    s = e.sum(-1, keepdim=True)
    w = e / torch.where(s > 0, s, torch.ones_like(s))
    return torch.einsum('bl,bld->bd', w, x), w


def _pool_lens(B, L, g):
    return _len_vectors(B, [L, 1, 0, L + 3], L, g)


POOL_L = [1, 4, 5, 20, 21, 52, 53, 100, 101, 130]
POOL_SHAPES = [(d, L) for d in (64, 128) for L in POOL_L] + [(d, L) for d in (32, 96) for L in (5, 53, 101)]


@pytest.mark.parametrize('d,L', POOL_SHAPES)
def test_xatt_pool_fwd_bwd(d, L):
    from intel_sigir2023_amd import ops
    dev = _dev()
    scale = d ** -0.5
    for B in (1, 5, 9):
        g = _gen(1, d, L, B)
        for slen in _pool_lens(B, L, g):
            tag = 'd=%d L=%d B=%d len=%s' % (d, L, B, slen.tolist())
            x, qk = _randn(g, B, L, d), _randn(g, B, d)
            ldxb = d + 8
            dxbar = _randn(g, B, ldxb)
            xr = x.double().requires_grad_(True)
            qr = qk.double().requires_grad_(True)
            xbar_ref, w_ref = _pool_ref(xr.detach(), qr.detach(), slen, scale)
            xbar_d, w_d = _pool_ref_diff(xr, qr, slen, scale)
            assert float((xbar_d.detach() - xbar_ref).abs().max()) <= 1e-12 and float((w_d.detach() - w_ref).abs().max()) <= 1e-12
            n = torch.clamp(slen.long(), max=L)
            valid = torch.arange(L)[None, :] < n[:, None]

            xbar, attw = ops.xatt_pool_fwd(x.to(dev), qk.to(dev), _i32(slen, dev), scale)
            _close(attw, w_ref, FWD_TOL, 'attw ' + tag)
            _close(xbar, xbar_ref, FWD_TOL, 'xbar ' + tag)
            assert bool((attw.cpu()[~valid] == 0).all()), 'attw must be exactly 0 beyond the session length: ' + tag
            assert bool((xbar.cpu()[n == 0] == 0).all()), 'xbar must be exactly 0 for an empty session: ' + tag

            (xbar_d * dxbar[:, :d].double()).sum().backward()
            dx, dqk = ops.xatt_pool_bwd(x.to(dev), qk.to(dev), w_ref.float().to(dev), dxbar.to(dev), scale)
            _close(dx, xr.grad, GRAD_TOL, 'dX ' + tag)
            _close(dqk, qr.grad, GRAD_TOL, 'dqk ' + tag)


def _ln_stash(z, eps=1e-5):
    mu = z.mean(-1, keepdim=True)
    var = z.var(-1, unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (z - mu) * rstd, rstd.squeeze(-1)


@pytest.mark.parametrize('d,L', [(d, L) for d in (64, 128) for L in POOL_L if L <= 100])
def test_xatt_pool_xhat_form_and_fused_ln_bwd(d, L):
    """x given as the x-hat stash of the tower's last LayerNorm: forward with gamma / beta, backward fused with that LayerNorm's."""
    from intel_sigir2023_amd import ops
    dev = _dev()
    scale = d ** -0.5
    for B in (1, 5, 9):
        g = _gen(2, d, L, B)
        for vi, slen in enumerate(_pool_lens(B, L, g)):
            tag = 'd=%d L=%d B=%d len=%s' % (d, L, B, slen.tolist())
            z = torch.randn(B, L, d, generator=g, dtype=torch.float64)
            gamma, beta, qk = _randn(g, d), _randn(g, d), _randn(g, B, d)
            ldxb = d + 4
            dxbar = _randn(g, B, ldxb)
            xhat64, rstd64 = _ln_stash(z)
            xhat, rstd = xhat64.float(), rstd64.float()

            # forward: the reference rows are x = xhat * gamma + beta
            x_rows = xhat.double() * gamma.double() + beta.double()
            xbar_ref, w_ref = _pool_ref(x_rows, qk.double(), slen, scale)
            xbar, attw = ops.xatt_pool_fwd(xhat.to(dev), qk.to(dev), _i32(slen, dev), scale, gamma.to(dev), beta.to(dev))
            _close(attw, w_ref, FWD_TOL, 'xhat attw ' + tag)
            _close(xbar, xbar_ref, FWD_TOL, 'xhat xbar ' + tag)

            # backward: autograd through layer_norm -> pooling
            zr = z.clone().requires_grad_(True)
            gr, br, qr = gamma.double().requires_grad_(True), beta.double().requires_grad_(True), qk.double().requires_grad_(True)
            xb, w64 = _pool_ref_diff(F.layer_norm(zr, (d,), gr, br, 1e-5), qr, slen, scale)
            (xb * dxbar[:, :d].double()).sum().backward()
            for accumulate in ((0, 1) if (B == 5 and vi == 0) else (0,)):
                dg0, db0 = _randn(g, d), _randn(g, d)
                dgamma, dbeta = dg0.clone().to(dev), db0.clone().to(dev)
                dz, dqk = ops.xatt_pool_ln_bwd(xhat.to(dev), rstd.reshape(-1).to(dev), gamma.to(dev), beta.to(dev), qk.to(dev),
                                               w64.detach().float().to(dev), dxbar.to(dev), scale, dgamma, dbeta, accumulate=bool(accumulate))
                _close(dz, zr.grad, GRAD_TOL, 'dz ' + tag)
                _close(dqk, qr.grad, GRAD_TOL, 'ln dqk ' + tag)
                _close(dgamma, gr.grad + (dg0.double() if accumulate else 0), GRAD_TOL, 'dgamma acc=%d ' % accumulate + tag)
                _close(dbeta, br.grad + (db0.double() if accumulate else 0), GRAD_TOL, 'dbeta acc=%d ' % accumulate + tag)


# one case per register form (LP = 5 / 13 / 25) and for the generic kernel (L > 100, or a width other than 64 / 128)
@pytest.mark.parametrize('d,L', [(64, 20), (128, 21), (64, 53), (128, 100), (64, 101), (128, 130), (32, 53)])
def test_xatt_pool_underflow_gives_zero_weights(d, L):
    """Session 0: a PADDED row whose scaled score exceeds every valid row's by ~1000.  The kernels subtract the max over ALL L rows
    (attention.py:57) and exponentiate themselves, so every valid exp(att - max) underflows -- in fp32 and in float64 alike -- and
    the convention session.hip documents applies: an empty sum gives weights 0 (the NaN -> 0 of attention.py:61), hence xbar = 0,
    and the backward with those weights gives dX = 0 and dqk = 0.  Session 0 is checked for these exact zeros only, without
    autograd and without torch.softmax (which re-centres its input and would not underflow: docs/PARITY_LOG.md); the other
    sessions of the batch keep every score gap far below 60 and are compared with float64 as usual."""
    from intel_sigir2023_amd import ops
    dev = _dev()
    scale = d ** -0.5
    B = 5
    g = _gen(3, d, L)
    x, qk, dxbar = _randn(g, B, L, d), _randn(g, B, d), _randn(g, B, d)
    slen = torch.tensor([L // 2, L, 1, L + 2, max(1, L - 1)], dtype=torch.int32)
    pad = L - 1
    x[0, pad] = qk[0] * (1000.0 / (scale * float((qk[0].double() ** 2).sum())))
    att0 = (x[0].double() @ qk[0].double()) * scale
    assert float(att0[pad] - att0[:int(slen[0])].max()) >= 800.0
    assert float(torch.exp(att0[:int(slen[0])] - att0.max()).sum()) == 0.0        # float64 underflows too
    xbar_ref, w_ref = _pool_ref(x.double(), qk.double(), slen, scale)
    w_ref[0], xbar_ref[0] = 0.0, 0.0
    xbar, attw = ops.xatt_pool_fwd(x.to(dev), qk.to(dev), _i32(slen, dev), scale)
    assert bool((attw[0] == 0).all()), 'attw of the underflowing session must be exactly 0'
    assert bool((xbar[0] == 0).all()), 'xbar of the underflowing session must be exactly 0'
    _close(attw[1:], w_ref[1:], FWD_TOL, 'attw')
    _close(xbar[1:], xbar_ref[1:], FWD_TOL, 'xbar')
    dx, dqk = ops.xatt_pool_bwd(x.to(dev), qk.to(dev), w_ref.float().to(dev), dxbar.to(dev), scale)
    assert bool((dx[0] == 0).all()), 'dX of a session with all-zero weights must be exactly 0'
    assert bool((dqk[0] == 0).all()), 'dqk of a session with all-zero weights must be exactly 0'
    # the other sessions against autograd
    xr, qr = x[1:].double().requires_grad_(True), qk[1:].double().requires_grad_(True)
    xb, _ = _pool_ref_diff(xr, qr, slen[1:], scale)
    (xb * dxbar[1:].double()).sum().backward()
    _close(dx[1:], xr.grad, GRAD_TOL, 'dX')
    _close(dqk[1:], qr.grad, GRAD_TOL, 'dqk')


# ======================================================================================================================
# fusion weights
# ======================================================================================================================
@pytest.mark.parametrize('B,L,K', [(5, 50, 3), (9, 130, 8), (1, 1, 1), (6, 64, 5), (7, 65, 2)])
@pytest.mark.parametrize('per_item', [0, 1])
def test_ens_fwd_bwd(B, L, K, per_item):
    from intel_sigir2023_amd import ops
    dev = _dev()
    g = _gen(4, B, L, K, per_item)
    for slen in _len_vectors(B, [L, 1, 0, L + 3], L, g):
        tag = 'B=%d L=%d K=%d per_item=%d len=%s' % (B, L, K, per_item, slen.tolist())
        scores = _randn(g, B, L, K)
        wv, wpad, wit = _randn(g, B, K), _randn(g, B, K), _randn(g, B, L, K)
        d_w, d_e = _randn(g, B, L, K), _randn(g, B, L)
        valid = (torch.arange(L)[None, :] < slen[:, None].long())
        s_dev, len_dev = scores.to(dev), _i32(slen, dev)

        def ref_forward():
            if per_item:
                leaf = [wit.double().requires_grad_(True)]
                w = leaf[0]
            else:
                leaf = [wv.double().requires_grad_(True), wpad.double().requires_grad_(True)]
                w = torch.where(valid[:, :, None], leaf[0][:, None, :], leaf[1][:, None, :])
            return leaf, w, (w * scores.double()).sum(-1)

        _, w_ref, ens_ref = ref_forward()
        if per_item:
            w_in = wit.to(dev)
            weights, ens = ops.ens_fwd(s_dev, len_dev, weights=w_in)
            assert torch.equal(weights.cpu(), wit), 'per-item weights are an input and stay untouched'
        else:
            weights, ens = ops.ens_fwd(s_dev, len_dev, wv=wv.to(dev), wpad=wpad.to(dev))
            assert torch.equal(weights.cpu(), w_ref.detach().float()), 'the broadcast weights are copies: ' + tag
        _close(ens, ens_ref, FWD_TOL, 'ens ' + tag)

        for use_w, use_e in ((False, True), (True, False), (True, True)):      # d_weights null, d_ens null, both given
            leaf, w, e = ref_forward()
            loss = 0
            if use_w:
                loss = loss + (w * d_w.double()).sum()
            if use_e:
                loss = loss + (e * d_e.double()).sum()
            loss.backward()
            got = ops.ens_bwd(s_dev, len_dev, d_weights=d_w.to(dev) if use_w else None, d_ens=d_e.to(dev) if use_e else None, per_item=bool(per_item))
            sub = ' dw=%d de=%d ' % (use_w, use_e) + tag
            if per_item:
                _close(got, leaf[0].grad, GRAD_TOL, 'dwt' + sub)
            else:
                _close(got[0], leaf[0].grad, GRAD_TOL, 'dwv' + sub)
                _close(got[1], leaf[1].grad, GRAD_TOL, 'dwpad' + sub)


# ======================================================================================================================
# last-row attention of the pruned encoder block
# ======================================================================================================================
def _lastq_ref(kv, q, n, heads):
    """kv [B, T, 2*dm] = [k | v], q [B, dm], n [B]: per (session, head) softmax(q k_j / sqrt(dk)) over the keys j < n; no key: zeros."""
    B, T, dm2 = kv.shape
    dm = dm2 // 2
    dk = dm // heads
    k = kv[:, :, :dm].reshape(B, T, heads, dk)
    v = kv[:, :, dm:].reshape(B, T, heads, dk)
    s = torch.einsum('bthc,bhc->bht', k, q.reshape(B, heads, dk)) / dk ** 0.5
    valid = (torch.arange(T)[None, :] < n[:, None].long())[:, None, :]
    s = s.masked_fill(~valid, float('-inf'))
    m = torch.where(valid.any(-1, keepdim=True), s.max(-1, keepdim=True)[0], torch.zeros_like(s[..., :1])).detach()
    e = torch.exp(s - m) * valid.double()
    den = e.sum(-1, keepdim=True)
    p = e / torch.where(den > 0, den, torch.ones_like(den))
    out = torch.einsum('bht,bthc->bhc', p, v).reshape(B, dm)
    return out, p.reshape(B * heads, T)


@pytest.mark.parametrize('dm,heads', [(128, 2), (64, 1), (32, 2), (16, 4), (256, 1)])
@pytest.mark.parametrize('T', [1, 3, 4, 5, 20, 64, 65, 200, 512])
def test_attn_lastq_fwd_bwd(dm, heads, T):
    from intel_sigir2023_amd import ops
    dev = _dev()
    GUARD = 3
    for B in (1, 3, 6):
        g = _gen(5, dm, heads, T, B)
        for n in _len_vectors(B, [T, 1, 0], T, g):
            tag = 'dm=%d heads=%d T=%d B=%d len=%s' % (dm, heads, T, B, n.tolist())
            kv, q, d_out = _randn(g, B, T, 2 * dm), _randn(g, B, dm), _randn(g, B, dm)
            kvr, qr = kv.double().requires_grad_(True), q.double().requires_grad_(True)
            out_ref, p_ref = _lastq_ref(kvr, qr, n, heads)
            (out_ref * d_out.double()).sum().backward()
            dkv_ref = kvr.grad if kvr.grad is not None else torch.zeros_like(kvr)
            dq_ref = qr.grad if qr.grad is not None else torch.zeros_like(qr)
            valid = torch.arange(T)[None, :] < n[:, None].long()
            assert bool((dkv_ref[~valid] == 0).all())
            n_dev, q_dev, do_dev, p_dev = _i32(n, dev), q.to(dev), d_out.to(dev), p_ref.detach().float().to(dev)

            # padded rows: session b owns rows b*T .. b*T + T - 1
            kv_dev = kv.reshape(B * T, 2 * dm).to(dev)
            out, P = ops.attn_lastq_fwd(kv_dev, q_dev, n_dev, T, heads)
            _close(out, out_ref, FWD_TOL, 'out ' + tag)
            _close(P, p_ref, FWD_TOL, 'P ' + tag)
            dkv = torch.full((B * T, 2 * dm), SENT, dtype=torch.float32, device=dev)
            dq = ops.attn_lastq_bwd(kv_dev, q_dev, p_dev, do_dev, n_dev, T, heads, dkv)
            _close(dq, dq_ref, GRAD_TOL, 'dq ' + tag)
            _close(dkv, dkv_ref.reshape(B * T, 2 * dm), GRAD_TOL, 'dkv ' + tag)
            assert bool((dkv.cpu().reshape(B, T, 2 * dm)[~valid] == 0).all()), 'padded rows of dkv must be exactly 0: ' + tag

            # packed rows: row_off = exclusive prefix sum of the lengths, exactly sum(len) session rows (between guard rows)
            off = torch.cumsum(n.long(), 0) - n.long() + GUARD
            total = int(n.sum())
            kvp = torch.full((total + 2 * GUARD, 2 * dm), SENT)
            for b in range(B):
                kvp[int(off[b]):int(off[b]) + int(n[b])] = kv[b, :int(n[b])]
            kvp_dev, off_dev = kvp.to(dev), _i32(off, dev)
            out, P = ops.attn_lastq_fwd(kvp_dev, q_dev, n_dev, T, heads, row_off=off_dev)
            _close(out, out_ref, FWD_TOL, 'packed out ' + tag)
            _close(P, p_ref, FWD_TOL, 'packed P ' + tag)
            dkvp = torch.full((total + 2 * GUARD, 2 * dm), SENT, dtype=torch.float32, device=dev)
            dq = ops.attn_lastq_bwd(kvp_dev, q_dev, p_dev, do_dev, n_dev, T, heads, dkvp, row_off=off_dev)
            _close(dq, dq_ref, GRAD_TOL, 'packed dq ' + tag)
            dkvp = dkvp.cpu()
            assert bool((dkvp[:GUARD] == SENT).all()) and bool((dkvp[GUARD + total:] == SENT).all()), 'packed dkv: rows outside the sessions changed: ' + tag
            for b in range(B):
                _close(dkvp[int(off[b]):int(off[b]) + int(n[b])], dkv_ref[b, :int(n[b])], GRAD_TOL, 'packed dkv session %d ' % b + tag)

            # select_last / add_at_last: row len-1 of every session; len == 0: zeros out, nothing added
            E = _randn(g, B, T, dm)
            ldo, col0 = dm + 5, 3
            sel_ref = torch.full((B, ldo), SENT)
            for b in range(B):
                sel_ref[b, col0:col0 + dm] = E[b, int(n[b]) - 1] if int(n[b]) > 0 else 0.0
            Ep = torch.full((total + 2 * GUARD, dm), SENT)
            for b in range(B):
                Ep[int(off[b]):int(off[b]) + int(n[b])] = E[b, :int(n[b])]
            sel = ops.select_last(E.reshape(B * T, dm).to(dev), n_dev, T, torch.full((B, ldo), SENT, device=dev), col0)
            assert torch.equal(sel.cpu(), sel_ref), 'select_last ' + tag
            sel = ops.select_last(Ep.to(dev), n_dev, T, torch.full((B, ldo), SENT, device=dev), col0, row_off=off_dev)
            assert torch.equal(sel.cpu(), sel_ref), 'packed select_last ' + tag
            src = _randn(g, B, dm + 4)
            add_ref = E.clone()
            addp_ref = Ep.clone()
            for b in range(B):
                if int(n[b]) > 0:
                    add_ref[b, int(n[b]) - 1] += src[b, :dm]
                    addp_ref[int(off[b]) + int(n[b]) - 1] += src[b, :dm]
            got = ops.add_at_last(src.to(dev), dm, n_dev, T, E.reshape(B * T, dm).to(dev))
            assert torch.equal(got.cpu(), add_ref.reshape(B * T, dm)), 'add_at_last ' + tag
            got = ops.add_at_last(src.to(dev), dm, n_dev, T, Ep.to(dev), row_off=off_dev)
            assert torch.equal(got.cpu(), addp_ref), 'packed add_at_last ' + tag


# ======================================================================================================================
# LayerNorm backward
# ======================================================================================================================
LN_N = [64, 128, 256, 32, 16, 30, 33, 96, 200, 512]
LN_M = [1, 15, 16, 17, 130, 4099]
LN_CASES = [(N, M, 0) for N in LN_N for M in LN_M] + \
           [(N, M, 0) for N in (128, 32, 96) for M in (16384, 16385, 16449)] + \
           [(N, M, 1) for N in (64, 128, 256) for M in LN_M]       # pitches N + 1: the generic kernel, as with the model's input pitch


@pytest.mark.parametrize('N,M,pad', LN_CASES)
def test_layernorm_bwd(N, M, pad):
    from intel_sigir2023_amd import ops
    dev = _dev()
    g = _gen(6, N, M, pad)
    z = torch.randn(M, N, generator=g, dtype=torch.float64)
    gamma, beta, dy = _randn(g, N), _randn(g, N), _randn(g, M, N)
    dg0, db0 = _randn(g, N), _randn(g, N)
    zr, gr, br = z.clone().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    (F.layer_norm(zr, (N,), gr, br, 1e-5) * dy.double()).sum().backward()
    xhat64, rstd64 = _ln_stash(z)
    ld = N + pad

    def pitched(t):
        buf = torch.full((M, ld), SENT)
        buf[:, :N] = t
        return buf.to(dev)
    dy_dev, xh_dev, rstd_dev, gamma_dev = pitched(dy), pitched(xhat64.float()), rstd64.float().to(dev), gamma.to(dev)
    for queued in (1, 0):
        for accumulate in (0, 1):
            tag = 'N=%d M=%d ld=%d queued=%d accumulate=%d' % (N, M, ld, queued, accumulate)
            dz = torch.full((M, ld), SENT, device=dev)
            dgamma, dbeta = dg0.clone().to(dev), db0.clone().to(dev)
            ops.layernorm_bwd(dy_dev, xh_dev, rstd_dev, N, gamma_dev, dz, dgamma, dbeta, accumulate=bool(accumulate), queued=bool(queued))
            _close(dz[:, :N], zr.grad, GRAD_TOL, 'dz ' + tag)
            assert bool((dz[:, N:] == SENT).all()), 'dz: columns beyond N changed: ' + tag
            _close(dgamma, gr.grad + (dg0.double() if accumulate else 0), GRAD_TOL, 'dgamma ' + tag)
            _close(dbeta, br.grad + (db0.double() if accumulate else 0), GRAD_TOL, 'dbeta ' + tag)


# ======================================================================================================================
# row softmax
# ======================================================================================================================
@pytest.mark.parametrize('M,N', [(1, 1), (5, 3), (4099, 8), (7, 64), (6, 65), (9, 200)])
def test_softmax_rows_fwd_bwd(M, N):
    from intel_sigir2023_amd import ops
    dev = _dev()
    g = _gen(7, M, N)
    x, dy = _randn(g, M, N), _randn(g, M, N)
    xr = x.double().requires_grad_(True)
    y_ref = torch.softmax(xr, -1)
    (y_ref * dy.double()).sum().backward()
    y = ops.softmax_rows(x.to(dev))
    _close(y, y_ref, FWD_TOL, 'softmax')
    buf = x.to(dev)
    assert ops.softmax_rows(buf, out=buf) is buf
    assert torch.equal(buf, y), 'in place and out of place must agree bit for bit'
    y_in = y_ref.detach().float().to(dev)
    dx = ops.softmax_rows_bwd(y_in, dy.to(dev))
    _close(dx, xr.grad, GRAD_TOL, 'softmax bwd')
    buf = dy.to(dev)
    ops.softmax_rows_bwd(y_in, buf, out=buf)          # dx aliasing dy, as the model calls it
    _close(buf, xr.grad, GRAD_TOL, 'softmax bwd (dx aliases dy)')
    assert torch.equal(buf, dx), 'the aliased form must agree with the out-of-place one bit for bit'


# ======================================================================================================================
# embedding scatter
# ======================================================================================================================
def _scatter_sorted_ids(dist, n, d, V, g):
    """The id multiset of one case as its SORTED sequence (negatives = skipped pairs first)."""
    per_wg = (256 // (d // 4)) * 16
    n_neg = min(n // 5, 3)

    def rand_sorted(count, lo, hi):
        return torch.sort(torch.randint(lo, hi, (count,), generator=g))[0] if count > 0 else torch.zeros(0, dtype=torch.long)

    def with_run_ending_at(p, run):
        lo = max(n_neg, p - run)
        hot = V // 3
        return torch.cat([torch.full((min(n_neg, lo),), -1, dtype=torch.long), rand_sorted(lo - min(n_neg, lo), 0, hot), torch.full((p - lo,), hot, dtype=torch.long),
                          rand_sorted(n - p, hot + 1, V)])
    if dist == 'distinct':
        ids = torch.sort(torch.randperm(V, generator=g)[:n])[0]
        ids[:n_neg] = -1
        return ids
    if dist == 'equal':
        return torch.full((n,), V // 2, dtype=torch.long)
    if dist == 'zipf':
        ids = torch.sort((V * torch.rand(n, generator=g) ** 6).long().clamp(max=V - 1))[0]
        ids[:n_neg] = -1
        return ids
    if dist == 'chunk_edge':       # a run that ends exactly on a 16-pair boundary (n < 16: at n)
        p = (n // 16) * 16 if n >= 16 else n
        return with_run_ending_at(p, 40 if p > 16 else 7)
    if dist == 'wg_edge':          # a run that ends exactly on a workgroup boundary (n smaller than one workgroup's span: at n)
        p = (n // per_wg) * per_wg if n >= per_wg else n
        return with_run_ending_at(p, per_wg + 40)
    raise AssertionError(dist)


@pytest.mark.parametrize('d', [16, 32, 64, 128])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 255, 256, 257, 5000])
def test_scatter_add_sorted_and_unsorted(d, n):
    from intel_sigir2023_amd import ops
    dev = _dev()
    V = 6000
    pitch, col0 = d + 8, 4
    for dist in ('distinct', 'equal', 'zipf', 'chunk_edge', 'wg_edge'):
        g = _gen(8, d, n, len(dist))
        tag = 'd=%d n=%d %s' % (d, n, dist)
        seq = _scatter_sorted_ids(dist, n, d, V, g)
        assert seq.numel() == n and int(seq.max()) < V and bool((seq[1:] >= seq[:-1]).all())
        idx = seq[torch.randperm(n, generator=g)]                    # the batch's ids in source-row order
        src = _randn(g, n, pitch)
        mask = _randn(g, n, pitch)
        table0 = _randn(g, V, d)
        order = torch.sort(idx, stable=True)[1]
        sorted_ids, sorted_rows = idx[order], order
        assert torch.equal(sorted_ids, seq)
        keep = idx >= 0
        block = src[:, col0:col0 + d].double()
        ref = table0.double().index_add_(0, idx[keep], block[keep])
        ref_relu = table0.double().index_add_(0, idx[keep], (block * (mask[:, col0:col0 + d] > 0))[keep])
        flags_ref = torch.zeros(V, dtype=torch.uint8)
        flags_ref[idx[keep]] = 1
        src_dev = src.to(dev)

        table, flags = table0.clone().to(dev), torch.zeros(V, dtype=torch.uint8, device=dev)
        ops.scatter_add_sorted(src_dev, col0, d, _i32(sorted_ids, dev), _i32(sorted_rows, dev), table, row_flags=flags)
        _close(table, ref, GRAD_TOL, 'sorted ' + tag)
        assert torch.equal(flags.cpu(), flags_ref), 'sorted row_flags ' + tag

        table, flags = table0.clone().to(dev), torch.zeros(V, dtype=torch.uint8, device=dev)
        ops.scatter_add_rows(src_dev, col0, d, _i32(idx, dev), table, row_flags=flags)
        _close(table, ref, GRAD_TOL, 'unsorted ' + tag)
        assert torch.equal(flags.cpu(), flags_ref), 'unsorted row_flags ' + tag

        table = table0.clone().to(dev)
        ops.scatter_add_rows(src_dev, col0, d, _i32(idx, dev), table, relu_out=mask.to(dev), rcol0=col0)
        _close(table, ref_relu, GRAD_TOL, 'unsorted relu ' + tag)


@pytest.mark.parametrize('d', [16, 32, 64, 128])
@pytest.mark.parametrize('B,T', [(3, 5), (9, 37)])
def test_scatter_add_sorted_packed_rows(d, B, T):
    """Pair rows b*T + t over PACKED source rows (row_off / len): the padded positions t >= len[b] carry the same few ids as the valid
    ones, so after the sort they lie inside runs of valid ids and must be skipped there."""
    from intel_sigir2023_amd import ops
    dev = _dev()
    V = 50
    pitch, col0 = d + 4, 4
    g = _gen(9, d, B, T)
    for n in _len_vectors(B, [T, 1, 0], T, g):
        tag = 'd=%d B=%d T=%d len=%s' % (d, B, T, n.tolist())
        ids = torch.randint(0, 4, (B, T), generator=g) * 7 + 2            # four hot ids: long runs
        ids[torch.rand(B, T, generator=g) < 0.1] = -1
        off = torch.cumsum(n.long(), 0) - n.long()
        total = int(n.sum())
        src = _randn(g, max(total, 1), pitch)
        table0 = _randn(g, V, d)
        flat = ids.reshape(-1)
        order = torch.sort(flat, stable=True)[1]
        ref = table0.double()
        flags_ref = torch.zeros(V, dtype=torch.uint8)
        for b in range(B):
            for t in range(int(n[b])):
                if int(ids[b, t]) >= 0:
                    ref[int(ids[b, t])] += src[int(off[b]) + t, col0:col0 + d].double()
                    flags_ref[int(ids[b, t])] = 1
        table, flags = table0.clone().to(dev), torch.zeros(V, dtype=torch.uint8, device=dev)
        ops.scatter_add_sorted(src.to(dev), col0, d, _i32(flat[order], dev), _i32(order, dev), table, row_flags=flags, row_off=_i32(off, dev),
                               length=_i32(n, dev), T=T)
        _close(table, ref, GRAD_TOL, 'packed sorted ' + tag)
        assert torch.equal(flags.cpu(), flags_ref), 'packed row_flags ' + tag


# ======================================================================================================================
# gates and column sums
# ======================================================================================================================
@pytest.mark.parametrize('d', [32, 64, 300])
def test_gates_and_session_colsum(d):
    from intel_sigir2023_amd import ops
    dev = _dev()
    for L in (1, 7, 50):
        for B in (1, 5):
            g = _gen(10, d, L, B)
            tag = 'd=%d L=%d B=%d' % (d, L, B)
            ldf, col0 = 2 * d + 7, d // 2 + 1
            x, vec = _randn(g, B, L, d), _randn(g, B, d)
            dfeat, dfeat_b = _randn(g, B * L, ldf), _randn(g, B, ldf)
            cols = torch.zeros(ldf, dtype=torch.bool)
            cols[col0:col0 + d] = True

            # elementwise gate
            xr, vr = x.double().requires_grad_(True), vec.double().requires_grad_(True)
            y_ref = xr * vr[:, None, :]
            (y_ref.reshape(B * L, d) * dfeat[:, cols].double()).sum().backward()
            dst = ops.gate_fwd(x.to(dev), vec.to(dev), torch.full((B * L, ldf), SENT, device=dev), col0).cpu()
            _close(dst[:, cols], y_ref.reshape(B * L, d), FWD_TOL, 'gate ' + tag)
            assert bool((dst[:, ~cols] == SENT).all()), 'gate: columns outside the block changed: ' + tag
            dx, dvec = ops.gate_bwd(dfeat.to(dev), col0, x.to(dev), vec.to(dev))
            _close(dx, xr.grad, GRAD_TOL, 'gate dx ' + tag)
            _close(dvec, vr.grad, GRAD_TOL, 'gate dvec ' + tag)

            # mean-pooled gate
            xr, vr = x.double().requires_grad_(True), vec.double().requires_grad_(True)
            xbar_ref = xr.mean(1)
            f_ref = xbar_ref * vr
            (f_ref * dfeat_b[:, cols].double()).sum().backward()
            xbar, feat = ops.gate_mean_fwd(x.to(dev), vec.to(dev), torch.full((B, ldf), SENT, device=dev), col0)
            feat = feat.cpu()
            _close(xbar, xbar_ref, FWD_TOL, 'gate_mean xbar ' + tag)
            _close(feat[:, cols], f_ref, FWD_TOL, 'gate_mean feat ' + tag)
            assert bool((feat[:, ~cols] == SENT).all()), 'gate_mean: columns outside the block changed: ' + tag
            dx, dvec = ops.gate_mean_bwd(dfeat_b.to(dev), col0, xbar_ref.detach().float().to(dev), vec.to(dev), L)
            _close(dx, xr.grad, GRAD_TOL, 'gate_mean dx ' + tag)
            _close(dvec, vr.grad, GRAD_TOL, 'gate_mean dvec ' + tag)

            # column sums over the list
            ldo, ocol0 = d + 9, 5
            ocols = torch.zeros(ldo, dtype=torch.bool)
            ocols[ocol0:ocol0 + d] = True
            sum_ref = dfeat[:, cols].double().reshape(B, L, d).sum(1)
            out0 = _randn(g, B, ldo)
            for accumulate in (0, 1):
                out = ops.session_colsum(dfeat.to(dev), col0, d, B, L, out0.clone().to(dev), ocol0, accumulate=bool(accumulate)).cpu()
                _close(out[:, ocols], sum_ref + (out0[:, ocols].double() if accumulate else 0), GRAD_TOL, 'colsum acc=%d ' % accumulate + tag)
                assert torch.equal(out[:, ~ocols], out0[:, ~ocols]), 'colsum: columns outside the block changed: ' + tag
