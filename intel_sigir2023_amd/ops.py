"""Thin tensor-level wrappers over the building-block entry points (used by tests and the model)."""
import torch

from . import _lib as L


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def linear(x, w, bias=None, relu=False):
    L.require_gpu(x)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    nb = L.lib().intel_op_workspace_bytes(M, N, K)
    ws = _ws(nb, x.device)
    L.check(L.lib().intel_op_linear(L.ptr(x), M, K, L.ptr(w), N, L.ptr(bias), int(relu), L.ptr(y), L.ptr(ws), nb,
                                    L.stream_ptr(x.device)), 'intel_op_linear')
    return y


def linear_dgrad(dy, w):
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    nb = L.lib().intel_op_workspace_bytes(M, N, K)
    ws = _ws(nb, dy.device)
    L.check(L.lib().intel_op_linear_dgrad(L.ptr(dy), M, N, L.ptr(w), K, L.ptr(dx), L.ptr(ws), nb, L.stream_ptr(dy.device)),
            'intel_op_linear_dgrad')
    return dx


def linear_wgrad(dy, x, want_bias=True):
    M, N = dy.shape
    K = x.shape[1]
    dw = torch.empty(N, K, dtype=torch.float32, device=dy.device)
    db = torch.empty(N, dtype=torch.float32, device=dy.device) if want_bias else None
    nb = L.lib().intel_op_workspace_bytes(M, N, K)
    ws = _ws(nb, dy.device)
    L.check(L.lib().intel_op_linear_wgrad(L.ptr(dy), L.ptr(x), M, N, K, L.ptr(dw), L.ptr(db), L.ptr(ws), nb,
                                          L.stream_ptr(dy.device)), 'intel_op_linear_wgrad')
    return dw, db


def linear_bwd(dy, x, w, relu_mask=False, want_bias=True):
    """Both products of a [d -> d] nn.Linear's backward in one pass over the rows (csrc/pair.hip): dx = (dy @ w) [* (x > 0)], dw = dy^T x,
    db = colsum(dy)."""
    M, d = dy.shape
    dx = torch.empty(M, d, dtype=torch.float32, device=dy.device)
    dw = torch.empty(d, d, dtype=torch.float32, device=dy.device)
    db = torch.empty(d, dtype=torch.float32, device=dy.device) if want_bias else None
    nb = L.lib().intel_op_linear_bwd_workspace_bytes(M, d)
    ws = _ws(nb, dy.device)
    L.check(L.lib().intel_op_linear_bwd(L.ptr(dy), L.ptr(x), M, d, L.ptr(w), 1 if relu_mask else 0, L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(ws), nb,
                                        L.stream_ptr(dy.device)), 'intel_op_linear_bwd')
    return dx, dw, db


def linear_bwd_qkv(dy, x, w, res=None, want_bias=False):
    """The backward of a fused q/k/v projection in one pass over the rows (csrc/pair.hip): dy [M, nb*d], w [nb*d, d] stacked, x [M, d]:
    dx = dy @ w (+ res), dw = dy^T x, db = colsum(dy)."""
    M, n = dy.shape
    d = x.shape[1]
    nb = n // d
    dx = torch.empty(M, d, dtype=torch.float32, device=dy.device)
    dw = torch.empty(n, d, dtype=torch.float32, device=dy.device)
    db = torch.empty(n, dtype=torch.float32, device=dy.device) if want_bias else None
    nbytes = L.lib().intel_op_linear_bwd_qkv_workspace_bytes(M, d, nb)
    ws = _ws(nbytes, dy.device)
    L.check(L.lib().intel_op_linear_bwd_qkv(L.ptr(dy), L.ptr(x), L.ptr(res), M, d, nb, L.ptr(w), L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(ws), nbytes,
                                            L.stream_ptr(dy.device)), 'intel_op_linear_bwd_qkv')
    return dx, dw, db


def attention(qkv, B, T, d, heads, key_len=None):
    out = torch.empty(B * T, d, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(B * heads * T, dtype=torch.float32, device=qkv.device)
    L.check(L.lib().intel_op_attention(L.ptr(qkv), B, T, d, heads, L.ptr(key_len), L.ptr(out), L.ptr(lse),
                                       L.stream_ptr(qkv.device)), 'intel_op_attention')
    return out, lse


def attention_bwd(qkv, out, dout, lse, B, T, d, heads, key_len=None):
    dqkv = torch.empty_like(qkv)
    nbytes = L.lib().intel_op_attention_bwd_workspace_bytes(B, T, d, heads)
    dsum = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=qkv.device)
    L.check(L.lib().intel_op_attention_bwd(L.ptr(qkv), L.ptr(out), L.ptr(dout), L.ptr(lse), B, T, d, heads,
                                           L.ptr(key_len), L.ptr(dqkv), L.ptr(dsum), L.stream_ptr(qkv.device)),
            'intel_op_attention_bwd')
    return dqkv


def add_layernorm(x, r, gamma, beta, stash=False):
    M, N = x.shape
    y = torch.empty_like(x)
    xhat = torch.empty_like(x) if stash else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if stash else None
    L.check(L.lib().intel_op_add_layernorm(L.ptr(x), L.ptr(r), M, N, L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(xhat),
                                           L.ptr(rstd), L.stream_ptr(x.device)), 'intel_op_add_layernorm')
    return (y, xhat, rstd) if stash else y


# ------------------------------------------------------------------------------------------------------------------------
# session / row kernels (csrc/session.hip, csrc/rowops.hip) for the unit tests (tests/test_session_gpu.py).  ctypes only: they
# are not dispatcher ops.  Buffers with a pitch (`ld*`) and a column offset (`col0`) are passed as the caller allocated them.
# ------------------------------------------------------------------------------------------------------------------------
def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def xatt_pool_fwd(x, qk, session_len, scale, gamma=None, beta=None):
    """x [B, L, d] (or its x-hat stash with gamma / beta), qk [B, d], session_len int32 [B] -> xbar [B, d], attw [B, L]."""
    B, Lm, d = x.shape
    xbar, attw = _f32((B, d), x), _f32((B, Lm), x)
    L.check(L.lib().intel_op_xatt_pool_fwd(L.ptr(x), B, Lm, d, L.ptr(qk), L.ptr(session_len), float(scale), L.ptr(gamma), L.ptr(beta), L.ptr(xbar),
                                           L.ptr(attw), L.stream_ptr(x.device)), 'intel_op_xatt_pool_fwd')
    return xbar, attw


def xatt_pool_bwd(x, qk, attw, dxbar, scale):
    """dxbar [B, ldxb] (the first d columns are used) -> dx [B, L, d], dqk [B, d]."""
    B, Lm, d = x.shape
    dx, dqk = torch.empty_like(x), _f32((B, d), x)
    L.check(L.lib().intel_op_xatt_pool_bwd(L.ptr(x), B, Lm, d, L.ptr(qk), L.ptr(attw), L.ptr(dxbar), dxbar.shape[1], float(scale), L.ptr(dx), L.ptr(dqk),
                                           L.stream_ptr(x.device)), 'intel_op_xatt_pool_bwd')
    return dx, dqk


def xatt_pool_ln_bwd(xhat, rstd, gamma, beta, qk, attw, dxbar, scale, dgamma, dbeta, accumulate=False):
    """The pooling backward fused with the LayerNorm backward: -> dz [B, L, d], dqk [B, d]; dgamma / dbeta [d] written or accumulated in place."""
    B, Lm, d = xhat.shape
    dz, dqk = torch.empty_like(xhat), _f32((B, d), xhat)
    nb = L.lib().intel_op_xatt_pool_ln_bwd_workspace_bytes(B, d)
    ws = _ws(nb, xhat.device)
    L.check(L.lib().intel_op_xatt_pool_ln_bwd(L.ptr(xhat), L.ptr(rstd), L.ptr(gamma), L.ptr(beta), B, Lm, d, L.ptr(qk), L.ptr(attw), L.ptr(dxbar),
                                              dxbar.shape[1], float(scale), L.ptr(dz), L.ptr(dqk), L.ptr(dgamma), L.ptr(dbeta), int(accumulate), L.ptr(ws),
                                              nb, L.stream_ptr(xhat.device)), 'intel_op_xatt_pool_ln_bwd')
    return dz, dqk


def ens_fwd(scores, session_len, wv=None, wpad=None, weights=None):
    """scores [B, L, K]; wv / wpad [B, K] (session weights) or weights [B, L, K] (per item) -> weights, ens [B, L]."""
    B, Lm, K = scores.shape
    per_item = weights is not None
    if not per_item:
        weights = torch.empty_like(scores)
    ens = _f32((B, Lm), scores)
    L.check(L.lib().intel_op_ens_fwd(L.ptr(wv), L.ptr(wpad), L.ptr(scores), L.ptr(session_len), B, Lm, K, int(per_item), L.ptr(weights), L.ptr(ens),
                                     L.stream_ptr(scores.device)), 'intel_op_ens_fwd')
    return weights, ens


def ens_bwd(scores, session_len, d_weights=None, d_ens=None, per_item=False):
    """-> (dwv, dwpad) [B, K] each, or dwt [B, L, K] when per_item."""
    B, Lm, K = scores.shape
    dwv = dwpad = dwt = None
    if per_item:
        dwt = torch.empty_like(scores)
    else:
        dwv, dwpad = _f32((B, K), scores), _f32((B, K), scores)
    L.check(L.lib().intel_op_ens_bwd(L.ptr(d_weights), L.ptr(d_ens), L.ptr(scores), L.ptr(session_len), B, Lm, K, int(per_item), L.ptr(dwv), L.ptr(dwpad),
                                     L.ptr(dwt), L.stream_ptr(scores.device)), 'intel_op_ens_bwd')
    return dwt if per_item else (dwv, dwpad)


def attn_lastq_fwd(kv, q, length, T, heads, row_off=None):
    """kv [rows, 2*dm] (padded: rows = B*T; packed: row_off[b] + t), q [B, dm] -> out [B, dm], P [B*heads, T]."""
    B, dm = q.shape
    out, P = torch.empty_like(q), _f32((B * heads, T), q)
    L.check(L.lib().intel_op_attn_lastq_fwd(L.ptr(kv), L.ptr(q), L.ptr(length), L.ptr(row_off), B, T, dm, heads, L.ptr(out), L.ptr(P),
                                            L.stream_ptr(q.device)), 'intel_op_attn_lastq_fwd')
    return out, P


def attn_lastq_bwd(kv, q, P, d_out, length, T, heads, dkv, row_off=None):
    """-> dq [B, dm]; dkv (same layout as kv) is written in place."""
    B, dm = q.shape
    dq = torch.empty_like(q)
    L.check(L.lib().intel_op_attn_lastq_bwd(L.ptr(kv), L.ptr(q), L.ptr(P), L.ptr(d_out), L.ptr(length), L.ptr(row_off), B, T, dm, heads, L.ptr(dq),
                                            L.ptr(dkv), L.stream_ptr(q.device)), 'intel_op_attn_lastq_bwd')
    return dq


def select_last(E, length, T, out, col0, row_off=None):
    """out[b, col0:col0+dm] = E[row of position length[b]-1] (in place on `out` [B, ldo])."""
    dm, B = E.shape[1], length.shape[0]
    L.check(L.lib().intel_op_select_last(L.ptr(E), dm, L.ptr(length), L.ptr(row_off), B, T, L.ptr(out), out.shape[1], col0, L.stream_ptr(E.device)),
            'intel_op_select_last')
    return out


def add_at_last(src, dm, length, T, dX, row_off=None):
    """dX[row of position length[b]-1, :] += src[b, 0:dm] (in place on dX [rows, dm]; src [B, lds])."""
    B = length.shape[0]
    L.check(L.lib().intel_op_add_at_last(L.ptr(src), src.shape[1], dm, L.ptr(length), L.ptr(row_off), B, T, L.ptr(dX), L.stream_ptr(src.device)),
            'intel_op_add_at_last')
    return dX


def layernorm_bwd(dy, xhat, rstd, N, gamma, dz, dgamma, dbeta, accumulate=False, queued=True):
    """dy / xhat / dz [M, pitch >= N] with their own pitches; dz is written in place, dgamma / dbeta [N] written or accumulated in place."""
    M = dy.shape[0]
    nb = L.lib().intel_op_layernorm_bwd_workspace_bytes(M, N)
    ws = _ws(nb, dy.device)
    L.check(L.lib().intel_op_layernorm_bwd(L.ptr(dy), dy.shape[1], L.ptr(xhat), xhat.shape[1], L.ptr(rstd), M, N, L.ptr(gamma), L.ptr(dz), dz.shape[1],
                                           L.ptr(dgamma), L.ptr(dbeta), int(accumulate), int(queued), L.ptr(ws), nb, L.stream_ptr(dy.device)),
            'intel_op_layernorm_bwd')
    return dz, dgamma, dbeta


def softmax_rows(x, out=None):
    M, N = x.shape
    y = torch.empty_like(x) if out is None else out
    L.check(L.lib().intel_op_softmax_rows(L.ptr(x), M, N, L.ptr(y), L.stream_ptr(x.device)), 'intel_op_softmax_rows')
    return y


def softmax_rows_bwd(y, dy, out=None):
    M, N = y.shape
    dx = torch.empty_like(y) if out is None else out
    L.check(L.lib().intel_op_softmax_rows_bwd(L.ptr(y), L.ptr(dy), M, N, L.ptr(dx), L.stream_ptr(y.device)), 'intel_op_softmax_rows_bwd')
    return dx


def scatter_add_rows(src, col0, d, idx, table, relu_out=None, rcol0=0, row_flags=None):
    """table[idx[m], :] += src[m, col0:col0+d] (* (relu_out[m, rcol0:rcol0+d] > 0)); in place on table [rows, d]."""
    L.check(L.lib().intel_op_scatter_add_rows(L.ptr(src), src.shape[1], col0, d, L.ptr(idx), idx.numel(), L.ptr(table), L.ptr(relu_out),
                                              relu_out.shape[1] if relu_out is not None else 0, rcol0, L.ptr(row_flags), L.stream_ptr(src.device)),
            'intel_op_scatter_add_rows')
    return table


def scatter_add_sorted(src, col0, d, sorted_ids, sorted_rows, table, row_flags=None, row_off=None, length=None, T=0):
    L.check(L.lib().intel_op_scatter_add_sorted(L.ptr(src), src.shape[1], col0, d, L.ptr(sorted_ids), L.ptr(sorted_rows), sorted_ids.numel(), L.ptr(table),
                                                L.ptr(row_flags), L.ptr(row_off), L.ptr(length), T, L.stream_ptr(src.device)), 'intel_op_scatter_add_sorted')
    return table


def gate_fwd(x, vec, dst, col0):
    B, Lm, d = x.shape
    L.check(L.lib().intel_op_gate_fwd(L.ptr(x), d, L.ptr(vec), B, Lm, L.ptr(dst), dst.shape[1], col0, L.stream_ptr(x.device)), 'intel_op_gate_fwd')
    return dst


def gate_bwd(dfeat, col0, x, vec):
    B, Lm, d = x.shape
    dx, dvec = torch.empty_like(x), torch.empty_like(vec)
    L.check(L.lib().intel_op_gate_bwd(L.ptr(dfeat), dfeat.shape[1], col0, L.ptr(x), d, L.ptr(vec), B, Lm, L.ptr(dx), L.ptr(dvec), L.stream_ptr(x.device)),
            'intel_op_gate_bwd')
    return dx, dvec


def gate_mean_fwd(x, vec, feat, col0):
    B, Lm, d = x.shape
    xbar = torch.empty_like(vec)
    L.check(L.lib().intel_op_gate_mean_fwd(L.ptr(x), d, L.ptr(vec), B, Lm, L.ptr(xbar), L.ptr(feat), feat.shape[1], col0, L.stream_ptr(x.device)),
            'intel_op_gate_mean_fwd')
    return xbar, feat


def gate_mean_bwd(dfeat, col0, xbar, vec, Lm):
    B, d = vec.shape
    dx, dvec = _f32((B, Lm, d), vec), torch.empty_like(vec)
    L.check(L.lib().intel_op_gate_mean_bwd(L.ptr(dfeat), dfeat.shape[1], col0, L.ptr(xbar), d, L.ptr(vec), B, Lm, L.ptr(dx), L.ptr(dvec),
                                           L.stream_ptr(vec.device)), 'intel_op_gate_mean_bwd')
    return dx, dvec


def session_colsum(src, col0, d, B, Lm, out, ocol0, accumulate=False):
    L.check(L.lib().intel_op_session_colsum(L.ptr(src), src.shape[1], col0, d, B, Lm, L.ptr(out), out.shape[1], ocol0, int(accumulate),
                                            L.stream_ptr(src.device)), 'intel_op_session_colsum')
    return out


# ------------------------------------------------------------------------------------------------------------------------
# GRU4Rec recurrence (csrc/gru.hip) for the unit tests (tests/test_gru_op_gpu.py).  ctypes only.  The caller owns the workspace:
# the backward reads the stash that the forward left in it.
# ------------------------------------------------------------------------------------------------------------------------
def gru_workspace(B, T, dm, device):
    return _ws(L.lib().intel_op_gru_workspace_bytes(B, T, dm), device)


def gru_fwd(E0, B, T, length, Wih, Whh, bih, bhh, Wout, out, col0, ws, form=-1, stash=True, off=None, order=None):
    """E0 [B*T, dm] padded rows, or with off (int32 [B], exclusive prefix sum of length) the packed valid rows; hidden size 128.
    out[:, col0:col0+dm] = h_last Wout^T is written in place.  form: 0 per step, 1 exact-fp32 recurrence, 2 three-plane recurrence."""
    dm = E0.shape[1]
    L.check(L.lib().intel_op_gru_fwd(L.ptr(E0), B, T, dm, L.ptr(length), L.ptr(off), E0.shape[0], L.ptr(order), L.ptr(Wih), L.ptr(Whh), L.ptr(bih),
                                     L.ptr(bhh), L.ptr(Wout), L.ptr(out), out.shape[1], col0, int(stash), form, L.ptr(ws), ws.numel(),
                                     L.stream_ptr(E0.device)), 'intel_op_gru_fwd')
    return out


def gru_bwd(E0, B, T, length, Whh, bhh, dout, col0, ws, form=-1, queued=False, off=None, order=None):
    """After gru_fwd(..., stash=True) with the same arguments on the same workspace: dvec = dout[:, col0:col0+dm] ->
    dict of dE0 (like E0), dWih, dWhh, dbih, dbhh, dWout."""
    dm = E0.shape[1]
    g = {'dE0': torch.empty_like(E0), 'dWih': _f32((384, dm), E0), 'dWhh': _f32((384, 128), E0), 'dbih': _f32((384,), E0), 'dbhh': _f32((384,), E0),
         'dWout': _f32((dm, 128), E0)}
    L.check(L.lib().intel_op_gru_bwd(L.ptr(E0), B, T, dm, L.ptr(length), L.ptr(off), E0.shape[0], L.ptr(order), L.ptr(Whh), L.ptr(bhh), L.ptr(dout),
                                     dout.shape[1], col0, L.ptr(g['dWih']), L.ptr(g['dWhh']), L.ptr(g['dbih']), L.ptr(g['dbhh']), L.ptr(g['dWout']),
                                     L.ptr(g['dE0']), int(queued), form, L.ptr(ws), ws.numel(), L.stream_ptr(E0.device)), 'intel_op_gru_bwd')
    return g


# ------------------------------------------------------------------------------------------------------------------------
# torch.library registration: the same entry points as dispatcher-visible custom ops, `torch.ops.intel_mi355x.*`
# (north_star: "exposed ... as PyTorch-ROCm custom ops").  The C ABI stays the lowest layer; these are
# thin schemas over it with shape ("fake") functions for tracing and autograd formulas where the reference differentiates
# through the op.  The whole model is registered too: torch.ops.intel_mi355x.intel_forward (+ intel_backward as its autograd
# formula) over the struct-based C entry points; model.forward takes it with INTEL_MODEL_OP=1 (ops.model_forward), otherwise the
# equivalent autograd.Function of model.py.
# ------------------------------------------------------------------------------------------------------------------------
NAMESPACE = 'intel_mi355x'


def _register():
    from torch.library import custom_op

    @custom_op(NAMESPACE + '::linear', mutates_args=(), device_types='cuda')
    def op_linear(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, relu: bool) -> torch.Tensor:
        return linear(x.contiguous(), w.contiguous(), bias if bias.numel() else None, relu)

    @op_linear.register_fake
    def _(x, w, bias, relu):
        return x.new_empty(x.shape[0], w.shape[0])

    @custom_op(NAMESPACE + '::linear_dgrad', mutates_args=(), device_types='cuda')
    def op_linear_dgrad(dy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        return linear_dgrad(dy.contiguous(), w.contiguous())

    @op_linear_dgrad.register_fake
    def _(dy, w):
        return dy.new_empty(dy.shape[0], w.shape[1])

    @custom_op(NAMESPACE + '::linear_wgrad', mutates_args=(), device_types='cuda')
    def op_linear_wgrad(dy: torch.Tensor, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        return linear_wgrad(dy.contiguous(), x.contiguous(), True)

    @op_linear_wgrad.register_fake
    def _(dy, x):
        return dy.new_empty(dy.shape[1], x.shape[1]), dy.new_empty(dy.shape[1])

    def _linear_setup(ctx, inputs, output):
        x, w, bias, relu = inputs
        ctx.save_for_backward(x, w, output)
        ctx.relu, ctx.has_bias = relu, bias.numel() > 0

    def _linear_backward(ctx, g):
        x, w, y = ctx.saved_tensors
        g = g.contiguous()
        if ctx.relu:
            g = g * (y > 0)
        dw, db = torch.ops.intel_mi355x.linear_wgrad(g, x)
        return torch.ops.intel_mi355x.linear_dgrad(g, w), dw, (db if ctx.has_bias else None), None

    op_linear.register_autograd(_linear_backward, setup_context=_linear_setup)

    @custom_op(NAMESPACE + '::attention', mutates_args=(), device_types='cuda')
    def op_attention(qkv: torch.Tensor, B: int, T: int, d: int, heads: int) -> tuple[torch.Tensor, torch.Tensor]:
        return attention(qkv.contiguous(), B, T, d, heads)

    @op_attention.register_fake
    def _(qkv, B, T, d, heads):
        return qkv.new_empty(B * T, d), qkv.new_empty(B * heads * T)

    @custom_op(NAMESPACE + '::attention_bwd', mutates_args=(), device_types='cuda')
    def op_attention_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, B: int, T: int, d: int,
                         heads: int) -> torch.Tensor:
        return attention_bwd(qkv.contiguous(), out.contiguous(), dout.contiguous(), lse.contiguous(), B, T, d, heads)

    @op_attention_bwd.register_fake
    def _(qkv, out, dout, lse, B, T, d, heads):
        return torch.empty_like(qkv)

    def _attn_setup(ctx, inputs, output):
        qkv, B, T, d, heads = inputs
        ctx.save_for_backward(qkv, output[0], output[1])
        ctx.shape = (B, T, d, heads)

    def _attn_backward(ctx, g_out, g_lse):
        qkv, out, lse = ctx.saved_tensors
        return torch.ops.intel_mi355x.attention_bwd(qkv, out, g_out.contiguous(), lse, *ctx.shape), None, None, None, None

    op_attention.register_autograd(_attn_backward, setup_context=_attn_setup)

    @custom_op(NAMESPACE + '::add_layernorm', mutates_args=(), device_types='cuda')
    def op_add_layernorm(x: torch.Tensor, r: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
        return add_layernorm(x.contiguous(), r.contiguous(), gamma, beta)

    @op_add_layernorm.register_fake
    def _(x, r, gamma, beta):
        return torch.empty_like(x)

    @custom_op(NAMESPACE + '::ndcg', mutates_args=(), device_types='cuda')
    def op_ndcg(ens_score: torch.Tensor, ranking: torch.Tensor, session_len: torch.Tensor, k: int) -> torch.Tensor:
        B, Lm = ens_score.shape
        out = torch.empty(B, dtype=torch.float32, device=ens_score.device)
        L.check(L.lib().intel_ndcg(B, Lm, k, L.ptr(ens_score.contiguous()), L.ptr(ranking.to(torch.int32).contiguous()),
                                   L.ptr(session_len.to(torch.int32).contiguous()), L.ptr(out), L.stream_ptr(ens_score.device)), 'intel_ndcg')
        return out

    @op_ndcg.register_fake
    def _(ens_score, ranking, session_len, k):
        return ens_score.new_empty(ens_score.shape[0])

    # ---- the whole model (models/IntEL/IntEL.py:117-124: IntEL.forward) as ONE dispatcher-visible op + its hand-written backward.
    # `handle` names the module (model_handle(model)): the op reads the hyper-parameters and the workspace from it; the parameter
    # tensors travel as a Tensor[] argument in the order of model.slot_items(), so autograd sees them and receives their gradients.
    # EAGER-ONLY: the op keeps hidden per-module state that its schema does not declare (the workspace with the activation stash, the
    # one-slot _op_stash that intel_backward continues from, _generation) -- exactly the state the reference's autograd graph would hold.
    # A tracing compiler (torch.compile / functionalization) may reorder, deduplicate or re-run a "pure" op and would corrupt that
    # stash: do not trace it.  One training forward per backward, as in the reference's loop (BaseRunner.py:283-289).
    from typing import List, Optional

    @custom_op(NAMESPACE + '::intel_forward', mutates_args=(), device_types='cuda')
    def op_intel_forward(handle: int, train: bool, i_id_s: torch.Tensor, i_class_c: torch.Tensor, scores: torch.Tensor, session_len: torch.Tensor,
                         u_id_c: torch.Tensor, context_mh: torch.Tensor, his_context_mh: torch.Tensor, his_intents: torch.Tensor,
                         history_len: torch.Tensor, his_item_id: torch.Tensor, his_item_idx: Optional[torch.Tensor],
                         his_item_int: Optional[torch.Tensor], history_item_len: torch.Tensor, his_rows: int, hisitem_rows: int,
                         params: List[torch.Tensor]) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        model = _model_of(handle)
        data = {'i_id_s': i_id_s, 'i_class_c': i_class_c, 'scores': scores, 'session_len': session_len, 'u_id_c': u_id_c,
                'context_mh': context_mh, 'his_context_mh': his_context_mh, 'his_intents': his_intents, 'history_len': history_len,
                'his_item_id': his_item_id, 'history_item_len': history_item_len}
        if his_item_idx is not None:
            data['his_item_idx'] = his_item_idx
        else:
            data['his_item_int'] = his_item_int
        if his_rows >= 0 and hisitem_rows >= 0:
            data['his_rows'], data['hisitem_rows'] = his_rows, hisitem_rows
        batch, keep = model.prepare_batch(data)
        out = model.run_forward(batch, keep, [p.detach() for p in params], train=train)
        model._generation = getattr(model, '_generation', 0) + 1
        if train:
            model._op_stash = (model._generation, batch, keep)      # what intel_backward continues from (one forward / backward pair at a time)
        return out

    @op_intel_forward.register_fake
    def _(handle, train, i_id_s, i_class_c, scores, session_len, u_id_c, context_mh, his_context_mh, his_intents, history_len, his_item_id,
          his_item_idx, his_item_int, history_item_len, his_rows, hisitem_rows, params):
        model = _model_of(handle)
        B, Lm = i_id_s.shape
        f = dict(dtype=torch.float32, device=i_id_s.device)
        return torch.empty(B, Lm, model.model_num, **f), torch.empty(B, Lm, **f), torch.empty(B, model.intent_num, **f)

    @custom_op(NAMESPACE + '::intel_backward', mutates_args=(), device_types='cuda')
    def op_intel_backward(handle: int, d_weights: torch.Tensor, d_ens_score: torch.Tensor, d_intents: torch.Tensor,
                          params: List[torch.Tensor]) -> List[torch.Tensor]:
        model = _model_of(handle)
        stash = getattr(model, '_op_stash', None)
        if stash is None or stash[0] != model._generation:
            raise L.IntelHipError('intel_backward: no matching intel_forward(train=True) (the activation stash was overwritten)')
        _, batch, keep = stash
        grads = model.run_backward(batch, keep, [p.detach() for p in params], d_weights.contiguous().float(), d_ens_score.contiguous().float(),
                                   d_intents.contiguous().float())
        items = model.slot_items()
        return [grads[s] if s in grads else torch.zeros_like(p) for (s, _, _), p in zip(items, params)]

    @op_intel_backward.register_fake
    def _(handle, d_weights, d_ens_score, d_intents, params):
        return [torch.empty_like(p) for p in params]

    def _model_setup(ctx, inputs, output):
        ctx.handle = inputs[0]
        ctx.n_inputs = len(inputs)
        ctx.save_for_backward(*inputs[-1])

    def _model_backward(ctx, d_weights, d_ens, d_intents):
        params = list(ctx.saved_tensors)
        model = _model_of(ctx.handle)
        B, Lm = model._op_stash[1].B, model._op_stash[1].L
        dev = params[0].device
        zw = lambda t, shape: torch.zeros(shape, dtype=torch.float32, device=dev) if t is None else t
        grads = torch.ops.intel_mi355x.intel_backward(ctx.handle, zw(d_weights, (B, Lm, model.model_num)), zw(d_ens, (B, Lm)),
                                                      zw(d_intents, (B, model.intent_num)), params)
        return (None,) * (ctx.n_inputs - 1) + (list(grads),)

    op_intel_forward.register_autograd(_model_backward, setup_context=_model_setup)

    return ['linear', 'linear_dgrad', 'linear_wgrad', 'attention', 'attention_bwd', 'add_layernorm', 'ndcg', 'intel_forward', 'intel_backward']


_HANDLES = {}


def model_handle(model):
    """Integer handle of an IntEL module for torch.ops.intel_mi355x.intel_forward / intel_backward (a weak reference is kept)."""
    import weakref
    h = id(model)
    _HANDLES[h] = weakref.ref(model)
    return h


def _model_of(handle):
    ref = _HANDLES.get(int(handle))
    model = ref() if ref is not None else None
    if model is None:
        raise L.IntelHipError('intel_forward: unknown or dead model handle %r (ops.model_handle(model))' % (handle,))
    return model


def model_forward(model, data):
    """IntEL.forward(data) through the dispatcher: torch.ops.intel_mi355x.intel_forward over the module's parameters
    (models/IntEL/IntEL.py:117-124).  Differentiable: the registered autograd formula is intel_backward."""
    if 'intel_forward' not in REGISTERED_OPS:
        raise L.IntelHipError('torch.library.custom_op is not available in this torch: %r' % (globals().get('_REGISTER_ERROR'),))
    params = [p for _, _, p in model.slot_items()]
    need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    i32 = lambda k: data[k]
    w, e, i = torch.ops.intel_mi355x.intel_forward(
        model_handle(model), bool(need_grad), i32('i_id_s'), data.get('i_class_c') if data.get('i_class_c') is not None else torch.zeros_like(data['i_id_s']),
        data['scores'], i32('session_len'), i32('u_id_c'), i32('context_mh'), i32('his_context_mh'), data['his_intents'], i32('history_len'),
        i32('his_item_id'), data.get('his_item_idx'), data.get('his_item_int') if 'his_item_idx' not in data else None, i32('history_item_len'),
        int(data.get('his_rows', -1)), int(data.get('hisitem_rows', -1)), params)
    return {'weights': w, 'ens_score': e, 'intents': i}


try:
    REGISTERED_OPS = _register()
except Exception as _e:        # an older torch without torch.library.custom_op: the ctypes wrappers above still work
    REGISTERED_OPS = []
    _REGISTER_ERROR = _e
