"""GPU parity of the GRU4Rec recurrence (csrc/gru.hip) through `intel_op_gru_fwd` / `intel_op_gru_bwd`, against a float64 GRU
step loop on the CPU (`gru_ref` below; tests/test_gru_ref_cpu.py checks that loop against float64 torch.nn.GRU).

All three forms of the recurrence are visited in one process through the entries' `form` argument: 0 the per-step form, 1 the
one-kernel recurrence with exact fp32 MFMAs, 2 the default one with three-plane bf16 products.  Gradients are torch autograd of
(vec * dout).sum() through the float64 loop.  Tolerances are those of tests/test_ops_gpu.py, per tensor and relative to
max(1, |ref|max): 2e-5 forward, 5e-5 gradients.  (An fp32 torch evaluation of the same loop differs from float64 by at most 8e-7
of that scale at B in {17, 33, 257}, T in {20, 21, 50} and both weight scales, so the hardware exp / rcp of the kernels, 2e-7
absolute per gate, has more than 20x headroom.)

The shapes are the smallest at which each branch of the kernels exists: the 16-session workgroup tile (B = 15 / 16 / 17 / 33: dead
slots, several tiles), a tile whose longest history is shorter than T (tail fill of the h_{t-1} stash, zero gate gradients) or 0
(the time loop does not run), odd and even loop counts of the double-buffered LDS rows, T = 1, packed rows with a trailing empty
session, the `order` permutation, the inference kernel without stash, pitched output columns.  Before every forward the whole
workspace is filled with NaN bit patterns: a stash row that a kernel forgets to write turns a weight gradient non-finite instead
of reading whatever an earlier case left there.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 2e-5, 5e-5
SENT = -12345.0
HID = 128
DMS = (64, 16, 24)          # 24: a ragged K of the input GEMM
GRADS = ('dE0', 'dWih', 'dWhh', 'dbih', 'dbhh', 'dWout')


# ======================================================================================================================
# reference
# ======================================================================================================================
def gru_ref(E, lens, Wih, Whh, bih, bhh, Wout):
    """torch.nn.GRU's step (gates r, z, n; h' = (1 - z) n + z h; h_0 = 0) over E [B, T, dm]; session b keeps its state from step
    lens[b] on (lens[b] == 0: h stays 0).  Returns vec = h_last Wout^T [B, dm].  Works in the dtype of its arguments."""
    B, T, _ = E.shape
    H = Whh.shape[1]
    h = E.new_zeros(B, H)
    for t in range(T):
        gi = E[:, t] @ Wih.t() + bih
        gh = h @ Whh.t() + bhh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = torch.where((lens > t).unsqueeze(1), (1.0 - z) * n + z * h, h)
    return h @ Wout.t()


def gru_ref_grads(E, lens, Wih, Whh, bih, bhh, Wout, dout):
    """float64 vec and the gradients of (vec * dout).sum(): dict with 'out' and the names of GRADS (dE0 padded [B, T, dm])."""
    leaves = [t.detach().double().requires_grad_(True) for t in (E, Wih, Whh, bih, bhh, Wout)]
    vec = gru_ref(leaves[0], lens, *leaves[1:])
    (vec * dout.double()).sum().backward()
    res = {'out': vec.detach()}
    for name, t in zip(('dE0', 'dWih', 'dWhh', 'dbih', 'dbhh', 'dWout'), leaves):
        res[name] = t.grad if t.grad is not None else torch.zeros_like(t)
    return res


# ======================================================================================================================
# inputs
# ======================================================================================================================
def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k) + 1
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _ragged(B, lo, hi, g):
    return torch.randint(lo, hi + 1, (B,), generator=g)


def _lens(kind, B, T):
    """The length vectors of the cases, by name (seeded: the same vector for every form and width)."""
    g = _gen(B, T, sum(map(ord, kind)))
    if kind == 'full':
        v = torch.full((B,), T)
    elif kind == 'zero':
        v = torch.zeros(B, dtype=torch.int64)
    elif kind == 'mixed':                      # uniform in 0..T, forced to contain 0, 1 and T
        v = _ragged(B, 0, T, g)
        p = torch.randperm(B, generator=g)
        v[p[0]], v[p[1]], v[p[2]] = 0, 1, T
    elif kind == 'ragged':                     # uniform in 0..T with at least one full history
        v = _ragged(B, 0, T, g)
        v[int(torch.randint(0, B, (1,), generator=g))] = T
    elif kind == 'early':                      # tile 0 ragged up to T, tile 1 stops at 7, the lone session of tile 2 runs to T
        assert B == 33 and T > 7
        v = _ragged(B, 0, T, g)
        v[5] = T
        v[16:32] = _ragged(16, 0, 7, g)
        v[20] = 7
        v[32] = T
    elif kind == 'never':                      # tile 0 never runs
        v = _ragged(B, 0, T, g)
        v[:16] = 0
        v[B - 1] = T
    elif kind == 'pos':                        # packed: every session has rows
        v = _ragged(B, 1, T, g)
        v[1] = T
    elif kind == 'holes':                      # packed: isolated empty sessions, the LAST one included (off[B-1] == rows)
        v = _ragged(B, 1, T, g)
        v[2] = T
        v[0] = v[5] = v[16] = v[B - 1] = 0
    else:
        raise KeyError(kind)
    return v.to(torch.int64)


@functools.lru_cache(maxsize=None)
def _case(B, T, dm, kind):
    """Inputs and the float64 reference of one (shape, lengths) case: computed once, shared by every test and form, never modified."""
    g = _gen(B, T, dm, 7)
    lens = _lens(kind, B, T)
    c = {'B': B, 'T': T, 'dm': dm, 'lens': lens, 'ldo': dm + 16, 'col0': 8}
    c['E'] = torch.randn(B, T, dm, generator=g)
    c['Wih'] = torch.randn(3 * HID, dm, generator=g) * (2.0 / dm ** 0.5)
    c['Whh'] = torch.randn(3 * HID, HID, generator=g) * (2.0 / HID ** 0.5)
    c['bih'] = 0.1 * torch.randn(3 * HID, generator=g)
    c['bhh'] = 0.1 * torch.randn(3 * HID, generator=g)
    c['Wout'] = torch.randn(dm, HID, generator=g) / HID ** 0.5
    c['dout'] = torch.randn(B, c['ldo'], generator=g)
    c['ref'] = gru_ref_grads(c['E'], lens, c['Wih'], c['Whh'], c['bih'], c['bhh'], c['Wout'], c['dout'][:, c['col0']:c['col0'] + dm])
    c['valid'] = (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1))        # [B, T]
    return c


def _order(kind, lens):
    if kind is None:
        return None
    if kind == 'asc':
        return torch.argsort(lens, stable=True)
    if kind == 'desc':
        return torch.argsort(lens, descending=True, stable=True)
    return torch.randperm(lens.numel(), generator=_gen(lens.numel(), 31))


# ======================================================================================================================
# running and comparing
# ======================================================================================================================
def _dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _i32(t, dev):
    return None if t is None else t.to(torch.int32).contiguous().to(dev)


def _run(c, form, packed=False, order=None, stash=True, backward=True, queued=False, ldo=None, col0=None):
    """One forward (and backward) on a NaN-filled workspace.  Returns (out [B, ldo] with sentinel columns, grads or None), on the CPU."""
    from intel_sigir2023_amd import ops
    dev = _dev()
    B, T, dm, lens = c['B'], c['T'], c['dm'], c['lens']
    ldo = c['ldo'] if ldo is None else ldo
    col0 = c['col0'] if col0 is None else col0
    E0 = (c['E'][c['valid']] if packed else c['E'].reshape(B * T, dm)).contiguous().to(dev)
    off = _i32(torch.cumsum(lens, 0) - lens, dev) if packed else None
    if packed:
        assert E0.shape[0] == int(lens.sum()) > 0
    W = {k: c[k].to(dev) for k in ('Wih', 'Whh', 'bih', 'bhh', 'Wout')}
    ln, od = _i32(lens, dev), _i32(order, dev)
    ws = ops.gru_workspace(B, T, dm, dev)
    ws.fill_(0xFF)                                                   # every float of the workspace is a NaN
    out = torch.full((B, ldo), SENT, dtype=torch.float32, device=dev)
    ops.gru_fwd(E0, B, T, ln, W['Wih'], W['Whh'], W['bih'], W['bhh'], W['Wout'], out, col0, ws, form=form, stash=stash, off=off, order=od)
    grads = None
    if backward:
        dout = torch.randn(B, ldo, generator=_gen(B, ldo, 3)).to(dev)      # columns outside [col0, col0 + dm): never read
        dout[:, col0:col0 + dm] = c['dout'][:, c['col0']:c['col0'] + dm].to(dev)
        grads = {k: v.cpu() for k, v in ops.gru_bwd(E0, B, T, ln, W['Whh'], W['bhh'], dout, col0, ws, form=form, queued=queued, off=off, order=od).items()}
    torch.cuda.synchronize()
    return out.cpu(), grads


def _close(got, ref, tol, name):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, '%s: shape %s vs %s' % (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), '%s: %d non-finite values' % (name, int((~torch.isfinite(got)).sum()))
    if ref.numel() == 0:
        return
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print('gru_op_err %-22s err/scale %.3e' % (name, err / scale))
    assert err <= tol * scale, '%s: max err %.3e (scale %.3e, bound %.1e)' % (name, err, scale, tol)


def _check_out(c, out, tag, ldo=None, col0=None):
    dm = c['dm']
    col0 = c['col0'] if col0 is None else col0
    keep = torch.ones(out.shape[1], dtype=torch.bool)
    keep[col0:col0 + dm] = False
    assert bool((out[:, keep] == SENT).all()), '%s: columns outside [col0, col0 + dm) were written' % tag
    _close(out[:, col0:col0 + dm], c['ref']['out'], FWD_TOL, tag + ' out')


def _check_grads(c, grads, tag, packed=False):
    B, T, dm = c['B'], c['T'], c['dm']
    ref = c['ref']
    for k in GRADS:
        assert bool(torch.isfinite(grads[k]).all()), '%s %s: %d non-finite values' % (tag, k, int((~torch.isfinite(grads[k])).sum()))
    if packed:
        _close(grads['dE0'], ref['dE0'][c['valid']], GRAD_TOL, tag + ' dE0')
    else:
        dE = grads['dE0'].reshape(B, T, dm)
        assert bool((dE[~c['valid']] == 0).all()), '%s dE0: rows at t >= len are not zero' % tag
        _close(dE, ref['dE0'], GRAD_TOL, tag + ' dE0')
    for k in GRADS[1:]:
        _close(grads[k], ref[k], GRAD_TOL, tag + ' ' + k)


def _fwd_bwd(c, form, **kw):
    tag = 'form%d' % form
    out, grads = _run(c, form, **kw)
    _check_out(c, out, tag, kw.get('ldo'), kw.get('col0'))
    _check_grads(c, grads, tag, packed=kw.get('packed', False))
    return out, grads


# ======================================================================================================================
# padded rows, all three forms
# ======================================================================================================================
PADDED = [(1, 1, 'full'), (1, 1, 'zero'),                                                    # one session, one step
          (15, 3, 'full'), (16, 3, 'full'), (17, 3, 'full'), (33, 3, 'full'),                # tile edges
          (17, 1, 'mixed'), (17, 2, 'mixed'), (17, 20, 'mixed'), (17, 21, 'mixed'),          # odd / even loop counts
          (33, 20, 'early'),                                                                 # a tile that stops early
          (33, 5, 'never'),                                                                  # a tile that never runs
          (16, 50, 'ragged')]                                                                # long loop


@pytest.mark.parametrize('form', [0, 1, 2])
@pytest.mark.parametrize('dm', DMS)
@pytest.mark.parametrize('B,T,kind', PADDED)
def test_padded_fwd_bwd(B, T, kind, dm, form):
    _fwd_bwd(_case(B, T, dm, kind), form)


@pytest.mark.parametrize('form', [0, 1, 2])
@pytest.mark.parametrize('dm', DMS)
def test_unaligned_output_columns(dm, form):
    """ldo and col0 that are no multiple of 4 floats (the output GEMMs and the dWout product leave their 16-byte paths)."""
    _fwd_bwd(_case(15, 3, dm, 'full'), form, ldo=dm + 7, col0=5)


@pytest.mark.parametrize('form', [0, 1, 2])
@pytest.mark.parametrize('dm', DMS)
def test_nothing_runs_gives_exact_zeros(dm, form):
    """Every history is empty: h stays 0, so vec and every gradient are exactly zero (and finite: the h_0 stash rows are written)."""
    c = _case(17, 4, dm, 'zero')
    out, grads = _fwd_bwd(c, form)
    assert bool((out[:, c['col0']:c['col0'] + dm] == 0).all())
    for k in GRADS:
        assert bool((grads[k] == 0).all()), '%s is not exactly zero' % k


# ======================================================================================================================
# the slot -> session permutation (one-kernel forms)
# ======================================================================================================================
@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('order', [None, 'asc', 'desc', 'perm'])
@pytest.mark.parametrize('dm', DMS)
@pytest.mark.parametrize('B', [33, 48])
def test_order_permutation(B, dm, order, form):
    c = _case(B, 20, dm, 'ragged')
    _fwd_bwd(c, form, order=_order(order, c['lens']))


# ======================================================================================================================
# packed rows (one-kernel forms)
# ======================================================================================================================
@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('order', [None, 'asc'])
@pytest.mark.parametrize('kind', ['pos', 'holes'])
@pytest.mark.parametrize('dm', DMS)
@pytest.mark.parametrize('B', [17, 33])
def test_packed_rows(B, dm, kind, order, form):
    c = _case(B, 20, dm, kind)
    if kind == 'holes':
        assert int(c['lens'][-1]) == 0           # off[B-1] == rows
    _fwd_bwd(c, form, packed=True, order=_order(order, c['lens']))


def test_packed_rows_per_step_form_is_rejected():
    """The per-step form has no packed rows: INTEL_E_ARG, and nothing is launched (output and workspace untouched)."""
    from intel_sigir2023_amd import _lib, ops
    dev = _dev()
    c = _case(17, 5, 64, 'pos')
    B, T, dm, lens = 17, 5, 64, c['lens']
    E0 = c['E'][c['valid']].contiguous().to(dev)
    off = _i32(torch.cumsum(lens, 0) - lens, dev)
    W = {k: c[k].to(dev) for k in ('Wih', 'Whh', 'bih', 'bhh', 'Wout')}
    ws = ops.gru_workspace(B, T, dm, dev)
    ws.fill_(0xFF)
    out = torch.full((B, c['ldo']), SENT, dtype=torch.float32, device=dev)
    with pytest.raises(_lib.IntelHipError, match=r'code -1\)'):
        ops.gru_fwd(E0, B, T, _i32(lens, dev), W['Wih'], W['Whh'], W['bih'], W['bhh'], W['Wout'], out, c['col0'], ws, form=0, off=off)
    with pytest.raises(_lib.IntelHipError, match=r'code -1\)'):
        ops.gru_bwd(E0, B, T, _i32(lens, dev), W['Whh'], W['bhh'], c['dout'].to(dev), c['col0'], ws, form=0, off=off)
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENT).all())
    assert bool((ws.cpu() == 0xFF).all())


# ======================================================================================================================
# inference: no stash (one-kernel forms)
# ======================================================================================================================
@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('dm', DMS)
@pytest.mark.parametrize('B', [17, 33])
def test_inference_without_stash(B, dm, packed, form):
    c = _case(B, 20, dm, 'ragged')
    out, _ = _run(c, form, packed=packed, stash=False, backward=False)
    _check_out(c, out, 'form%d' % form)


# ======================================================================================================================
# both reductions of the weight gradients
# ======================================================================================================================
@pytest.mark.parametrize('form', [0, 1, 2])
@pytest.mark.parametrize('dm', DMS)
def test_queued_and_immediate_reduction(dm, form):
    c = _case(33, 20, dm, 'ragged')
    _, g0 = _fwd_bwd(c, form, queued=False)
    _, g1 = _fwd_bwd(c, form, queued=True)
    for k in GRADS:
        scale = max(1.0, float(c['ref'][k].abs().max()))
        err = float((g1[k].double() - g0[k].double()).abs().max())
        assert err <= 1e-6 * scale, '%s: queued vs immediate %.3e (scale %.3e)' % (k, err, scale)
