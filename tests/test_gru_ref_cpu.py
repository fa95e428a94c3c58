"""The float64 GRU step loop that tests/test_gru_op_gpu.py compares the HIP recurrence with, checked against float64
torch.nn.GRU over pack_padded_sequence (the reference model's own path, models/GeneralSeq.py:64-78): the loop must not be a
second copy of the project's reading of the formula.  Lengths >= 1 only: pack_padded_sequence takes no empty sequence, which is
why the loop exists."""
import torch

from tests.test_gru_op_gpu import HID, gru_ref


def test_step_loop_matches_torch_gru_on_a_ragged_batch():
    g = torch.Generator().manual_seed(2023)
    B, T, dm = 9, 7, 24
    lens = torch.tensor([7, 1, 3, 7, 2, 5, 1, 6, 4])
    E = torch.randn(B, T, dm, generator=g, dtype=torch.float64)
    dout = torch.randn(B, dm, generator=g, dtype=torch.float64)
    gru = torch.nn.GRU(dm, HID, batch_first=True).double()
    with torch.no_grad():
        for p, fan in ((gru.weight_ih_l0, dm), (gru.weight_hh_l0, HID)):
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (2.0 / fan ** 0.5))
        for p in (gru.bias_ih_l0, gru.bias_hh_l0):
            p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    Wout = (torch.randn(dm, HID, generator=g, dtype=torch.float64) / HID ** 0.5).requires_grad_(True)

    # torch.nn.GRU on the packed batch: the state after each session's own last step
    Ea = E.clone().requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(Ea, lens, batch_first=True, enforce_sorted=False)
    _, hn = gru(packed)
    vec_a = hn[0] @ Wout.t()
    (vec_a * dout).sum().backward()
    want = [vec_a.detach(), Ea.grad.clone(), Wout.grad.clone()] + [p.grad.clone() for p in gru.parameters()]
    Wout.grad = None
    gru.zero_grad()

    # the step loop on the padded batch
    Eb = E.clone().requires_grad_(True)
    vec_b = gru_ref(Eb, lens, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, Wout)
    (vec_b * dout).sum().backward()
    got = [vec_b.detach(), Eb.grad, Wout.grad] + [p.grad for p in gru.parameters()]

    names = ['vec', 'dE', 'dWout', 'dWih', 'dWhh', 'dbih', 'dbhh']
    for name, a, b in zip(names, got, want):
        scale = max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        assert err <= 1e-12 * scale, '%s: %.3e (scale %.3e)' % (name, err, scale)
    pad = torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)
    assert bool((Eb.grad[pad] == 0).all())
