"""Standalone timing of the ERA population-fitness launch (csrc/era.hip: intel_era_fitness) at the reference's GA size.
usage: python tools/era_bench.py [--solutions 100] [--sessions 65536] [--L 50] [--K 3] [--H 16] [--launches 20] [--ref_threads 16]
Prints the median launch time (HIP events on the launch stream, after a warm-up), the achieved FMA rate against the fp32 vector
peak, and the time the float64 numpy restatement of the same fitness takes for the same population on --ref_threads host threads
(--ref_threads 0 skips it).  Needs an MI355X."""
import argparse
import ctypes
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from intel_sigir2023_amd import era, _lib as L

PEAK_FP32_VECTOR_TFLOPS = 157.3      # MI355X datasheet: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def numpy_fitness(pop, feat, ranking, slen, width, H, threads, chunk=1024):
    """float64 restatement: gain_sum [P] over all sessions; one solution per task, sessions in cache-sized chunks."""
    N, Lm, F = feat.shape
    lab = np.maximum(ranking, 0).astype(np.int64)
    valid = np.arange(Lm)[None, :] < slen[:, None]
    maxlab = np.maximum(np.where(valid, lab, 0).max(1), 1).astype(np.float64)
    has_pad = slen < width
    f64 = feat.astype(np.float64)
    big = np.iinfo(np.int64).max

    def one(p):
        w = pop[p].astype(np.float64)
        W1, b1, W2, b2 = w[:H * F].reshape(H, F), w[H * F:H * F + H], w[H * F + H:H * F + 2 * H], w[-1]
        total = 0.0
        for lo in range(0, N, chunk):
            hi = min(N, lo + chunk)
            x = f64[lo:hi].reshape(-1, F)
            pred = (np.maximum(x @ W1.T + b1, 0.0) @ W2 + b2).reshape(hi - lo, Lm)
            pred = np.where(valid[lo:hi], pred, -np.inf)
            best = pred.max(1)
            win = np.where(pred == best[:, None], np.where(valid[lo:hi], lab[lo:hi], big), big).min(1)
            pad_wins = has_pad[lo:hi] & ((0.0 > best) | ((0.0 == best) & (win > 0)))
            win = np.where(pad_wins | (win == big), 0, win)
            total += float((win / maxlab[lo:hi]).sum())
        return total
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return np.array(list(ex.map(one, range(pop.shape[0]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--solutions', type=int, default=100)
    ap.add_argument('--sessions', type=int, default=65536)
    ap.add_argument('--L', type=int, default=50)
    ap.add_argument('--K', type=int, default=3)
    ap.add_argument('--H', type=int, default=16)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--ref_threads', type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/era_bench.py needs an MI355X')
    dev = torch.device('cuda:0')
    P, N, Lm, K, H = a.solutions, a.sessions, a.L, a.K, a.H
    F = K + 2
    g = torch.Generator(device=dev).manual_seed(0)
    scores = torch.rand(N, Lm, K, generator=g, device=dev)
    slen = torch.full((N,), Lm, dtype=torch.int32, device=dev)
    ranking = torch.randint(-1, 4, (N, Lm), generator=g, device=dev, dtype=torch.int32)
    pop = (torch.rand(P, H * F + 2 * H + 1, generator=g, device=dev) * 2 - 1).contiguous()
    feat = era.era_features(scores, slen, 10)
    lib = L.lib()
    nbytes = int(lib.intel_era_fitness_workspace_bytes(P, N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    gain = torch.zeros(P, dtype=torch.float64, device=dev)
    hid = (ctypes.c_int * 1)(H)
    st = L.stream_ptr(dev)
    launch = lambda: L.check(lib.intel_era_fitness(P, N, Lm, F, 1, hid, L.ptr(pop), L.ptr(feat), L.ptr(ranking), L.ptr(slen), Lm, L.ptr(gain),
                                                   None, L.ptr(ws), st), 'intel_era_fitness')
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(20, a.launches)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    ms = ts[len(ts) // 2]
    fmas = float(P) * N * Lm * (H * F + H)
    rate = fmas / (ms * 1e-3)
    print('intel_era_fitness P=%d sessions=%d L=%d K=%d H=%d: median %.3f ms of %d launches (min %.3f, max %.3f)'
          % (P, N, Lm, K, H, ms, len(ts), ts[0], ts[-1]))
    print('  %.3e FMAs per launch -> %.2f TFMA/s = %.2f TFLOP/s = %.1f %% of the %.1f TFLOP/s fp32 vector peak'
          % (fmas, rate / 1e12, 2 * rate / 1e12, 100 * 2 * rate / 1e12 / PEAK_FP32_VECTOR_TFLOPS, PEAK_FP32_VECTOR_TFLOPS))
    print('  per solution: %.1f us' % (1e3 * ms / P))
    if a.ref_threads > 0:
        gain.zero_()
        launch()
        got = gain.cpu().numpy()
        host = (pop.cpu().numpy(), feat.cpu().numpy(), ranking.cpu().numpy(), slen.cpu().numpy())
        t0 = time.perf_counter()
        ref = numpy_fitness(*host, Lm, H, a.ref_threads)
        dt = time.perf_counter() - t0
        print('float64 numpy restatement, %d threads: %.2f s for the same population (%.0fx the launch); max |fitness difference| %.3g'
              % (a.ref_threads, dt, dt / (ms * 1e-3), np.abs(got - ref).max() / N))


if __name__ == '__main__':
    main()
