"""K12 (fused full-catalogue cross entropy) against the library path, the loss alone, per
hidden size: HIP-event time of ops.full_ce_fwd + ops.full_ce_bwd and of torch's matmul +
cross_entropy + autograd.grad on the same inputs (median of 10 after a warm-up call,
host-inclusive), the share of the fp32 MFMA peak over K12's 5 GEMM passes of 2*B*I*d, and
the largest gradient difference between the two paths. One JSON line per width.

usage: python tools/probe_full_ce.py [--items 90001] [--batch 2048] [--widths 32,64,128,256]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3


def _event_time(fn, reps=10):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=90_001)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--widths', default='32,64,128,256')
    args = ap.parse_args()
    from recbole_amd import ops
    dev = torch.device('cuda', 0)
    B, I = args.batch, args.items
    g = torch.Generator().manual_seed(2020)
    for d in (int(x) for x in args.widths.split(',')):
        S = (torch.randn(B, d, generator=g) * 0.05).to(dev)
        E = (torch.randn(I, d, generator=g) * 0.05).to(dev)
        t = torch.randint(0, I, (B,), generator=g).to(dev)
        one = torch.ones(1, device=dev)
        lse, _ = ops.full_ce_fwd(S, E, t)
        gS, dE = ops.full_ce_bwd(S, E, t, lse, one)
        Sg, Eg = S.clone().requires_grad_(), E.clone().requires_grad_()

        def lib():
            return torch.autograd.grad(
                torch.nn.functional.cross_entropy(Sg @ Eg.T, t), (Sg, Eg))
        rS, rE = lib()
        tf = _event_time(lambda: ops.full_ce_fwd(S, E, t))
        tb = _event_time(lambda: ops.full_ce_bwd(S, E, t, lse, one))
        tl = _event_time(lib)
        gemm = 2 * B * I * d
        print(json.dumps({
            'd': d, 'B': B, 'I': I, 'splits': ops.full_ce_splits(B, I, d, 0),
            'k12_fwd_us': round(tf * 1e6, 1), 'k12_bwd_us': round(tb * 1e6, 1),
            'library_fwd_bwd_us': round(tl * 1e6, 1),
            'library_over_k12': round(tl / (tf + tb), 3),
            'k12_frac_of_peak': round(5 * gemm / (tf + tb) / 1e12 / PEAK_TFLOPS, 3),
            'max_abs_diff_gS': float((gS - rS).abs().max()),
            'max_abs_diff_dE': float((dE - rE).abs().max())}), flush=True)


if __name__ == '__main__':
    main()
