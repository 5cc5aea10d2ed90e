#!/usr/bin/env python3
"""The weight-gradient launches of the 64 x 128 training step alone on the chip, ss_tune("gemm_pipe") 0 (one-buffer k-loop) against 1 (pipelined
k-loop, csrc/gemm_bf16x3.hip PIPE): interleaved rounds in one process, the launch made as the engine makes it (largest tile, the images the
engine has for that class, split-K through partial slabs with the ksplit engine.hip pick_ksplit gives at DW_WGS).

    python tools/gemm_pipe_bench.py [--wgs 384] [--rounds 5] [--n 20]

us per launch include the split-K reduce.  The decoder's input gradients run as ONE 8192-row matrix here (the step issues them as 64 batch
entries of 128 rows: the same 512 tiles), and with the stacked weights' image only under gemm_pipe 1, as engine.hip lstm_input_grad passes it."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speechsplit_amd import engine as E  # noqa: E402

# name, M, N, K, A reduction-major, which operands come with an image ('b': the hidden-state image of the decoder; 'ab': both, the conv
# trunk; 'b1': B's only with gemm_pipe 1)
SHAPES = [('dec dW_ih TN 2048x1024x8448', 2048, 1024, 8448, True, 'b'),
          ('dec dW_hh TN 2048x512x8447', 2048, 512, 8447, True, 'b'),
          ('conv dW   TN 512x2560x8448', 512, 2560, 8448, True, 'ab'),
          ('dec dX    NN 8192x1024x4096', 8192, 1024, 4096, False, 'b1')]


def pick_ksplit(M, N, K, wgs):
    tiles = -(-M // 128) * -(-N // 128)
    return max(1, min(wgs // tiles, K // 256, 32))


def timeit(fn, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--wgs', type=int, default=384)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--n', type=int, default=20)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(1)
    for name, M, N, K, ta, imgs in SHAPES:
        A = torch.randn((K, M) if ta else (M, K), generator=g).cuda()
        Bm = (torch.randn(K, N, generator=g) * 0.05).cuda()
        ai = E.split_image(A) if 'a' in imgs else None
        bi = E.split_image(Bm)
        ks = pick_ksplit(M, N, K, a.wgs) if ta else 1
        part = torch.empty(ks * M * N, device='cuda')
        out = torch.zeros(M, N, device='cuda')
        ref = (A.double().t() if ta else A.double()) @ Bm.double()

        def run(v):
            out.zero_()
            return E.gemm(A, Bm, None, ta, True, ks, out=out, f16x2=True, as_engine=True, a_img=ai, b_img=bi if v or imgs != 'b1' else None, part=part)

        res, outs = {0: [], 1: []}, {}
        for r in range(a.rounds + 1):
            for v in ((0, 1) if r % 2 == 0 else (1, 0)):
                E.tune('gemm_pipe', v)
                run(v)
                outs[v] = out.clone()
                t = timeit(lambda: run(v), a.n)
                if r:
                    res[v].append(t)
        E.tune('gemm_pipe', 1)
        err = float((outs[1].double() - ref).abs().max() / ref.abs().max())
        m0, m1 = statistics.median(res[0]), statistics.median(res[1])
        print(f'{name} ks{ks} images {imgs:2s}: gemm_pipe 0 {m0:7.1f} us (min {min(res[0]):.1f} max {max(res[0]):.1f})   1 {m1:7.1f} us (min {min(res[1]):.1f} '
              f'max {max(res[1]):.1f})   ratio {m1 / m0:.3f}   bit-identical {torch.equal(outs[0], outs[1])}   err vs float64 {err:.1e}', flush=True)


if __name__ == '__main__':
    main()
