#!/usr/bin/env python3
"""Runs each GEMM shape of the training step a few times with the kernel the step uses for it (for rocprofv3 --pmc collection)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# (name, bench.py kernel class, kernel, M, N, K, ta, tb, ksplit).  kernel: 'img' = gemm_img.hip over operand images; 'pipe' / 'pipe0' =
# gemm_bf16x3.hip with the in-loop split, launched as the engine launches the class (largest tile, B's image, split-K through partial slabs at
# the engine's ksplit) with ss_tune("gemm_pipe") 1 / 0 -- 0 is the one-buffer loop, which gets no weight image for dX (engine.hip lstm_input_grad)
SHAPES = [('proj NT 8192x4096x1024 (image GEMM, 256x256)', 'dec_proj', 'img', 8192, 4096, 1024, False, False, 1),
          ('conv NT 8192x512x2560 (image GEMM, 128x128)', 'conv_fwd', 'img', 8192, 512, 2560, False, False, 1),
          ('dX NN 8192x1024x4096', 'dec_dx', 'pipe', 8192, 1024, 4096, False, True, 1),
          ('dW_ih TN 2048x1024x8448 ks3', 'dec_dw', 'pipe', 2048, 1024, 8448, True, True, 3),
          ('dW_hh TN 2048x512x8447 ks6', 'dec_dw', 'pipe', 2048, 512, 8447, True, True, 6),
          ('dX NN 8192x1024x4096 (one-buffer loop; not the step\'s default)', 'dec_dx_loop0', 'pipe0', 8192, 1024, 4096, False, True, 1),
          ('dW_ih TN 2048x1024x8448 ks3 (one-buffer loop; not the step\'s default)', 'dec_dw_loop0', 'pipe0', 2048, 1024, 8448, True, True, 3),
          ('dW_hh TN 2048x512x8447 ks6 (one-buffer loop; not the step\'s default)', 'dec_dw_loop0', 'pipe0', 2048, 512, 8447, True, True, 6),
          ('dW_ih TN 2048x1024x8448 ks4 (image GEMM, 256x128; not the step\'s default)', 'dec_dw_img', 'img', 2048, 1024, 8448, True, True, 4)]
LAUNCHES = 4

if __name__ == '__main__':
    import torch
    from speechsplit_amd import engine as E, _capi
    lib = _capi.lib()
    want = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    _capi.check(lib.ss_tune(b'gemm_want', want))
    if len(sys.argv) > 2:      # timing ablations: run with SS_DIAG_LIB=1 (make -C speechsplit_amd/csrc diag)
        _capi.check(lib.ss_tune(b'gemm_diag', int(sys.argv[2])))
    for name, _, kern, M, N, K, ta, tb, ks in SHAPES:
        A = torch.randn((K, M) if ta else (M, K), device='cuda')
        B = torch.randn((K, N) if tb else (N, K), device='cuda')
        c = torch.zeros(M, N, device='cuda')
        if kern == 'img':
            ai, bi = E.split_image(A), E.split_image(B)
        else:
            E.tune('gemm_pipe', 1 if kern == 'pipe' else 0)
            bi = E.split_image(B) if ta or kern == 'pipe' else None
        part = torch.empty(ks * M * N, device='cuda') if ks > 1 else None
        for _ in range(LAUNCHES):
            if kern == 'img':
                E.gemm_img(ai, bi, ta, tb, None, ks, -1 if ks == 1 else 2, out=c, part=part)
            else:
                E.gemm(A, B, None, ta, tb, ks, out=c, f16x2=True, as_engine=True, b_img=bi, part=part)      # fp16 x 2, fixed scale here
        torch.cuda.synchronize()
    print('ok')
