#!/usr/bin/env python3
"""Headline benchmark: Generator_3 training step (reference solver.py:157-172) throughput in utterances/s.

  python bench.py --gpus N --steps K --warmup W

N=1: one process.  N>1: launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`,
one rank per GPU; each rank processes its own 64-utterance shard (weak scaling), gradients are summed with RCCL
all-reduces over the flat gradient arena (decoder bucket beside the encoder backward, then the encoder bucket), then every
rank applies the same Adam update with the 1/N mean folded in.  The collectives are launched by the engine itself on its own
streams (ss_g3_dp_train_step; torch.distributed only hands the 128-byte communicator id round and reduces the timing).

Workload (BASELINE.json metric / SURVEY.md section 8(d)): batch 64 per GPU, 128 frames, 80-bin mel + F0, max_len_pad=128,
synthetic batch resident in HBM before the timed region, weights from a fixed seed.  A step = resample -> quantise ->
forward -> MSE -> backward -> [all-reduce] -> Adam, nothing skipped; every timed step draws FRESH resampling randomness on
the host with the reference's generator calls (model.py:392-393, 399-402) and uploads it from pinned memory, non-blocking.

Rank 0 prints ONE JSON line (contract in the task statement).  A plain run sets up, warms up, times the --steps steps (no profiling
brackets in them) and prints it; --dump-outputs DIR also writes what the last timed step computes from the state the run started
from (dump_outputs; the same every run).  Every other
measurement and check is taken with --full only (and each of them can still be switched off there by its own --no-* option); without
it their fields below are null.  Besides the contract's fields:
  config.products   the product format of the contractions (the default mode is fp32 storage / accumulation with every
                    product formed from an fp16 x 2 split on the 16-bit matrix pipe: 22 significand bits, see the header)
  roofline          the kernel class with the most GPU time in the timed region (hipEvent brackets on the launch streams,
                    ss_profile), algorithmic FLOPs / its summed duration, against the pipe it runs on
  kernel_classes    time / launches / rate of every kernel class per step, from an all-class survey pass before the timed region
  recurrence        the six persistent decoder-recurrence launches: us per time step forward / backward, share of the step
  alt_precisions    the same step with the GEMMs on the exact bf16 x 3 split (recurrences still fp16 x 2), and with EVERY product on the fp32 MFMA
  solver_loop       Solver.train() iterations/s through the device-side batch producer (loader-to-loss, N=1 only)
  cpu_baseline      the oracle on the host cores: batch 64 on the box's CPU share, plus the 1-thread figure
  dp_collectives    (data parallel, native RCCL) where each bucket's collective sat relative to the end of the backward
  dp_replicas       (data parallel) whether every rank holds bit-identical weights after the run
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic work, SURVEY.md section 8(d): 19 405 064 MAC / frame / utterance, fwd+bwd = 3 x 2 x MAC
MAC_PER_FRAME_G3 = 19405064
MAC_PER_FRAME_G6 = 3474184
PEAK_16BIT_MFMA_TFLOPS = 2500.0    # dense bf16 / fp16 MFMA peak (MI355X_MICROARCH.md)
PEAK_F32_MFMA_TFLOPS = 157.3       # MI355X_MICROARCH.md: v_mfma_f32_* dense peak
PRODUCTS = {'f32': 'fp32 operands/accumulate/storage; products on the 16-bit matrix pipe from an fp16 x 2 split (3 MFMAs, '
                   '22 significand bits rel. to the operand maximum); head + encoder BLSTMs bf16 x 3 (6 MFMAs, exact to 2^-24)',
            'bf16': '16-bit data path: weights, hidden states, resampled activations and gradient slabs also stored as bf16 tensors by their producers and '
                    'contracted from there (1 MFMA per product, fp32 accumulation); persistent recurrences multiply the high fp16 pieces of h and W_hh '
                    '(1 MFMA); cell state, GroupNorm statistics, master weights and Adam fp32; small / unaligned contractions round fp32 operands inside the GEMM'}


def synth(B, T, seed, device):
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, T, 80, generator=g)
    f0 = torch.rand(B, T, 1, generator=g)
    uv = torch.rand(B, T, 1, generator=g) < 0.4
    lens = torch.randint(64, T + 1, (B,), generator=g)
    pad = torch.arange(T)[None, :, None] >= lens[:, None, None]
    f0 = torch.where(uv | pad, torch.full_like(f0, -1e10), f0)
    mel = torch.where(pad, torch.zeros_like(mel), mel)
    emb = torch.nn.functional.one_hot(torch.randint(0, 82, (B,), generator=g), 82).float()
    return [t.to(device) for t in (mel, f0, emb, lens.to(torch.int32))]


def cpu_baseline(T, budget=12.0):
    """The oracle (PyTorch-CPU restatement of the reference step, same ATen / oneDNN kernels as the reference) timed on the
    host: the SAME shape as the GPU line (batch 64) on the CPU share of one GPU slot, and one thread at batch 16."""
    from oracle import ref_model, weights as W
    from oracle.gen_fixtures import synth_batch, draws_for
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cores = int(os.environ.get('SS_CPU_THREADS', min(avail, 16)))   # a one-GPU box owns 16 host cores of the 256 the kernel lists
    hp = W.default_hparams(max_len_pad=T)

    def run(B, threads, budget, min_steps):
        torch.set_num_threads(threads)
        st = ref_model.TrainState(W.make_weights('G3', hp, 0))
        mel, f0, emb, lens = synth_batch(1, B, T, 64)
        draws = draws_for(2, B, 4)
        st.step_g3(hp, mel, f0, emb, lens.numpy(), draws)          # warm-up
        n, t0 = 0, time.time()
        while n < min_steps or (time.time() - t0 < budget and n < 20):
            st.step_g3(hp, mel, f0, emb, lens.numpy(), draws)
            n += 1
            print(f'[bench] cpu_baseline B={B} threads={threads} step {n}: {(time.time() - t0) / n:.2f} s/step', file=sys.stderr, flush=True)
        return B / ((time.time() - t0) / n), n

    v64, n64 = run(64, cores, budget, 3)
    v1, n1 = run(16, 1, 6.0, 1)
    torch.set_num_threads(cores)
    return dict(value=round(v64, 2), unit='utterances/s', cores=cores, kind='port',
                sample=f'{n64} full training steps of Generator_3 at batch 64 x {T} frames on {cores} threads (of {avail} visible; '
                       f'PyTorch-CPU oracle, fp32)',
                one_thread=dict(value=round(v1, 2), cores=1, sample=f'{n1} step(s) at batch 16 x {T} frames'))


def class_table(rec, steps, mfmas):
    return {k: dict(launches_per_step=round(n / steps, 2), us_per_step=round(us / steps, 1),
                    tflops=round(fl / us / 1e6, 2) if us else None, mfma_per_product=mfmas[k]) for k, (n, us, fl) in rec.items()}


def mfma_per_product(rec, precision):
    """the pipe each class runs on, as MFMA instructions per algorithmic fp32 product"""
    if precision == 'bf16':
        return {k: 1 for k in rec}
    m = {k: 3 for k in rec}                              # fp16 x 2
    for k in ('head', 'enc_lstm'):
        m[k] = 6                                         # bf16 x 3
    return m


def dominant_class(rec):
    gemm = {k: v for k, v in rec.items() if not k.startswith('rec_')}
    return max(gemm, key=lambda k: gemm[k][1])


def kernel_report(eng, steps, ms_step, precision, top, survey, T):
    """roofline / recurrence from the hipEvent brackets recorded DURING the timed region (dominant class + recurrences);
    kernel_classes from the all-class survey pass that ran before it (same process, same inputs)."""
    rec = eng.profile_read()
    if not rec or top not in rec:
        return None, None, None
    mfmas = mfma_per_product({**survey[0], **rec}, precision)
    classes = class_table(survey[0], survey[1], mfmas)
    n, us, fl = rec[top]
    ach = fl / us / 1e6
    peak = PEAK_16BIT_MFMA_TFLOPS / mfmas[top]
    names = {'dec_dw': 'gemm_bf16x3_kernel<128,128,TN> split-K: decoder weight gradients dW_ih / dW_hh (12 launches per step, beside the encoder backward)',
             'dec_proj': 'gemm_img_kernel<128,64,2,4,NT> (256 x 256 tiles, LDS-DMA ring): decoder input projection, layers 1-2',
             'dec_dx': 'gemm_bf16x3_kernel<128,128,NN>: decoder input gradients',
             'conv_fwd': 'gemm_img_kernel<64,64,.,.,NT> segmented-K: conv trunk forward (layer 0: gemm_bf16x3_kernel)',
             'conv_dw': 'gemm_bf16x3_kernel<.,.,TN> split-K: conv weight gradients',
             'conv_dx': 'gemm_img_kernel<64,64,.,.,NT> segmented-K: conv input gradients'}
    traffic, traffic_source, alone = None, None, None
    # HBM bytes per launch: NOT measured in this run (a PMC pass needs rocprofv3 as the parent) -- from the separate rocprofv3 --pmc passes kept
    # under profiles/ (tools/pmc_summary.py), and ONLY while the kernel sources are the ones those counters were read from: the record
    # carries a hash of them, and a stale profile gives null instead of a number that no longer describes the kernel
    try:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        from kernel_sha import kernel_sources_sha
        sha_now = kernel_sources_sha()
    except Exception:
        sha_now = None
    for rnd in ('r04', 'r03', 'r02'):
        try:
            path = os.path.join('profiles', rnd, 'gemm_pmc.json')
            recs = [r for r in json.load(open(os.path.join(ROOT, path))) if r.get('class') == top]
            if recs:      # mean over the shapes of the class (dec_dw: dW_ih and dW_hh, six launches each per step)
                if sha_now is None or recs[0].get('kernel_sources_sha') != sha_now:
                    traffic_source = f'{path} is stale (GEMM kernel sources changed since its counters were read): traffic not reported'
                    break
                traffic = sum(r['hbm_read_bytes'] + r['hbm_write_bytes'] for r in recs) / len(recs)
                # the same launches ALONE on the chip (the profile's durations): `achieved` above is what a launch gets inside the step, where
                # the class runs on two or three streams beside the encoder backward -- co-scheduling shortens the step and lengthens each launch
                alone = [{'shape': r['shape'], 'us': round(r['us'], 1), 'tflops': round(r['tflops'], 1), 'frac': round(r['tflops'] / peak, 4)} for r in recs if not r['shape'].endswith('default)')]
                traffic_source = f'{path} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of tools/gemm_pmc.py with the gfx950 correction; a profile figure of these kernel sources, not measured in this run)'
                break
        except Exception:
            pass
    roof = {'bound': 'mfma', 'kernel': names.get(top, top), 'class': top, 'achieved': round(ach, 2), 'peak': round(peak, 1),
            'unit': 'TFLOP/s', 'frac': round(ach / peak, 4),
            'peak_basis': f'dense 16-bit MFMA {PEAK_16BIT_MFMA_TFLOPS:.0f} TFLOP/s / {mfmas[top]} MFMA products per fp32 multiply-add',
            'mfma_tflops_executed': round(mfmas[top] * ach, 1), 'fp32_mfma_peak': PEAK_F32_MFMA_TFLOPS,
            'vs_fp32_mfma_peak': round(ach / PEAK_F32_MFMA_TFLOPS, 4), 'launches_timed': n,
            'flops_per_launch': round(fl / n), 'us_per_launch': round(us / n, 2),
            'share_of_bracketed_gpu_time': round(survey[0][top][1] / sum(v[1] for v in survey[0].values()), 3), 'traffic': traffic,
            'traffic_source': traffic_source, 'alone_on_the_chip': alone,
            'flops_basis': 'algorithmic: reductions and stored rows over the B x T real frames (halo rows of the slabs not counted)'}
    recur = None
    if 'rec_fwd' in rec and 'rec_bwd' in rec:
        nf, uf, _ = rec['rec_fwd']
        nb, ub, _ = rec['rec_bwd']
        recur = {'launches_per_step': round((nf + nb) / steps, 2), 'fwd_us_per_time_step': round(uf / nf / T, 3),
                 'bwd_us_per_time_step': round(ub / nb / T, 3), 'ms_per_step': round((uf + ub) / steps / 1e3, 3),
                 'share_of_step_wall_time': round((uf + ub) / steps / 1e3 / ms_step, 3)}
    return roof, classes, recur


def solver_loop(B, T, iters=120, warm=8):
    """Loader-to-loss: Solver.train() as main.py runs it, batches cropped / clipped / padded on the GPU from an HBM-resident
    synthetic corpus (data_loader.get_device_loader), host draws per step, H2D staging, log line every 10 iterations."""
    import contextlib
    import io
    import tempfile
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HP, solver
    hp = HP.default_hparams(batch_size=B, max_len_pad=T)
    loader = data_loader.get_device_loader(hp, dataset=data_loader.SyntheticUtterances(4 * B, seed=5))
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        cfg = SimpleNamespace(num_iters=warm, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False, device_id=torch.cuda.current_device(),
                              log_dir=tmp, sample_dir=tmp, model_save_dir=tmp, log_step=10, sample_step=10 ** 9, model_save_step=10 ** 9)
        s = solver.Solver(loader, cfg, hp)
        s.validation_pt = []
        s.train()
        torch.cuda.synchronize()
        s.num_iters = iters
        t0 = time.perf_counter()
        s.train()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {'iterations_per_s': round(iters / dt, 2), 'utterances_per_s': round(B * iters / dt, 1), 'ms_per_iteration': round(dt / iters * 1e3, 3),
            'what': f'speechsplit_amd.solver.Solver.train(), {iters} iterations, batch {B} x {T}, DeviceBatcher + DevicePrefetcher, loss read every 10 iterations'}


def dump_outputs(eng, out_dir, cap=1 << 22):
    """What a training step left its caller, as float32 .npy files: loss.npy (the loss it returned), params.npy (the updated
    parameter arena) and grads.npy (the gradient arena Adam applied).  An arena of more than `cap` elements (Generator_3: 19.4 M) is
    written at the same `cap` positions every run, a seeded sample in ascending order: 2 x 16 MB at most."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    n = eng.params.numel()
    idx = None
    if n > cap:
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:cap].sort().values.to(eng.device)
    for name, t in (('loss', eng.loss), ('params', eng.params), ('grads', eng.grads)):
        if idx is not None and t.numel() == n:
            t = t[idx]
        np.save(os.path.join(out_dir, name + '.npy'), t.detach().to(torch.float32).cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64, help='utterances per GPU')
    ap.add_argument('--frames', type=int, default=128)
    ap.add_argument('--global-batch', type=int, default=0,
                    help='STRONG scaling: the global batch is fixed and split over the ranks (BASELINE config 3 is --global-batch 64 --precision bf16 on 2 GPUs: '
                         '32 utterances per GPU; config 4 --global-batch 256 --model G6 --frames 192 on 8).  Default 0: weak scaling, --batch utterances per GPU')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-extras', action='store_true', help='skip alt_precisions and solver_loop')
    ap.add_argument('--precision', choices=['f32', 'bf16'], default='f32',
                    help="f32 (default): the 1e-4 parity mode the headline is quoted on; bf16: BASELINE configs 3-5's arithmetic")
    ap.add_argument('--model', choices=['G3', 'G6'], default='G3', help='G6: Generator_6 (pitch converter, CE loss; BASELINE config 4 is --model G6 --batch 32 --frames 192 --precision bf16)')
    ap.add_argument('--workload', choices=['fixed', 'config5'], default='fixed',
                    help='config5: BASELINE config 5 -- crops of 96..192 frames, every batch from one length bucket (speechsplit_amd/buckets.py), '
                         'assembled on the GPU and staged by DevicePrefetcher inside the timed region; use with --frames 192')
    ap.add_argument('--force-dp', action='store_true', help='run the data-parallel step (bucketed all-reduce, sliced draws) even at world size 1')
    ap.add_argument('--dp-backend', choices=['torch', 'native'], default='native',
                    help="data-parallel collectives: torch.distributed's ProcessGroupNCCL (Engine.dp_train_step) or the engine's own RCCL "
                         "communicator (ss_g3_dp_train_step: the decoder bucket is launched on the engine's side stream itself).  Default native: "
                         "at world 1 it costs nothing over the plain step (6.32 ms) while the torch path costs +0.5 ms -- ProcessGroupNCCL's own "
                         "stream shares a hardware queue with one of the engine's.  (Generator_6 always takes the torch path.)")
    ap.add_argument('--no-profile', action='store_true', help='no hipEvent brackets in the timed region (to measure their cost)')
    ap.add_argument('--tune', action='append', default=[], metavar='KEY=VALUE', help='experiment knob of the HIP library (ss_tune)')
    ap.add_argument('--full', action='store_true',
                    help='also everything beyond the headline: the kernel-class survey and the roofline / recurrence brackets in the timed steps, '
                         'alt_precisions, solver_loop, dp_collectives, dp_replicas and cpu_baseline.  Default: the timed steps only')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='after the timed steps, run the last one again from the start state (initial weights, fresh Adam) and write what it '
                         'computed to DIR/{loss,params,grads}.npy (float32; see dump_outputs)')
    args = ap.parse_args()

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if args.gpus != world and world == 1 and args.gpus > 1:
        sys.exit('bench.py: for --gpus N > 1 launch with torch.distributed.run --nproc-per-node N')
    torch.cuda.set_device(local)
    dev = torch.device(f'cuda:{local}')

    from speechsplit_amd import hparams as HP, model as M
    from speechsplit_amd.engine import Engine, draw_interp, tune
    for kv in args.tune:
        k, v = kv.split('=')
        tune(k, int(v))
    B, T = args.batch, args.frames
    if args.global_batch:
        if args.global_batch % world:
            sys.exit(f'bench.py: --global-batch {args.global_batch} is not a multiple of the {world} ranks')
        B = args.global_batch // world
    kind = args.model
    hp = HP.default_hparams(max_len_pad=T, batch_size=B * world)
    eng = Engine(kind, hp, B, T, device=dev)
    eng.load_weights(M.init_weights(kind, hp, 0))          # the reference's initialisers, fixed seed
    dp = world > 1 or args.force_dp
    dist = None
    if dp:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29511')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    adam = (1e-4, 0.9, 0.999, 1e-8, 0)
    eng.set_adam(*adam)
    # --dump-outputs: the state every run starts from, for the replay of the last timed step (see below)
    start = eng.params.clone() if args.dump_outputs else None
    eng.set_precision(args.precision)
    native = dp and args.dp_backend == 'native'             # the engine's own RCCL communicator, both generators (round 3: ss_g6_dp_train_step)
    if native:
        eng.comm_init(rank, world)
    mel, f0, emb, lens = synth(B, T, 1000 + rank, dev)
    torch.manual_seed(1234)
    S = hp.max_len_seq // hp.min_len_seg + 1
    ncalls = 4 if kind == 'G3' else 3
    if kind == 'G6':        # quantised F0 of the batch: input one-hot and cross-entropy target
        from speechsplit_amd.utils import quantize_f0_torch
        onehot, qidx = quantize_f0_torch(f0[:, :, 0].clone())
        onehot, qidx = onehot.contiguous(), qidx.to(torch.int32).contiguous()
    stream = None
    frames_done = [0]
    timed_frames = [0]
    if args.workload == 'config5':
        from speechsplit_amd import buckets, data_loader, staging
        corpus = data_loader.DeviceCorpus(data_loader.SyntheticUtterances(4 * B, seed=7 + rank), dev)
        loader = buckets.BucketedDeviceBatcher(hp, corpus, 96, 192, rank=rank, world=world, seed=11, steps_per_epoch=10 ** 9)
        stream = staging.DevicePrefetcher(loader, dev)

    last = [None]                                   # the draws (and config 5 batch) of the latest step

    def step(replay=None):
        if replay is None:
            # fresh randomness every step: one global draw stream (the reference's generator calls), each rank takes its utterances' slice
            sc, ls = draw_interp(B * world, ncalls, hp)
            if world > 1:
                sc = sc.view(ncalls, world, B * S)[:, rank]
                ls = ls.view(ncalls, world, B * S)[:, rank]
            batch = None
            if stream is not None:                   # config 5: the next length-bucketed batch, already staged on the device
                batch = next(stream)
                frames_done[0] += batch[0].shape[1]
            last[0] = (sc, ls, batch)
        else:
            sc, ls, batch = replay
        if stream is not None:
            bm, be, bf, bl = batch
            if native:
                eng.dp_train_step_native(bm, bf, be, bl, (sc, ls), bucket=True)
            elif dp:
                eng.dp_train_step(bm, bf, be, bl, (sc, ls), world, bucket=True)
            else:
                eng.g3_train_step(bm, bf, be, bl, (sc, ls), bucket=True)
        elif kind == 'G6':
            if native:
                eng.g6_dp_train_step_native(mel, onehot, qidx, (sc, ls))
            elif dp:
                eng.dp_g6_train_step(mel, onehot, qidx, (sc, ls), world)
            else:
                eng.g6_train_step(mel, onehot, qidx, (sc, ls))
        elif native:
            eng.dp_train_step_native(mel, f0, emb, lens, (sc, ls))
        elif dp:
            eng.dp_train_step(mel, f0, emb, lens, (sc, ls), world)
        else:
            eng.g3_train_step(mel, f0, emb, lens, (sc, ls))

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(steps, warmup, profile, every=1):
        for _ in range(warmup):
            step()
        barrier()
        if profile:
            eng.profile(profile, every)
        f0_ = frames_done[0]
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        barrier()
        dt = time.perf_counter() - t0
        timed_frames[0] = frames_done[0] - f0_          # frames of the batches of THIS timed region (config 5: their lengths vary)
        if profile:
            eng.profile(False)
        if dist is not None:
            tt = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt)
        return dt

    # survey pass (untimed): every kernel class bracketed, to find the class with the most GPU time; the timed region then
    # carries brackets on that class and on the recurrences only, and only in every PROF_EVERY-th step: a bracket costs 4-8 us of
    # stream time (the launch behind it waits for the one in front to retire), all 71 per step +4.5 %, these 18 +2.9 % if every
    # step carried them (5.44 vs 5.29 ms measured in one call) -- sampled, under 0.6 %
    PROF_EVERY = 5
    profile = args.full and not args.no_profile
    top, survey = None, None
    if profile:
        timed(6, 2, True)
        survey = (eng.profile_read(), 6)
        top = dominant_class(survey[0])
    dt = timed(args.steps, args.warmup, [top, 'rec_fwd', 'rec_bwd'] if profile else None, PROF_EVERY)
    bracketed = (args.steps + PROF_EVERY - 1) // PROF_EVERY      # steps of the timed region that carried the brackets
    eng.check()                  # outside the timed region: no persistent kernel reported a bounded-wait expiry
    fallbacks = eng.scratch_fallbacks()      # launches that ran out of scratch and took a slower path: must be 0
    if args.dump_outputs:
        # The timed steps' weights and Adam moments drift apart from run to run: split-K atomics commit in arrival order, and Adam turns
        # that last-bit noise in near-zero gradients into whole lr-sized moves that the next steps carry on.  So the step that is dumped
        # starts from the state every run starts from (initial weights, Adam moments and step counter zero) and takes the last timed
        # step's batch and draws: the same inputs every run, through the same path (every rank: the collectives must match)
        eng.params.copy_(start)
        eng.adam_m.zero_()
        eng.adam_v.zero_()
        eng.set_adam(*adam)
        step(last[0])
        eng.check()
        if rank == 0:
            dump_outputs(eng, args.dump_outputs)
    # data parallel, native path: where every bucket's collective sat relative to the end of the backward -- hipEvent brackets on the
    # communication stream (ss_dp_profile) over a few steps OUTSIDE the timed region; the record of the last one, from real RCCL kernels
    dp_coll = None
    if native and args.full:
        eng.dp_profile(True)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        rec = eng.dp_profile_read()
        eng.dp_profile(False)
        if dist is not None:
            dist.barrier()
        if rec:
            dp_coll = {'what': 'collectives of one data-parallel step in enqueue order, microseconds relative to the END OF THE BACKWARD on the main stream '
                               '(negative: hidden beside the backward); offset -1 = the grouped rest (layer-0 convolutions, encoder BLSTMs, Encoder_t, status slot)',
                       'world': world, 'rank': rank,
                       'buckets': [{'arena_offset': o, 'mbytes': round(c * 4 / 1e6, 2), 'start_us': round(a, 1), 'end_us': round(b, 1)} for o, c, a, b in rec],
                       'last_end_us': round(max(b for _, _, _, b in rec), 1)}
    # data parallel: every rank saw different utterances, so the replicas' weights agree bit for bit only if every bucket was reduced over all
    # ranks and the same update applied -- a 64-bit sum over the weights' bit patterns, gathered from all ranks (outside the timed region)
    dp_rep = None
    if dist is not None and args.full:
        torch.cuda.synchronize()
        mine = eng.params.view(torch.int32).to(torch.int64).sum().reshape(1)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        sums = [int(t) for t in every]
        dp_rep = {'identical': all(v == sums[0] for v in sums), 'ranks': world, 'weights_bit_sum': sums[0]}
        if not dp_rep['identical']:
            print(f'[bench] rank {rank}: REPLICAS DIVERGED: per-rank sums of the weights bit patterns {sums}', file=sys.stderr, flush=True)
    ms = dt / args.steps * 1e3
    value = B * world / (dt / args.steps)
    mean_T = timed_frames[0] / max(1, args.steps) if stream is not None else T      # config 5: mean frames per batch over the timed batches only

    if rank == 0:
        print(f'[bench] gpu: {ms:.3f} ms/step, {value:.1f} utt/s on {world} GPU(s)', file=sys.stderr, flush=True)
        roof, classes, recur = kernel_report(eng, bracketed, ms, args.precision, top, survey, T if stream is None else mean_T) if top else (None, None, None)
        if roof:
            roof['bracketed_steps'] = f'{bracketed} of the {args.steps} timed steps (every {PROF_EVERY}th: a bracket holds the next launch back by 4-8 us)'
        print(f'[bench] roofline: {roof}', file=sys.stderr, flush=True)
    alt = None
    if args.full and not args.no_extras and args.precision == 'f32' and kind == 'G3' and args.workload == 'fixed':
        # the same step with the other product formats of the fp32 mode (every rank runs them: the collectives must match).  Keys say what they
        # switch: the headline multiplies fp16 x 2 pieces (22 significand bits) everywhere;
        #   gemms_bf16x3: the GEMMs on the exact 3-way bf16 split (6 MFMAs), the six persistent recurrences STILL fp16 x 2 (32 % of the MACs);
        #   all_fp32_mfma: EVERY product of the step -- GEMMs and recurrences -- on v_mfma_f32_*_f32: 24-bit significands, fused fp32 accumulate, the
        #     reference's arithmetic width (gemm_mode = 0; persist = 0: the recurrences as one fp32-MFMA launch per time step).  This is the price
        #     of the headline's 22-bit products as a driver-observed number.
        alt = {}
        modes = (('gemms_bf16x3', {'fwd_f16x2': 0, 'bwd_f16x2': 0}, {'fwd_f16x2': 1, 'bwd_f16x2': 1}, PEAK_16BIT_MFMA_TFLOPS / 6,
                  'dense 16-bit MFMA 2500 TFLOP/s / 6 MFMA products per fp32 multiply-add', 'GEMMs: exact bf16 x 3 split (6 MFMAs); the six persistent recurrences stay fp16 x 2'),
                 ('all_fp32_mfma', {'gemm_mode': 0, 'persist': 0}, {'gemm_mode': 1, 'persist': 1}, PEAK_F32_MFMA_TFLOPS, 'dense fp32 MFMA 157.3 TFLOP/s',
                  'EVERY product fp32-wide: GEMMs and recurrences on v_mfma_f32_*_f32 (recurrences as one launch per time step)'))
        for name, knobs, restore, peak, basis, what in modes:
            for k, v in knobs.items():
                tune(k, v)
            prof = [top] if top else False
            ms_alt = round(timed(8, 2, prof) / 8 * 1e3, 3)
            rec_alt = {'ms_per_step': ms_alt, 'utterances_per_s': round(B * world / ms_alt * 1e3, 1), 'what': what}
            if prof and rank == 0:
                r2 = eng.profile_read()
                if r2 and top in r2:
                    n2, us2, fl2 = r2[top]
                    rec_alt['roofline'] = {'bound': 'mfma', 'class': top, 'achieved': round(fl2 / us2 / 1e6, 2), 'peak': round(peak, 1), 'unit': 'TFLOP/s',
                                           'frac': round(fl2 / us2 / 1e6 / peak, 4), 'launches_timed': n2, 'us_per_launch': round(us2 / n2, 2), 'peak_basis': basis}
            alt[name] = rec_alt
            for k, v in restore.items():
                tune(k, v)
        eng.check()
    sl = None
    if rank == 0 and args.full and not (args.no_extras or world > 1 or kind != 'G3' or args.workload != 'fixed'):
        # Solver builds its own engine: release this one first (its four streams would otherwise change which hardware queues the
        # second engine's streams land on -- measured 7.4 vs 6.7 ms per iteration)
        eng_hp = eng.hp
        del eng
        import gc
        gc.collect()
        torch.cuda.synchronize()
        sl = solver_loop(B, T)
    if rank == 0:
        out = {
            'metric': 'utterances/sec (fwd+bwd, 128-frame 80-mel, batch 64) at 1/2/4/8 MI355X',
            'value': round(value, 1), 'unit': 'utterances/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(ms, 3), 'higher_is_better': True, 'scaling': 'strong' if args.global_batch else 'weak', 'vs_baseline': None,
            'dtype': 'f32 (fp16x2 products)' if args.precision == 'f32' else 'bf16 (operand images stored in bf16, fp32 accumulation, state and master weights)', 'data': 'synthetic',
            'config': {'workload': (f'Generator_3 full training step (host draws+resample+quantise+fwd+MSE+bwd+Adam), '
                                    f'{B} utterances/GPU x {T} frames x 80 mel + F0, max_len_pad={T}' if kind == 'G3' and args.workload == 'fixed' else
                                    f'Generator_3 full training step over length-bucketed batches (BASELINE config 5): crops of 96..192 frames, one bucket '
                                    f'(multiple of 8) per batch, max_len_pad = bucket, {B} utterances/GPU, mean {mean_T:.1f} frames/batch in the timed region, '
                                    f'batches assembled on the GPU + DevicePrefetcher inside the timed region' if kind == 'G3' else
                                    f'Generator_6 full training step (host draws+fwd+cross-entropy+bwd+Adam; BASELINE config 4 shape), {B} utterances/GPU x {T} frames'),
                       'global_batch': B * world, 'seq_len': T, 'parallelism': f'dp{world}' + (' (forced DP path)' if args.force_dp and world == 1 else '') + (f', {args.dp_backend} RCCL' if dp else ''),
                       'products': PRODUCTS[args.precision]},
            'step_tflops': round(3 * 2 * (MAC_PER_FRAME_G3 if kind == 'G3' else MAC_PER_FRAME_G6) * mean_T * B * world / (dt / args.steps) / 1e12, 2),
            'roofline': roof, 'kernel_classes': classes, 'recurrence': recur, 'alt_precisions': alt,
            'solver_loop': sl, 'dp_collectives': dp_coll, 'dp_replicas': dp_rep, 'scratch_fallbacks': fallbacks,
            'cpu_baseline': cpu_baseline(T) if args.full and not args.no_cpu_baseline else None,
        }
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
