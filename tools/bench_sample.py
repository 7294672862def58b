#!/usr/bin/env python
"""A/B timing of the generator's sampling path: how long until a batch of clips is uint8 on the host.
  A: ImageGenerator.__call__ under config.train = False, fp32 (T,N,C,H,W) copied to the host and quantised there
     ((x / 2 + 0.5) * 255 truncated) -- what a test-mode user of the training-side code does;
  B: ImageGenerator.sample(as_uint8=True): folded BatchNorm, ReLU in the deconvolutions' store, bytes formed on the device.
Both draw their latents from np.random under one seed and end with uint8 (N,T,H,W,C) on the host.  Batches above --chunk clips run
in chunks (a launch's tensors must stay below 2 GiB, i.e. below 512 clips at full width): A by repeated __call__, B through
sample_many.  A and B alternate in one process after a warm-up; per call HIP events around everything the call enqueues (copies to the
host included) and a host clock around the whole call.  Medians over the iterations; one JSON line per (precision, clips).
(With chunks the latents of A and B differ -- A draws per chunk -- so the byte comparison at the end is meaningful below --chunk only.)
usage: python tools/bench_sample.py [--clips 36,1024] [--precisions f32,f32x3,bf16] [--iters 20] [--chunk 256] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl
from model.net import ImageGenerator, config


def run_a(gen, n):
    prev, config.train = config.train, False
    try:
        x = gen(n)[0]
    finally:
        config.train = prev
    gen.last_saved = None
    return x


def host_bytes_a(x):
    v = x.detach().cpu().numpy()
    return ((v / 2. + 0.5) * 255).astype(np.uint8)


def call_a(gen, n, chunk):
    """-> uint8 (N,T,H,W,C) on the host, chunk clips per __call__ (a launch's tensors must stay below 2 GiB: include/mocogan_hip.h)"""
    return np.concatenate([host_bytes_a(run_a(gen, min(chunk, n - lo))).transpose(1, 0, 3, 4, 2) for lo in range(0, n, chunk)])


def call_b(gen, n, chunk):
    if n <= chunk:
        return gen.sample(n, as_uint8=True)[0].cpu().numpy().transpose(1, 0, 3, 4, 2)
    return np.concatenate(list(gen.sample_many(n, chunk)))


def device_only(fn, gen, n, reps):
    """ms per call of the device work alone (latent draws on the host included, nothing copied back): HIP events around reps calls"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        x = fn(gen, n)
    e1.record()
    torch.cuda.synchronize()
    del x
    return e0.elapsed_time(e1) / reps


def timed(fn, gen, n, chunk):
    """-> (device ms: HIP events around the call's launches, end-to-end ms: host clock, the call ends in a synchronising copy)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn(gen, n, chunk)
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    assert out.dtype == np.uint8 and out.shape[0] == n
    return e0.elapsed_time(e1), (t1 - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', default='36,1024')
    ap.add_argument('--precisions', default='f32,f32x3,bf16')
    ap.add_argument('--n_filters', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20, help='timed A/B pairs at the small size (the large size takes iters / 4, at least 5)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--chunk', type=int, default=256, help='clips per call: larger batches run in chunks, A by repeated __call__, B through sample_many')
    ap.add_argument('--autotune', type=int, default=1, help='1: tile tuner on with the shipped table, as bench.py / train.py; A tunes the geometries it '
                    'meets during the warm-up and B, which never tunes, takes those table entries')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sample.py measures on the GPU; there is no CPU fallback"
    hl.load()
    hl.set_autotune(bool(args.autotune))
    lines = []
    for prec in args.precisions.split(','):
        np.random.seed(0)
        gen = ImageGenerator(n_filters=args.n_filters)
        rng = np.random.RandomState(1)
        p = dict(gen.serialize_dict())
        for l in (1, 2, 3, 4):                       # running statistics of a generator that has been trained, not the (0, 1) defaults
            c = p['bn%d/gamma' % l].shape[0]
            p['bn%d/avg_mean' % l] = rng.normal(0, 0.05, c).astype(np.float32)
            p['bn%d/avg_var' % l] = rng.uniform(0.02, 0.2, c).astype(np.float32)
        gen.load_dict(p)
        gen.impl.set_precision(prec)
        for n in (int(c) for c in args.clips.split(',')):
            iters = args.iters if n <= 128 else max(5, args.iters // 4)
            for _ in range(args.warmup):
                call_a(gen, n, args.chunk)
                call_b(gen, n, args.chunk)
            a, b = [], []
            for _ in range(iters):                   # alternate: drift of the box hits both alike
                np.random.seed(7)
                a.append(timed(call_a, gen, n, args.chunk))
                np.random.seed(7)
                b.append(timed(call_b, gen, n, args.chunk))
            np.random.seed(7)
            xa = call_a(gen, n, args.chunk)
            np.random.seed(7)
            xb = call_b(gen, n, args.chunk)
            d = np.abs(xa.astype(np.int64) - xb.astype(np.int64))
            m = min(n, args.chunk)                   # the device work of one call, without the copy out and the host's part
            dev_a = min(device_only(run_a, gen, m, 10) for _ in range(3))
            dev_b = min(device_only(lambda g_, k: g_.sample(k, as_uint8=True)[0], gen, m, 10) for _ in range(3))
            med = lambda v, i: statistics.median(t[i] for t in v)
            line = {'precision': prec, 'clips': n, 'chunk': min(n, args.chunk), 'n_filters': args.n_filters, 'iters': iters,
                    'A_device_only_ms_per_call': round(dev_a, 3), 'B_device_only_ms_per_call': round(dev_b, 3), 'device_only_clips': m,
                    'A_events_ms': round(med(a, 0), 3), 'B_events_ms': round(med(b, 0), 3),
                    'A_call_end_to_end_ms': round(med(a, 1), 3), 'B_sample_end_to_end_ms': round(med(b, 1), 3),
                    'A_min_max_end_to_end_ms': [round(min(t[1] for t in a), 3), round(max(t[1] for t in a), 3)],
                    'B_min_max_end_to_end_ms': [round(min(t[1] for t in b), 3), round(max(t[1] for t in b), 3)],
                    'speedup_device_only': round(dev_a / dev_b, 3), 'speedup_end_to_end': round(med(a, 1) / med(b, 1), 3),
                    'clips_per_s_B': round(n / med(b, 1) * 1e3, 1),
                    'bytes_differing_share': float((d != 0).mean()), 'bytes_max_abs_diff': int(d.max())}
            print(json.dumps(line), flush=True)
            lines.append(line)
            gen.impl._sbuf = [None, None, None]
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
