#!/usr/bin/env python
"""Sliced Wasserstein distance (Karras et al. 2018, section 5) between clips of a dataset and clips of a trained generator, on the
device (mocogan-chainer_amd/metrics.py; no reference counterpart -- the reference has no metric).  Prints one JSON line:
per-level distances x 1e3 and their average, and with --baseline the same figure between the two halves of the real set -- the
noise floor the number has to be read against.  The measure sees only 7x7(x --patch_frames) patches of a Laplacian pyramid."""
import argparse
import json

import numpy as np

from datasets import MugDataset, MovingMnistDataset, SyntheticDataset


def build_parser():
    cli = argparse.ArgumentParser(description='sliced Wasserstein distance between real clips and an ImageGenerator\'s clips')
    cli.add_argument('model_weight', help='generator .npz (image_gen_epoch_*.npz or image_gen_ema_epoch_*.npz)')
    cli.add_argument('--dataset_type', default='mug', choices=['mug', 'mnist', 'synthetic'], help='as train.py')
    cli.add_argument('--dataset', default='data/dataset/train', help='root directory of the frame-directory dataset (as train.py)')
    cli.add_argument('--synthetic_size', type=int, default=256, help='clips in the synthetic dataset (as train.py)')
    for flags, default, text in ((('--num', '-n'), 1024, 'clips per set (the first --num clips of the dataset against --num generated ones)'),
                                 (('--patches',), 128, 'patches per clip and pyramid level'),
                                 (('--patch_frames',), 1, 'consecutive frames per patch; 2 or 3 makes the descriptor see motion'),
                                 (('--repeats',), 4, 'independent draws of --dirs directions'),
                                 (('--dirs',), 128, 'directions per repeat'),
                                 (('--seed',), 0, 'seed of the latent draws, the patch positions and the directions'),
                                 (('--chunk',), 64, 'clips generated / uploaded at a time'),
                                 (('--dim_zl',), 0, 'label dimension the generator was trained with'),
                                 (('--n_filters',), 64, 'generator width'),
                                 (('--channel',), 3, 'image channels (1 or 3)'),
                                 (('--video_len',), 16, 'frames per clip')):
        cli.add_argument(*flags, type=int, default=default, help=text)
    cli.add_argument('--test_mode', type=int, choices=[0, 1], default=1,
                     help="1 (default): BatchNorm's running statistics (ImageGenerator.sample_many); 0: batch statistics per chunk, as "
                          "generate_samples.py's default")
    cli.add_argument('--labels', default=None, help='with --dim_zl: the label of every generated clip, "0,3,5" (one per clip) or one value for all')
    cli.add_argument('--mfma', choices=['f32', 'bf16', 'f32x3'], default='f32', help='MFMA operand type of the generator (as train.py)')
    cli.add_argument('--baseline', action='store_true', help='also report the first half of the real set against its second half')
    return cli


def parse_args(argv=None):
    cli = build_parser()
    args = cli.parse_args(argv)
    if args.num < 1 or args.chunk < 1 or min(args.patches, args.patch_frames, args.repeats, args.dirs) < 1:
        cli.error('--num, --chunk, --patches, --patch_frames, --repeats and --dirs are positive')
    if args.patch_frames > args.video_len:
        cli.error('--patch_frames exceeds --video_len')
    if args.channel not in (1, 3):
        cli.error('--channel is 1 or 3')
    if args.baseline and args.num % 2:
        cli.error('--baseline splits the real set in halves: --num must be even')
    if args.labels is not None:
        if not args.dim_zl:
            cli.error('--labels needs --dim_zl')
        try:
            labels = [int(v) for v in args.labels.split(',')]
        except ValueError:
            cli.error('--labels: integers separated by commas')
        if any(v < 0 or v >= args.dim_zl for v in labels):
            cli.error('--labels: every value must lie in [0, --dim_zl)')
        if len(labels) not in (1, args.num):
            cli.error('--labels: one value, or one per clip (--num)')
        args.labels = labels
        if not args.test_mode:
            cli.error('--labels chooses the latents: it needs --test_mode 1')
    return args


def make_dataset(args):
    if args.dataset_type == 'mug':
        if args.channel != 3:
            raise ValueError('--channel 1 needs --dataset_type mnist or synthetic (MUG clips are RGB)')
        return MugDataset(args.dataset, args.video_len)
    if args.dataset_type == 'mnist':
        return MovingMnistDataset(args.dataset, args.video_len, channels=args.channel)
    return SyntheticDataset(args.synthetic_size, 6, args.channel, args.video_len, 64)


def to_bytes(video):
    """a dataset item (C,T,H,W) in [-1, 1] -> (T,H,W,C) uint8, generate_samples.py's ((x / 2 + 0.5) * 255) truncated"""
    x = (np.asarray(video, np.float32) / 2. + 0.5) * 255
    return np.clip(x, 0, 255).astype(np.uint8).transpose(1, 2, 3, 0)


def real_chunks(dataset, num, chunk):
    if len(dataset) < num:
        raise ValueError('the dataset holds %d clips, --num asks for %d' % (len(dataset), num))
    raw = getattr(dataset, 'get_example_raw', None)
    for lo in range(0, num, chunk):
        idx = range(lo, min(lo + chunk, num))
        yield np.stack([raw(i)[0] if raw is not None else to_bytes(dataset[i][0]) for i in idx])


def fake_chunks(gen, args):
    labels = None
    if gen.use_label:
        labels = np.random.randint(gen.dim_zl, size=args.num) if args.labels is None else \
            np.broadcast_to(np.asarray(args.labels), (args.num,)).copy()
    if args.test_mode:
        yield from gen.sample_many(args.num, args.chunk, labels=labels, video_len=args.video_len)
        return
    for lo in range(0, args.num, args.chunk):
        x = gen(min(args.chunk, args.num - lo))[0].detach().cpu().numpy()           # (T, N, C, H, W) in [-1, 1]
        yield (255 * (0.5 * x + 0.5)).astype(np.uint8).transpose(1, 0, 3, 4, 2)     # truncating cast, as generate_samples.py


def main(argv=None):
    args = parse_args(argv)
    from model.net import ImageGenerator
    from mocogan_chainer_amd.trainer import load_npz
    from mocogan_chainer_amd.metrics import SlicedWasserstein
    import mocogan_chainer_amd.hiplib as hl

    gen = ImageGenerator(dim_zl=args.dim_zl, out_channels=args.channel, n_filters=args.n_filters, video_len=args.video_len)
    load_npz(args.model_weight, gen)
    if args.mfma != 'f32':
        gen.impl.set_precision(args.mfma)
    hl.use_pretuned_table()                                              # (sampling never times candidates)
    np.random.seed(args.seed)
    swd = SlicedWasserstein(args.patches, args.patch_frames, args.repeats, args.dirs, args.seed)
    real_raw = swd.raw_descriptors(real_chunks(make_dataset(args), args.num, args.chunk))       # the real descriptors: once per run
    baseline = None
    if args.baseline:
        half = args.num // 2
        baseline = swd.distance(swd.normalized(real_raw, 0, half), swd.normalized(real_raw, half, args.num))
    real = swd.normalized(real_raw, inplace=True)
    fake = swd.descriptors(fake_chunks(gen, args))
    out = {'swd': swd.distance(real, fake), 'baseline': baseline, 'baseline_clips': args.num // 2 if args.baseline else None,
           'num': args.num, 'patches': args.patches, 'patch_frames': args.patch_frames, 'repeats': args.repeats, 'dirs': args.dirs,
           'seed': args.seed, 'test_mode': args.test_mode, 'model_weight': str(args.model_weight), 'dataset_type': args.dataset_type}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
