#!/usr/bin/env python
"""Nearest-neighbour metrics between clips of a dataset and clips of a trained generator, on the device
(mocogan-chainer_amd/metrics.py: KnnMetrics; no reference counterpart -- the reference has no metric).  Prints one JSON line:
improved precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) and, with --holdout_num, a
data-copying score (after Meehan et al. 2020): whether generated clips lie closer to the training clips than fresh real clips do.
Distances are squared L2 between --pool x --pool box means of whole, aligned clips -- a shifted copy is not a copy -- and every
figure depends on --num and --k: compare at equal settings."""
import argparse
import json

import numpy as np

from evaluate_swd import fake_chunks, make_dataset, real_chunks, to_bytes


def build_parser():
    cli = argparse.ArgumentParser(description='k-NN precision / recall, density / coverage and a data-copying score between real clips and '
                                              'an ImageGenerator\'s clips')
    cli.add_argument('model_weight', help='generator .npz (image_gen_epoch_*.npz or image_gen_ema_epoch_*.npz)')
    cli.add_argument('--dataset_type', default='mug', choices=['mug', 'mnist', 'synthetic'], help='as train.py')
    cli.add_argument('--dataset', default='data/dataset/train', help='root directory of the frame-directory dataset (as train.py)')
    cli.add_argument('--synthetic_size', type=int, default=256, help='clips in the synthetic dataset (as train.py)')
    for flags, default, text in ((('--num', '-n'), 1024, 'clips per set (the first --num clips of the dataset, the training clips, against --num generated ones)'),
                                 (('--k',), 5, 'the neighbour that sets a clip\'s radius (1..16; at most --num - 1)'),
                                 (('--pool',), 4, 'box the frames are averaged over: 2, 4 or 8 (2 only for short or grey clips: '
                                                  'video_len * (64 / pool)^2 * channel may not exceed 32768)'),
                                 (('--holdout_num',), 0, 'held-out real clips for copy_auc (0: no copy_auc).  They MUST be clips training never '
                                                         'saw; nothing here can check that -- it is the user\'s responsibility'),
                                 (('--seed',), 0, 'seed of the latent draws'),
                                 (('--chunk',), 64, 'clips generated / uploaded at a time'),
                                 (('--dim_zl',), 0, 'label dimension the generator was trained with'),
                                 (('--n_filters',), 64, 'generator width'),
                                 (('--channel',), 3, 'image channels (1 or 3)'),
                                 (('--video_len',), 16, 'frames per clip')):
        cli.add_argument(*flags, type=int, default=default, help=text)
    cli.add_argument('--holdout_dataset', default=None,
                     help='directory the held-out clips are read from (its clips [0, --holdout_num)); default: clips [--num, --num + '
                          '--holdout_num) of --dataset.  Either way they have to be clips training never saw: with the default, train on '
                          'the first --num clips only.  That is the user\'s responsibility')
    cli.add_argument('--dump_pairs', default=None, metavar='OUT.npz',
                     help='write nn_index (every generated clip\'s nearest training clip) and nn_dist (its squared distance) to this .npz')
    cli.add_argument('--test_mode', type=int, choices=[0, 1], default=1,
                     help="1 (default): BatchNorm's running statistics (ImageGenerator.sample_many); 0: batch statistics per chunk, as "
                          "generate_samples.py's default")
    cli.add_argument('--labels', default=None, help='with --dim_zl: the label of every generated clip, "0,3,5" (one per clip) or one value for all')
    cli.add_argument('--mfma', choices=['f32', 'bf16', 'f32x3'], default='f32', help='MFMA operand type of the generator (as train.py)')
    return cli


def parse_args(argv=None):
    cli = build_parser()
    args = cli.parse_args(argv)
    if args.num < 1 or args.chunk < 1 or args.video_len < 1:
        cli.error('--num, --chunk and --video_len are positive')
    if not 1 <= args.k <= 16:
        cli.error('--k lies in 1..16')
    if args.k > args.num - 1:
        cli.error('--k may not exceed --num - 1')
    if args.pool not in (2, 4, 8):
        cli.error('--pool is 2, 4 or 8')
    if args.channel not in (1, 3):
        cli.error('--channel is 1 or 3')
    if args.video_len * (64 // args.pool) ** 2 * args.channel > 32768:
        cli.error('--video_len * (64 / --pool)^2 * --channel exceeds 32768: use a larger --pool')
    if args.holdout_num < 0:
        cli.error('--holdout_num is not negative')
    if args.holdout_dataset is not None and not args.holdout_num:
        cli.error('--holdout_dataset needs --holdout_num')
    if args.holdout_dataset is not None and args.dataset_type == 'synthetic':
        cli.error('--holdout_dataset names a directory: the synthetic dataset has none')
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


def clip_chunks(dataset, lo, hi, chunk):
    """clips lo .. hi of the dataset as uint8 (n,T,64,64,C) chunks (evaluate_swd.real_chunks with a first clip)"""
    if len(dataset) < hi:
        raise ValueError('the dataset holds %d clips, clips %d .. %d are asked for' % (len(dataset), lo, hi))
    raw = getattr(dataset, 'get_example_raw', None)
    for first in range(lo, hi, chunk):
        idx = range(first, min(first + chunk, hi))
        yield np.stack([raw(i)[0] if raw is not None else to_bytes(dataset[i][0]) for i in idx])


def holdout_chunks(args, dataset):
    if args.holdout_dataset is None:
        return clip_chunks(dataset, args.num, args.num + args.holdout_num, args.chunk)
    other = argparse.Namespace(**dict(vars(args), dataset=args.holdout_dataset))
    return clip_chunks(make_dataset(other), 0, args.holdout_num, args.chunk)


def main(argv=None):
    args = parse_args(argv)
    from model.net import ImageGenerator
    from mocogan_chainer_amd.trainer import load_npz
    from mocogan_chainer_amd.metrics import KnnMetrics
    import mocogan_chainer_amd.hiplib as hl

    gen = ImageGenerator(dim_zl=args.dim_zl, out_channels=args.channel, n_filters=args.n_filters, video_len=args.video_len)
    load_npz(args.model_weight, gen)
    if args.mfma != 'f32':
        gen.impl.set_precision(args.mfma)
    hl.use_pretuned_table()                                              # (sampling never times candidates)
    np.random.seed(args.seed)
    knn = KnnMetrics(args.k, args.pool)
    dataset = make_dataset(args)
    real = knn.descriptors(real_chunks(dataset, args.num, args.chunk))
    holdout = knn.descriptors(holdout_chunks(args, dataset)) if args.holdout_num else None
    fake = knn.descriptors(fake_chunks(gen, args))
    res = knn.report(real, fake, holdout)
    pairs = {key: res.pop(key) for key in ('nn_index', 'nn_dist')}
    if args.dump_pairs:
        np.savez(args.dump_pairs, **pairs)
    out = dict(res, num=args.num, k=args.k, pool=args.pool, holdout_num=args.holdout_num, holdout_dataset=args.holdout_dataset,
               dim=real.dim, nn_dist_median=float(np.median(pairs['nn_dist'])), seed=args.seed, test_mode=args.test_mode,
               model_weight=str(args.model_weight), dataset_type=args.dataset_type)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
