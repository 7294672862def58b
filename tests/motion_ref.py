"""The NumPy statement of the motion and content metrics (include/mocogan_hip.h: mcg_mc_*; mocogan-chainer_amd/metrics.py:
MotionContent), in int64 / float64.  Every figure is an integer until one float64 expression, written here as metrics.py writes it;
pair_sum alone is a sum of square roots, added in the order the header fixes."""
import math

import numpy as np

import knn_ref as kr


def frame_sqdist(x):
    """int8 x [N][T][Df] -> int64 [N][T][T]: dist[n][s][t] = sum_d (x[n][s][d] - x[n][t][d])^2, through the Gram matrix"""
    x = x.astype(np.int64)
    g = x @ x.transpose(0, 2, 1)
    nrm = np.diagonal(g, axis1=1, axis2=2)
    return nrm[:, :, None] + nrm[:, None, :] - 2 * g


def pair_sum(dist):
    """[n]: sum over s < t of sqrt(dist[n][s][t]), one float64 chain per clip, s ascending, then t ascending"""
    out = np.zeros(len(dist), np.float64)
    T = dist.shape[1]
    for n, d in enumerate(dist):
        acc = 0.0
        for s in range(T):
            for t in range(s + 1, T):
                acc += math.sqrt(int(d[s, t]))
        out[n] = acc
    return out


def lag_sum(dist):
    """[n][l] = sum_t dist[n][t][t + l], l = 0 .. T - 1"""
    T = dist.shape[1]
    return np.stack([np.diagonal(dist.astype(np.int64), l, 1, 2).sum(axis=1) for l in range(T)], axis=1)


def motion_descriptors(x):
    """int8 x [N][T][Df] -> (mdesc [N][(T-1) Df] int8, mnorms [N] int64): floor((x[t+1] - x[t]) / 2) and the rows' sums of squares"""
    x = x.astype(np.int64)
    m = ((x[:, 1:] - x[:, :-1]) >> 1).reshape(len(x), -1)
    assert m.min(initial=0) >= -128 and m.max(initial=0) <= 127
    return m.astype(np.int8), (m * m).sum(axis=1)


def clip_set(clips, pool):
    """uint8 clips (N,T,64,64,C) -> what MotionContent.clip_set keeps, as host arrays"""
    n, T = clips.shape[:2]
    desc = kr.descriptors(clips, pool)[0]
    return frame_set(desc.reshape(n, T, -1))


def frame_set(x):
    """the same from per-frame descriptors x [N][T][Df] int8"""
    n, T, Df = x.shape
    dist = frame_sqdist(x)
    mdesc, mnorms = motion_descriptors(x)
    return {'n': n, 'frames': T, 'frame_dim': Df, 'desc': x.reshape(n, -1), 'dist': dist, 'pair_sum': pair_sum(dist), 'lag_sum': lag_sum(dist),
            'mdesc': mdesc, 'mnorms': mnorms}


def summary(s):
    n, T, Df = s['n'], s['frames'], s['frame_dim']
    P = T * (T - 1) // 2
    lag_tot = s['lag_sum'].astype(np.int64).sum(axis=0)
    return {'acd': float(np.mean(s['pair_sum'])) / (P * math.sqrt(Df)),
            'lag': [math.sqrt(int(lag_tot[l]) / (n * (T - l) * Df)) for l in range(1, T)],
            'lag1_q': [float(v) for v in np.quantile(np.sqrt(s['lag_sum'][:, 1].astype(np.int64) / ((T - 1) * Df)), [0.05, 0.5, 0.95])]}


def report(real, fake, k):
    if (real['frames'], real['frame_dim']) != (fake['frames'], fake['frame_dim']):
        raise ValueError('the sets differ in frames or descriptor size')
    sr, sf = summary(real), summary(fake)
    motion = kr.report(real['mdesc'], fake['mdesc'], k)
    out = {'real': sr, 'fake': sf, 'acd_ratio': sf['acd'] / sr['acd'] if sr['acd'] != 0 else None,
           'lag_l1': float(np.mean(np.abs(np.asarray(sf['lag']) - np.asarray(sr['lag']))))}
    out.update({'motion_' + key: motion[key] for key in ('precision', 'recall', 'density', 'coverage')})
    return out


def class_means(dist, K):
    """the means of a K^2 x K^2 matrix (clip c K + m: content c, motion m) over the ordered pairs of three classes"""
    idx = np.arange(K * K)
    c, m = idx // K, idx % K
    same_c, same_m = c[:, None] == c[None, :], m[:, None] == m[None, :]
    masks = {'same_content': same_c & ~same_m, 'same_motion': ~same_c & same_m, 'neither': ~same_c & ~same_m}
    return {key: int(dist[mask].astype(np.int64).sum()) / int(mask.sum()) for key, mask in masks.items()}


def grid_report(s, K):
    if s['n'] != K * K:
        raise ValueError('a K x K grid holds K^2 clips')
    app_dist, mot_dist = kr.self_sqdist(s['desc'], s['desc']), kr.self_sqdist(s['mdesc'], s['mdesc'])
    app, mot = class_means(app_dist, K), class_means(mot_dist, K)
    ratio = lambda a, b: a / b if b != 0 else None
    return {'content_ratio': ratio(app['same_content'], app['neither']), 'motion_leak': ratio(app['same_motion'], app['neither']),
            'motion_ratio': ratio(mot['same_motion'], mot['neither']), 'content_leak': ratio(mot['same_content'], mot['neither']),
            'appearance_means': app, 'motion_means': mot, 'appearance_dist': app_dist, 'motion_dist': mot_dist}


def planted_grid(K, seed, T=8, size=16, C=1):
    """K^2 byte clips (K K, T, size, size, C) in content-major order: content = a random static background in 0..191, motion = a
    3 x 3 blob of 255 on a random walk (steps of -1, 0, 1 per axis, kept inside the frame)"""
    g = np.random.RandomState(seed)
    back = g.randint(0, 192, (K, size, size, C)).astype(np.uint8)
    paths = np.zeros((K, T, 2), np.int64)
    for m in range(K):
        pos = g.randint(0, size - 2, 2)
        for t in range(T):
            paths[m, t] = pos
            pos = np.clip(pos + g.randint(-1, 2, 2), 0, size - 3)
    clips = np.zeros((K, K, T, size, size, C), np.uint8)
    for c in range(K):
        for m in range(K):
            for t in range(T):
                clips[c, m, t] = back[c]
                y, x = paths[m, t]
                clips[c, m, t, y:y + 3, x:x + 3] = 255
    return clips.reshape(K * K, T, size, size, C)


def upscale(clips, f):
    """every pixel repeated over f x f: (N,T,h,w,C) -> (N,T,f h,f w,C); a pool of f gives back the pixels"""
    return clips.repeat(f, axis=2).repeat(f, axis=3)


def byte_frames(clips):
    """small uint8 clips (N,T,h,w,C) as per-frame int8 descriptors [N][T][h w C] (value - 128), as a pool of 1 would give"""
    n, T = clips.shape[:2]
    return (clips.astype(np.int64) - 128).reshape(n, T, -1).astype(np.int8)
