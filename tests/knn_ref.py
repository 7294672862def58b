"""The NumPy statement of the nearest-neighbour metrics (include/mocogan_hip.h: mcg_knn_*; mocogan-chainer_amd/metrics.py:
KnnMetrics), in int64 with the tie rules as the header writes them.  Every figure is an integer until one float64 division."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def descriptors(clips, pool):
    """uint8 (N,T,64,64,C) -> (desc [N][D] int8, norms [N] int64): pool x pool box means rounded half up, minus 128"""
    n, t, h, w, c = clips.shape
    s = clips.astype(np.int64).reshape(n, t, h // pool, pool, w // pool, pool, c).sum(axis=(3, 5))
    q = (2 * s + pool * pool) // (2 * pool * pool)
    desc = (q - 128).reshape(n, -1)
    return desc.astype(np.int8), (desc * desc).sum(axis=1)


def sqdist(a, na, b, nb):
    """out[i][j] = na[i] + nb[j] - 2 a[i].b[j] (the norms are arguments: the kernel does not form them)"""
    return np.asarray(na, np.int64)[:, None] + np.asarray(nb, np.int64)[None, :] - 2 * (a.astype(np.int64) @ b.astype(np.int64).T)


def norms(a):
    return (a.astype(np.int64) ** 2).sum(axis=1)


def self_sqdist(a, b):
    return sqdist(a, norms(a), b, norms(b))


def smallest(dist, k, exclude_self=False, self_col0=0):
    """(val, idx) [M][k]: the k smallest of every row in ascending (value, column) order; row i skips column self_col0 + i with
    exclude_self; missing neighbours are (INT32_MAX, -1)"""
    m, n = dist.shape
    val = np.full((m, k), INT32_MAX, np.int64)
    idx = np.full((m, k), -1, np.int64)
    for i in range(m):
        cols = np.arange(n)
        if exclude_self:
            cols = cols[cols != self_col0 + i]
        order = cols[np.lexsort((cols, dist[i, cols]))][:k]         # (the last key is the primary one)
        val[i, :len(order)], idx[i, :len(order)] = dist[i, order], order
    return val, idx


def ball_counts(dist, radius):
    return (dist <= np.asarray(radius)[None, :]).sum(axis=1)


def radii(x, k):
    """rad[i]: the k-th smallest squared distance from x[i] to the other members of x"""
    return smallest(self_sqdist(x, x), k, exclude_self=True)[0][:, k - 1]


def report(real, fake, k, holdout=None):
    """the dict of KnnMetrics.report from int8 descriptor matrices (R: real / train, F: fake, H: held-out real)"""
    if k > min(len(real), len(fake)) - 1:
        raise ValueError('k <= n - 1 is required of both sets')
    rad_r, rad_f = radii(real, k), radii(fake, k)
    d_fr, d_rf = self_sqdist(fake, real), self_sqdist(real, fake)
    counts_f, counts_r = ball_counts(d_fr, rad_r), ball_counts(d_rf, rad_f)
    nn_dist, nn_index = (v[:, 0] for v in smallest(d_fr, 1))
    out = {'precision': int((counts_f > 0).sum()) / len(fake), 'recall': int((counts_r > 0).sum()) / len(real),
           'density': int(counts_f.sum()) / (k * len(fake)),
           'coverage': int((smallest(d_rf, 1)[0][:, 0] <= rad_r).sum()) / len(real),
           'copy_auc': None, 'nn_index': nn_index, 'nn_dist': nn_dist}
    if holdout is not None:
        d_h = smallest(self_sqdist(holdout, real), 1)[0][:, 0]
        less = int((nn_dist[:, None] < d_h[None, :]).sum())
        equal = int((nn_dist[:, None] == d_h[None, :]).sum())
        out['copy_auc'] = (2 * less + equal) / (2 * len(fake) * len(holdout))
    return out


def blobs(n, seed):
    """n smooth random clips (n,2,64,64,3) uint8: 8 x 8 random colours per frame, each repeated over 8 x 8 pixels, plus noise"""
    g = np.random.RandomState(seed)
    base = g.randint(0, 256, (n, 2, 8, 8, 3)).astype(np.float64).repeat(8, axis=2).repeat(8, axis=3)
    return np.clip(base + g.normal(0, 8, base.shape), 0, 255).astype(np.uint8)
