"""CPU checks of the nearest-neighbour metrics: tests/knn_ref.py (the NumPy statement the GPU tests compare with) against
brute-force loops, the int32 extreme, what the figures say on sets whose relation is known, the command line of evaluate_knn.py,
and the mcg_knn_* entry points' refusals on the host (the library cross-compiles and loads without a GPU)."""
import ctypes

import numpy as np
import pytest

import knn_ref as kr


# ---- the reference against loops -------------------------------------------------------------------------------------------------
def brute_smallest(dist, k, exclude_self, self_col0):
    val, idx = [], []
    for i, row in enumerate(dist):
        cand = sorted((int(v), j) for j, v in enumerate(row) if not (exclude_self and j == self_col0 + i))[:k]
        cand += [(kr.INT32_MAX, -1)] * (k - len(cand))
        val.append([v for v, _ in cand])
        idx.append([j for _, j in cand])
    return np.array(val), np.array(idx)


def test_descriptor_rounds_half_up_and_orders_rows_as_the_header_says():
    rng = np.random.RandomState(0)
    clips = rng.randint(0, 256, (2, 2, 64, 64, 3)).astype(np.uint8)
    clips[0, 0, :2, :2, 0] = [[1, 0], [1, 0]]                        # sum 2 over 4: mean 0.5 -> 1
    clips[0, 0, :2, 2:4, 0] = [[1, 0], [0, 0]]                       # mean 0.25 -> 0
    clips[1, 1, 62:, 62:, 2] = 255
    for pool in (2, 4, 8):
        desc, norms = kr.descriptors(clips, pool)
        S = 64 // pool
        assert desc.shape == (2, 2 * S * S * 3) and desc.dtype == np.int8 and desc.shape[1] % 64 == 0
        for n, t, y, x, c in [(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (1, 1, S - 1, S - 1, 2), (1, 0, 3, 5, 1)]:
            s = sum(int(clips[n, t, y * pool + dy, x * pool + dx, c]) for dy in range(pool) for dx in range(pool))
            q = int(np.floor(s / (pool * pool) + 0.5))               # round half up (s / pool^2 is exact in binary)
            assert desc[n, ((t * S + y) * S + x) * 3 + c] == q - 128
        assert [int(v) for v in norms] == [sum(int(v) ** 2 for v in row) for row in desc]
    d2 = kr.descriptors(clips, 2)[0]
    assert d2[0, 0] == 1 - 128 and d2[0, 3] == 0 - 128 and d2[1, -1] == 127


def test_reference_matches_brute_force_with_ties_and_short_rows():
    rng = np.random.RandomState(1)
    a, b = rng.randint(-128, 128, (7, 64)).astype(np.int8), rng.randint(-128, 128, (5, 64)).astype(np.int8)
    dist = kr.self_sqdist(a, b)
    for i in range(7):
        for j in range(5):
            assert dist[i, j] == sum((int(a[i, d]) - int(b[j, d])) ** 2 for d in range(64))
    ties = rng.randint(0, 3, (6, 9)).astype(np.int64)                 # three values over nine columns: ties in every row
    for k in (1, 3, 9, 12):                                           # 12 > the 9 (8 with exclude_self) candidates
        for ex, c0 in ((False, 0), (True, 0), (True, 2), (True, 7)):
            val, idx = kr.smallest(ties, k, ex, c0)
            bv, bi = brute_smallest(ties, k, ex, c0)
            assert np.array_equal(val, bv) and np.array_equal(idx, bi), (k, ex, c0)
    assert kr.smallest(ties, 12)[0][0, -1] == kr.INT32_MAX and kr.smallest(ties, 12)[1][0, -1] == -1
    radius = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2])
    assert list(kr.ball_counts(ties, radius)) == [sum(1 for j in range(9) if ties[i, j] <= radius[j]) for i in range(6)]


def test_reference_report_matches_loops():
    rng = np.random.RandomState(2)
    R, F, H = (rng.randint(-3, 4, (n, 64)).astype(np.int8) for n in (9, 7, 6))       # a small alphabet: equal distances occur
    k = 2
    d = lambda x, y: int(((x.astype(np.int64) - y.astype(np.int64)) ** 2).sum())
    rad = lambda X: [sorted(d(X[i], X[j]) for j in range(len(X)) if j != i)[k - 1] for i in range(len(X))]
    rad_r, rad_f = rad(R), rad(F)
    counts_f = [sum(d(f, R[j]) <= rad_r[j] for j in range(len(R))) for f in F]
    counts_r = [sum(d(r, F[j]) <= rad_f[j] for j in range(len(F))) for r in R]
    dF = [min(d(f, r) for r in R) for f in F]
    dH = [min(d(h, r) for r in R) for h in H]
    got = kr.report(R, F, k, H)
    assert got['precision'] == sum(c > 0 for c in counts_f) / 7 and got['recall'] == sum(c > 0 for c in counts_r) / 9
    assert got['density'] == sum(counts_f) / (k * 7)
    assert got['coverage'] == sum(min(d(r, f) for f in F) <= rad_r[i] for i, r in enumerate(R)) / 9
    assert got['copy_auc'] == sum(1.0 if x < y else 0.5 if x == y else 0.0 for x in dF for y in dH) / (7 * 6)
    assert list(got['nn_dist']) == dF and all(d(F[i], R[j]) == dF[i] for i, j in enumerate(got['nn_index']))
    assert kr.report(R, F, k)['copy_auc'] is None
    with pytest.raises(ValueError):
        kr.report(R, F, 7)                                             # k <= n - 1 of both sets: F has 7


def test_extreme_distance_fits_int32():
    lo, hi = np.full((1, 32768), -128, np.int8), np.full((1, 32768), 127, np.int8)
    assert int(kr.self_sqdist(lo, hi)[0, 0]) == 2130739200 == 255 ** 2 * 32768 < kr.INT32_MAX
    assert int(kr.norms(lo)[0]) == 2 ** 29 and abs(int(lo.astype(np.int64)[0] @ hi.astype(np.int64)[0])) < 2 ** 29


# ---- what the figures say ----------------------------------------------------------------------------------------------------------
K, POOL = 3, 8


def desc(clips):
    return kr.descriptors(clips, POOL)[0]


@pytest.fixture(scope="module")
def sets():
    return {'T': kr.blobs(48, 1), 'H': kr.blobs(32, 2), 'F': kr.blobs(40, 3)}


def test_fresh_samples_lie_as_far_from_the_training_set_as_held_out_ones(sets):
    """measured with this reference: copy_auc 0.4992, precision 0.725, coverage 0.6875; the band only has to separate from 1.0"""
    r = kr.report(desc(sets['T']), desc(sets['F']), K, desc(sets['H']))
    print({k: v for k, v in r.items() if not k.startswith('nn_')})
    assert 0.4 <= r['copy_auc'] <= 0.6
    assert 0 < r['precision'] < 1 and 0 < r['coverage'] < 1


def test_noisy_copies_of_training_clips_score_one(sets):
    T = sets['T']
    F = np.clip(T[:40].astype(np.int64) + np.random.RandomState(5).randint(-2, 3, T[:40].shape), 0, 255).astype(np.uint8)
    r = kr.report(desc(T), desc(F), K, desc(sets['H']))
    assert r['precision'] == 1.0 and r['coverage'] == 1.0 and r['copy_auc'] == 1.0
    assert list(r['nn_index']) == list(range(40))                      # every copy finds its original


def test_the_training_set_itself_scores_one_everywhere(sets):
    T = desc(sets['T'])
    r = kr.report(T, T, K, desc(sets['H']))
    assert r['precision'] == r['recall'] == r['coverage'] == r['copy_auc'] == 1.0
    assert list(r['nn_index']) == list(range(48)) and not r['nn_dist'].any()


def test_disjoint_sets_score_zero_everywhere():
    F, T = (255 - kr.blobs(40, 7) // 4).astype(np.uint8), (kr.blobs(48, 8) // 4).astype(np.uint8)
    r = kr.report(desc(T), desc(F), K, desc((kr.blobs(32, 2) // 4).astype(np.uint8)))
    assert r['precision'] == r['recall'] == r['density'] == r['coverage'] == r['copy_auc'] == 0.0


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_parses_and_validates():
    import evaluate_knn as ev
    a = ev.parse_args(['g.npz'])
    assert (a.num, a.k, a.pool, a.holdout_num, a.holdout_dataset, a.dump_pairs, a.seed, a.test_mode) == (1024, 5, 4, 0, None, None, 0, 1)
    assert (a.dataset_type, a.dataset, a.synthetic_size, a.mfma, a.labels, a.chunk, a.video_len, a.channel) == \
        ('mug', 'data/dataset/train', 256, 'f32', None, 64, 16, 3)
    a = ev.parse_args(['g.npz', '--dataset_type', 'synthetic', '--synthetic_size', '32', '--num', '8', '--k', '3', '--pool', '8',
                       '--holdout_num', '4', '--dump_pairs', 'p.npz', '--mfma', 'f32x3', '--test_mode', '0', '--n_filters', '8'])
    assert (a.dataset_type, a.synthetic_size, a.num, a.k, a.pool, a.holdout_num, a.dump_pairs, a.mfma, a.test_mode) == \
        ('synthetic', 32, 8, 3, 8, 4, 'p.npz', 'f32x3', 0)
    assert ev.parse_args(['g.npz', '--holdout_num', '9', '--holdout_dataset', 'data/dataset/test']).holdout_dataset == 'data/dataset/test'
    assert ev.parse_args(['g.npz', '--pool', '2', '--video_len', '8']).pool == 2            # 8 * 32^2 * 3 = 24576
    assert ev.parse_args(['g.npz', '--pool', '2', '--channel', '1']).pool == 2              # 16 * 32^2 = 16384
    for bad in (['g.npz', '--num', '0'], ['g.npz', '--k', '0'], ['g.npz', '--k', '17'], ['g.npz', '--num', '5', '--k', '5'],
                ['g.npz', '--pool', '3'], ['g.npz', '--pool', '16'], ['g.npz', '--pool', '2'], ['g.npz', '--holdout_num', '-1'],
                ['g.npz', '--holdout_dataset', 'd'], ['g.npz', '--dataset_type', 'synthetic', '--holdout_num', '4', '--holdout_dataset', 'd'],
                ['g.npz', '--channel', '2'], ['g.npz', '--labels', '1'], ['--num', '4'], ['g.npz', '--mfma', 'fp8'], ['g.npz', '--chunk', '0']):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    text = ' '.join(ev.build_parser().format_help().split())
    assert 'training never saw' in text and "user's responsibility" in text
    ds = ev.make_dataset(ev.parse_args(['g.npz', '--dataset_type', 'synthetic', '--synthetic_size', '7', '--channel', '1', '--video_len', '4']))
    chunks = list(ev.clip_chunks(ds, 3, 7, 3))
    assert [c.shape for c in chunks] == [(3, 4, 64, 64, 1), (1, 4, 64, 64, 1)] and chunks[0].dtype == np.uint8
    assert np.array_equal(np.concatenate(chunks), np.concatenate(list(ev.real_chunks(ds, 7, 7)))[3:])
    with pytest.raises(ValueError):
        list(ev.clip_chunks(ds, 3, 8, 3))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def test_knn_entry_points_refuse_on_the_host(hl):
    """A null pointer, a non-positive extent, ld < N, a k outside 1..16 (and what the header adds: a pool outside {2, 4, 8}, C outside
    1..3, a D that is no multiple of 64, a misaligned operand) are refused before anything is launched.  `one` is a non-null,
    16-byte aligned pointer that is never dereferenced, the outputs are small host buffers that must come back untouched; no call
    below passes an acceptable argument set."""
    lib = hl.load()
    one = ctypes.c_void_p(16)
    BAD, UNSUPPORTED = -1, -2
    bufs = [(ctypes.c_int32 * 16)(*([3] * 16)) for _ in range(2)]
    o1, o2 = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    calls = []

    def refused(code, rc, *what):
        calls.append(what)
        assert rc == code, (what, rc)
        assert all(list(b) == [3] * 16 for b in bufs), what

    descr = lambda N, C, T, H, W, pool, clips=one, desc=o1, norms=o2: lib.mcg_knn_descriptors(N, C, T, H, W, pool, clips, desc, norms, None)
    for ext in ((0, 3, 2, 64, 64, 8), (-1, 3, 2, 64, 64, 8), (2, 0, 2, 64, 64, 8), (2, 4, 2, 64, 64, 8), (2, 3, 0, 64, 64, 8), (2, 3, -2, 64, 64, 8),
                (2, 3, 2, 0, 64, 8), (2, 3, 2, 64, 0, 8), (2, 3, 2, 64, 64, 0), (2, 3, 2, 64, 64, 3), (2, 3, 2, 64, 64, 16), (2, 3, 2, 64, 64, -4)):
        refused(BAD, descr(*ext), "mcg_knn_descriptors", ext)
    for hole in ('clips', 'desc', 'norms'):
        refused(BAD, descr(2, 3, 2, 64, 64, 8, **{hole: None}), "mcg_knn_descriptors", "no " + hole)
    refused(UNSUPPORTED, descr(2, 3, 2, 32, 32, 8), "mcg_knn_descriptors", "32 x 32 frames")
    refused(UNSUPPORTED, descr(2, 3, 2, 64, 128, 8), "mcg_knn_descriptors", "64 x 128 frames")
    refused(UNSUPPORTED, descr(2, 3, 16, 64, 64, 2), "mcg_knn_descriptors", "D = 49152")
    refused(UNSUPPORTED, descr(2, 1, 33, 64, 64, 2), "mcg_knn_descriptors", "D = 33792")

    def sq(M, N, D, ld, a=one, na=one, b=one, nb=one, out=o1):
        return lib.mcg_knn_sqdist(M, N, D, a, na, b, nb, out, ld, None)
    for ext in ((0, 4, 64, 4), (4, 0, 64, 4), (4, 4, 0, 4), (-4, 4, 64, 4), (4, -4, 64, 4), (4, 4, -64, 4)):
        refused(BAD, sq(*ext), "mcg_knn_sqdist", ext)
    refused(BAD, sq(4, 4, 64, 3), "mcg_knn_sqdist", "ld < N")
    refused(BAD, sq(4, 4, 64, 0), "mcg_knn_sqdist", "ld = 0")
    for D in (1, 32, 63, 65, 96, 32767):
        refused(BAD, sq(4, 4, D, 4), "mcg_knn_sqdist", "D no multiple of 64", D)
    refused(UNSUPPORTED, sq(4, 4, 32768 + 64, 4), "mcg_knn_sqdist", "D > 32768")
    for hole in ('a', 'na', 'b', 'nb', 'out'):
        refused(BAD, sq(4, 4, 64, 4, **{hole: None}), "mcg_knn_sqdist", "no " + hole)
    refused(BAD, sq(4, 4, 64, 4, a=ctypes.c_void_p(24)), "mcg_knn_sqdist", "a not 16-byte aligned")
    refused(BAD, sq(4, 4, 64, 4, b=ctypes.c_void_p(20)), "mcg_knn_sqdist", "b not 16-byte aligned")

    def small(M, N, ld, k, dist=one, val=o1, idx=o2):
        return lib.mcg_knn_smallest(M, N, dist, ld, k, 1, 0, val, idx, None)
    for ext in ((0, 4, 4, 1), (4, 0, 4, 1), (-1, 4, 4, 1), (4, -1, 4, 1)):
        refused(BAD, small(*ext), "mcg_knn_smallest", ext)
    refused(BAD, small(4, 4, 3, 1), "mcg_knn_smallest", "ld < N")
    for k in (0, -1, 17, 64):
        refused(BAD, small(4, 4, 4, k), "mcg_knn_smallest", "k", k)
    for hole in ('dist', 'val', 'idx'):
        refused(BAD, small(4, 4, 4, 2, **{hole: None}), "mcg_knn_smallest", "no " + hole)

    def ball(M, N, ld, dist=one, radius=one, counts=o1):
        return lib.mcg_knn_ball_counts(M, N, dist, ld, radius, counts, None)
    for ext in ((0, 4, 4), (4, 0, 4), (-1, 4, 4), (4, -1, 4)):
        refused(BAD, ball(*ext), "mcg_knn_ball_counts", ext)
    refused(BAD, ball(4, 4, 3), "mcg_knn_ball_counts", "ld < N")
    for hole in ('dist', 'radius', 'counts'):
        refused(BAD, ball(4, 4, 4, **{hole: None}), "mcg_knn_ball_counts", "no " + hole)
    assert len(calls) > 60


def test_knn_wrappers_refuse_host_tensors_and_misfits(hl):
    import torch
    from mocogan_chainer_amd.metrics import KnnMetrics
    with pytest.raises(hl.McgError):
        hl.knn_descriptors(torch.zeros(1, 1, 64, 64, 1, dtype=torch.uint8), 8)            # a host tensor
    with pytest.raises(hl.McgError):
        hl.knn_descriptors(torch.zeros(1, 1, 64, 64, 1, dtype=torch.uint8), 3)
    with pytest.raises(hl.McgError):
        hl.knn_sqdist(torch.zeros(2, 64, dtype=torch.int8), torch.zeros(2, dtype=torch.int32), torch.zeros(3, 128, dtype=torch.int8),
                      torch.zeros(3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32))
    for kwargs in ({'k': 0}, {'k': 17}, {'pool': 3}, {'row_block': 0}):
        with pytest.raises(ValueError):
            KnnMetrics(device='cpu', **kwargs)
    knn = KnnMetrics(k=3, pool=2, device='cpu')
    with pytest.raises(ValueError):
        knn.descriptors([np.zeros((1, 16, 64, 64, 3), np.uint8)])                         # D = 49152 at pool 2
    with pytest.raises(ValueError):
        knn.descriptors([np.zeros((1, 2, 32, 32, 3), np.uint8)])
    with pytest.raises(ValueError):
        knn.descriptors([])
