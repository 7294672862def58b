"""GPU checks of the nearest-neighbour metric kernels (csrc/knn.hip) and of KnnMetrics against tests/knn_ref.py.  Everything is an
integer, so every comparison is np.array_equal.  Every operand and output of a stage call is a view into ONE guard.Arena
(poisoned margins; outputs start as poison), arena.check() follows every call, and inputs are compared with a snapshot.
The lane map of v_mfma_i32_32x32x32_i8 comes first: one-hot rows against an asymmetric matrix."""
import json

import numpy as np
import pytest
import torch

import guard
import knn_ref as kr

pytestmark = pytest.mark.gpu
POISON = np.int32(guard.POISON)
TILE = 128                                                           # SQ_T of csrc/knn.hip: the workgroup's tile edge


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    assert torch.cuda.is_available()
    return hiplib


@pytest.fixture(scope="module")
def _arena():
    return guard.Arena(64 << 20)


@pytest.fixture()
def arena(_arena):
    _arena.reset()
    return _arena


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def host(t):
    return t.cpu().numpy()


def sqdist(hl, arena, a, na, b, nb, pad=0, same=False):
    """mcg_knn_sqdist on arena views -> out [M][N + pad] on the host; inputs checked against their snapshots"""
    da, dna = arena.put(dev(a)), arena.put(dev(np.asarray(na, np.int32)))
    db, dnb = (da, dna) if same else (arena.put(dev(b)), arena.put(dev(np.asarray(nb, np.int32))))
    out = arena.empty((a.shape[0], b.shape[0] + pad), torch.int32)
    hl.knn_sqdist(da, dna, db, dnb, out)
    arena.check()
    assert np.array_equal(host(da), a) and np.array_equal(host(db), b)
    assert np.array_equal(host(dna), na) and np.array_equal(host(dnb), nb)
    return host(out)


# ---- 1. the lane map --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [33, 130])
def test_one_hot_rows_pick_single_elements_of_an_asymmetric_matrix(hl, arena, N):
    """a[i] is one-hot at p_i = i, i < 192 = D: every k mod 64 in each of three 64-byte K-steps, a second row tile.  With zero norms
    out[i][j] = -2 b[j][p_i]: a wrong k pairing, a swapped row / column or a wrong register-to-row map each move elements."""
    D = 192
    a = np.eye(D, dtype=np.int8)
    b = np.random.RandomState(N).randint(-128, 128, (N, D)).astype(np.int8)
    assert not np.array_equal(b[:N, :N], b[:N, :N].T)
    zeros = lambda n: np.zeros(n, np.int32)
    got = sqdist(hl, arena, a, zeros(D), b, zeros(N))
    assert np.array_equal(got, -2 * b.astype(np.int32).T)
    got = sqdist(hl, arena, b, zeros(N), a, zeros(D))                 # the one-hot matrix as the column operand
    assert np.array_equal(got, -2 * b.astype(np.int32))


# ---- 2. squared distances -----------------------------------------------------------------------------------------------------------
def rand_i8(rng, n, D):
    x = rng.randint(-128, 128, (n, D)).astype(np.int8)
    x[0, 0], x[-1, -1] = -128, 127
    return x


@pytest.mark.parametrize("M,N,D", [(1, 2, 64), (2, 1, 128), (31, 33, 192), (33, 31, 64), (TILE - 1, TILE, 128), (TILE, TILE + 1, 192),
                                   (TILE + 1, TILE - 1, 64), (2 * TILE + 1, 1, 128), (2, 2 * TILE + 1, 192), (2 * TILE + 1, TILE + 1, 64),
                                   (33, 33, 32768)])
def test_sqdist_is_exact_at_every_tile_edge(hl, arena, M, N, D):
    """one, two and three K-steps; below, at and above one tile and past two; the longest row.  ld = N + 3: the tail stays poison."""
    rng = np.random.RandomState(M * 1000 + N)
    a, b = rand_i8(rng, M, D), rand_i8(rng, N, D)
    na, nb = kr.norms(a).astype(np.int32), kr.norms(b).astype(np.int32)
    got = sqdist(hl, arena, a, na, b, nb, pad=3)
    assert np.array_equal(got[:, :N], kr.sqdist(a, na, b, nb))
    assert np.array_equal(got[:, N:], np.full((M, 3), POISON))


def test_sqdist_extremes_and_a_set_against_itself(hl, arena):
    D = 32768
    lo, hi = np.full((1, D), -128, np.int8), np.full((2, D), 127, np.int8)
    got = sqdist(hl, arena, lo, kr.norms(lo).astype(np.int32), hi, kr.norms(hi).astype(np.int32))
    assert got.tolist() == [[2130739200, 2130739200]]
    arena.reset()
    x = rand_i8(np.random.RandomState(3), TILE + 2, 128)
    x[5] = x[TILE + 1]                                                # a duplicate: an exact zero off the diagonal
    nx = kr.norms(x).astype(np.int32)
    got = sqdist(hl, arena, x, nx, x, nx, same=True)
    assert np.array_equal(got, kr.self_sqdist(x, x)) and np.array_equal(got, got.T)
    assert not np.diag(got).any() and got[5, TILE + 1] == 0


# ---- 3. descriptors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,C,pool", [(3, 2, 1, 8), (2, 1, 3, 8), (2, 2, 3, 4), (1, 1, 1, 2)])
def test_descriptors_and_norms(hl, arena, N, T, C, pool):
    """random bytes with boxes of all 0, all 255 and sums that hit the rounding half exactly"""
    rng = np.random.RandomState(N * 100 + T * 10 + C + pool)
    clips = rng.randint(0, 256, (N, T, 64, 64, C)).astype(np.uint8)
    clips[0, 0, :pool, :pool, 0] = 0
    clips[0, 0, :pool, pool:2 * pool, 0] = 255
    half = np.zeros(pool * pool, np.uint8)
    half[:pool * pool // 2] = 1                                       # sum pool^2 / 2: a mean of exactly 0.5 -> 1
    clips[-1, -1, -pool:, -pool:, C - 1] = half.reshape(pool, pool)
    half[:pool * pool // 2] = 255                                     # 127.5 -> 128
    clips[-1, -1, -pool:, -2 * pool:-pool, C - 1] = half.reshape(pool, pool)
    u8 = arena.put(dev(clips))
    S = 64 // pool
    desc, norms = arena.empty((N, T * S * S * C), torch.int8), arena.empty((N,), torch.int32)
    hl.knn_descriptors(u8, pool, desc, norms)
    arena.check()
    assert np.array_equal(host(u8), clips)
    rd, rn = kr.descriptors(clips, pool)
    assert rd[0, 0] == -128 and rd[0, C] == 127 and rd[-1, -1] == 1 - 128 and rd[-1, -1 - C] == 0
    assert np.array_equal(host(desc), rd) and np.array_equal(host(norms), rn)


# ---- 4. the k smallest ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_smallest_with_ties_sentinels_and_excluded_diagonals(hl, arena, N, k):
    """M = 9 rows (a third, ragged block of four waves), ld = N + 2.  Values from an alphabet of 4: ties across lanes and within a
    lane in every row; one row all equal, one holding INT32_MAX itself and INT32_MIN.  exclude_self at self_col0 = 0 and 7;
    k > N (and k > N - 1 with the diagonal left out) gives the sentinels."""
    M = 9
    rng = np.random.RandomState(N * 100 + k)
    dist = rng.randint(0, 4, (M, N + 2)).astype(np.int32)
    dist[1] = 7
    dist[2, ::3] = kr.INT32_MAX
    dist[2, N // 2] = -2 ** 31
    dist[:, N:] = -5                                                  # beyond N, inside the stride: must not be seen
    d = arena.put(dev(dist))
    for ex, c0 in ((False, 0), (True, 0), (True, 7)):
        val, idx = arena.empty((M, k), torch.int32), arena.empty((M, k), torch.int32)
        hl.knn_smallest(d, k, n=N, exclude_self=ex, self_col0=c0, val=val, idx=idx)
        arena.check()
        rv, ri = kr.smallest(dist[:, :N].astype(np.int64), k, ex, c0)
        assert np.array_equal(host(val), rv) and np.array_equal(host(idx), ri), (ex, c0)
        if k > N:
            assert (host(val)[:, N:] == kr.INT32_MAX).all() and (host(idx)[:, N:] == -1).all()
    assert np.array_equal(host(d), dist)


# ---- 5. counts inside per-column radii --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(1, 1), (5, 63), (9, 200)])
def test_ball_counts_at_the_edge_of_the_radius(hl, arena, M, N):
    rng = np.random.RandomState(M + N)
    dist = rng.randint(0, 50, (M, N + 1)).astype(np.int32)
    radius = rng.randint(0, 50, N).astype(np.int32)
    radius[0] = 0
    radius[N // 2] = kr.INT32_MAX
    dist[0, N // 2] = kr.INT32_MAX
    dist[-1, :N] = radius                                             # exactly a distance: <= counts it
    if N > 4:
        dist[1, :N] = radius.astype(np.int64).clip(None, kr.INT32_MAX - 1) + 1    # one above: not counted
        dist[1, N // 2] = kr.INT32_MAX
    dist[:, N] = -9                                                   # beyond N, inside the stride
    d, r = arena.put(dev(dist)), arena.put(dev(radius))
    counts = arena.empty((M,), torch.int32)
    hl.knn_ball_counts(d, r, n=N, counts=counts)
    arena.check()
    assert np.array_equal(host(d), dist) and np.array_equal(host(r), radius)
    ref = kr.ball_counts(dist[:, :N].astype(np.int64), radius)
    assert ref[-1] == N and (M == 1 or N <= 4 or ref[1] == 1)
    assert np.array_equal(host(counts), ref)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------
K, POOL = 3, 8


@pytest.fixture(scope="module")
def blob_sets():
    T, H, F = kr.blobs(48, 1), kr.blobs(32, 2), kr.blobs(40, 3)
    d = lambda c: kr.descriptors(c, POOL)[0]
    return (T, F, H), kr.report(d(T), d(F), K, d(H))


def same_report(got, ref):
    assert set(got) == set(ref) == {'precision', 'recall', 'density', 'coverage', 'copy_auc', 'nn_index', 'nn_dist'}
    for key in ref:
        if key.startswith('nn_'):
            assert np.array_equal(got[key], ref[key]), key
        else:
            assert got[key] == ref[key], (key, got[key], ref[key])


@pytest.mark.parametrize("row_block", [7, 4096])
def test_report_equals_the_reference(hl, blob_sets, row_block):
    from mocogan_chainer_amd.metrics import KnnMetrics
    (T, F, H), ref = blob_sets
    knn = KnnMetrics(K, POOL, row_block)
    real, fake, hold = (knn.descriptors([c]) for c in (T, F, H))
    assert np.array_equal(host(real.desc), kr.descriptors(T, POOL)[0]) and np.array_equal(host(real.norms), kr.descriptors(T, POOL)[1])
    got = knn.report(real, fake, hold)
    print({k: v for k, v in got.items() if not k.startswith('nn_')})
    same_report(got, ref)
    assert 0.4 <= got['copy_auc'] <= 0.6
    same_report(knn.report(real, fake), dict(ref, copy_auc=None))
    with pytest.raises(ValueError):
        KnnMetrics(16, POOL).report(real, knn.descriptors([F[:16]]))  # k <= n - 1 of both sets


def test_report_does_not_depend_on_the_chunking(hl, blob_sets):
    from mocogan_chainer_amd.metrics import KnnMetrics
    (T, F, H), ref = blob_sets
    knn = KnnMetrics(K, POOL)
    chunked = lambda x, n: [x[i:i + n] for i in range(0, len(x), n)]
    whole = knn.descriptors([T])
    for n in (1, 5, len(T)):
        real, fake = knn.descriptors(chunked(T, n)), knn.descriptors(iter(chunked(dev(F), n)))       # host arrays; device tensors
        assert torch.equal(real.desc, whole.desc) and torch.equal(real.norms, whole.norms) and real.n == 48 and real.dim == 384
        same_report(knn.report(real, fake), dict(ref, copy_auc=None))


# ---- 7. the entry point ----------------------------------------------------------------------------------------------------------------
def test_cli_on_the_synthetic_dataset_with_a_fresh_generator(hl, tmp_path, capsys):
    import evaluate_knn
    from model.net import ImageGenerator
    from mocogan_chainer_amd import trainer
    np.random.seed(4)
    gen = ImageGenerator(n_filters=8, video_len=4)
    path, pairs = tmp_path / 'image_gen_ema_epoch_1.npz', tmp_path / 'pairs.npz'
    trainer.save_npz(path, gen)
    argv = [str(path), '--dataset_type', 'synthetic', '--synthetic_size', '16', '--num', '8', '--k', '3', '--pool', '8', '--n_filters', '8',
            '--video_len', '4', '--chunk', '3', '--seed', '2', '--holdout_num', '4', '--dump_pairs', str(pairs)]
    res = evaluate_knn.main(argv)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
    assert len(line) == 1 and json.loads(line[0]) == res             # one JSON line
    print("evaluate_knn:", line[0])
    for key in ('precision', 'recall', 'density', 'coverage', 'copy_auc'):
        assert 0.0 <= res[key] and np.isfinite(res[key]), key
    assert max(res['precision'], res['recall'], res['coverage'], res['copy_auc']) <= 1.0
    assert (res['num'], res['k'], res['pool'], res['holdout_num'], res['dim']) == (8, 3, 8, 4, 4 * 8 * 8 * 3)
    dumped = np.load(pairs)
    assert dumped['nn_index'].shape == dumped['nn_dist'].shape == (8,) and ((0 <= dumped['nn_index']) & (dumped['nn_index'] < 8)).all()
    assert res['nn_dist_median'] == float(np.median(dumped['nn_dist']))
    again = evaluate_knn.main(argv[:-4])                              # the same run without the hold-out: the same numbers
    assert again['copy_auc'] is None and all(again[k] == res[k] for k in ('precision', 'recall', 'density', 'coverage', 'nn_dist_median'))
