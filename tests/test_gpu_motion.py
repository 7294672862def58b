"""GPU checks of the motion and content kernels (csrc/motion.hip) and of MotionContent against tests/motion_ref.py.  Every operand
and output of a stage call is a view into ONE guard.Arena (poisoned margins; outputs start as poison), arena.check() follows every
call, and inputs are compared with a snapshot.  Integer outputs are compared with np.array_equal.  The lane map of
v_mfma_i32_16x16x64_i8 comes first: one-hot frames against random ones."""
import json
import math

import numpy as np
import pytest
import torch

import guard
import knn_ref as kr
import motion_ref as mr

pytestmark = pytest.mark.gpu
WAVES = 4                                                            # MC_WAVES of csrc/motion.hip: clips per workgroup (one per wave)
MAX_DIST = 199756800                                                 # 255^2 * 3072


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


def frame_sqdist(hl, arena, x):
    """mcg_mc_frame_sqdist on arena views -> dist [N][T][T] on the host; the input checked against its snapshot"""
    d = arena.put(dev(x))
    out = arena.empty((x.shape[0], x.shape[1], x.shape[1]), torch.int32)
    hl.mc_frame_sqdist(d, out)
    arena.check()
    assert np.array_equal(host(d), x)
    return host(out)


def rand_i8(rng, *shape):
    x = rng.randint(-128, 128, shape).astype(np.int8)
    x.reshape(-1)[0], x.reshape(-1)[-1] = -128, 127
    return x


# ---- 1. the lane map --------------------------------------------------------------------------------------------------------------
PLACE = {'ascending': lambda n, s: 8 * n + s, 'strided': lambda n, s: 24 * s + n, 'descending': lambda n, s: 191 - 8 * n - s}


@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("place", sorted(PLACE))
def test_one_hot_frames_pick_single_elements_of_random_frames(hl, arena, place, upper):
    """T = 16 (one MFMA tile), Df = 192 (three K-steps), 24 clips.  Eight frames of clip n are one-hot (value 1) at p(n, s): over the
    clips every k of 0..191 -- every k mod 64 in each K-step -- is hit, at a lane / step that depends on the placement.  The other
    eight are random int8 with -128 and 127 planted.  dist[s][t] = 1 + |b_t|^2 - 2 b_t[p_s] between a one-hot frame s and a random
    frame t: a wrong k pairing or register-to-row map moves elements.  Then the one-hot frames in the upper half of the tile."""
    N, T, Df = 24, 16, 192
    rng = np.random.RandomState(len(place) + upper)
    x = rand_i8(rng, N, T, Df)
    hot, rnd = (range(8, 16), range(0, 8)) if upper else (range(0, 8), range(8, 16))
    pos = np.array([[PLACE[place](n, s) for s in range(8)] for n in range(N)])
    assert sorted(pos.reshape(-1)) == list(range(Df))
    for n in range(N):
        for s, f in enumerate(hot):
            x[n, f] = 0
            x[n, f, pos[n, s]] = 1
    x[0, rnd[0], 0], x[-1, rnd[-1], -1] = -128, 127
    got = frame_sqdist(hl, arena, x)
    x64 = x.astype(np.int64)
    for n in range(N):
        for s, f in enumerate(hot):
            for t in rnd:
                want = 1 + int((x64[n, t] ** 2).sum()) - 2 * int(x64[n, t, pos[n, s]])
                assert got[n, f, t] == want == got[n, t, f], (n, f, t)
    assert np.array_equal(got, mr.frame_sqdist(x))


# ---- 2. frame distances -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,Df", [(1, 2, 64), (3, 3, 128), (4, 15, 192), (5, 16, 768), (9, 17, 64), (3, 17, 128), (5, 17, 192), (4, 17, 768),
                                    (2, 17, 3072), (5, 31, 64), (3, 32, 128), (5, 33, 192), (4, 48, 64), (5, 64, 128), (2, 64, 3072)])
def test_frame_sqdist_is_exact_at_every_edge(hl, arena, N, T, Df):
    """one to four row tiles with ragged and full last tiles; one, two, three K-steps, three unrolled groups of four and twelve;
    N below, at and above the WAVES = 4 clips of a workgroup and past two workgroups (the grid is ceil(N / 4) in x alone: no cap,
    no stride).  desc lies between poisoned margins and dist starts as poison: every element is written, nothing else is."""
    x = rand_i8(np.random.RandomState(N * 1000 + T * 10 + Df % 7), N, T, Df)
    got = frame_sqdist(hl, arena, x)
    assert np.array_equal(got, mr.frame_sqdist(x))
    assert not np.diagonal(got, 0, 1, 2).any() and np.array_equal(got, got.transpose(0, 2, 1))


def test_frame_sqdist_extremes_duplicates_and_clips_apart(hl, arena):
    N, T, Df = 5, 33, 3072
    x = rand_i8(np.random.RandomState(7), N, T, Df)
    x[0, 0], x[0, 1], x[0, 32] = -128, 127, 127                       # the all-extreme pair, in one tile and across three
    x[1, 5], x[4, 32] = x[1, 20], x[4, 0]                             # duplicate frames: exact zeros off the diagonal
    got = frame_sqdist(hl, arena, x)
    assert np.array_equal(got, mr.frame_sqdist(x))
    assert got[0, 0, 1] == got[0, 1, 0] == got[0, 32, 0] == MAX_DIST and got[0, 1, 32] == 0
    assert got[1, 5, 20] == got[1, 20, 5] == got[4, 32, 0] == got[4, 0, 32] == 0
    assert not np.diagonal(got, 0, 1, 2).any() and np.array_equal(got, got.transpose(0, 2, 1))
    # every clip as an operand of its own, poison on both sides of it: the rows a ragged tile clamps to are the clip's own
    arena.reset()
    T, Df = 17, 64
    parts = [arena.put(dev(x[n, :T, :Df])).view(1, T, Df) for n in range(N)]
    outs = [arena.empty((1, T, T), torch.int32) for _ in range(N)]
    for p, o in zip(parts, outs):
        hl.mc_frame_sqdist(p, o)
    arena.check()
    whole = np.ascontiguousarray(x[:, :T, :Df])
    assert np.array_equal(np.concatenate([host(o) for o in outs]), mr.frame_sqdist(whole))
    arena.reset()
    assert np.array_equal(frame_sqdist(hl, arena, whole), mr.frame_sqdist(whole))


# ---- 3. motion descriptors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,Df", [(3, 2, 64), (2, 2, 768), (5, 16, 64), (2, 16, 768), (1, 513, 64), (2, 17, 2048)])
def test_motion_descriptors_and_norms(hl, arena, N, T, Df):
    """differences of -255, -254, -1, 0, 1, 254 and 255 planted in the first and in the last frame pair; one difference (T = 2) and
    fifteen; the longest row, (T - 1) Df = 32768, as 512 x 64 and as 16 x 2048"""
    x = rand_i8(np.random.RandomState(N + T + Df), N, T, Df)
    lo, hi = [127, 127, 0, 5, 0, -127, -128], [-128, -127, -1, 5, 1, 127, 127]
    x[0, 0, :7], x[0, 1, :7] = lo, hi
    x[-1, -2, -7:], x[-1, -1, -7:] = lo, hi
    d = arena.put(dev(x))
    mdesc, mnorms = arena.empty((N, (T - 1) * Df), torch.int8), arena.empty((N,), torch.int32)
    hl.mc_motion_descriptors(d, mdesc, mnorms)
    arena.check()
    assert np.array_equal(host(d), x)
    rd, rn = mr.motion_descriptors(x)
    assert rd[0, :7].tolist() == rd[-1, -7:].tolist() == [-128, -127, -1, 0, 0, 127, 127]
    assert np.array_equal(host(mdesc), rd) and np.array_equal(host(mnorms), rn)


def test_motion_descriptors_refuse_rows_past_the_knn_limit(hl, arena):
    for T, Df in ((514, 64), (17, 2048 + 64), (2, 32768 + 64)):        # the next multiple of 64 after 32768, three ways
        d = arena.zeros((1, T, Df), torch.int8)
        mdesc, mnorms = arena.empty((1, (T - 1) * Df), torch.int8), arena.empty((1,), torch.int32)
        with pytest.raises(hl.McgError):
            hl.mc_motion_descriptors(d, mdesc, mnorms)
        arena.check()
        assert (host(mnorms).view(np.uint32) == guard.POISON).all()


# ---- 4. clip statistics -------------------------------------------------------------------------------------------------------------
def check_pair_sums(got, dist):
    """|pair_sum - S| <= (P + 1) 2^-52 S for S = math.fsum of the correctly rounded square roots (math.sqrt of an integer below 2^53):
    one ulp (2^-52 relative) per square root covers a device sqrt that is not correctly rounded, and every one of the P - 1
    additions of non-negative terms rounds a partial sum <= S by at most 2^-53 S."""
    T = dist.shape[1]
    P = T * (T - 1) // 2
    for n, d in enumerate(dist.tolist()):
        s = math.fsum(math.sqrt(d[p][q]) for p in range(T) for q in range(p + 1, T))
        print('pair_sum[%d] = %r, fsum %r, |difference| %.3e, bound %.3e' % (n, float(got[n]), s, abs(float(got[n]) - s), (P + 1) * 2.0 ** -52 * s))
        assert abs(float(got[n]) - s) <= (P + 1) * 2.0 ** -52 * s, n


@pytest.mark.parametrize("N,T", [(1, 2), (5, 2), (4, 17), (3, 64), (9, 64)])
def test_clip_stats(hl, arena, N, T):
    """one pair and 2016; clips below, at and above one workgroup's four; an all-zero and an all-maximal matrix among random ones
    (the kernel reads what it is given: the matrices need not be distance matrices).  lag_sum bit for bit; pair_sum within the
    bound of check_pair_sums; a second call gives the same bits."""
    rng = np.random.RandomState(N * 100 + T)
    dist = rng.randint(0, MAX_DIST + 1, (N, T, T)).astype(np.int32)
    dist[0] = MAX_DIST
    if N > 2:
        dist[1] = 0
        dist[2, 0, 1], dist[2, -2, -1] = 0, 1
    d = arena.put(dev(dist))
    outs = []
    for _ in range(2):
        pair, lag = arena.empty((N,), torch.float64), arena.empty((N, T), torch.int64)
        hl.mc_clip_stats(d, pair, lag)
        arena.check()
        outs.append((host(pair), host(lag)))
    assert np.array_equal(host(d), dist)
    (pair, lag), (pair2, lag2) = outs
    assert np.array_equal(pair.view(np.int64), pair2.view(np.int64)) and np.array_equal(lag, lag2)
    ref = mr.lag_sum(dist)
    assert np.array_equal(lag, ref) and lag.dtype == np.int64
    assert int(lag[0, 1]) == (T - 1) * MAX_DIST and (T < 64 or int(lag[0, 1]) > 2 ** 31)
    check_pair_sums(pair, dist)
    assert pair[0] == pytest.approx(T * (T - 1) // 2 * math.sqrt(MAX_DIST), rel=1e-12) and (N <= 2 or pair[1] == 0.0)


# ---- 5. MotionContent against the reference -----------------------------------------------------------------------------------------
K = 3
INT_KEYS = ('lag_l1', 'motion_precision', 'motion_recall', 'motion_density', 'motion_coverage')


def same_but_acd(got, ref, n, T):
    """every figure that derives from integers alone is equal; acd lies within the bound of check_pair_sums of the reference's, twice
    (either side against the exact sum), plus the roundings of the mean over n clips and of two more operations on each side"""
    assert set(got) == set(ref)
    for key in INT_KEYS:
        assert got[key] == ref[key], (key, got[key], ref[key])
    P = T * (T - 1) // 2
    for side in ('real', 'fake'):
        assert got[side]['lag'] == ref[side]['lag'] and got[side]['lag1_q'] == ref[side]['lag1_q'], side
        a, b = got[side]['acd'], ref[side]['acd']
        print('%s acd %r, reference %r' % (side, a, b))
        assert abs(a - b) <= 2 * ((P + 1) * 2.0 ** -52 + (n + 2) * 2.0 ** -53) * b, side


@pytest.mark.parametrize("pool,C", [(4, 1), (4, 3), (8, 1), (8, 3)])
def test_report_equals_the_reference_whatever_the_chunking(hl, pool, C):
    """33 real and 33 fake clips of 5 frames of random bytes, k = 3; in chunks of 1, 5 and all, host arrays and device tensors"""
    from mocogan_chainer_amd.metrics import MotionContent
    n, T = 33, 5
    rng = np.random.RandomState(pool * 10 + C)
    R, F = (rng.randint(0, 256, (n, T, 64, 64, C)).astype(np.uint8) for _ in range(2))
    F[:, 1:] = (F[:, :1].astype(np.int64) + rng.randint(-9, 10, F[:, 1:].shape)).clip(0, 255).astype(np.uint8)     # fake: jitter round a still
    ref_r, ref_f = mr.clip_set(R, pool), mr.clip_set(F, pool)
    ref = mr.report(ref_r, ref_f, K)
    mc = MotionContent(K, pool)
    chunked = lambda x, m: [x[i:i + m] for i in range(0, len(x), m)]
    first = None
    for m in (n, 5, 1):
        real, fake = mc.clip_set(chunked(R, m)), mc.clip_set(iter(chunked(dev(F), m)))
        for s, r in ((real, ref_r), (fake, ref_f)):
            assert (s.n, s.frames, s.frame_dim) == (n, T, (64 // pool) ** 2 * C)
            assert np.array_equal(host(s.clips.desc), r['desc']) and np.array_equal(host(s.motion.desc), r['mdesc'])
            assert np.array_equal(host(s.motion.norms), r['mnorms']) and np.array_equal(s.lag_sum, r['lag_sum'])
            check_pair_sums(s.pair_sum, r['dist'])
        got = mc.report(real, fake)
        same_but_acd(got, ref, n, T)
        if first is None:
            first = (real.pair_sum, fake.pair_sum, got)
            print({key: got[key] for key in ('acd_ratio',) + INT_KEYS})
        else:                                                           # the chunking changes no bit
            assert np.array_equal(real.pair_sum.view(np.int64), first[0].view(np.int64))
            assert np.array_equal(fake.pair_sum.view(np.int64), first[1].view(np.int64)) and got == first[2]
    with pytest.raises(ValueError):
        mc.report(real, mc.clip_set([R[:8, :4]]))                       # other frames


def test_grid_report_on_the_planted_grid_equals_the_reference(hl):
    """the planted 3 x 3 grid of the CPU test, every pixel repeated over 4 x 4 so that a pool of 4 gives the pixels back"""
    from mocogan_chainer_amd.metrics import MotionContent
    small = mr.planted_grid(K, 11)
    ref_set = mr.frame_set(mr.byte_frames(small))
    ref = mr.grid_report(ref_set, K)
    mc = MotionContent(K, 4)
    s = mc.clip_set([mr.upscale(small, 4)])
    assert np.array_equal(host(s.clips.desc), ref_set['desc']) and np.array_equal(host(s.motion.desc), ref_set['mdesc'])
    got = mc.grid_report(s, K)
    assert set(got) == set(ref)
    for key in ref:
        if key.endswith('_dist'):
            assert np.array_equal(got[key], ref[key]) and got[key].shape == (K * K, K * K), key
        else:
            assert got[key] == ref[key], (key, got[key], ref[key])
    print({key: got[key] for key in ('content_ratio', 'motion_leak', 'motion_ratio', 'content_leak')})
    assert got['content_ratio'] < 0.5 and got['motion_ratio'] < 0.5 and abs(got['content_leak'] - 1) < 0.1
    with pytest.raises(ValueError):
        mc.grid_report(s, K + 1)


# ---- 6. the entry point ----------------------------------------------------------------------------------------------------------------
def test_cli_on_the_synthetic_dataset_with_a_fresh_generator(hl, tmp_path, capsys):
    import evaluate_motion
    from model.net import ImageGenerator
    from mocogan_chainer_amd import trainer
    np.random.seed(4)
    gen = ImageGenerator(n_filters=8, video_len=4)
    for _ in range(30):                                               # training-mode calls: the running BatchNorm statistics leave (0, 1),
        gen(8)                                                        # without which a fresh generator's test-mode clips are all one grey frame
    path, dump = tmp_path / 'image_gen_epoch_1.npz', tmp_path / 'motion.npz'
    trainer.save_npz(path, gen)
    argv = [str(path), '--dataset_type', 'synthetic', '--synthetic_size', '16', '--num', '16', '--k', '3', '--pool', '8', '--n_filters', '8',
            '--video_len', '4', '--chunk', '5', '--seed', '2', '--grid', '2', '--dump', str(dump)]
    res = evaluate_motion.main(argv)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
    assert len(line) == 1 and json.loads(line[0]) == res             # one JSON line
    print("evaluate_motion:", line[0])
    assert set(res) == {'real', 'fake', 'acd_ratio', 'lag_l1', 'motion_precision', 'motion_recall', 'motion_density', 'motion_coverage',
                        'content_ratio', 'motion_leak', 'motion_ratio', 'content_leak', 'appearance_means', 'motion_means',
                        'num', 'k', 'pool', 'grid', 'frames', 'frame_dim', 'seed', 'test_mode', 'model_weight', 'dataset_type'}
    for key in ('motion_precision', 'motion_recall', 'motion_coverage'):
        assert 0.0 <= res[key] <= 1.0, key
    finite = lambda v: v is None or (np.isfinite(v) and v >= 0)
    assert all(finite(res[key]) for key in ('acd_ratio', 'lag_l1', 'motion_density', 'content_ratio', 'motion_leak', 'motion_ratio', 'content_leak'))
    for side in ('real', 'fake'):
        su = res[side]
        assert set(su) == {'acd', 'lag', 'lag1_q'} and len(su['lag']) == 3 and len(su['lag1_q']) == 3
        assert all(np.isfinite(v) and 0 <= v <= 255 for v in [su['acd']] + su['lag'] + su['lag1_q'])
    assert res['fake']['acd'] > 0 and res['appearance_means']['neither'] > 0      # the generated clips differ, in themselves and from one another
    assert all(set(res[key]) == {'same_content', 'same_motion', 'neither'} for key in ('appearance_means', 'motion_means'))
    assert (res['num'], res['k'], res['pool'], res['grid'], res['frames'], res['frame_dim']) == (16, 3, 8, 2, 4, 8 * 8 * 3)
    dumped = np.load(dump)
    assert dumped['real_pair_sum'].shape == dumped['fake_pair_sum'].shape == (16,) and dumped['real_lag_sum'].shape == dumped['fake_lag_sum'].shape == (16, 4)
    assert dumped['grid_appearance_dist'].shape == dumped['grid_motion_dist'].shape == (4, 4)
    assert not np.diag(dumped['grid_appearance_dist']).any() and np.array_equal(dumped['grid_motion_dist'], dumped['grid_motion_dist'].T)
    again = evaluate_motion.main(argv[:-4])                           # the same run without the grid: the same figures
    assert 'content_ratio' not in again and again['grid'] == 0
    assert all(again[key] == res[key] for key in ('real', 'fake', 'acd_ratio', 'lag_l1', 'motion_precision', 'motion_recall'))
