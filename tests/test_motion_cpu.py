"""CPU checks of the motion and content metrics: tests/motion_ref.py (the NumPy statement the GPU tests compare with) against
brute-force loops, what the figures say on sets whose relation is known, the command line of evaluate_motion.py, and the mcg_mc_*
entry points' refusals on the host (the library cross-compiles and loads without a GPU)."""
import ctypes
import math

import numpy as np
import pytest

import knn_ref as kr
import motion_ref as mr


# ---- the reference against loops -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,Df", [(2, 2, 64), (3, 5, 64), (1, 17, 128)])
def test_reference_matches_brute_force(N, T, Df):
    rng = np.random.RandomState(N * 100 + T)
    x = rng.randint(-128, 128, (N, T, Df)).astype(np.int8)
    x[0, 0, :7], x[0, 1, :7] = [127, -128, 0, -1, 0, 127, -127], [-128, 127, -1, 0, 1, -127, 127]   # differences -255, 255, -1, 1, 1, -254, 254
    s = mr.frame_set(x)
    v = x.tolist()
    for n in range(N):
        d = [[sum((a - b) ** 2 for a, b in zip(v[n][p], v[n][q])) for q in range(T)] for p in range(T)]
        assert s['dist'][n].tolist() == d
        acc = 0.0
        for p in range(T):
            for q in range(p + 1, T):
                acc += math.sqrt(d[p][q])
        assert s['pair_sum'][n] == acc
        assert s['lag_sum'][n].tolist() == [sum(d[t][t + l] for t in range(T - l)) for l in range(T)]
        m = [(v[n][t + 1][e] - v[n][t][e]) // 2 for t in range(T - 1) for e in range(Df)]             # // floors, as >> does
        assert s['mdesc'][n].tolist() == m and int(s['mnorms'][n]) == sum(q * q for q in m)
    assert s['mdesc'][0, :7].tolist() == [-128, 127, -1, 0, 0, -127, 127]
    assert s['lag_sum'][:, 0].tolist() == [0] * N and s['mdesc'].shape == (N, (T - 1) * Df) and s['mdesc'].dtype == np.int8


def test_reference_summary_report_and_grid_match_loops():
    rng = np.random.RandomState(5)
    T, Df, K, k = 4, 64, 3, 2
    real, fake = (mr.frame_set(rng.randint(-20, 21, (K * K, T, Df)).astype(np.int8)) for _ in range(2))
    su = mr.summary(real)
    P = T * (T - 1) // 2
    assert su['acd'] == float(np.mean(real['pair_sum'])) / (P * math.sqrt(Df))
    d = real['dist']
    for l in range(1, T):
        tot = sum(int(d[n, t, t + l]) for n in range(K * K) for t in range(T - l))
        assert su['lag'][l - 1] == math.sqrt(tot / (K * K * (T - l) * Df))
    per_clip = sorted(math.sqrt(sum(int(d[n, t, t + 1]) for t in range(T - 1)) / ((T - 1) * Df)) for n in range(K * K))
    assert su['lag1_q'][1] == pytest.approx(per_clip[K * K // 2], rel=1e-15) and per_clip[0] <= su['lag1_q'][0] <= su['lag1_q'][2] <= per_clip[-1]
    r = mr.report(real, fake, k)
    assert set(r) == {'real', 'fake', 'acd_ratio', 'lag_l1', 'motion_precision', 'motion_recall', 'motion_density', 'motion_coverage'}
    assert r['acd_ratio'] == r['fake']['acd'] / r['real']['acd']
    assert r['lag_l1'] == pytest.approx(sum(abs(a - b) for a, b in zip(r['fake']['lag'], r['real']['lag'])) / (T - 1), rel=1e-14)
    knn = kr.report(real['mdesc'], fake['mdesc'], k)
    assert [r['motion_' + key] for key in ('precision', 'recall', 'density', 'coverage')] == [knn[key] for key in ('precision', 'recall', 'density', 'coverage')]
    with pytest.raises(ValueError):
        mr.report(real, mr.frame_set(np.zeros((4, T + 1, Df), np.int8)), k)
    g = mr.grid_report(real, K)
    for space, rows in (('appearance', real['desc']), ('motion', real['mdesc'])):
        sums, counts = {'same_content': 0, 'same_motion': 0, 'neither': 0}, {'same_content': 0, 'same_motion': 0, 'neither': 0}
        for i in range(K * K):
            for j in range(K * K):
                sc, sm = i // K == j // K, i % K == j % K
                if sc and sm:
                    continue
                key = 'same_content' if sc else 'same_motion' if sm else 'neither'
                sums[key] += sum((int(a) - int(b)) ** 2 for a, b in zip(rows[i], rows[j]))
                counts[key] += 1
        assert counts == {'same_content': K * K * (K - 1), 'same_motion': K * K * (K - 1), 'neither': K * K * (K - 1) ** 2}
        assert g[space + '_means'] == {key: sums[key] / counts[key] for key in sums}
    assert g['content_ratio'] == g['appearance_means']['same_content'] / g['appearance_means']['neither']
    assert g['motion_leak'] == g['appearance_means']['same_motion'] / g['appearance_means']['neither']
    assert g['motion_ratio'] == g['motion_means']['same_motion'] / g['motion_means']['neither']
    assert g['content_leak'] == g['motion_means']['same_content'] / g['motion_means']['neither']
    with pytest.raises(ValueError):
        mr.grid_report(real, K + 1)


def test_extreme_frame_distance_and_lag_sum_sizes():
    x = np.full((1, 64, 3072), -128, np.int8)
    x[0, 1::2] = 127
    s = mr.frame_set(x)
    assert int(s['dist'][0, 0, 1]) == 199756800 == 255 ** 2 * 3072 < 2 ** 31 and int(s['dist'][0, 0, 2]) == 0
    assert int(s['lag_sum'][0, 1]) == 63 * 199756800 > 2 ** 31           # needs int64
    assert mr.summary(s)['lag'][0] == 255.0 and mr.summary(s)['lag'][1] == 0.0
    assert s['mdesc'][0, :3072].tolist() == [127] * 3072 and s['mdesc'][0, 3072:6144].tolist() == [-128] * 3072


# ---- what the figures say ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """a 4 x 4 grid of 8-frame 16 x 16 clips: content = a static random background, motion = a bright 3 x 3 blob's random walk"""
    return mr.frame_set(mr.byte_frames(mr.planted_grid(4, 11)))


def test_planted_grid_separates_content_from_motion(planted):
    """pinned with this reference at seed 11: content_ratio 0.26303, motion_leak 0.76399, motion_ratio 0.10002, content_leak 1.00000"""
    g = mr.grid_report(planted, 4)
    print({key: g[key] for key in ('content_ratio', 'motion_leak', 'motion_ratio', 'content_leak')})
    assert g['content_ratio'] < 0.5 and g['motion_ratio'] < 0.5 and abs(g['content_leak'] - 1) < 0.1
    assert g['content_ratio'] == pytest.approx(PINNED['content_ratio'], abs=5e-6)
    assert g['motion_leak'] == pytest.approx(PINNED['motion_leak'], abs=5e-6)
    assert g['motion_ratio'] == pytest.approx(PINNED['motion_ratio'], abs=5e-6)
    assert g['content_leak'] == pytest.approx(PINNED['content_leak'], abs=5e-6)
    assert g['motion_ratio'] > 0                                         # a difference image still depends on what moves


PINNED = {'content_ratio': 0.26303, 'motion_leak': 0.76399, 'motion_ratio': 0.10002, 'content_leak': 1.0}


def test_frozen_clips_have_no_content_distance_and_no_motion(planted):
    x = planted['desc'].reshape(16, 8, -1)
    frozen = mr.frame_set(np.repeat(x[:, :1], 8, axis=1))
    su = mr.summary(frozen)
    assert su['acd'] == 0.0 and su['lag'] == [0.0] * 7 and su['lag1_q'] == [0.0] * 3
    r = mr.report(frozen, planted, 3)
    assert r['acd_ratio'] is None and r['lag_l1'] > 0
    assert mr.report(planted, frozen, 3)['acd_ratio'] == 0.0


def test_shuffling_frames_in_time_keeps_acd_and_flattens_the_lag_profile():
    """a slow drift: frame t = base + t * step, so the frame distance grows with the lag; the shuffle permutes the pair set"""
    rng = np.random.RandomState(3)
    n, T, Df = 12, 8, 64
    base, step = rng.randint(-40, 41, (n, 1, Df)), rng.randint(-6, 7, (n, 1, Df))
    x = (base + np.arange(T)[None, :, None] * step).astype(np.int8)
    shuffled = np.stack([c[rng.permutation(T)] for c in x])
    a, b = mr.frame_set(x), mr.frame_set(shuffled)
    sa, sb = mr.summary(a), mr.summary(b)
    assert sb['acd'] == pytest.approx(sa['acd'], rel=1e-13)              # the same square roots in another order
    assert np.array_equal(np.sort(a['dist'].reshape(n, -1), axis=1), np.sort(b['dist'].reshape(n, -1), axis=1))
    assert all(p < q for p, q in zip(sa['lag'], sa['lag'][1:]))          # ordered: rising
    assert sa['lag'][-1] / sa['lag'][0] == pytest.approx(T - 1, rel=1e-12)
    assert max(sb['lag']) / min(sb['lag']) < 2.5                         # shuffled: flat by comparison with 7
    r = mr.report(a, b, 3)
    assert r['acd_ratio'] == pytest.approx(1.0, rel=1e-13) and r['lag_l1'] > 0.5


def test_a_set_against_itself(planted):
    r = mr.report(planted, planted, 3)
    assert r['acd_ratio'] == 1.0 and r['lag_l1'] == 0.0
    assert r['motion_precision'] == r['motion_recall'] == r['motion_coverage'] == 1.0
    rng = np.random.RandomState(8)
    distinct = mr.frame_set(rng.randint(-128, 128, (20, 4, 64)).astype(np.int8))      # no two clips alike: every ball holds k + 1 members
    r = mr.report(distinct, distinct, 3)
    assert r['motion_precision'] == r['motion_recall'] == r['motion_coverage'] == 1.0 and r['motion_density'] >= 1.0


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_parses_and_validates():
    import evaluate_motion as ev
    a = ev.parse_args(['g.npz'])
    assert (a.num, a.k, a.pool, a.grid, a.dump, a.seed, a.test_mode) == (1024, 5, 4, 0, None, 0, 1)
    assert (a.dataset_type, a.dataset, a.synthetic_size, a.mfma, a.labels, a.chunk, a.video_len, a.channel, a.dim_zl, a.n_filters) == \
        ('mug', 'data/dataset/train', 256, 'f32', None, 64, 16, 3, 0, 64)
    a = ev.parse_args(['g.npz', '--dataset_type', 'synthetic', '--num', '256', '--grid', '8', '--dump', 'm.npz', '--k', '3', '--pool', '8',
                       '--mfma', 'f32x3', '--n_filters', '8', '--dim_zl', '4', '--labels', '2'])
    assert (a.dataset_type, a.num, a.grid, a.dump, a.k, a.pool, a.mfma, a.labels) == ('synthetic', 256, 8, 'm.npz', 3, 8, 'f32x3', [2])
    assert ev.parse_args(['g.npz', '--pool', '2', '--video_len', '8']).pool == 2            # 8 * 32^2 * 3 = 24576
    assert ev.parse_args(['g.npz', '--video_len', '2']).video_len == 2 and ev.parse_args(['g.npz', '--video_len', '64', '--pool', '8']).video_len == 64
    for bad in (['g.npz', '--num', '0'], ['g.npz', '--k', '0'], ['g.npz', '--k', '17'], ['g.npz', '--num', '5', '--k', '5'],
                ['g.npz', '--pool', '3'], ['g.npz', '--pool', '16'], ['g.npz', '--pool', '2'], ['g.npz', '--video_len', '1'],
                ['g.npz', '--video_len', '65', '--pool', '8'], ['g.npz', '--grid', '1'], ['g.npz', '--grid', '-2'],
                ['g.npz', '--grid', '4', '--test_mode', '0'], ['g.npz', '--channel', '2'], ['g.npz', '--labels', '1'], ['--num', '4'],
                ['g.npz', '--mfma', 'fp8'], ['g.npz', '--chunk', '0'], ['g.npz', '--dim_zl', '3', '--labels', '3']):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    text = ' '.join(ev.__doc__.split())
    assert 'appearance, not identity' in text and 'depends on --num and --k' in text


def test_grid_latents_are_content_major():
    import evaluate_motion as ev

    class Gen:                                                          # the draws of ImageGenerator._latents, without a device
        dim_zl, dim_zm, dim_zc = 3, 4, 5

        def _latents(self, n, labels, zc, h0, e, T):
            hid = lambda w: np.random.normal(0, 0.33, size=[n, w]).astype(np.float32)
            labels = np.random.randint(self.dim_zl, size=n)
            h0 = hid(self.dim_zm)
            e = np.stack([hid(self.dim_zm) for _ in range(T)])
            return labels, h0, e, hid(self.dim_zc)

    K, T = 3, 2
    np.random.seed(1)
    labels, h0, e, zc = Gen()._latents(K, None, None, None, None, T)
    np.random.seed(1)
    lat = ev.grid_latents(Gen(), K, T)
    assert lat['zc'].shape == (9, 5) and lat['h0'].shape == (9, 4) and lat['e'].shape == (T, 9, 4) and lat['labels'].shape == (9,)
    for c in range(K):
        for m in range(K):
            i = c * K + m
            assert np.array_equal(lat['zc'][i], zc[c]) and np.array_equal(lat['h0'][i], h0[m])
            assert np.array_equal(lat['e'][:, i], e[:, m]) and lat['labels'][i] == labels[m]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


NAMES = ('mcg_mc_frame_sqdist', 'mcg_mc_clip_stats', 'mcg_mc_motion_descriptors')


def test_library_exports_the_entry_points_with_prototypes(hl):
    lib = hl.load()
    for name in NAMES:
        assert name in hl.SIGNATURES and getattr(lib, name).argtypes == hl.SIGNATURES[name][1]
    assert [len(hl.SIGNATURES[name][1]) for name in NAMES] == [6, 6, 7]
    assert lib.mcg_version() == 8


def test_mc_entry_points_refuse_on_the_host(hl):
    """A null pointer, a non-positive extent and a misaligned descriptor pointer are MCG_ERR_BAD_ARG; T = 1, T = 65, Df = 32, a Df
    that is no multiple of 64 or exceeds 3072, and a motion row past 32768 bytes are MCG_ERR_UNSUPPORTED -- all before anything is
    launched.  `one` is a non-null, 16-byte aligned pointer that is never dereferenced, the outputs are small host buffers that
    must come back untouched; no call below passes an acceptable argument set."""
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

    fs = lambda N, T, Df, desc=one, dist=o1: lib.mcg_mc_frame_sqdist(N, T, Df, desc, dist, None)
    for ext in ((0, 16, 64), (-1, 16, 64), (4, 0, 64), (4, -3, 64), (4, 16, 0), (4, 16, -64)):
        refused(BAD, fs(*ext), NAMES[0], ext)
    for hole in ('desc', 'dist'):
        refused(BAD, fs(4, 16, 64, **{hole: None}), NAMES[0], "no " + hole)
    refused(BAD, fs(4, 16, 64, desc=ctypes.c_void_p(24)), NAMES[0], "desc not 16-byte aligned")
    for T, Df in ((1, 64), (65, 64), (1000, 64), (16, 32), (16, 1), (16, 96), (16, 3072 + 64), (16, 32768)):
        refused(UNSUPPORTED, fs(4, T, Df), NAMES[0], (T, Df))

    cs = lambda N, T, dist=one, pair=o1, lag=o2: lib.mcg_mc_clip_stats(N, T, dist, pair, lag, None)
    for ext in ((0, 16), (-1, 16), (4, 0), (4, -1)):
        refused(BAD, cs(*ext), NAMES[1], ext)
    for hole in ('dist', 'pair', 'lag'):
        refused(BAD, cs(4, 16, **{hole: None}), NAMES[1], "no " + hole)
    for T in (1, 65, 4096):
        refused(UNSUPPORTED, cs(4, T), NAMES[1], T)

    md = lambda N, T, Df, desc=one, mdesc=one, mnorms=o2: lib.mcg_mc_motion_descriptors(N, T, Df, desc, mdesc, mnorms, None)
    for ext in ((0, 16, 64), (-1, 16, 64), (4, 0, 64), (4, -3, 64), (4, 16, 0), (4, 16, -64)):
        refused(BAD, md(*ext), NAMES[2], ext)
    for hole in ('desc', 'mdesc', 'mnorms'):
        refused(BAD, md(4, 16, 64, **{hole: None}), NAMES[2], "no " + hole)
    refused(BAD, md(4, 16, 64, desc=ctypes.c_void_p(24)), NAMES[2], "desc not 16-byte aligned")
    refused(BAD, md(4, 16, 64, mdesc=ctypes.c_void_p(20)), NAMES[2], "mdesc not 16-byte aligned")
    for T, Df in ((1, 64), (16, 32), (16, 100), (514, 64), (17, 2048 + 64), (12, 3072), (2 ** 30, 64), (3, 2 ** 30)):
        refused(UNSUPPORTED, md(4, T, Df), NAMES[2], (T, Df))
    assert len(calls) > 45


def test_mc_wrappers_and_motion_content_refuse_misfits(hl):
    import torch
    from mocogan_chainer_amd.metrics import MotionContent
    x = torch.zeros(2, 4, 64, dtype=torch.int8)
    for call in (lambda: hl.mc_frame_sqdist(x), lambda: hl.mc_motion_descriptors(x), lambda: hl.mc_clip_stats(torch.zeros(2, 4, 4, dtype=torch.int32)),
                 lambda: hl.mc_frame_sqdist(x.view(8, 64)), lambda: hl.mc_clip_stats(torch.zeros(2, 4, 5, dtype=torch.int32)),
                 lambda: hl.mc_frame_sqdist(x, torch.zeros(2, 4, 3, dtype=torch.int32))):
        with pytest.raises(hl.McgError):                                # host tensors and misfits
            call()
    for kwargs in ({'k': 0}, {'k': 17}, {'pool': 3}, {'row_block': 0}):
        with pytest.raises(ValueError):
            MotionContent(device='cpu', **kwargs)
    mc = MotionContent(k=3, pool=2, device='cpu')
    with pytest.raises(ValueError, match='larger pool'):
        mc.clip_set([np.zeros((1, 16, 64, 64, 3), np.uint8)])            # 16 * 32^2 * 3 = 49152 at pool 2
    with pytest.raises(ValueError, match='2..64 frames'):
        MotionContent(k=3, pool=8, device='cpu').clip_set([np.zeros((1, 1, 64, 64, 3), np.uint8)])
    with pytest.raises(ValueError):
        mc.clip_set([])
