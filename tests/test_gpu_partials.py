"""The consumers of per-tile partial sums -- mcg_bn_stats_from_partials, mcg_bn_act_bwd_from_partials, mcg_colsum_from_partials
-- on SYNTHETIC partials at the slot counts, widths and strides where the host code of csrc/small_ops.hip changes its path, and
the column passes mcg_colsum_acc / mcg_bn_sums at the row counts where plan_partial changes its plan.

The entry points are public ABI: any n_slots, any slot_stride >= 2 C, any C % 4 == 0.  Every other test feeds them the slot
counts a conv epilogue happens to produce.  Here: 96 slots go straight to the finalize kernel, 97 are folded first; a fold takes
chunks of 32 slots until that makes more than 512 chunks (16385 slots), then of ceil(n / 512); the last chunk may hold one slot;
the finalize kernel's eight-in-flight loop needs more than 224 partials (8192 slots unfolded, or 8193 folded into 257); C = 4
leaves half of the fold's lanes idle, C = 12 is never folded, C = 96 is folded with a part-dead second channel block; and a
grouped stride (4 C, `part` offset to the second group) puts poison where the other group's columns are.

The partials are small integers ({-2..2} in the sum columns, {0..4} in the second ones), so every sum is an integer below 2^24:
exact in fp32 and in double in ANY order, and the tests demand equality -- a dropped or doubled slot at 16385 slots, 6e-5 of the
sum, cannot hide below a tolerance.  Derived quantities (statistics, running averages, gx) are held against tests/sync_bn_ref.py
of the exact sums at the project's SUM_TOL / BWD_TOL.  Exact sums are the same on either side of the 96 / 97 edge, so the column-sum
test also looks at WHICH path ran: the poisoned workspace is untouched up to 96 slots (and at C = 12), written beyond.  Run with -s: the PARITY lines go to profiles/layout_partials_parity.md.

Everything a launch touches is carved from one guard.Arena (the workspace has exactly bn_workspace_floats(C) floats); outputs are
poison until written, the margins are checked after every launch, inputs are compared bit for bit with a snapshot afterwards."""
import functools

import numpy as np
import pytest
import torch

import sync_bn_ref as R
from guard import POISON, Arena

pytestmark = pytest.mark.gpu

SUM_TOL, BWD_TOL = 1e-5, 1e-4           # tests/test_gpu_sync_bn.py, tests/test_gpu_ops.py
F32, BF, F64, I32 = torch.float32, torch.bfloat16, torch.float64, torch.int32
SLOTS = [1, 2, 32, 33, 96, 97, 128, 8192, 8193, 16384, 16385, 40001]
WIDTHS = [4, 8, 32, 64, 128]            # 4 * 2^k
ODD_WIDTHS, ODD_SLOTS = [12, 96], [97, 8193, 16385]       # accepted, not 4 * 2^k
# (n_slots, C, slot_stride / C): the dense stride at every width and slot count, the grouped one where the paths differ
CASES = [(n, C, 2) for C in WIDTHS for n in SLOTS]
CASES += [(n, 512, 2) for n in (97, 8193)]                 # eight channel blocks in the fold, 64 in the finalize kernel
CASES += [(n, C, 2) for C in ODD_WIDTHS for n in ODD_SLOTS]
CASES += [(n, C, 4) for C in (4, 64) for n in (96, 97, 8193, 16385)] + [(n, C, 4) for C in ODD_WIDTHS for n in (96, 97, 16385)]
FOLD_ABOVE = 96                         # small_ops.hip: slot counts up to this go straight to the finalize kernels
BWD_ROWS = 7                          # rows of g / y in the backward cases: the sums come from the partials, not from these rows


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(256 << 20)


def raw(t):
    t = t.detach().contiguous()
    return t.view({F32: torch.int32, BF: torch.int16, F64: torch.int64}.get(t.dtype, t.dtype)).cpu().numpy()


def rel_l2(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def held(case, what, got, want, tol):
    err = rel_l2(got, want)
    print("PARITY %-22s %-34s %.2e  (tol %.0e)" % (case, what, err, tol))
    assert err < tol, (case, what, err, tol)


def exact(case, what, got, want):
    """a device tensor equals an integer-valued array exactly"""
    g = got.detach().cpu().double().numpy()
    w = np.asarray(want, np.float64)
    assert g.shape == w.shape
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError("%s %s: %d of %d values differ, first at %d: got %r, want %r (difference %r)" % (
            case, what, len(bad), g.size, bad[0], g[bad[0]], w[bad[0]], g[bad[0]] - w[bad[0]]))


class Launch:
    """inputs: copies inside the arena, snapshots outside it; outputs: poison"""

    def __init__(self, arena):
        arena.reset()
        self.arena, self.inputs = arena, []

    def watch(self, t):
        self.inputs.append((t, t.clone()))
        return t

    def put(self, a, dtype=F32):
        return self.watch(self.arena.put(torch.from_numpy(np.array(a, copy=True)).to(dtype).cuda()))

    def done(self):
        self.arena.check()
        for t, snap in self.inputs:
            assert np.array_equal(raw(t), raw(snap)), "a launch wrote to one of its inputs"


@functools.lru_cache(maxsize=4)
def _ints(n_slots, C):
    """the partials of a case: (sums [n][C] in {-2..2}, second column block [n][C] in {0..4}), and their exact totals"""
    rng = np.random.RandomState(n_slots % 9973 + C)
    a, b = rng.randint(-2, 3, (n_slots, C)).astype(np.float32), rng.randint(0, 5, (n_slots, C)).astype(np.float32)
    total = np.concatenate([a.sum(0, dtype=np.float64), b.sum(0, dtype=np.float64)])
    assert np.abs(total).max() < 2 ** 24 and 4 * n_slots < 2 ** 24           # every partial sum is an exact fp32 integer
    return a, b, total


def make_partials(L, n_slots, C, mult):
    """[n_slots][mult * C] inside the arena: the group's 2 C columns hold the integers, every other column stays poison.
    Returns (the pointer-carrying view at the group's first column, slot_stride, the exact totals)."""
    a, b, total = _ints(n_slots, C)
    stride, off = mult * C, (mult - 2) * C                                   # mult = 4: the SECOND of two groups
    full = L.arena.empty((n_slots, stride))
    full[:, off:off + C] = torch.from_numpy(a).cuda()
    full[:, off + C:off + 2 * C] = torch.from_numpy(b).cuda()
    L.watch(full)
    return full.view(-1)[off:], stride, total


def case_id(case):
    return "n%d-c%d-stride%dC" % case


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_colsum_from_partials_is_exact(hl, arena, case):
    n, C, mult = case
    for with_ws in (True, False):                                            # (without a workspace nothing is folded)
        L = Launch(arena)
        part, stride, total = make_partials(L, n, C, mult)
        ws = arena.empty((hl.bn_workspace_floats(C),)) if with_ws else None
        db = arena.full((C,), 1.0)
        hl.colsum_from_partials(C, part, n, stride, db, ws)
        L.done()
        exact(case_id(case), "db%s" % ("" if with_ws else " (no workspace)"), db, 1 + total[:C])
        if with_ws:
            # which path ran: up to FOLD_ABOVE slots, and at a width the fold's 256 threads cannot be divided among, the finalize
            # kernel reads the caller's partials and the workspace stays as it was; beyond, the folded sums are written into it
            written = int((ws.view(I32) != POISON).sum())
            folds = n > FOLD_ABOVE and 256 % min(C, 64) == 0
            assert (written > 0) == folds, "%s: %d workspace floats written, fold expected: %s" % (case_id(case), written, folds)
            assert written % (2 * C) == 0 and written <= 512 * 2 * C         # whole [2][C] rows, at most MAX_PART of them


def _bn_params(C, seed):
    rng = np.random.RandomState(seed)
    f = lambda a: np.asarray(a, np.float32)
    return dict(gamma=f(1 + 0.1 * rng.randn(C)), beta=f(0.1 * rng.randn(C)), avg_mean=f(0.2 * rng.randn(C)), avg_var=f(1 + 0.5 * rng.rand(C)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bn_stats_from_partials(hl, arena, case):
    n, C, mult = case
    name, M = case_id(case), 4 * n
    p = _bn_params(C, n + C)
    _, _, total = _ints(n, C)
    st = R.stats_from_sums(total, M, p['gamma'], p['beta'])
    am_ref, av_ref = R.running(p['avg_mean'], p['avg_var'], st, M)
    runs = []
    for tag, with_ws in (("folded", True), ("again", True), ("no workspace", False)):
        L = Launch(arena)
        part, stride, _ = make_partials(L, n, C, mult)
        gamma, beta = L.put(p['gamma']), L.put(p['beta'])
        am, av = arena.put(torch.from_numpy(p['avg_mean']).cuda()), arena.put(torch.from_numpy(p['avg_var']).cuda())
        ws = arena.empty((hl.bn_workspace_floats(C),)) if with_ws else None
        stats = arena.empty((4 * C,))
        hl.bn_stats_from_partials(M, C, part, n, stride, gamma, beta, stats, am, av, ws)
        L.done()
        assert all(bool(torch.isfinite(t).all()) for t in (stats, am, av)), "an output holds a non-finite value"
        if tag != "again":
            for i, k in enumerate(('mean', 'inv_std', 'scale', 'shift')):
                held(name, "%s %s" % (tag, k), stats[i * C:(i + 1) * C], st[k], SUM_TOL)
            held(name, tag + " avg_mean", am, am_ref, SUM_TOL)
            held(name, tag + " avg_var", av, av_ref, SUM_TOL)
        runs.append([t.clone() for t in (stats, am, av)])
    for a, b in zip(runs[0], runs[1]):                                       # a second call on the same partials: the same bits
        assert np.array_equal(raw(a), raw(b)), "%s: two calls on the same partials differ" % name
    # the sums are exact integers whichever path adds them, and the finalize arithmetic is the same code: folded == unfolded
    for a, b in zip(runs[0], runs[2]):
        assert np.array_equal(raw(a), raw(b)), "%s: the folded and the unfolded path differ" % name


def _bwd_inputs(C, seed, bf16):
    """g, y [BWD_ROWS][C], stats (mean, inv_std, scale, shift) and gamma as fp32 values (bf16-representable g, y when bf16);
    g is zeroed where the pre-activation lies within KINK of the activation's kink"""
    rng = np.random.RandomState(seed)
    f = lambda a: np.asarray(a, np.float32)
    y, g = f(rng.randn(BWD_ROWS, C) * 1.7 + 0.3), f(rng.randn(BWD_ROWS, C))
    if bf16:
        y, g = R._bf16_round(y), R._bf16_round(g)
    gamma0, beta0 = f(1 + 0.1 * rng.randn(C)), f(0.1 * rng.randn(C))
    mean, inv_std = f(0.3 * rng.randn(C)), f(rng.uniform(0.5, 2.0, C))
    scale = f(gamma0 * inv_std)
    shift = f(beta0 - mean * scale)
    st = dict(mean=mean.astype(np.float64), inv_std=inv_std.astype(np.float64), scale=scale.astype(np.float64), shift=shift.astype(np.float64))
    keep = np.abs(y.astype(np.float64) * st['scale'] + st['shift']) > R.KINK
    g = g * keep
    return y, g, st, f(np.concatenate([mean, inv_std, scale, shift])), f(gamma0 * 1.01)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bn_act_bwd_from_partials(hl, arena, case, bf16):
    n, C, mult = case
    name = case_id(case) + (" bf16" if bf16 else "")
    M, act = BWD_ROWS, R.ACT_LRELU
    y, g, st, stats_np, gamma_cur = _bwd_inputs(C, n + 3 * C, bf16)
    L = Launch(arena)
    part, stride, total = make_partials(L, n, C, mult)
    yd, gd = L.put(y, BF if bf16 else F32), L.put(g, BF if bf16 else F32)
    stats, gamma = L.put(stats_np), L.put(gamma_cur)
    ws = arena.empty((hl.bn_workspace_floats(C),))
    gx, dgamma, dbeta = arena.empty((M, C)), arena.full((C,), 1.0), arena.full((C,), 1.0)
    hl.bn_act_bwd_from_partials(M, C, gd, yd, stats, gamma, act, part, n, stride, gx, dgamma, dbeta, ws)
    L.done()
    exact(name, "dbeta", dbeta, 1 + total[:C])                               # the first columns are sum g'
    exact(name, "dgamma", dgamma, 1 + total[C:])                             # the second sum g' x_hat
    assert bool(torch.isfinite(gx).all()), "gx holds a non-finite value"
    gx_ref, _, _ = R.bwd_from_sums(y, g, st, gamma_cur, act, total, total, M)
    held(name, "gx", gx, gx_ref, BWD_TOL)


def _boundary_slots(n):
    """first, last, and both sides of the first two and the last two multiples of each chunk length the header's "folded in a
    fixed order" can mean here: 32, 33 (= ceil(16385 / 512)) and 79 (= ceil(40001 / 512)) -- computed from n alone"""
    slots = {0, n - 1}
    for per in (32, 33, 79):
        last = (n - 1) // per
        for k in (1, 2, last - 1, last):
            if 0 < k * per < n:
                slots |= {k * per - 1, k * per}
    return sorted(slots)


@pytest.mark.parametrize("n", [97, 16385, 40001])
def test_one_hot_slot_is_counted_once(hl, arena, n):
    """all partials zero but 1.0 in every column of ONE slot: the column sums must be exactly 1.0 wherever the slot lies -- at
    the ends of the list and on both sides of the chunk boundaries of a fold"""
    C = 64
    arena.reset()
    part = arena.zeros((n, 2 * C))
    ws = arena.empty((hl.bn_workspace_floats(C),))
    db = arena.empty((C,))
    slots = _boundary_slots(n)
    assert len(slots) >= 12
    for s in slots:
        part[s] = 1.0
        db.zero_()
        hl.colsum_from_partials(C, part, n, 2 * C, db, ws)
        arena.check()
        assert bool((db == 1.0).all()), "n_slots %d: slot %d is counted %r times" % (n, s, db.cpu().numpy().tolist())
        assert bool((part[s] == 1.0).all()) and float(part.sum()) == 2 * C, "the launch wrote to its partials"
        part[s] = 0.0
    assert not bool(part.any())
    print("PARITY n_slots %-14d one-hot at slots %s: column sums exactly 1.0" % (n, slots))


# ---- the column passes themselves: mcg_colsum_acc and mcg_bn_sums on integer-valued tensors ----
# plan_partial's extremes: C = 4 has 256 row lanes and 2048 rows a block at least, C = 1024 one row lane and 8 rows a block;
# 512 * 2048 + 5 rows of C = 4 and 4099 of C = 1024 are more than MAX_PART = 512 blocks of the least size can take
COLUMN_CASES = [(1, 4), (2047, 4), (2048, 4), (2049, 4), (512 * 2048 + 5, 4), (7, 1024), (8, 1024), (9, 1024), (4099, 1024), (37, 8)]


@pytest.mark.parametrize("M,C", COLUMN_CASES)
def test_column_passes_are_exact_on_integers(hl, arena, M, C):
    rng = np.random.RandomState(M % 1000 + C)
    v = rng.randint(-2, 3, (M, C)).astype(np.float32)
    s, ss = v.sum(0, dtype=np.float64), (v * v).sum(0, dtype=np.float64)
    assert max(np.abs(s).max(), ss.max()) < 2 ** 24 and 4 * M < 2 ** 24
    L = Launch(arena)
    vd = L.put(v)
    ws = arena.empty((hl.bn_workspace_floats(C),))
    db, sums = arena.full((C,), 1.0), arena.empty((2 * C,), F64)
    hl.colsum_acc(M, C, vd, db, ws)
    L.done()
    exact((M, C), "colsum_acc", db, 1 + s)
    hl.bn_sums(M, C, vd, sums, ws)
    L.done()
    exact((M, C), "bn_sums", sums, np.concatenate([s, ss]))
    print("PARITY M %-8d C %-5d colsum_acc, bn_sums: exactly the integer sums" % (M, C))
