"""The full-window layers (mcg_fc_fprop / mcg_fc_dgrad / mcg_fc_wgrad) in the guard arena, element by element against float64.

Every operand and output of a launch is a view into ONE poisoned arena (tests/guard.py).  For every row of tests/fc_ref.py's FC_CASES
-- the loop, tile and split edges of the eight launch paths -- and every variant of it (bias or none; no bias plane, period 4,
period K; db or none):
  * the margins are intact after every launch (no store leaves its tensor);
  * the forward output and the input gradient start as poison, dw / db from non-trivial values: every element is finite (no poison
    left, no out-of-tensor load consumed) and within fc_ref.bound of the float64 statement -- the DERIVED bound (L + 8) 2^-24 S of an
    fp32 inner product in any order, which tests/test_fc_ref_cpu.py shows every defect of its list to leave on these very inputs;
    outputs of 64 elements and more also hold the project's relative-L2 limits;
  * the inputs are bit-identical afterwards;
  * a second launch from the same starting state agrees bit for bit where nothing is added atomically, within 2 x bound where it is;
  * a weight gradient called twice accumulates: the second result is held to the reference that starts from the first;
  * a forward GEMM that splits K gives the right result from a POISONED y: the clear ahead of its atomics happened.
Refused argument sets (their status codes are pinned without a device in tests/test_cabi_cpu.py) leave every output as poison.  The
last test asserts that the (pass, path, split kind) combinations that ran are the ones the table promises.  Worst |error| / bound per
path as measured on an MI355X: profiles/fc_loss_parity.md."""
import numpy as np
import pytest
import torch

from guard import Arena, POISON
import fc_ref as FR

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 1e-5, 1e-4
RAN = set()                                # (pass, path, split kind)
RATIO = {}                                 # (pass, path, split kind, output) -> worst |error| / bound

PROMISED = {('fprop', 'dot', 'single'), ('fprop', 'gemm', 'single'), ('fprop', 'gemm', 'equal'), ('fprop', 'gemm', 'ragged'),
            ('dgrad', 'row1', 'single'), ('dgrad', 'rows8', 'single'),
            ('wgrad', 'slices', 'single'), ('wgrad', 'gemm', 'single'), ('wgrad', 'gemm', 'equal'), ('wgrad', 'gemm', 'ragged')}


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(16 << 20)


def _words(t):
    return t.reshape(-1).view(torch.int32)


def _bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_words(a), _words(b))


def _is_poison(t):
    return bool((_words(t) == POISON).all())


def _poison(t):
    _words(t).fill_(POISON)


def _np(t):
    return t.detach().cpu().double().numpy()


def _put(arena, a):
    return None if a is None else arena.put(torch.from_numpy(np.ascontiguousarray(a)))


def _rel_l2(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _accept(tag, key, what, out, ref, L, S, tol):
    """finite, every element within the bound, the whole within the project's relative-L2 limit; the figures first"""
    o = _np(out)
    ratio = FR.worst_ratio(o, ref, L, S)
    rel = _rel_l2(o, ref) if np.isfinite(o).all() else float('inf')
    print("fc-guard %s %s: worst |err| / bound %.3f, rel-L2 %.2e" % (tag, what, ratio, rel))
    RATIO[key + (what,)] = max(RATIO.get(key + (what,), 0.0), ratio)
    bad = np.argwhere(FR.violations(o, ref, L, S))
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        assert False, "%s %s: %d of %d elements outside the bound, first at %s: %r against %r (bound %.3e)" % (
            tag, what, len(bad), o.size, at, float(o[at]), float(ref[at]), float(FR.bound(L, S)[at]))
    if o.size >= 64:
        assert rel < tol, (tag, what, rel)


def _agree(tag, what, a, b, atomic, L, S):
    """two launches from the same starting state"""
    if not atomic:
        assert _bit_equal(a, b), "%s %s: a second launch differs (no atomics on this path)" % (tag, what)
        return
    assert not FR.violations(_np(a), _np(b), L, S, scale=2.0).any(), "%s %s: two launches further apart than 2 x bound" % (tag, what)
    print("fc-guard %s %s: second launch %s" % (tag, what, "bit-identical" if _bit_equal(a, b) else "differs inside 2 x bound (atomics)"))


def _unchanged(tag, tensors, snaps):
    for i, (t, s) in enumerate(zip(tensors, snaps)):
        assert _bit_equal(t, s), "%s: input %d was written" % (tag, i)


def _run_fprop(hl, arena, case, var, tag, key):
    _, M, K, Co, _, _ = case
    d = FR.inputs(case)
    bias = d['bias'] if var['bias'] else None
    x, w, b = _put(arena, d['x']), _put(arena, d['w']), _put(arena, bias)
    y = arena.empty((M, Co))
    ins = [t for t in (x, w, b) if t is not None]
    snaps = [t.clone() for t in ins]
    ref, S = FR.fprop(d['x'], d['w'], bias)
    hl.fc_fprop(M, K, Co, x, w, b, y)                      # y is poison: a GEMM that splits K must have cleared it first
    arena.check()
    y1 = y.clone()
    _accept(tag, key, 'y', y1, ref, K, S, FWD_TOL)
    _unchanged(tag, ins, snaps)
    _poison(y)
    hl.fc_fprop(M, K, Co, x, w, b, y)
    arena.check()
    _agree(tag, 'y', y, y1, FR.atomic('fprop', M, K, Co), K, S)
    _unchanged(tag, ins, snaps)


def _run_dgrad(hl, arena, case, var, tag, key):
    _, M, K, Co, _, _ = case
    d = FR.inputs(case)
    period = var['period']
    bias = {0: None, 4: d['bias4'], K: d['biasK']}[period]
    gy, w, b = _put(arena, d['gy']), _put(arena, d['w']), _put(arena, bias)
    gx = arena.empty((M, K))
    ins = [t for t in (gy, w, b) if t is not None]
    snaps = [t.clone() for t in ins]
    ref, S = FR.dgrad(d['gy'], d['w'], bias, period)
    hl.fc_dgrad(M, K, Co, gy, w, b, period, gx)
    arena.check()
    g1 = gx.clone()
    _accept(tag, key, 'x', g1, ref, Co, S, FWD_TOL)
    _unchanged(tag, ins, snaps)
    _poison(gx)
    hl.fc_dgrad(M, K, Co, gy, w, b, period, gx)
    arena.check()
    _agree(tag, 'x', gx, g1, False, Co, S)
    _unchanged(tag, ins, snaps)


def _run_wgrad(hl, arena, case, var, tag, key):
    _, M, K, Co, _, _ = case
    d = FR.inputs(case)
    with_db = var['db']
    atomic = FR.atomic('wgrad', M, K, Co, with_db)
    x, gy = _put(arena, d['x']), _put(arena, d['gy'])
    dw, db = _put(arena, d['dw0']), _put(arena, d['db0'] if with_db else None)
    ins, snaps = [x, gy], [x.clone(), gy.clone()]
    ref, S, rb, Sb = FR.wgrad(d['x'], d['gy'], d['dw0'], d['db0'] if with_db else None)
    hl.fc_wgrad(M, K, Co, x, gy, dw, db)
    arena.check()
    dw1, db1 = dw.clone(), (db.clone() if with_db else None)
    _accept(tag, key, 'dw', dw1, ref, M, S, BWD_TOL)
    if with_db:
        _accept(tag, key, 'db', db1, rb, M, Sb, BWD_TOL)
    _unchanged(tag, ins, snaps)
    # called again it accumulates: the reference that starts from what the first call left (as the device holds it)
    ref2, S2, rb2, Sb2 = FR.wgrad(d['x'], d['gy'], dw1.cpu().numpy(), db1.cpu().numpy() if with_db else None)
    hl.fc_wgrad(M, K, Co, x, gy, dw, db)
    arena.check()
    _accept(tag, key, 'dw', dw, ref2, M, S2, BWD_TOL)
    if with_db:
        _accept(tag, key, 'db', db, rb2, M, Sb2, BWD_TOL)
    _unchanged(tag, ins, snaps)
    # and once more from the starting state
    dw.copy_(torch.from_numpy(d['dw0']))
    if with_db:
        db.copy_(torch.from_numpy(d['db0']))
    hl.fc_wgrad(M, K, Co, x, gy, dw, db)
    arena.check()
    _agree(tag, 'dw', dw, dw1, atomic, M, S)
    if with_db:
        _agree(tag, 'db', db, db1, False, M, Sb)
    _unchanged(tag, ins, snaps)


@pytest.mark.parametrize("case", FR.FC_CASES, ids=[FR.case_id(c) for c in FR.FC_CASES])
def test_fc_case_in_the_arena(hl, arena, case):
    pass_, M, K, Co, opts, pins = case
    with_db = 'db' in opts
    key = (pass_, FR.branch(pass_, M, K, Co, with_db), FR.split_kind(pass_, M, K, Co, with_db))
    run = {'fprop': _run_fprop, 'dgrad': _run_dgrad, 'wgrad': _run_wgrad}[pass_]
    for var in FR.variants(case):
        arena.reset()
        tag = "%s %s/%s n=%d %s" % (FR.case_id(case), key[1], key[2], FR.split(pass_, M, K, Co)[0] if key[1] == 'gemm' else 1,
                                    ",".join("%s=%s" % kv for kv in sorted(var.items())))
        run(hl, arena, case, var, tag, key)
    RAN.add(key)


def test_refused_shapes_leave_the_outputs_poison(hl, arena):
    """K % 4 != 0; a bias plane of period 0, 6 or one that does not divide K; M or Co <= 0: MCG_ERR_BAD_ARG before anything is
    launched (the codes themselves: tests/test_cabi_cpu.py) -- seen here from the device's side: no output word changes."""
    arena.reset()
    M, K, Co = 8, 16, 8
    rng = np.random.RandomState(5)
    x, w, gy = (_put(arena, rng.randn(*s).astype(np.float32)) for s in ((M, K), (Co, K), (M, Co)))
    b, plane = _put(arena, rng.randn(Co).astype(np.float32)), _put(arena, rng.randn(K).astype(np.float32))
    y, gx, dw, db = arena.empty((M, Co)), arena.empty((M, K)), arena.empty((Co, K)), arena.empty((Co,))
    refused = 0
    for m, k, co in ((M, 6, Co), (M, 14, Co), (0, K, Co), (-8, K, Co), (M, K, 0), (M, K, -1)):
        for call in (lambda: hl.fc_fprop(m, k, co, x, w, b, y), lambda: hl.fc_dgrad(m, k, co, gy, w, plane, 4, gx),
                     lambda: hl.fc_dgrad(m, k, co, gy, w, None, 0, gx), lambda: hl.fc_wgrad(m, k, co, x, gy, dw, db),
                     lambda: hl.fc_wgrad(m, k, co, x, gy, dw, None)):
            with pytest.raises(hl.McgError, match="MCG_ERR_BAD_ARG"):
                call()
            refused += 1
    for period in (0, 6, 12, 32, -4):                       # zero, no multiple of 4, no divisor of K (twice), negative
        with pytest.raises(hl.McgError, match="MCG_ERR_BAD_ARG"):
            hl.fc_dgrad(M, K, Co, gy, w, plane, period, gx)
        refused += 1
    assert refused == 35
    arena.check()
    assert all(_is_poison(t) for t in (y, gx, dw, db))


def test_every_promised_path_ran():
    """(pass, path, split kind): what the table promises, what fc_ref derives from it, and what ran are one set"""
    table = {(c[0], FR.branch(c[0], c[1], c[2], c[3], 'db' in c[4]), FR.split_kind(c[0], c[1], c[2], c[3], 'db' in c[4])) for c in FR.FC_CASES}
    assert table == PROMISED
    assert RAN == PROMISED, sorted(PROMISED - RAN)
    for key in sorted(RATIO):
        print("fc-guard worst |err| / bound  %-6s %-7s %-7s %-3s %.3f" % (key + (RATIO[key],)))
