"""tests/fc_ref.py held to account without a device: the case table reaches the launch paths and split plans it claims, the float64
statements agree with values worked out by hand, and -- the condition that keeps tests/test_gpu_fc_guard.py from hiding a failure --
for EVERY row of the table, with the GPU test's own seeded inputs, each defect the table is there to find moves at least one element
out of fc_ref.bound.  No GPU, no library call."""
from collections import Counter

import numpy as np
import pytest

import fc_ref as FR

IDS = [FR.case_id(c) for c in FR.FC_CASES]


def test_table_rows_are_distinct_and_small():
    assert len(set(IDS)) == len(IDS)
    for pass_, M, K, Co, opts, pins in FR.FC_CASES:
        assert pass_ in ('fprop', 'dgrad', 'wgrad') and K % 4 == 0 and set(opts) <= {'db'} and pins
        assert 4 * max(M * K, Co * K, M * Co) <= 65 * 1024 * 4, (pass_, M, K, Co)          # no tensor beyond 65 x 1024 floats (260 KB)
        assert M * K * Co <= 64 * 1024 * 65                                                # ... and no launch beyond 4.3 M products


def test_table_reaches_every_branch_twice():
    hit = Counter((c[0], FR.branch(c[0], c[1], c[2], c[3], 'db' in c[4])) for c in FR.FC_CASES)
    for key in (('fprop', 'gemm'), ('fprop', 'dot'), ('dgrad', 'rows8'), ('dgrad', 'row1'), ('wgrad', 'gemm'), ('wgrad', 'slices')):
        assert hit[key] >= 2, (key, hit)
    assert len(hit) == 6
    for c in FR.FC_CASES:                                     # the row's own words name the path it takes
        assert c[5].startswith(FR.branch(c[0], c[1], c[2], c[3], 'db' in c[4]) + ":"), c


def test_table_reaches_every_split_kind_on_both_gemms():
    kinds = {(c[0], FR.split_kind(c[0], c[1], c[2], c[3], 'db' in c[4])) for c in FR.FC_CASES
             if FR.branch(c[0], c[1], c[2], c[3], 'db' in c[4]) == 'gemm'}
    assert kinds == {(p, k) for p in ('fprop', 'wgrad') for k in ('single', 'equal', 'ragged')}
    # a weight-gradient GEMM whose last 32-row step is cut by M inside a split's last chunk, and inside an unsplit one
    cut = [(M, FR.split('wgrad', M, K, Co)) for p, M, K, Co, o, _ in FR.FC_CASES if p == 'wgrad' and FR.branch(p, M, K, Co, 'db' in o) == 'gemm' and M % 32]
    assert any(n >= 2 for _, (n, _) in cut) and any(n == 1 for _, (n, _) in cut)


def test_split_plans_are_the_ones_the_table_names():
    """the plans as csrc/conv_gemm.hip's plan_ksplit / plan_pixsplit produce them for the table's GEMM shapes"""
    want = {('fprop', 64, 64, 16): (1, 64), ('fprop', 64, 448, 16): (1, 448), ('fprop', 64, 512, 16): (2, 256),
            ('fprop', 64, 576, 16): (2, 320), ('fprop', 65, 832, 17): (3, 320), ('fprop', 64, 1024, 65): (4, 256),
            ('wgrad', 64, 64, 16): (1, 64), ('wgrad', 65, 64, 16): (1, 96), ('wgrad', 127, 68, 20): (1, 128),
            ('wgrad', 256, 64, 16): (2, 128), ('wgrad', 300, 64, 16): (2, 160), ('wgrad', 300, 132, 68): (2, 160)}
    got = {c[:4]: FR.split(*c[:4]) for c in FR.FC_CASES if FR.branch(c[0], c[1], c[2], c[3], 'db' in c[4]) == 'gemm'}
    assert got == want
    assert FR.split('fprop', 3, 1024, 7) == (1, 1024) and FR.split('dgrad', 64, 64, 11) == (1, 11) and FR.split('wgrad', 7, 132, 3) == (1, 7)
    # the planner itself at the sizes the step uses (G's dc1 at batch 32: 512 rows, 8192 inputs, 60 outputs)
    assert FR.split('fprop', 512, 8192, 60) == (32, 256) and FR.split('wgrad', 512, 8192, 60) == (4, 128)
    assert not FR.atomic('fprop', 64, 448, 16) and FR.atomic('fprop', 64, 512, 16) and FR.atomic('wgrad', 64, 64, 16)
    assert not FR.atomic('wgrad', 64, 64, 16, True) and not FR.atomic('dgrad', 64, 64, 11)


def test_dispatch_thresholds():
    B = FR.branch
    assert B('fprop', 64, 64, 16) == 'gemm' and B('fprop', 63, 64, 16) == 'dot' and B('fprop', 64, 64, 15) == 'dot' and B('fprop', 64, 96, 16) == 'dot'
    assert B('dgrad', 64, 4, 8) == 'rows8' and B('dgrad', 56, 4, 8) == 'row1' and B('dgrad', 68, 4, 8) == 'row1' and B('dgrad', 64, 4, 7) == 'row1'
    assert B('wgrad', 64, 4, 16) == 'gemm' and B('wgrad', 64, 4, 16, True) == 'slices' and B('wgrad', 64, 4, 18) == 'slices'
    assert B('wgrad', 63, 4, 16) == 'slices' and B('wgrad', 64, 4, 12) == 'slices'


# ---- the references against hand-computed 2 x 4 x 2 cases ----
X = np.array([[1, 2, 3, 4], [-1, 0, 2, -3]], np.float32)          # [M = 2][K = 4]
W = np.array([[1, 0, -1, 2], [0.5, 0.5, 0.5, -0.5]], np.float32)  # [Co = 2][K = 4]
GY = np.array([[1, -2], [3, 0.5]], np.float32)                    # [M = 2][Co = 2]


def test_fprop_by_hand():
    y, S = FR.fprop(X, W, np.array([10, -20], np.float32))
    # row 0: 1 - 3 + 8 = 6, (1 + 2 + 3 - 4) / 2 = 1; row 1: -1 - 2 - 6 = -9, (-1 + 0 + 2 + 3) / 2 = 2
    assert np.array_equal(y, [[16, -19], [1, -18]]) and y.dtype == np.float64
    assert np.array_equal(S, [[1 + 3 + 8 + 10, 5 + 20], [1 + 2 + 6 + 10, 3 + 20]])
    y, S = FR.fprop(X, W, None)
    assert np.array_equal(y, [[6, 1], [-9, 2]]) and np.array_equal(S, [[12, 5], [9, 3]])


def test_dgrad_by_hand():
    x, S = FR.dgrad(GY, W, None, 0)
    # row 0: 1 * W[0] - 2 * W[1] = (0, -1, -2, 3); row 1: 3 * W[0] + 0.5 * W[1] = (3.25, 0.25, -2.75, 5.75)
    assert np.array_equal(x, [[0, -1, -2, 3], [3.25, 0.25, -2.75, 5.75]])
    assert np.array_equal(S, [[2, 1, 2, 3], [3.25, 0.25, 3.25, 6.25]])
    x4, S4 = FR.dgrad(GY, W, np.array([1, 2, 3, -4], np.float32), 4)
    assert np.array_equal(x4, x + [1, 2, 3, -4]) and np.array_equal(S4, S + [1, 2, 3, 4])
    GY8, W8 = np.ones((1, 1), np.float32), np.arange(8, dtype=np.float32).reshape(1, 8)      # a period of 4 inside K = 8
    x8, S8 = FR.dgrad(GY8, W8, np.array([10, 20, 30, 40], np.float32), 4)
    assert np.array_equal(x8, [[10, 21, 32, 43, 14, 25, 36, 47]]) and np.array_equal(S8, x8)
    with pytest.raises(AssertionError):
        FR.dgrad(GY8, W8, np.ones(3, np.float32), 3)


def test_wgrad_by_hand():
    dw0, db0 = np.array([[1, 1, 1, 1], [-2, -2, -2, -2]], np.float32), np.array([0.5, -0.5], np.float32)
    dw, S, db, Sb = FR.wgrad(X, GY, dw0, db0)
    # filter 0: 1 * X[0] + 3 * X[1] = (-2, 2, 9, -5); filter 1: -2 * X[0] + 0.5 * X[1] = (-2.5, -4, -5, -9.5)
    assert np.array_equal(dw, [[-1, 3, 10, -4], [-4.5, -6, -7, -11.5]])
    assert np.array_equal(S, [[1 + 4, 1 + 2, 1 + 9, 1 + 13], [2 + 2.5, 2 + 4, 2 + 7, 2 + 9.5]])
    assert np.array_equal(db, [4.5, -2]) and np.array_equal(Sb, [4.5, 3])
    assert FR.wgrad(X, GY, dw0, None)[2:] == (None, None)


def test_bound_and_acceptance():
    assert FR.bound(1024, 2.0) == (1024 + 8) * 2.0 ** -24 * 2.0
    ref, S = np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 4.0])
    b = FR.bound(8, S)
    assert not FR.violations(ref + [b[0], -b[1], 0], ref, 8, S).any()
    assert FR.violations(ref + [1.01 * b[0], 0, 0], ref, 8, S).tolist() == [True, False, False]
    assert not FR.violations(ref + [1.01 * b[0], 0, 0], ref, 8, S, scale=2).any()
    assert FR.violations([1.0, np.nan, np.inf], ref, 8, S).tolist() == [False, True, True]           # poison left behind violates
    assert FR.worst_ratio(ref + [0.5 * b[0], 0, -0.25 * b[2]], ref, 8, S) == pytest.approx(0.5)
    assert FR.worst_ratio([1.0, np.nan, 3.0], ref, 8, S) == float('inf')
    assert FR.worst_ratio(np.zeros(2), np.zeros(2), 4, np.zeros(2)) == 0.0                          # an exact zero of zero magnitude


# ---- sensitivity: every row, the GPU test's inputs, every applicable defect ----
def _defects(case, var):
    """(name, output with the defect, reference, L, S) for every simulated defect that applies to the launch"""
    pass_, M, K, Co, opts, _ = case
    d = FR.inputs(case)
    x, w, gy = (d[k].astype(np.float64) for k in ('x', 'w', 'gy'))
    n, chunk = FR.split(pass_, M, K, Co) if FR.branch(pass_, M, K, Co, 'db' in opts) == 'gemm' else (1, None)
    out = []
    if pass_ == 'fprop':
        bias = d['bias'] if var['bias'] else None
        ref, S = FR.fprop(d['x'], d['w'], bias)
        add = lambda name, bad: out.append((name, bad, ref, K, S))
        if n >= 2:
            k0 = (n - 1) * chunk
            add("last K chunk dropped", ref - x[:, k0:] @ w[:, k0:].T)
            if bias is not None:
                add("bias added once per chunk", ref + (n - 1) * bias.astype(np.float64)[None, :])
        bad = ref.copy(); bad[M - 1, :] = np.nan
        add("row M-1 not written", bad)
        bad = ref.copy(); bad[:, Co - 1] = np.nan
        add("column Co-1 not written", bad)
    elif pass_ == 'dgrad':
        period = var['period']
        bias = {0: None, 4: d['bias4'], K: d['biasK']}[period]
        ref, S = FR.dgrad(d['gy'], d['w'], bias, period)
        add = lambda name, bad: out.append((name, bad, ref, Co, S))
        bad = ref.copy(); bad[M - 1, :] = np.nan
        add("row M-1 not written", bad)
        add("filter Co-1 skipped", ref - gy[:, Co - 1:] @ w[Co - 1:])
        if Co % 4:
            c0 = Co - Co % 4
            add("last Co % 4 filters skipped", ref - gy[:, c0:] @ w[c0:])
        if period and K > period:
            once = np.concatenate([bias.astype(np.float64), np.zeros(K - period)])
            add("bias plane not repeated", ref - np.tile(bias, K // period)[None, :] + once[None, :])
    else:
        db0 = d['db0'] if var['db'] else None
        ref, S, rb, Sb = FR.wgrad(d['x'], d['gy'], d['dw0'], db0)
        add = lambda name, bad: out.append((name, bad, ref, M, S))
        if n >= 2:
            m0 = (n - 1) * chunk
            add("last M chunk dropped", ref - gy[m0:].T @ x[m0:])
        bad = ref.copy(); bad[Co - 1] = d['dw0'][Co - 1]
        add("column Co-1 not written", bad)
        add("dw0 overwritten", ref - d['dw0'])
        if db0 is not None:
            bad = rb.copy(); bad[Co - 1] = db0[Co - 1]
            out.append(("db[Co-1] not written", bad, rb, M, Sb))
            out.append(("db0 overwritten", rb - db0, rb, M, Sb))
            if M > 256:
                out.append(("db sums its first 256 rows", rb - gy[256:].sum(0), rb, M, Sb))
    return out


@pytest.mark.parametrize("case", FR.FC_CASES, ids=IDS)
def test_every_defect_leaves_the_bound(case):
    pass_, M, K, Co, opts, _ = case
    for var in FR.variants(case):
        defects = _defects(case, var)
        assert len(defects) >= 2
        for name, bad, ref, L, S in defects:
            assert not FR.violations(ref, ref, L, S).any()
            # (the float64 reference rounded to fp32, the best a kernel can store, is inside the bound with room to spare)
            assert FR.worst_ratio(ref.astype(np.float32), ref, L, S) <= 0.5, (name, var)
            assert FR.violations(bad, ref, L, S, scale=2.0).any(), "%s %s: '%s' stays inside the bound" % (FR.case_id(case), var, name)


def test_every_defect_applies_to_some_row():
    """a defect that no row could show would be a hole in the table: each one meets at least two launches"""
    applied = Counter(name for case in FR.FC_CASES for var in FR.variants(case) for name, *_ in _defects(case, var))
    assert set(applied) == {"last K chunk dropped", "bias added once per chunk", "row M-1 not written", "column Co-1 not written",
                            "filter Co-1 skipped", "last Co % 4 filters skipped", "bias plane not repeated", "last M chunk dropped",
                            "dw0 overwritten", "db[Co-1] not written", "db0 overwritten", "db sums its first 256 rows"}
    assert all(v >= 2 for k, v in applied.items() if k != "db sums its first 256 rows"), applied


def test_inputs_are_as_the_sensitivity_needs_them():
    for case in FR.FC_CASES:
        d = FR.inputs(case)
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in d.values())
        assert np.abs(d['gy']).min() >= 0.25 and np.abs(d['x']).min() >= 0.25                # no zero rows
        assert min(np.abs(d[k]).min() for k in ('bias', 'bias4', 'biasK', 'dw0', 'db0')) >= 0.5
        again = FR.inputs(case)
        assert all(np.array_equal(d[k], again[k]) for k in d)
