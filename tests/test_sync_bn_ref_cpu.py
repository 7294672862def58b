"""tests/sync_bn_ref.py (synchronised BatchNorm on shards, float64) against the oracle's BatchNorm on the concatenated batch.

The two differ in how the variance is formed: the oracle's is the mean of (y - mean)^2, the sharded statement's -- like the
device's -- is sum y^2 / M - mean^2 from the shards' sums, which cancels.  In float64 the cancellation costs a few 2^-53 of
sum y^2 / M (about 3 for these inputs, at most 4 in the C = 4 cases) ABSOLUTELY: some 1e-15, which the smallest variance there
can be, eps = 2e-5 for a channel whose rows are equal, turns into 1e-10 of the variance and of everything derived from it.  TOL
is ten times that; measured: exact on the C = 4 cases (their sums are exact), 2e-14 at 40 777 rows."""
import numpy as np
import pytest

import sync_bn_ref as R
from oracle import functions as F

TOL = 1e-9


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def close(a, b):
    """rel-L2 within TOL (<=: the one-row batch's gx is exactly zero on both sides)"""
    b = np.asarray(b, np.float64)
    return np.linalg.norm(np.asarray(a, np.float64) - b) <= TOL * np.linalg.norm(b)


@pytest.mark.parametrize("act", [R.ACT_RELU, R.ACT_LRELU])
@pytest.mark.parametrize("name", list(R.CASES))
def test_sharded_statement_equals_the_oracle_on_the_whole_batch(name, act):
    d = R.case_inputs(name)
    C, M = d['C'], d['m_total']
    assert d['dropped'] <= R.MAX_DROPPED, d['dropped']
    y, g = np.concatenate(d['ys']), np.concatenate(d['gs'])
    am, av = d['avg_mean'].copy(), d['avg_var'].copy()
    bn, cache = F.bn_train_fwd(y.T.reshape(1, C, M, 1), d['gamma'], d['beta'], am, av)
    out = F.relu_fwd(bn) if act == R.ACT_RELU else F.leaky_relu_fwd(bn)
    g4 = g.T.reshape(1, C, M, 1)
    g_bn = F.relu_bwd(out, g4) if act == R.ACT_RELU else F.leaky_relu_bwd(out, g4)
    gx_ref, gg_ref, gb_ref = F.bn_train_bwd(cache, d['gamma_cur'], g_bn)             # Q5: the updated gamma

    fwd = R.forward(d['ys'], d['gamma'], d['beta'], d['avg_mean'], d['avg_var'])
    st = fwd['st']
    assert close(st['mean'], cache['mean']) and close(st['inv_std'], cache['inv_std'])
    assert close(st['scale'], d['gamma'] * cache['inv_std']) and close(st['shift'], d['beta'] - cache['mean'] * d['gamma'] * cache['inv_std'])
    assert close(y * st['scale'] + st['shift'], bn[0, :, :, 0].T)
    assert close(fwd['avg_mean'], am) and close(fwd['avg_var'], av)
    assert not np.array_equal(fwd['avg_mean'], d['avg_mean']) and not np.array_equal(fwd['avg_var'], d['avg_var'])

    bwd = R.backward(d['ys'], d['gs'], fwd, d['gamma_cur'], act)
    assert close(np.concatenate(bwd['gx']), gx_ref[0, :, :, 0].T)
    assert close(np.sum(bwd['dgamma'], axis=0), gg_ref) and close(np.sum(bwd['dbeta'], axis=0), gb_ref)
    # dgamma / dbeta are LOCAL: one shard's are not the batch's unless it is the only shard
    if len(d['rows']) > 1:
        assert rel(bwd['dbeta'][0], gb_ref) > 1e-3
    print("%s act %d: gx %.1e, inv_std %.1e, avg_var %.1e, dropped %.1e" % (
        name, act, rel(np.concatenate(bwd['gx']), gx_ref[0, :, :, 0].T), rel(st['inv_std'], cache['inv_std']), rel(fwd['avg_var'], av), d['dropped']))


def test_running_variance_is_unbiased_by_the_global_row_count():
    st = dict(mean=np.zeros(2), var=np.ones(2))
    assert np.allclose(R.running(np.zeros(2), np.zeros(2), st, 1)[1], 0.1)            # m = 1: m / max(m - 1, 1) = 1
    assert np.allclose(R.running(np.zeros(2), np.zeros(2), st, 2)[1], 0.2)            # m = 2: 2
    assert np.allclose(R.running(np.zeros(2), np.zeros(2), st, 5)[1], 0.125)          # m = 5: 5 / 4


def test_bf16_rounding_helper_matches_torch():
    import torch
    a = np.random.RandomState(0).randn(4096).astype(np.float32)
    assert np.array_equal(R._bf16_round(a), torch.tensor(a).to(torch.bfloat16).float().numpy())
