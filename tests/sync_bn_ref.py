"""Synchronised BatchNorm stated in float64 on shards: what mcg_bn_sums -> (all-reduce) -> mcg_bn_stats_from_sums and
mcg_bn_bwd_sums -> (all-reduce) -> mcg_bn_act_bwd_from_sums compute when rank k holds the rows y_k [M_k][C] and the output
gradient g_k of one global batch of M_total = sum M_k rows.

Only per-channel SUMS cross the ranks.  The statistics, the running averages (Chainer 3.1's m / max(m - 1, 1) of the GLOBAL row
count) and the two coefficients of gx come from the total of the shards' sums; dgamma and dbeta are each shard's OWN sums (the
gradient exchange adds the ranks' parameter gradients afterwards, so a global sum here would be counted `world` times).
tests/test_sync_bn_ref_cpu.py holds this statement to oracle.functions.bn_train_fwd / bn_train_bwd on the concatenated batch."""
import numpy as np

ACT_RELU, ACT_LRELU = 1, 2              # MCG_ACT_*
LRELU_SLOPE = 0.2
EPS, DECAY = 2e-5, 0.9


def _f64(a):
    return np.asarray(a, np.float64)


def act_mask(pre, act):
    """act'(pre): relu masks pre <= 0, leaky_relu scales pre < 0 (the oracle's relu_bwd / leaky_relu_bwd on the retained output)"""
    if act == ACT_RELU:
        return np.where(pre > 0, 1.0, 0.0)
    if act == ACT_LRELU:
        return np.where(pre < 0, LRELU_SLOPE, 1.0)
    raise ValueError(act)


def fwd_sums(y):
    """[sum y | sum y^2] of one shard, (2C,)"""
    y = _f64(y)
    return np.concatenate([y.sum(0), (y * y).sum(0)])


def stats_from_sums(total, m_total, gamma, beta, eps=EPS):
    """dict(mean, var (eps included), inv_std, scale, shift) of the global batch from the total of the shards' fwd_sums"""
    total = _f64(total)
    C = total.size // 2
    mean = total[:C] / m_total
    var = np.maximum(total[C:] / m_total - mean * mean, 0.0) + eps       # Chainer 3.1: var += eps before everything else
    inv_std = 1.0 / np.sqrt(var)
    scale = _f64(gamma) * inv_std
    return dict(mean=mean, var=var, inv_std=inv_std, scale=scale, shift=_f64(beta) - mean * scale)


def running(avg_mean, avg_var, st, m_total, decay=DECAY):
    """the running averages after this batch: (avg_mean', avg_var'), unbiased by the GLOBAL row count"""
    adjust = m_total / max(m_total - 1.0, 1.0)
    return _f64(avg_mean) * decay + (1 - decay) * st['mean'], _f64(avg_var) * decay + (1 - decay) * adjust * st['var']


def _g_bn(y, g, st, act):
    y = _f64(y)
    return _f64(g) * act_mask(y * st['scale'] + st['shift'], act), (y - st['mean']) * st['inv_std']


def bwd_sums(y, g, st, act):
    """[sum g' | sum g' x_hat] of one shard, g' = g * act'(y * scale + shift), (2C,)"""
    gb, xh = _g_bn(y, g, st, act)
    return np.concatenate([gb.sum(0), (gb * xh).sum(0)])


def bwd_from_sums(y, g, st, gamma_cur, act, local, total, m_total):
    """(gx_k, dgamma_k, dbeta_k) of one shard: gx from the GLOBAL sums `total` over m_total rows, dgamma / dbeta the shard's own
    `local` sums.  gamma_cur: the parameter as it is NOW (quirk Q5: Adam may have updated it since the forward pass)."""
    gb, xh = _g_bn(y, g, st, act)
    C = gb.shape[1]
    local, total = _f64(local), _f64(total)
    gx = _f64(gamma_cur) * st['inv_std'] * (gb - (xh * total[C:] + total[:C]) / m_total)
    return gx, local[C:].copy(), local[:C].copy()


def forward(ys, gamma, beta, avg_mean=None, avg_var=None, eps=EPS, decay=DECAY):
    """shards -> dict(sums=[per shard], total, m_total, st, avg_mean, avg_var)"""
    sums = [fwd_sums(y) for y in ys]
    m_total = sum(len(y) for y in ys)
    total = np.sum(sums, axis=0)
    st = stats_from_sums(total, m_total, gamma, beta, eps)
    out = dict(sums=sums, total=total, m_total=m_total, st=st, avg_mean=None, avg_var=None)
    if avg_mean is not None:
        out['avg_mean'], out['avg_var'] = running(avg_mean, avg_var, st, m_total, decay)
    return out


def backward(ys, gs, fwd, gamma_cur, act):
    """shards -> dict(sums=[per shard], total, gx=[...], dgamma=[...], dbeta=[...])"""
    st, m_total = fwd['st'], fwd['m_total']
    sums = [bwd_sums(y, g, st, act) for y, g in zip(ys, gs)]
    total = np.sum(sums, axis=0)
    res = [bwd_from_sums(y, g, st, gamma_cur, act, s, total, m_total) for y, g, s in zip(ys, gs, sums)]
    return dict(sums=sums, total=total, gx=[r[0] for r in res], dgamma=[r[1] for r in res], dbeta=[r[2] for r in res])


# ---- the cases of tests/test_sync_bn_ref_cpu.py and tests/test_gpu_sync_bn.py ----
NT, MAX_PART = 256, 512                 # small_ops.hip: threads of a block, cap on the blocks of the partial sums


def plan_partial(M, C):
    """(blocks, rows_per_block) of col_partial_kernel: small_ops.hip's plan_partial, restated"""
    min_rows = NT // (C >> 2) * 8
    b = min(max(-(-M // min_rows), 1), MAX_PART)
    rpb = -(-M // b)
    return -(-M // rpb), rpb


# name: (C, shard rows, act, blocks of each shard's partial sums as plan_partial gives them at this commit)
CASES = {
    # one block whose 256 row lanes (C/4 = 1 column) find one row; M_total = 2: the running variance's adjust is 2 / max(1, 1) = 2
    "c4-two-rows": (4, (1, 1), ACT_RELU, (1, 1)),
    "c4-one-row": (4, (1,), ACT_LRELU, (1,)),                      # M_total = 1: adjust = 1 / max(0, 1) = 1
    # three unequal shards; with a bf16 tensor C = 8 is ONE eight-wide column (256 row lanes, at most 37 rows)
    "c8-three-shards": (8, (37, 5, 22), ACT_LRELU, (1, 1, 1)),
    # 16 row lanes, 128 rows a block at least: ceil(5000 / 128) = 40 blocks of 125 rows, 24 of 125 -- each of the finalize
    # kernel's 32 slices has one or two partials (fewer than the eight its unrolled loop takes), none is empty
    "c64": (64, (5000, 3000), ACT_LRELU, (40, 24)),
    # 2 row lanes, 16 rows a block: 263 blocks -- slices 0..38 take one eight-in-flight trip (b + 224 < 263) and a tail of one,
    # the others a tail of eight; the second shard has 4 blocks (28 empty slices)
    "c512": (512, (4200, 64), ACT_RELU, (263, 4)),
    # 8 row lanes, 64 rows a block: 625 wanted, capped at MAX_PART = 512 -> 79 rows each -> 507 blocks (workspace nearly full)
    "c128-block-cap": (128, (40000, 777), ACT_LRELU, (507, 13)),
    # the widest supported width: C / 4 = 256 columns, ONE row lane, 8 rows a block
    "c1024": (1024, (50, 3), ACT_RELU, (7, 1)),
}
for _name, (_C, _rows, _act, _blocks) in CASES.items():
    assert tuple(plan_partial(m, _C)[0] for m in _rows) == _blocks, (_name, [plan_partial(m, _C) for m in _rows])

KINK = 1e-4                             # |pre-activation| up to this: the output gradient is zeroed (tests/test_gpu_ops.py, _bn_edge_fwd_bwd)
MAX_DROPPED = 1e-3                      # share of a case's elements that may be zeroed so


def case_inputs(name, bf16_values=False):
    """Seeded fp32-representable inputs of a case (float64 arrays holding fp32 values): shards ys, gs (kink-masked), gamma, beta,
    gamma_cur (Q5), the running averages' start -- test_batchnorm_activation_fwd_bwd's distributions.  The C = 4 cases instead
    take multiples of 1/8 in [-2, 2], so every fp32 sum of y, y^2, g is exact; the two rows of a channel differ by 0 or 1/8:
    gx of a two-row batch is gamma inv_std g' (1 - x_hat^2) / 2-sized with 1 - x_hat^2 = eps / var, so the fp32 rounding of
    inv_std alone (2^-24) moves it by 2^-23 var / eps of itself -- 2e-5 at var = (1/16)^2, but 6e-3 at var = 1: rows further
    apart would fail BWD_TOL from the conditioning of the float64 function, on any correct fp32 code.
    bf16_values: y and g rounded to bf16-representable values (for the bf16 flag forms)."""
    C, rows, act, _ = CASES[name]
    rng = np.random.RandomState(1000 + C + sum(rows))
    m_total = sum(rows)
    if C == 4:
        y = rng.randint(-15, 16, (m_total, C)) / 8.0
        if m_total == 2:
            y[1] = y[0] + np.array([1, 0, -1, 1]) / 8.0
        g = rng.randint(-16, 17, (m_total, C)) / 8.0
        g[g == 0] = 0.125
    else:
        y = (rng.randn(m_total, C) * 1.7 + 0.3).astype(np.float32)
        g = rng.randn(m_total, C).astype(np.float32)
    if bf16_values:
        y, g = _bf16_round(y), _bf16_round(g)
    y, g = _f64(y), _f64(g)
    gamma = _f64((1 + 0.1 * rng.randn(C)).astype(np.float32))
    beta = _f64((0.1 * rng.randn(C)).astype(np.float32))
    gamma_cur = _f64((gamma * 1.01).astype(np.float32))
    avg_mean, avg_var = _f64((0.2 * rng.randn(C)).astype(np.float32)), _f64((1 + 0.5 * rng.rand(C)).astype(np.float32))
    st = stats_from_sums(fwd_sums(y), m_total, gamma, beta)
    keep = np.abs(y * st['scale'] + st['shift']) > KINK
    dropped = 1.0 - keep.mean()
    g = g * keep
    cuts = np.cumsum(rows)[:-1]
    return dict(C=C, rows=rows, act=act, m_total=m_total, ys=np.split(y, cuts), gs=np.split(g, cuts), gamma=gamma, beta=beta,
                gamma_cur=gamma_cur, avg_mean=avg_mean, avg_var=avg_var, dropped=dropped)


def _bf16_round(a):
    """round-to-nearest-even to bf16, as fp32 values"""
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)
