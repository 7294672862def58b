"""The full-window ("fc") layers mcg_fc_fprop / mcg_fc_dgrad / mcg_fc_wgrad stated in float64, their acceptance bound, the launch path
the library takes for a shape, the split plan of the two MFMA GEMMs, and the case table of tests/test_gpu_fc_guard.py.  NumPy only:
tests/test_fc_ref_cpu.py holds every statement here to hand-computed values and shows, without a device, that the acceptance check
used on the GPU notices each defect the table is there to find.

Conventions (include/mocogan_hip.h): x [M][K], w [Co][K], y / gy [M][Co], dw [Co][K], db [Co]; the input gradient's bias is a plane
of `period` floats added at k % period.  Every reference takes the fp32 values the device holds and computes in float64; beside the
result it returns the element-wise magnitude S = sum |a||b| (+ |bias| or |dw0|) the bound is relative to."""
import numpy as np

U = 2.0 ** -24                      # fp32 unit roundoff


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def fprop(x, w, bias):
    """y = x w^T + bias -> (y, S)"""
    x, w, bias = _f64(x), _f64(w), _f64(bias)
    y, S = x @ w.T, np.abs(x) @ np.abs(w).T
    if bias is not None:
        y, S = y + bias[None, :], S + np.abs(bias)[None, :]
    return y, S


def dgrad(gy, w, bias, period):
    """x = gy w + bias[k % period] -> (x, S)"""
    gy, w, bias = _f64(gy), _f64(w), _f64(bias)
    x, S = gy @ w, np.abs(gy) @ np.abs(w)
    if bias is not None:
        K = w.shape[1]
        assert period > 0 and K % period == 0 and bias.shape == (period,)
        plane = np.tile(bias, K // period)
        x, S = x + plane[None, :], S + np.abs(plane)[None, :]
    return x, S


def wgrad(x, gy, dw0, db0):
    """dw = dw0 + gy^T x, db = db0 + sum_m gy -> (dw, S_dw, db, S_db); db and S_db are None without db0"""
    x, gy, dw0, db0 = _f64(x), _f64(gy), _f64(dw0), _f64(db0)
    dw, S = dw0 + gy.T @ x, np.abs(dw0) + np.abs(gy).T @ np.abs(x)
    if db0 is None:
        return dw, S, None, None
    return dw, S, db0 + gy.sum(0), np.abs(db0) + np.abs(gy).sum(0)


def bound(L, S):
    """The forward error bound of an fp32 inner product of length L in ANY summation order (Higham, Accuracy and Stability, 3.1:
    |fl(a.b) - a.b| <= gamma_L sum |a_i||b_i|, gamma_L ~ L u), with eight more roundings for what surrounds the sum: the bias or the
    accumulated-into value, the partial sums of a split reduction meeting in atomics, the slices meeting in LDS.  Derived, not fitted:
    fused multiply-adds and pairwise orders only stay further inside."""
    return (L + 8) * U * np.asarray(S, np.float64)


def violations(out, ref, L, S, scale=1.0):
    """element-wise: True where `out` is NOT within scale * bound of ref -- a NaN (poison left in place, a consumed out-of-tensor load)
    violates.  The one acceptance check: the GPU test applies it to the kernel's output, the CPU test to simulated defects."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.shape == ref.shape == np.shape(S), (out.shape, ref.shape, np.shape(S))
    with np.errstate(invalid='ignore'):
        return ~(np.abs(out - ref) <= scale * bound(L, S))


def worst_ratio(out, ref, L, S):
    """max |err| / bound (inf where an element is not finite; 0 / 0 counts as 0)"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    err, b = np.abs(out - ref), bound(L, S)
    if not np.isfinite(err).all():
        return float('inf')
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0.0, err / b)
    return float(r.max())


# ---- the dispatch (csrc/small_ops.hip: mcg_fc_fprop / mcg_fc_dgrad / mcg_fc_wgrad; csrc/conv_gemm.hip: mcg_detail_fc_*_gemm).  The
# GEMMs also refuse tensors of 2 GiB and more, which nothing here comes near. ----
FPROP_BK, WGRAD_BK, TILE = 64, 32, 64


def branch(pass_, M, K, Co, with_db=False):
    if pass_ == 'fprop':
        return 'gemm' if Co >= 16 and M >= 64 and K % FPROP_BK == 0 else 'dot'
    if pass_ == 'dgrad':
        return 'rows8' if Co >= 8 and M % 8 == 0 and M >= 64 else 'row1'
    assert pass_ == 'wgrad', pass_
    return 'gemm' if Co >= 16 and Co % 4 == 0 and M >= 64 and not with_db else 'slices'


def plan_ksplit(length, step, want, min_steps):
    """conv_gemm.hip plan_ksplit: `length` terms in steps of `step` over at most `want` blocks of >= min_steps steps -> (n, chunk)"""
    steps = (length + step - 1) // step
    n = max(1, min(want, steps // min_steps))
    chunk = (steps + n - 1) // n * step
    return (length + chunk - 1) // chunk, chunk


def split(pass_, M, K, Co):
    """(n, chunk) of the GEMM a shape runs on: fprop splits K, wgrad splits M (plan_pixsplit); the scalar kernels and dgrad do not split"""
    tiles = lambda a, b: ((a + TILE - 1) // TILE) * ((b + TILE - 1) // TILE)
    if pass_ == 'fprop' and branch(pass_, M, K, Co) == 'gemm':
        t = tiles(M, Co)
        return plan_ksplit(K, FPROP_BK, (512 + t - 1) // t, 4)
    if pass_ == 'wgrad' and branch(pass_, M, K, Co) == 'gemm':
        t = tiles(Co, K)
        return plan_ksplit(M, WGRAD_BK, (1024 + t - 1) // t, 4)
    return 1, {'fprop': K, 'dgrad': Co, 'wgrad': M}[pass_]


def reduction_length(pass_, M, K, Co):
    return {'fprop': K, 'dgrad': Co, 'wgrad': M}[pass_]


def split_kind(pass_, M, K, Co, with_db=False):
    """'single' (one block per tile; chunk >= length), 'equal' (n >= 2 equal chunks), 'ragged' (n >= 2, a shorter last chunk)"""
    if branch(pass_, M, K, Co, with_db) != 'gemm':
        return 'single'
    n, chunk = split(pass_, M, K, Co)
    L = reduction_length(pass_, M, K, Co)
    if n == 1:
        assert chunk >= L
        return 'single'
    return 'equal' if L % chunk == 0 else 'ragged'


def atomic(pass_, M, K, Co, with_db=False):
    """does the launch add into its output with float atomics (so that two runs may differ in the last bits)?"""
    if branch(pass_, M, K, Co, with_db) != 'gemm':
        return False
    return pass_ == 'wgrad' or split(pass_, M, K, Co)[0] > 1


# ---- the case table: (pass, M, K, Co, options, what it pins).  options: 'db' = the weight gradient is asked for the bias gradient
# too.  fprop rows run with and without a bias, dgrad rows without a bias, with period 4 and with period K. ----
FC_CASES = [
    ('fprop', 1, 4, 1, (), "dot: one live thread"),
    ('fprop', 3, 1024, 7, (), "dot: exactly one trip of every thread"),
    ('fprop', 3, 1028, 7, (), "dot: a second trip by one thread"),
    ('fprop', 63, 64, 16, (), "dot: one row short of the GEMM"),
    ('fprop', 64, 96, 20, (), "dot: K % 64 != 0, refused by the GEMM"),
    ('fprop', 64, 64, 16, (), "gemm: one K-step, plain store"),
    ('fprop', 64, 448, 16, (), "gemm: 7 steps, unsplit"),
    ('fprop', 64, 512, 16, (), "gemm: the smallest split, 2 equal chunks"),
    ('fprop', 64, 576, 16, (), "gemm: 320 + 256"),
    ('fprop', 65, 832, 17, (), "gemm: 320 + 320 + 192, a second row tile of one row, a ragged column"),
    ('fprop', 64, 1024, 65, (), "gemm: a second column tile of one column, 4 chunks"),
    ('dgrad', 1, 4, 1, (), "row1: one thread"),
    ('dgrad', 63, 1028, 16, (), "row1: a second block of one thread"),
    ('dgrad', 64, 64, 7, (), "row1: Co < 8"),
    ('dgrad', 68, 64, 8, (), "row1: M % 8 != 0"),
    ('dgrad', 64, 4, 8, (), "rows8: the smallest"),
    ('dgrad', 64, 1028, 9, (), "rows8: unroll remainder 1, a second block of one thread"),
    ('dgrad', 72, 64, 10, (), "rows8: unroll remainder 2"),
    ('dgrad', 64, 64, 11, (), "rows8: unroll remainder 3"),
    ('wgrad', 1, 4, 1, (), "slices: fewer rows than slices"),
    ('wgrad', 7, 132, 3, (), "slices: a second block with one quad"),
    ('wgrad', 9, 128, 16, (), "slices: one row in slice 0's second trip"),
    ('wgrad', 257, 64, 2, ('db',), "slices: db's second trip"),
    ('wgrad', 64, 64, 18, (), "slices: Co % 4 != 0 at M >= 64"),
    ('wgrad', 64, 64, 16, ('db',), "slices: db forces them"),
    ('wgrad', 64, 64, 16, (), "gemm: chunk = M"),
    ('wgrad', 65, 64, 16, (), "gemm: one live row in the last step"),
    ('wgrad', 127, 68, 20, (), "gemm: a second K tile of one quad, a ragged Co tile"),
    ('wgrad', 256, 64, 16, (), "gemm: 128 + 128"),
    ('wgrad', 300, 64, 16, (), "gemm: 160 + 140, 12 live rows in the last step"),
    ('wgrad', 300, 132, 68, (), "gemm: 160 + 140 with two tiles each way"),
]


def case_id(case):
    pass_, M, K, Co, opts, _ = case
    return "%s-%dx%dx%d%s" % (pass_, M, K, Co, "".join("+" + o for o in opts))


def variants(case):
    """the launches of a row: fprop -> bias yes / no; dgrad -> (bias, period) = none, 4, K; wgrad -> one"""
    pass_, M, K, Co, opts, _ = case
    if pass_ == 'fprop':
        return [dict(bias=True), dict(bias=False)]
    if pass_ == 'dgrad':
        return [dict(period=0), dict(period=4), dict(period=K)]
    return [dict(db='db' in opts)]


def _away_from_zero(rng, shape, floor):
    """normal deviates pushed away from zero by `floor`: no element, hence no row, is zero or nearly so"""
    v = rng.randn(*shape)
    return np.where(v < 0, v - floor, v + floor)


def inputs(case):
    """The seeded fp32 operands of a row, shared by the GPU test and the sensitivity test: activations and upstream gradients of
    unit size with no element inside (-0.25, 0.25), filters of size 0.05 (the step's initialisation scale), biases and starting
    values of dw / db with no element inside (-0.5, 0.5) -- so that a dropped row, filter, chunk or starting value, or a bias added
    twice, moves some element by far more than its bound."""
    pass_, M, K, Co, opts, _ = case
    rng = np.random.RandomState(4200 + FC_CASES.index(case))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(x=f32(_away_from_zero(rng, (M, K), 0.25)), w=f32(_away_from_zero(rng, (Co, K), 0.25) * 0.05),
                gy=f32(_away_from_zero(rng, (M, Co), 0.25)), bias=f32(_away_from_zero(rng, (Co,), 0.5)),
                bias4=f32(_away_from_zero(rng, (4,), 0.5)), biasK=f32(_away_from_zero(rng, (K,), 0.5)),
                dw0=f32(_away_from_zero(rng, (Co, K), 0.5)), db0=f32(_away_from_zero(rng, (Co,), 0.5)))
