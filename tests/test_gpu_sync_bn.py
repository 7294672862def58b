"""Synchronised BatchNorm at op level: mcg_bn_sums -> (+ over the shards) -> mcg_bn_stats_from_sums and mcg_bn_bwd_sums -> (+) ->
mcg_bn_act_bwd_from_sums on ONE device in one process, against the float64 statement of tests/sync_bn_ref.py (which
tests/test_sync_bn_ref_cpu.py holds to the oracle's BatchNorm on the concatenated batch).  The all-reduce is a float64 `+` of the
shards' sums tensors on the device.

What only these entry points have: the M / M_total split (inv_m and the running variance's m / max(m - 1, 1) belong to the GLOBAL
row count), the local / global split of the backward sums (coef from the global, dgamma / dbeta from the shard's own), and the
three kernels sums_finalize_kernel, bn_stats_from_sums_kernel, bn_bwd_from_sums_kernel.

Shapes (sync_bn_ref.CASES): the smallest at which each path of plan_partial / reduce_partials differs; the block counts there are
recomputed from small_ops.hip's plan_partial by sync_bn_ref.plan_partial when the module is imported.

Tolerances are the project's: 1e-5 rel-L2 for per-channel sums, statistics and running averages, FWD_TOL / BWD_TOL of
tests/test_gpu_ops.py for gx, dgamma, dbeta.  Every case also runs the single-device bn_stats / bn_act_bwd on the concatenated
batch through the SAME assertions: the bar is one the plain path clears, not one fitted to the code under test.

Every tensor a launch touches lives in a guard.Arena (the workspace has exactly bn_workspace_floats(C) floats), arena.check()
runs after every call, and every output must be finite (the arena's poison is a NaN: an element left unwritten, or computed from
a load outside a tensor, fails that)."""
import functools

import numpy as np
import pytest
import torch

import sync_bn_ref as R
from guard import Arena

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 1e-5, 1e-4           # tests/test_gpu_ops.py
SUM_TOL = 1e-5                          # sums, statistics, running averages (test_batchnorm_activation_fwd_bwd)
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(96 << 20)              # the largest case: y, g, gx of 40 777 x 128 floats each


def dev(a, dtype=F32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def rel_l2(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def held(case, what, got, want, tol):
    """assert rel-L2(got, want) < tol, printing the figure first (run with -s: profiles/data_parallel_parity.md is made of these)"""
    err = rel_l2(got, want)
    print("PARITY %-18s %-34s %.2e  (tol %.0e)" % (case, what, err, tol))
    assert err < tol, (case, what, err, tol)


def finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t.float() if t.dtype == BF else t).all()), "an output holds a non-finite value"


def bits(t):
    return t.view({F32: torch.int32, BF: torch.int16, F64: torch.int64}[t.dtype])


def same_bits(case, what, a, b):
    """bit-for-bit equality; a failure says how many elements differ and by how many fp32 ulp at the most"""
    if torch.equal(bits(a), bits(b)):
        return
    msg = "%s %s: " % (case, what)
    if a.dtype == F32:
        # (distance in units in the last place: the integer patterns of same-sign floats are ordered)
        ulp = (bits(a).long() - bits(b).long()).abs()
        msg += "%d of %d elements differ, by up to %d fp32 ulp" % (int((ulp != 0).sum()), a.numel(), int(ulp.max()))
    else:
        msg += "%d of %d elements differ" % (int((bits(a) != bits(b)).sum()), a.numel())
    raise AssertionError(msg)


@functools.lru_cache(maxsize=None)
def _case(name, bf16_values=False):
    """inputs and the float64 results of a case, computed once for all tests that use it (and never changed)"""
    d = R.case_inputs(name, bf16_values)
    assert d['dropped'] <= R.MAX_DROPPED, (name, d['dropped'])              # the kink mask may drop 0.1 % of a case at the most
    fwd = R.forward(d['ys'], d['gamma'], d['beta'], d['avg_mean'], d['avg_var'])
    bwd = R.backward(d['ys'], d['gs'], fwd, d['gamma_cur'], d['act'])
    return d, fwd, bwd


def _add_in_rank_order(parts, out):
    """out = ((p0 + p1) + p2) + ...: one fixed order, so the total is the same double wherever it is formed"""
    out.copy_(parts[0])
    for t in parts[1:]:
        out += t


class Run:
    """The tensors of one case in the arena and the four entry points on them, a check of the arena's margins after each."""

    def __init__(self, hl, arena, d, ys=None, gs=None, y16=False, g16=False, out16=False, in_place=False):
        arena.reset()
        self.hl, self.arena, self.C, self.act = hl, arena, d['C'], d['act']
        C = self.C
        ys, gs = d['ys'] if ys is None else ys, d['gs'] if gs is None else gs
        self.rows = [len(y) for y in ys]
        self.m_total = sum(self.rows)
        self.y32 = [arena.put(dev(y)) for y in ys]                          # the forward pass has fp32 inputs only
        self.y = [arena.put(y.to(BF)) for y in self.y32] if y16 else self.y32
        self.g = [arena.put(dev(g, BF if g16 else F32)) for g in gs]
        assert not in_place or g16 == out16
        self.gx = self.g if in_place else [arena.empty((m, C), BF if out16 else F32) for m in self.rows]
        self.gamma, self.beta, self.gamma_cur = (arena.put(dev(d[k])) for k in ('gamma', 'beta', 'gamma_cur'))
        self.am, self.av = arena.put(dev(d['avg_mean'])), arena.put(dev(d['avg_var']))
        self.ws = arena.empty((hl.bn_workspace_floats(C),))                  # exactly what the library asks for
        self.stats = arena.empty((4 * C,))
        self.sums = [arena.empty((2 * C,), F64) for _ in self.rows]
        self.local = [arena.empty((2 * C,), F64) for _ in self.rows]
        self.total, self.glob = arena.empty((2 * C,), F64), arena.empty((2 * C,), F64)
        self.dgamma = [arena.full((C,), 1.0) for _ in self.rows]            # accumulated into: 1 + the shard's own sum afterwards
        self.dbeta = [arena.full((C,), 1.0) for _ in self.rows]

    def forward(self):
        hl, C = self.hl, self.C
        for k, m in enumerate(self.rows):
            hl.bn_sums(m, C, self.y32[k], self.sums[k], self.ws)
            self.arena.check()
        _add_in_rank_order(self.sums, self.total)                           # the all-reduce: float64 + on the device
        hl.bn_stats_from_sums(self.m_total, C, self.total, self.gamma, self.beta, self.stats, self.am, self.av)
        self.arena.check()
        finite(self.stats, self.am, self.av, *self.sums)
        return self

    def backward(self):
        hl, C = self.hl, self.C
        for k, m in enumerate(self.rows):
            hl.bn_bwd_sums(m, C, self.g[k], self.y[k], self.stats, self.act, self.local[k], self.ws)
            self.arena.check()
        _add_in_rank_order(self.local, self.glob)
        for k, m in enumerate(self.rows):
            hl.bn_act_bwd_from_sums(m, self.m_total, C, self.g[k], self.y[k], self.stats, self.gamma_cur, self.act, self.local[k],
                                    self.glob, self.gx[k], self.dgamma[k], self.dbeta[k], self.ws)
            self.arena.check()
        finite(*self.local, *self.gx, *self.dgamma, *self.dbeta)
        return self


class Plain:
    """the single-device bn_stats / bn_act_bwd on the concatenated batch, in the arena as well"""

    def __init__(self, hl, arena, d, ys=None, gs=None):
        arena.reset()
        C = d['C']
        M = self.M = d['m_total']
        y = np.concatenate(d['ys'] if ys is None else ys)
        g = np.concatenate(d['gs'] if gs is None else gs)
        self.y, self.g, self.gx = arena.put(dev(y)), arena.put(dev(g)), arena.empty((M, C))
        gamma, beta, gamma_cur = (arena.put(dev(d[k])) for k in ('gamma', 'beta', 'gamma_cur'))
        self.am, self.av = arena.put(dev(d['avg_mean'])), arena.put(dev(d['avg_var']))
        ws, self.stats = arena.empty((hl.bn_workspace_floats(C),)), arena.empty((4 * C,))
        self.dgamma, self.dbeta = arena.full((C,), 1.0), arena.full((C,), 1.0)
        hl.bn_stats(M, C, self.y, gamma, beta, self.stats, self.am, self.av, ws)
        arena.check()
        hl.bn_act_bwd(M, C, self.g, self.y, self.stats, gamma_cur, d['act'], self.gx, self.dgamma, self.dbeta, ws)
        arena.check()
        finite(self.stats, self.am, self.av, self.gx, self.dgamma, self.dbeta)

    def keep(self):
        """copies outside the arena (the next run resets it)"""
        return {k: getattr(self, k).clone() for k in ('stats', 'am', 'av', 'gx', 'dgamma', 'dbeta')}


def _hold_stats(case, tag, stats, am, av, fwd):
    C = stats.numel() // 4
    st = fwd['st']
    for i, k in enumerate(('mean', 'inv_std', 'scale', 'shift')):
        held(case, "%s %s" % (tag, k), stats[i * C:(i + 1) * C], st[k], SUM_TOL)
    held(case, tag + " avg_mean", am, fwd['avg_mean'], SUM_TOL)
    held(case, tag + " avg_var", av, fwd['avg_var'], SUM_TOL)


@pytest.mark.parametrize("name", list(R.CASES))
def test_shards_against_float64_and_against_the_whole(hl, arena, name):
    """(a) every output of the four entry points against float64; (b) the single-device path on the concatenated batch through the
    same assertions; (c) the shards' gx concatenated, and their dgamma / dbeta added, against the single-device results."""
    d, fwd, bwd = _case(name)
    C, shards = d['C'], range(len(d['rows']))
    plain = Plain(hl, arena, d).keep()
    _hold_stats(name, "plain", plain['stats'], plain['am'], plain['av'], fwd)
    gx_ref = np.concatenate(bwd['gx'])
    held(name, "plain gx", plain['gx'], gx_ref, BWD_TOL)
    held(name, "plain dgamma", plain['dgamma'], 1 + np.sum(bwd['dgamma'], axis=0), BWD_TOL)
    held(name, "plain dbeta", plain['dbeta'], 1 + np.sum(bwd['dbeta'], axis=0), BWD_TOL)

    r = Run(hl, arena, d).forward()
    for k in shards:
        held(name, "shard %d sums" % k, r.sums[k], fwd['sums'][k], SUM_TOL)
    _hold_stats(name, "sync", r.stats, r.am, r.av, fwd)
    r.backward()
    for k in shards:
        held(name, "shard %d bwd sums" % k, r.local[k], bwd['sums'][k], SUM_TOL)
        held(name, "shard %d gx" % k, r.gx[k], bwd['gx'][k], BWD_TOL)
        held(name, "shard %d dgamma" % k, r.dgamma[k], 1 + bwd['dgamma'][k], BWD_TOL)      # started at 1: 1 + the LOCAL sum
        held(name, "shard %d dbeta" % k, r.dbeta[k], 1 + bwd['dbeta'][k], BWD_TOL)
    held(name, "gx, all shards", torch.cat(r.gx), gx_ref, BWD_TOL)
    # shards equal the whole
    held(name, "gx vs plain", torch.cat(r.gx), plain['gx'].double().cpu().numpy(), BWD_TOL)
    for what, mine, whole in (("dgamma", r.dgamma, plain['dgamma']), ("dbeta", r.dbeta, plain['dbeta'])):
        added = sum(t.double() - 1 for t in mine)
        held(name, "sum of %s vs plain" % what, added, (whole.double() - 1).cpu().numpy(), BWD_TOL)


@pytest.mark.parametrize("name", list(R.CASES))
def test_one_shard_equals_the_plain_path_bit_for_bit(hl, arena, name):
    """M_total == M: the same partial sums enter the same reduce_partials, the same doubles the same inline bn_stats_write /
    bn_bwd_write (both stats kernels compile the running averages to v_pk_mul_f32 + v_add_f32, neither contracts them), and
    the apply kernel is the same launch -- stats, running averages, gx, dgamma, dbeta must not differ in a single bit."""
    d, _, _ = _case(name)
    ys, gs = [np.concatenate(d['ys'])], [np.concatenate(d['gs'])]
    plain = Plain(hl, arena, d).keep()
    r = Run(hl, arena, d, ys, gs).forward().backward()
    assert torch.equal(r.total, r.sums[0]) and torch.equal(r.glob, r.local[0])
    for what, a, b in (("stats", r.stats, plain['stats']), ("avg_mean", r.am, plain['am']), ("avg_var", r.av, plain['av']),
                       ("gx", r.gx[0], plain['gx']), ("dgamma", r.dgamma[0], plain['dgamma']), ("dbeta", r.dbeta[0], plain['dbeta'])):
        same_bits(name, what, a, b)
    print("PARITY %-18s one shard == plain path: bit for bit" % name)


@pytest.mark.parametrize("name", ["c8-three-shards", "c512"])
def test_flag_forms(hl, arena, name):
    """Every MCG_IO_* combination: Y_BF16 / G_BF16 of bn_bwd_sums, all of io & 7 of bn_act_bwd_from_sums, on bf16-representable
    inputs (so a tensor held in bf16 holds the same numbers).  The sums of every input form and the fp32 gx against float64; the
    bf16 output equal to the fp32 output of the same inputs, rounded; in place (gx is g_out) equal to out of place."""
    d, fwd, bwd = _case(name, True)
    shards = range(len(d['rows']))
    base = None
    for y16 in (False, True):
        for g16 in (False, True):
            tag = "y%d g%d" % (16 if y16 else 32, 16 if g16 else 32)
            r = Run(hl, arena, d, y16=y16, g16=g16).forward().backward()
            for k in shards:
                held(name, "%s shard %d bwd sums" % (tag, k), r.local[k], bwd['sums'][k], SUM_TOL)
                held(name, "%s shard %d dgamma" % (tag, k), r.dgamma[k], 1 + bwd['dgamma'][k], BWD_TOL)
                held(name, "%s shard %d dbeta" % (tag, k), r.dbeta[k], 1 + bwd['dbeta'][k], BWD_TOL)
            held(name, tag + " gx", torch.cat(r.gx), np.concatenate(bwd['gx']), BWD_TOL)
            gx32 = [t.clone() for t in r.gx]
            dg32, db32, local32 = [t.clone() for t in r.dgamma], [t.clone() for t in r.dbeta], [t.clone() for t in r.local]
            if base is None:
                base = (r.stats.clone(), r.am.clone(), r.av.clone())
            else:                                       # (the forward pass does not depend on how the backward's inputs are held)
                assert all(torch.equal(a, b) for a, b in zip(base, (r.stats, r.am, r.av)))
            forms = [(True, False)] + ([(False, True)] if not g16 else []) + ([(True, True)] if g16 else [])    # (bf16 out, in place)
            for out16, in_place in forms:
                q = Run(hl, arena, d, y16=y16, g16=g16, out16=out16, in_place=in_place).forward().backward()
                for k in shards:
                    form = "%s out%d%s shard %d" % (tag, 16 if out16 else 32, " in place" if in_place else "", k)
                    assert q.gx[k].dtype == (BF if out16 else F32)
                    same_bits(name, form + " gx", q.gx[k], gx32[k].to(BF) if out16 else gx32[k])
                    same_bits(name, form + " dgamma", q.dgamma[k], dg32[k])
                    same_bits(name, form + " dbeta", q.dbeta[k], db32[k])
                    same_bits(name, form + " sums", q.local[k], local32[k])
    print("PARITY %-18s bf16 / in-place forms == fp32 form rounded: bit for bit" % name)


def test_refusals_leave_the_outputs_untouched(hl, arena):
    arena.reset()
    M, C = 64, 8
    BAD, UNSUP = "MCG_ERR_BAD_ARG", "MCG_ERR_UNSUPPORTED"
    mk = lambda c, m=M: (arena.put(torch.randn((m, c), device="cuda")), arena.put(torch.randn((m, c), device="cuda")))
    y, g = mk(C)
    ws = arena.full((hl.bn_workspace_floats(64),), 3.0)
    filled = lambda n, dt=F32: arena.full((n,), 3.0, dt)
    stats_in = arena.put(torch.cat([torch.zeros(64), torch.ones(64), torch.ones(64), torch.zeros(64)]).cuda())
    gamma, beta = arena.put(torch.ones(64, device="cuda")), arena.put(torch.zeros(64, device="cuda"))
    sums, stats, am, av = filled(2 * 64, F64), filled(4 * 64), filled(64), filled(64)
    loc, glo = arena.put(torch.randn(2 * 64, device="cuda", dtype=F64)), arena.put(torch.randn(2 * 64, device="cuda", dtype=F64))
    gx, dg, db = arena.full((M, 24), 3.0), filled(64), filled(64)
    outputs = (ws, sums, stats, am, av, gx, dg, db)

    def untouched():
        arena.check()
        assert all(bool((t == 3.0).all()) for t in outputs)

    def refused(code, fn, *a, **kw):
        with pytest.raises(hl.McgError, match=code):
            fn(*a, **kw)
        untouched()

    # fewer rows in the global batch than in the shard
    refused(BAD, hl.bn_act_bwd_from_sums, M, M - 1, C, g, y, stats_in[:4 * C], gamma[:C], hl.ACT_RELU, loc[:2 * C], glo[:2 * C],
            gx.view(-1)[:M * C].view(M, C), dg[:C], db[:C], ws)
    refused(BAD, hl.bn_stats_from_sums, 0, C, loc[:2 * C], gamma[:C], beta[:C], stats[:4 * C], am[:C], av[:C])
    # 6 channel quads do not divide a block
    y24, g24 = mk(24)
    refused(UNSUP, hl.bn_sums, M, 24, y24, sums[:48], ws)
    refused(UNSUP, hl.bn_bwd_sums, M, 24, g24, y24, stats_in[:96], hl.ACT_LRELU, sums[:48], ws)
    # channels come in quads (mcg_bn_stats_from_sums alone takes any C > 0: one thread per channel, no vector access)
    y6, g6 = mk(6)
    refused(BAD, hl.bn_sums, M, 6, y6, sums[:12], ws)
    refused(BAD, hl.bn_bwd_sums, M, 6, g6, y6, stats_in[:24], hl.ACT_LRELU, sums[:12], ws)
    refused(BAD, hl.bn_act_bwd_from_sums, M, M, 6, g6, y6, stats_in[:24], gamma[:6], hl.ACT_LRELU, loc[:12], glo[:12],
            gx.view(-1)[:M * 6].view(M, 6), dg[:6], db[:6], ws)
    # only one of the running averages
    refused(BAD, hl.bn_stats_from_sums, M, C, loc[:2 * C], gamma[:C], beta[:C], stats[:4 * C], am[:C], None)
    refused(BAD, hl.bn_stats_from_sums, M, C, loc[:2 * C], gamma[:C], beta[:C], stats[:4 * C], None, av[:C])
    # in place between tensors of different element types: an fp32 gx that starts where the bf16 g_out starts
    g16 = arena.put(torch.randn((M, C), device="cuda").to(BF))
    alias = torch.empty(0, dtype=F32, device="cuda").set_(g16.untyped_storage(), g16.storage_offset() // 2, (M, C // 2), (C // 2, 1))
    assert alias.data_ptr() == g16.data_ptr()
    before = g16.clone()
    refused(BAD, hl.bn_act_bwd_from_sums, M, M, C // 2, g16, y, stats_in[:4 * C], gamma[:C], hl.ACT_RELU, loc[:2 * C], glo[:2 * C],
            alias, dg[:C], db[:C], ws)
    assert torch.equal(bits(g16), bits(before))
    # flags outside an entry point's set: the wrappers derive the flags from the tensors' types, so these go to the C entry points
    lib, p = hl.load(), hl._p
    gxc = gx.view(-1)[:M * C].view(M, C)
    for flag in (hl.IO_OUT_BF16, hl.IO_OUT_SPLIT, hl.IO_OUT_BF16 | hl.IO_Y_BF16, 16):
        rc = lib.mcg_bn_bwd_sums(M, C, p(g), p(y), p(stats_in), hl.ACT_RELU, flag, p(sums, F64), p(ws), hl._stream())
        assert rc == -1, (flag, rc)
        untouched()
    for flag in (hl.IO_OUT_SPLIT, hl.IO_OUT_SPLIT | hl.IO_G_BF16, 16, -1):
        rc = lib.mcg_bn_act_bwd_from_sums(M, M, C, p(g), p(y), p(stats_in), p(gamma), hl.ACT_RELU, p(loc, F64), p(glo, F64), p(gxc),
                                          flag, p(dg), p(db), p(ws), hl._stream())
        assert rc == -1, (flag, rc)
        untouched()
    assert hl._STATUS[-1] == BAD


class _Recorder:
    """sync stub: keeps what it was asked to all-reduce, reduces nothing"""

    def __init__(self, world):
        self.world, self.seen = world, []

    def all_reduce_sum(self, t):
        self.seen.append(t.clone())


class _Adder:
    """sync stub of rank `rank`: the tensor becomes the sum over the ranks, its own value and what the others recorded, added in
    rank order (as Run adds them) -- call by call"""

    def __init__(self, world, rank, seen):
        self.world, self.rank, self.seen, self.calls = world, rank, seen, 0

    def all_reduce_sum(self, t):
        parts = [t.clone() if j == self.rank else self.seen[j][self.calls] for j in range(self.world)]
        assert torch.equal(parts[self.rank], self.seen[self.rank][self.calls])          # (what this rank recorded in pass 1)
        _add_in_rank_order(parts, t)
        self.calls += 1


@pytest.mark.parametrize("world", [2, 4])
def test_through_the_sync_argument_of_bn_stats_and_bn_act_bwd(hl, arena, world):
    """hl.bn_stats(..., sync=) / hl.bn_act_bwd(..., sync=) with a stub in place of the process group reproduce the direct calls bit
    for bit: the wrapper's M * world, its local.clone() and the order of its launches.  Equal shards (the wrapper assumes them)."""
    d, _, _ = _case("c64")
    C, act = d['C'], d['act']
    y, g = np.concatenate(d['ys']), np.concatenate(d['gs'])
    M = len(y) // world
    ys, gs = [y[k * M:(k + 1) * M] for k in range(world)], [g[k * M:(k + 1) * M] for k in range(world)]
    fwd = R.forward(ys, d['gamma'], d['beta'], d['avg_mean'], d['avg_var'])
    bwd = R.backward(ys, gs, fwd, d['gamma_cur'], act)
    r = Run(hl, arena, d, ys, gs).forward().backward()
    name = "c64 world %d" % world
    _hold_stats(name, "direct", r.stats, r.am, r.av, fwd)
    held(name, "direct gx", torch.cat(r.gx), np.concatenate(bwd['gx']), BWD_TOL)
    want = dict(stats=r.stats.clone(), am=r.am.clone(), av=r.av.clone(), gx=[t.clone() for t in r.gx],
                dgamma=[t.clone() for t in r.dgamma], dbeta=[t.clone() for t in r.dbeta])

    arena.reset()
    put = lambda a: arena.put(dev(a))
    yd, gd = [put(a) for a in ys], [put(a) for a in gs]
    gamma, beta, gamma_cur = put(d['gamma']), put(d['beta']), put(d['gamma_cur'])
    ws = arena.empty((hl.bn_workspace_floats(C),))
    # pass 1: every rank's own sums (the statistics this pass writes are of the rank's rows counted `world` times: thrown away)
    rec = [_Recorder(world) for _ in range(world)]
    for k in range(world):
        hl.bn_stats(M, C, yd[k], gamma, beta, arena.empty((4 * C,)), put(d['avg_mean']), put(d['avg_var']), ws, sync=rec[k])
        arena.check()
        assert len(rec[k].seen) == 1
    # pass 2: the ranks' sums added
    stats = []
    for k in range(world):
        st, am, av = arena.empty((4 * C,)), put(d['avg_mean']), put(d['avg_var'])
        add = _Adder(world, k, [q.seen for q in rec])
        hl.bn_stats(M, C, yd[k], gamma, beta, st, am, av, ws, sync=add)
        arena.check()
        assert add.calls == 1
        same_bits(name, "rank %d stats" % k, st, want['stats'])
        same_bits(name, "rank %d avg_mean" % k, am, want['am'])
        same_bits(name, "rank %d avg_var" % k, av, want['av'])
        stats.append(st)
    # backward, from the global statistics of the forward pass
    rec = [_Recorder(world) for _ in range(world)]
    for k in range(world):
        hl.bn_act_bwd(M, C, gd[k], yd[k], stats[k], gamma_cur, act, arena.empty((M, C)), arena.full((C,), 1.0), arena.full((C,), 1.0), ws,
                      sync=rec[k])
        arena.check()
        assert len(rec[k].seen) == 1
    for k in range(world):
        gx, dg, db = arena.empty((M, C)), arena.full((C,), 1.0), arena.full((C,), 1.0)
        add = _Adder(world, k, [q.seen for q in rec])
        hl.bn_act_bwd(M, C, gd[k], yd[k], stats[k], gamma_cur, act, gx, dg, db, ws, sync=add)
        arena.check()
        assert add.calls == 1
        finite(gx, dg, db)
        same_bits(name, "rank %d gx" % k, gx, want['gx'][k])
        same_bits(name, "rank %d dgamma" % k, dg, want['dgamma'][k])          # the LOCAL sums: no other rank's numbers in them
        same_bits(name, "rank %d dbeta" % k, db, want['dbeta'][k])
    print("PARITY %-18s hl.bn_stats / hl.bn_act_bwd (sync=) == direct calls: bit for bit" % name)
