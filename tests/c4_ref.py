"""The convolution of the 3-channel clip padded to 4 channels (Ci = 4, Co = 64: D's first layer, G's last) stated in float64 in the
device layout, its acceptance bound, the dispatch of csrc/conv_gemm.hip restated as pure functions of the geometry, the launch plans of
the six kernels written for the layer, and the case table of tests/test_gpu_c4_guard.py.  NumPy only, nothing from the package:
tests/test_c4_ref_cpu.py holds every statement here to the library's return codes, to oracle.functions and to hand-computed values,
and shows without a device that the acceptance check used on the GPU notices each defect the table is there to find.

Layout (include/mocogan_hip.h): x [N][Ti][Hi][Wi][4], w [64][kt][4][4][4], y / gy [N][To][Ho][Wo][64], To = Ti - kt + 1, Ho = Hi / 2,
Wo = Wi / 2; channel 3 of x and of w is the padding and holds zeros.  The references take the fp32 values the device holds and compute in
float64; beside the result they return S, the same operation on the operands' magnitudes, which the bound is relative to.  They are
written on the operations NumPy arrays and torch tensors share, so the GPU test runs them in float64 on the device."""
import numpy as np

U = 2.0 ** -24                      # fp32 unit roundoff
CO, CI, CV = 64, 4, 3               # filters; channels in memory; channels that carry data
UNSUPPORTED = 'UNSUPPORTED'
TILES = (0, 6, 2)                   # the library's choice, the kernels written for the layer, a register-staged GEMM tile
PRECS = ('f32', 'bf16', 'bf16y')    # bf16y (y bf16 in memory beside fp32 x and w): dgrad and wgrad only
PASSES = ('fprop', 'dgrad', 'wgrad')
CLIP_T = 3                          # frames of the clip the views are taken from


# ---- float64 references ------------------------------------------------------------------------------------------------------------
def _zeros(like, shape):
    return like.new_zeros(shape) if hasattr(like, 'new_zeros') else np.zeros(shape, like.dtype)


def _f64(a):
    if a is None:
        return None
    return a.double() if hasattr(a, 'double') else np.asarray(a, np.float64)


def _pad_hw(x):
    N, T, H, W, C = x.shape
    xp = _zeros(x, (N, T, H + 2, W + 2, C))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    return xp


def taps(kt):
    return [(a, kh, kw) for a in range(kt) for kh in range(4) for kw in range(4)]


def _tap_rows(xp, a, kh, kw, To, Ho, Wo):
    """the input pixels tap (a, kh, kw) reads, one row per output pixel: [N To Ho Wo][Ci]"""
    return xp[:, a:a + To, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :].reshape(-1, xp.shape[-1])


def _fprop(x, w, bias):
    N, T, H, W, Ci = x.shape
    Co, kt = w.shape[0], w.shape[1]
    To, Ho, Wo = T - kt + 1, H // 2, W // 2
    xp = _pad_hw(x)
    y = _zeros(x, (N * To * Ho * Wo, Co))
    for a, kh, kw in taps(kt):
        y += _tap_rows(xp, a, kh, kw, To, Ho, Wo) @ w[:, a, kh, kw, :].T
    if bias is not None:
        y += bias
    return y.reshape(N, To, Ho, Wo, Co)


def fprop(x, w, bias=None):
    """y = conv(x, w) + bias -> (y, S)"""
    x, w, bias = _f64(x), _f64(w), _f64(bias)
    return _fprop(x, w, bias), _fprop(abs(x), abs(w), None if bias is None else abs(bias))


def _dgrad(gy, w, T, H, W, bias, x0):
    N, To, Ho, Wo, Co = gy.shape
    kt, Ci = w.shape[1], w.shape[4]
    assert To == T - kt + 1 and Ho == H // 2 and Wo == W // 2
    gxp = _zeros(gy, (N, T, H + 2, W + 2, Ci))
    g2 = gy.reshape(-1, Co)
    for a, kh, kw in taps(kt):
        gxp[:, a:a + To, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :] += (g2 @ w[:, a, kh, kw, :]).reshape(N, To, Ho, Wo, Ci)
    gx = gxp[:, :, 1:H + 1, 1:W + 1] + 0
    if bias is not None:
        gx += bias
    if x0 is not None:
        gx += x0
    return gx


def dgrad(gy, w, T, H, W, bias=None, x0=None):
    """x = x0 + conv_transpose(gy, w) + bias (before any tanh) -> (x, S); x0: what an accumulating launch adds onto"""
    gy, w, bias, x0 = _f64(gy), _f64(w), _f64(bias), _f64(x0)
    ab = lambda v: None if v is None else abs(v)
    return _dgrad(gy, w, T, H, W, bias, x0), _dgrad(abs(gy), abs(w), T, H, W, ab(bias), ab(x0))


def _wgrad(x, gy, kt, dw0, frames, twice):
    N, T, H, W, Ci = x.shape
    _, To, Ho, Wo, Co = gy.shape
    assert To == T - kt + 1 and Ho == H // 2 and Wo == W // 2
    xp = _pad_hw(x)
    dw = _zeros(x, (Co, kt, 4, 4, Ci))
    for lo, hi in ([(0, To)] if frames is None else frames):          # output frames [lo, hi)
        if hi <= lo:
            continue
        g2t = gy[:, lo:hi].reshape(-1, Co).T
        for a, kh, kw in taps(kt):
            dw[:, a, kh, kw, :] += g2t @ _tap_rows(xp[:, lo:hi + kt - 1], a, kh, kw, hi - lo, Ho, Wo)
    if twice is not None:
        dw += _wgrad(x, gy, kt, None, [(twice, twice + 1)], None)
    if dw0 is not None:
        dw += dw0
    return dw


def wgrad(x, gy, kt, dw0=None, frames=None, twice=None):
    """dw = dw0 + sum over pixels of gy (x) the tap's input -> (dw, S).  frames / twice: for the simulated defects only (the sum over
    the listed ranges of output frames; one output frame counted a second time)"""
    x, gy, dw0 = _f64(x), _f64(gy), _f64(dw0)
    return (_wgrad(x, gy, kt, dw0, frames, twice), _wgrad(abs(x), abs(gy), kt, None if dw0 is None else abs(dw0), None, None))


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
def bound(L, S, rounded=False):
    """The forward error bound of an fp32 inner product of length L in ANY summation order (Higham, Accuracy and Stability, 3.1:
    |fl(a.b) - a.b| <= gamma_L sum |a_i||b_i|, gamma_L ~ L u), with eight more roundings for what surrounds the sum (partial sums
    meeting in LDS and in atomics, the value accumulated onto).  rounded: both operands of every product were rounded to bf16 by the
    kernel (relative 2^-9 each): 2^-8 S more.  Derived, not fitted."""
    return ((L + 8) * U + (2.0 ** -8 if rounded else 0.0)) * S


def terms(pass_, g, blocks=1):
    """L of an output element: forward kt * 16 taps * 4 channels + the bias; input gradient at most kt * 4 taps * 64 filters + the two
    addends (neighbouring blocks, or bias and the accumulated-onto value); weight gradient one term per pixel + one per adding block"""
    if pass_ == 'fprop':
        return g.kt * 64 + 1
    if pass_ == 'dgrad':
        return g.kt * 4 * 64 + 2
    assert pass_ == 'wgrad', pass_
    return g.N * g.To * g.Ho * g.Wo + blocks


def violations(out, ref, L, S, scale=1.0, rounded=False):
    """element-wise: True where `out` is NOT within scale * bound of ref -- a NaN (poison left in place, a consumed out-of-tensor load)
    violates.  The one acceptance check: the GPU test applies it to the kernel's output, the CPU test to simulated defects."""
    assert tuple(out.shape) == tuple(ref.shape) == tuple(S.shape), (out.shape, ref.shape, S.shape)
    return ~(abs(_f64(out) - ref) <= scale * bound(L, S, rounded))


def worst_ratio(out, ref, L, S, rounded=False):
    """max |err| / bound (inf where an element is not finite or misses a bound of zero; 0 / 0 counts as 0)"""
    err, b = abs(_f64(out) - ref), bound(L, S, rounded)
    if bool((err != err).any()) or bool(((b == 0) & (err > 0)).any()):
        return float('inf')
    live = b > 0
    return float((err[live] / b[live]).max()) if bool(live.any()) else 0.0


# ---- geometry and dispatch (csrc/conv_gemm.hip: make_geom, c4_*_ok, conv_fprop_impl / conv_dgrad_impl / mcg_conv_wgrad) ----------------
class Geo:
    """a launch geometry: the row (N, Ti, (Hi, Wi), kt) or a view of a CLIP_T-frame clip.  dense: x is one buffer of N frames in batch
    order; whole: the N frames of x tile one dense buffer (batch order, or the clip-order permutation)"""

    def __init__(self, row, view=None, clips=None):
        self.N, self.Ti, (self.Hi, self.Wi), self.kt = row
        self.view, self.clips = view, clips
        frame = self.Ti * self.Hi * self.Wi * CI
        self.x_perm_n, self.x_stride0, self.x_stride1 = 0, frame, 0
        if view is not None:
            assert self.Ti == 1 and self.kt == 1 and clips >= 1, "views are frames of a clip"
        if view == 'frame':                                   # x[:, t] of [clips][T][Hi][Wi][4]
            self.N, self.x_stride0 = clips, CLIP_T * frame
        elif view == 'perm':                                  # launch item t * clips + b is frame t of clip b
            self.N, self.x_perm_n, self.x_stride0, self.x_stride1 = clips * CLIP_T, clips, CLIP_T * frame, frame
        else:
            assert view is None, view
        self.To, self.Ho, self.Wo = self.Ti - self.kt + 1, self.Hi // 2, self.Wi // 2
        self.dense = not self.x_perm_n and self.x_stride0 == frame
        self.whole = (self.x_stride1 == frame and self.x_stride0 == (self.N // self.x_perm_n) * frame) if self.x_perm_n else self.dense

    def item_offset(self, n):
        """element offset of batch item n of x (include/mocogan_hip.h)"""
        if self.x_perm_n:
            return (n % self.x_perm_n) * self.x_stride0 + (n // self.x_perm_n) * self.x_stride1
        return n * self.x_stride0


def c4_layer(g, pixels):
    """what the kernels written for the layer share: rows of 16 or 32 output pixels, whole `pixels`-pixel block steps per frame"""
    return g.Wo in (16, 32) and g.Ho % (pixels // g.Wo) == 0


def c4_fprop_ok(g):
    return c4_layer(g, 256) and g.dense


def c4_dgrad_mfma_ok(g, bias=False, act=False, accumulate=False):
    """x must be ONE dense buffer (it is cleared as a whole); no bias, activation or accumulation"""
    return c4_layer(g, 128) and g.whole and not bias and not act and not accumulate


def c4_wgrad_ok(g, prec):
    """fp32, or the bf16 MFMA with y bf16 in memory"""
    return c4_layer(g, 256) and g.dense and prec in ('f32', 'bf16y')


def c4_dgrad_valu_ok(g):
    return g.Wo % 16 == 0


def plan_ksplit(length, step, want, min_steps):
    """conv_gemm.hip plan_ksplit -> (n, chunk)"""
    steps = (length + step - 1) // step
    n = max(1, min(want, steps // min_steps))
    chunk = (steps + n - 1) // n * step
    return (length + chunk - 1) // chunk, chunk


C4_DGRAD_MAX_BLOCKS = 1024
VALU_RUNS_PER_BLOCK = 16            # 4 waves x C4_RUNS_PER_WAVE


def plan_fprop(g):
    R = 256 // g.Wo
    grid = g.N * (g.Ho // R)
    return dict(grid=grid, cls=frozenset(['one block per item' if g.Ho == R else 'row blocks']))


def plan_col2im(g):
    R = 128 // g.Wo
    ntiles = g.N * (g.Ho // R)
    grid = min(ntiles, C4_DGRAD_MAX_BLOCKS)
    return dict(grid=grid, ntiles=ntiles, cls=frozenset(['ntiles > 1024' if ntiles > grid else 'one tile per block']))


def plan_valu(g):
    runs = g.N * g.Ti * g.Ho * g.Wo // 16
    grid = (runs + VALU_RUNS_PER_BLOCK - 1) // VALU_RUNS_PER_BLOCK
    return dict(grid=grid, runs=runs, cls=frozenset(['partly filled block' if runs % VALU_RUNS_PER_BLOCK else 'full blocks']))


def plan_wgrad(g, prec):
    """launch_wgrad_c4: (row block, item) pairs on at most 512 blocks; below 256 blocks the output frames are split, while a part
    keeps To / (2 tsplit) >= 2; parts: [t0, t1) of every frame part"""
    BM = 128 if (prec == 'bf16y' and g.kt == 4) else 256
    hblocks = g.Ho // (BM // g.Wo)
    nsplit, tsplit = g.N, 1
    if hblocks * nsplit > 512:
        nsplit = max(512 // hblocks, 1)
    while hblocks * nsplit * tsplit < 256 and 4 * tsplit <= g.To:
        tsplit *= 2
    tper = (g.To + tsplit - 1) // tsplit
    parts = [(ts * tper, max(ts * tper, min(ts * tper + tper, g.To))) for ts in range(tsplit)]
    lens = [b - a for a, b in parts]
    cls = {'tsplit = %d' % tsplit}
    if len({n for n in lens if n}) > 1:
        cls.add('ragged part')
    if 1 in lens and tsplit > 1:
        cls.add('one-step part')
    if 0 in lens:
        cls.add('empty part')
    if nsplit < g.N:
        cls.add('nsplit < N')
    return dict(grid=hblocks * nsplit * tsplit, BM=BM, hblocks=hblocks, nsplit=nsplit, tsplit=tsplit, tper=tper, parts=parts,
                blocks_per_element=hblocks * nsplit * tsplit, cls=frozenset(cls))


def plan_wgrad_gemm(g, tile, prec):
    """the register-staged weight gradient (tile 0 -> 64x64 for Co <= 64; tile 2 = 128x64): pixel splits that add with atomics"""
    BM, BN = (128, 64) if tile == 2 else (64, 64)
    tiles = ((CO + BM - 1) // BM) * ((g.kt * 64 + BN - 1) // BN)
    n, _ = plan_ksplit(g.N * g.To * g.Ho * g.Wo, 32 if prec == 'f32' else 64, (1024 + tiles - 1) // tiles, 4)
    return dict(grid=tiles * n, blocks_per_element=n, cls=frozenset(['gemm']))


def dispatch(g, pass_, tile, prec, bias=False, act=False, accumulate=False):
    """-> (kernel, <KT, WO> instantiation or None, plan): the kernel that must run -- 'gemm' for the register-staged family -- or
    (UNSUPPORTED, None, None).  bias / act / accumulate: of an input-gradient launch."""
    assert pass_ in PASSES and tile in TILES and prec in PRECS
    inst = (g.kt, g.Wo)
    gemm = ('gemm', None, dict(cls=frozenset(['gemm'])))
    refused = (UNSUPPORTED, None, None)
    if pass_ == 'fprop':                                      # (bf16y: the forward pass has no y input and treats it as bf16)
        if tile in (0, 6) and c4_fprop_ok(g):
            return ('fprop_c4_kernel' if prec == 'f32' else 'fprop_c4_bf16_kernel'), inst, plan_fprop(g)
        return refused if tile == 6 else gemm
    if pass_ == 'dgrad':
        if tile in (0, 6) and c4_dgrad_mfma_ok(g, bias, act, accumulate):
            return 'dgrad_c4_mfma_kernel', inst, plan_col2im(g)
        if prec == 'bf16y':                                   # a bf16 y beside fp32 w: the col2im kernel only
            return refused
        if tile in (0, 6) and c4_dgrad_valu_ok(g):            # elsewhere the layer's code means "the kernel written for it"
            return 'dgrad_c4_kernel', (g.kt,), plan_valu(g)
        return gemm
    if tile == 6:
        if c4_wgrad_ok(g, prec):
            return ('wgrad_c4_kernel' if prec == 'f32' else 'wgrad_c4_bf16_kernel'), inst, plan_wgrad(g, prec)
        return refused
    return 'gemm', None, plan_wgrad_gemm(g, tile, prec)


def bit_reproducible(pass_):
    """does a repeat launch stay bit-equal?  Everything but the weight gradients (float atomics of many blocks onto one dw): the col2im
    kernel's shared rows get exactly two addends onto zero, which commute, and no tile code of the table splits K"""
    return pass_ != 'wgrad'


# ---- the case table: N, Ti, (Hi, Wi), kt -- Ci = 3 padded to 4, Co = 64; the smallest shapes that reach each edge ------------------------
WGRAD_SPLIT_TO = (4, 5, 9, 13, 17)
C4_ROWS = [
    (1, 1, (32, 32), 1),            # <1, 16>; N = 1; one forward block per item; two col2im tiles per frame
    (1, 1, (16, 64), 1),            # <1, 32>
    (2, 4, (32, 32), 4),            # <4, 16>
    (2, 5, (16, 64), 4),            # <4, 32>
    (1, 1, (64, 32), 1),            # H > W, two row blocks
    (2, 1, (16, 32), 1),            # Ho = 8, Wo = 16: col2im accepts (8 % 8), tile 6 refused in fprop and wgrad (8 % 16), tile 0 -> GEMM
    (3, 1, (2, 32), 1),             # VALU only: runs = 3, a partly filled block
    (17, 1, (2, 32), 1),            # VALU only: runs = 17, a second block with one run
    (1, 1, (4, 128), 1),            # VALU only: Wo = 64 (no first-layer width), runs = 8
] + [(1, To + 3, (16, 64), 4) for To in WGRAD_SPLIT_TO] + [      # frame split 2 (2+2), 2 (3+2), 4 (3,3,3,0), 4 (4,4,4,1), 8 (3x5,2,0,0)
    (520, 1, (16, 64), 1),          # 520 pairs on 512 weight-gradient blocks; 1040 col2im tiles on 1024 blocks
]
VIEW_ROWS = [C4_ROWS[0], C4_ROWS[1]]
VIEW_CLIPS = (1, 2)                 # the row as it stands, and two clips so that the clip-order permutation is no identity
FULL_MANTISSA_ROW = C4_ROWS[3]      # the row the bf16 modes also run on full-mantissa operands


def row_id(row):
    N, Ti, (Hi, Wi), kt = row
    return "%dx%dx%dx%d-kt%d" % (N, Ti, Hi, Wi, kt)


def dgrad_variants(g):
    """the launches of an input-gradient row: plain; accumulating onto a non-zero x"""
    return [dict(bias=False, act=False, accumulate=False), dict(bias=False, act=False, accumulate=True)]


def _away_from_zero(rng, shape, floor):
    v = rng.randn(*shape)
    return np.where(v < 0, v - floor, v + floor)


def bf16_round(a):
    """fp32 -> the nearest bf16-representable fp32 (ties to even)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).astype(np.uint32)
    return u.view(np.float32)


def inputs(row, exact=True, seed=0):
    """The seeded fp32 operands of a row.  Activations and gradients of unit size with no element inside (-0.25, 0.25), filters of
    size 0.05, biases and the starting values of dw and x with no element inside (-0.5, 0.5): a dropped pixel, tap, frame, item or
    starting value moves some element by far more than its bound.  The padding channel of x, w, bias4, dw0 and x0 is zero.
    exact: every value is bf16-representable, so that the bf16 modes form exact products and the fp32 bound applies to them."""
    N, Ti, (Hi, Wi), kt = row
    rng = np.random.RandomState(6400 + 97 * seed + (C4_ROWS.index(row) if row in C4_ROWS else 50))
    rnd = bf16_round if exact else (lambda a: np.ascontiguousarray(a, np.float32))

    def padded(a):
        a[..., CV:] = 0
        return rnd(a)
    To, Ho, Wo = Ti - kt + 1, Hi // 2, Wi // 2
    gy = _away_from_zero(rng, (N, To, Ho, Wo, CO), 0.25)
    # Items a weight-gradient block reaches on its SECOND walk (n >= 512) carry 64 x the gradient: a sum over 133 120 pixels has a
    # bound of 0.8 % of S, and eight items of unit size with random signs would vanish inside it (their sum is ~45 terms' worth
    # against a bound of ~1000); scaled by a power of two they stay bf16-representable and move every element of dw by about the bound
    # of the whole sum and more
    gy[512:] *= 64
    return dict(x=padded(_away_from_zero(rng, (N, Ti, Hi, Wi, CI), 0.25)), w=padded(_away_from_zero(rng, (CO, kt, 4, 4, CI), 0.25) * 0.05),
                gy=rnd(gy), bias=rnd(_away_from_zero(rng, (CO,), 0.5)),
                bias4=padded(_away_from_zero(rng, (CI,), 0.5)), dw0=padded(_away_from_zero(rng, (CO, kt, 4, 4, CI), 0.5)),
                x0=padded(_away_from_zero(rng, (N, Ti, Hi, Wi, CI), 0.5)))


def to_clip_order(frames, clips):
    """[T * clips][1][H][W][C] in launch order (item t * clips + b) -> the clip [clips][T][H][W][C] the permuted launch writes"""
    n, one, H, W, C = frames.shape
    v = frames.reshape(n // clips, clips, H, W, C)
    return v.permute(1, 0, 2, 3, 4).contiguous() if hasattr(v, 'permute') else np.ascontiguousarray(v.transpose(1, 0, 2, 3, 4))
