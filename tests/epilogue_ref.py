"""What a fused convolution epilogue produces, restated from include/mocogan_hip.h in NumPy float64 (mcg_conv_epilogue), and which
(pass, kernel family, precision, epilogue class, output type) the library runs or refuses, restated from the dispatch code of
csrc/conv_gemm.hip (with_epi<MAXC>, c4_fprop_ok, dgrad_patch_ok, make_epi, the table above conv_fprop_impl).

Everything is taken from the launch's own STORED output v ("the sums are those of the STORED values"): the caller casts the device
tensor to float64 and hands it over as rows [rows][C] in the order of the output tensor ([N][T][H][W][C] of either pass).
No device code and no torch here: tests/test_epilogue_ref_cpu.py checks this module by hand, tests/test_gpu_epilogue_guard.py the
kernels against it."""
import numpy as np

LRELU_SLOPE = float(np.float32(0.2))         # EPI_LRELU_SLOPE: leaky_relu's slope as the fp32 number the kernels multiply by
U = 2.0 ** -24                               # unit roundoff of fp32
TALLEST_TILE = 256                           # rows of the tallest block tile: a slot entry is an fp32 sum of at most that many terms


def sums_bound(abs_sum):
    """|sum over slots (float64) of part - reference| is at most this.  A slot entry is an fp32 sum, in some order, of n <= 256 row
    terms: error <= n u sum|t|.  A term carries at most four roundings of its own (BN_BWD: v * act', y - mean, two products;
    STATS: one square), doubled for margin: 8 u sum|t|.  Derived, not measured."""
    return (TALLEST_TILE + 8) * U * np.asarray(abs_sum, np.float64)


# ---- group row ranges ---------------------------------------------------------------------------------------------------------
def group_rows(pass_, N, T, H, W, groups):
    """boolean row selectors [groups][rows] over the output rows [N][T][H][W] (fprop: T, H, W = To, Ho, Wo; dgrad: Ti, Hi, Wi).
    fprop: the halves of the batch are the halves of the rows.  dgrad: the kernel walks one output-parity class at a time in
    (t, n, h/2, w/2) order; a row belongs to group 0 when its batch item n < N / 2, in every class -- decoded here from the row."""
    rows = N * T * H * W
    if groups == 1:
        return [np.ones(rows, bool)]
    assert groups == 2 and N % 2 == 0
    r = np.arange(rows)
    if pass_ == 'fprop':
        first = r < rows // 2
    else:
        first = (r // (T * H * W)) < N // 2
    return [first, ~first]


# ---- partial sums -------------------------------------------------------------------------------------------------------------
def act_derivative(pre, act):
    """act'(pre) as mcg_bn_act_bwd defines it: ReLU 1 for pre > 0 else 0; leaky ReLU the slope for pre < 0 else 1"""
    if act == 'relu':
        return np.where(pre > 0, 1.0, 0.0)
    assert act == 'lrelu'
    return np.where(pre < 0, LRELU_SLOPE, 1.0)


def bn_pre_activation(y, stats, C):
    """y * scale + shift with the fp32 numbers of a 4C bn_stats buffer (mean, inv_std, scale, shift), in float64"""
    st = np.asarray(stats, np.float32).astype(np.float64)
    return np.asarray(y, np.float64) * st[2 * C:3 * C] + st[3 * C:4 * C]


def sums_terms(cls, v, bn=None, stats=None):
    """the two row terms [2][rows][C] a sums class adds per column: STATS (v, v^2); COL (v, 0); BN_BWD (g', g' x_hat) with
    g' = v * act'(y scale + shift), x_hat = (y - mean) * inv_std.  bn = (y rows [rows][C], 'relu' | 'lrelu'); stats: 4C floats."""
    v = np.asarray(v, np.float64)
    if cls == 'stats':
        return np.stack([v, v * v])
    if cls == 'col':
        return np.stack([v, np.zeros_like(v)])
    assert cls == 'bn_bwd'
    y, act = bn
    C = v.shape[1]
    st = np.asarray(stats, np.float32).astype(np.float64)
    y = np.asarray(y, np.float64)
    g = v * act_derivative(bn_pre_activation(y, stats, C), act)
    return np.stack([g, g * ((y - st[:C]) * st[C:2 * C])])


def partial_sums(cls, v, selectors, bn=None, stats=(None, None)):
    """(sums, abs_sums), each [groups][2][C] float64: per group and column the two sums of the class and the sums of |term|"""
    sums, asum = [], []
    for gi, sel in enumerate(selectors):
        t = sums_terms(cls, np.asarray(v, np.float64)[sel], None if bn is None else (np.asarray(bn[0])[sel], bn[1]), stats[gi])
        sums.append(t.sum(1))
        asum.append(np.abs(t).sum(1))
    return np.stack(sums), np.stack(asum)


# ---- mask bits ----------------------------------------------------------------------------------------------------------------
def mask_words(pre):
    """[rows][(C+31)//32] uint32: bit c & 31 of word c >> 5 set <=> pre[row][c] >= 0; bits of columns >= C are zero HERE (the
    kernels leave them unspecified: compare through valid_bits)"""
    pre = np.asarray(pre)
    rows, C = pre.shape
    words = np.zeros((rows, (C + 31) // 32), np.uint32)
    for c in range(C):
        words[:, c >> 5] |= (pre[:, c] >= 0).astype(np.uint32) << np.uint32(c & 31)
    return words


def valid_bits(C):
    """per word of a row the bits that belong to columns < C"""
    nw = (C + 31) // 32
    m = np.full(nw, 0xffffffff, np.uint32)
    if C % 32:
        m[-1] = np.uint32((1 << (C % 32)) - 1)
    return m


def unpack_bits(words, C):
    w = np.asarray(words).astype(np.uint32)
    cols = np.arange(C)
    return ((w[:, cols >> 5] >> (cols & 31).astype(np.uint32)) & 1).astype(bool)


def lrelu_bwd_multiplier(words, C):
    """leaky_relu's backward from stored sign bits (mcg_conv_epilogue.mask_in): 1 where the bit is set, else the slope"""
    return np.where(unpack_bits(words, C), 1.0, LRELU_SLOPE)


def leaky_relu(pre):
    pre = np.asarray(pre, np.float64)
    return np.where(pre >= 0, pre, LRELU_SLOPE * pre)


# ---- kernel families, support matrix ------------------------------------------------------------------------------------------
# 'posmajor37' is code 37 of the position-major family: 27 with nothing skipped, instantiated up to class 1 only (launch_fprop_live's
# with_epi<LV == 2 ? 1 : 2>), so it has a row of its own.
FAMILIES = {
    'reg': (1, 2, 3, 4, 5, 101, 203),        # register-staged gemm_kernel / gemm_bf16_kernel
    'c4': (0, 6),                            # the kernels of the Ci = 4 layers (0: the library's choice picks them there)
    'lds': (7, 8, 10),                       # LDS-DMA gemm_bf16_v2_kernel
    'patch': (9,),                           # dgrad_patch_kernel
    'dense': (17, 20),                       # the dense LDS form of split operands
    'posmajor': (27, 40),                    # ... with position-major rows (forward only)
    'posmajor37': (37,),
}
PRECS = ('f32', 'bf16', 'bf16s', 'f32x3')
# (epilogue class, output type) pairs the module launches, per pass:
#   stats  MCG_SUMS_STATS with a bias          bn_bwd MCG_SUMS_BN_BWD (f32: fp32 bn_y and output; bf16: bf16 bn_y and out_bf16)
#   act    leaky_relu + noise + mask_out       col    mask_in + MCG_SUMS_COL        mask   mask_in alone
#   plain  no epilogue class: out_bf16 alone (fprop) / act = MCG_ACT_RELU + out_bf16 (dgrad)
FORMS = {
    'fprop': (('stats', 'f32'), ('bn_bwd', 'f32'), ('bn_bwd', 'bf16'), ('act', 'f32'), ('act', 'bf16'), ('act', 'split'), ('plain', 'bf16')),
    'dgrad': (('stats', 'f32'), ('bn_bwd', 'f32'), ('bn_bwd', 'bf16'), ('col', 'f32'), ('mask', 'f32'), ('plain', 'bf16')),
}
_S, _B, _B16, _A, _A16, _ASP, _P16 = FORMS['fprop']
_C, _M = ('col', 'f32'), ('mask', 'f32')
# what RUNS; every other (pass, family, precision, form) of the domain FAMILIES x PRECS x FORMS is refused with MCG_ERR_UNSUPPORTED.
#   register-staged: classes 2 / 3 exist for fp32-stored operands only (with_epi<PM == 2 ? 1 : 3 / 2>), class 2 reads and writes fp32
#   Ci = 4 forward: the activation class only (c4_fprop_ok); a plain bf16 output with 'bf16' only; no dgrad kernel of that family
#       carries an epilogue or a bf16 output (c4_dgrad_mfma_ok, conv_dgrad_impl: e.out16 && Ci == 4)
#   LDS-DMA: class 2 with bf16-stored / split operands (with_epi<PM == 2 ? 2 : 1>), never class 3; split operands never with out16
#   patch: class 1 (with_epi<1>); position-major: forward only, 37 up to class 1
_RUNS = {
    ('fprop', 'reg'): {'f32': (_S, _B, _A, _A16, _ASP, _P16), 'bf16': (_S, _B, _A, _A16, _ASP, _P16), 'bf16s': (_S, _P16)},
    ('fprop', 'c4'): {'f32': (_A, _A16, _ASP), 'bf16': (_A, _A16, _ASP, _P16)},
    ('fprop', 'lds'): {'f32': (_S, _P16), 'bf16s': (_S, _B, _B16, _P16), 'f32x3': (_S, _B)},
    ('fprop', 'dense'): {'f32x3': (_S, _B)},
    ('fprop', 'posmajor'): {'f32x3': (_S, _B)},
    ('fprop', 'posmajor37'): {'f32x3': (_S,)},
    ('dgrad', 'reg'): {'f32': (_S, _B, _C, _M, _P16), 'bf16': (_S, _B, _C, _M, _P16), 'bf16s': (_S, _C, _M, _P16)},
    ('dgrad', 'lds'): {'f32': (_S, _C, _M, _P16), 'bf16s': (_S, _B, _B16, _C, _M, _P16), 'f32x3': (_S, _B, _C, _M)},
    ('dgrad', 'dense'): {'f32x3': (_S, _B, _C, _M)},
    ('dgrad', 'patch'): {'bf16s': (_S, _C, _M, _P16), 'f32x3': (_S, _C, _M)},
}
SUPPORT = {(p, fam, prec, cls, out): (cls, out) in _RUNS.get((p, fam), {}).get(prec, ())
           for p in FORMS for fam in FAMILIES for prec in PRECS for cls, out in FORMS[p]}


def family_of(tile):
    for fam, codes in FAMILIES.items():
        if tile in codes:
            return fam
    raise KeyError(tile)


# ---- cases --------------------------------------------------------------------------------------------------------------------
CASES = [
    # N, Ti, H (or (H, W)), Ci, Co, kt
    (6, 3, 8, 64, 40, 1),        # 288 rows in both passes, group boundary at row 144; Co = 40
    (6, 4, 8, 64, 40, 4),        # 3-D, 96 forward rows, 48 per group
    (2, 9, 8, 16, 20, 4),        # C not a multiple of 8
    (2, 1, 16, 16, 160, 1),      # three column tiles, the last ragged, five mask words
    (2, 5, 32, 3, 64, 4),        # the Ci = 4 kernels
    (3, 1, 32, 3, 64, 1),        # ... odd N
    (2, 5, (64, 32), 3, 64, 4),  # ... H != W
    (6, 3, 8, 64, 128, 1),       # LDS-DMA, dense, position-major at 288 ragged rows
    (2, 4, 8, 64, 192, 4),       # LDS-DMA: ragged column tile for 128 / 256 wide tiles
    (2, 6, 16, 128, 256, 4),     # LDS-DMA: two groups on the 256x256 tile
    (2, 7, 32, 64, 128, 4),      # code 9
    (2, 1, 8, 64, 20, 1),        # (added) Co = 8 k + 4 on the LDS-DMA kernels, whose bf16 store writes runs of 8 channels: refused
]


def dims(case):
    """everything the tests derive from a case: extents, padded channels, rows per pass"""
    N, Ti, H, Ci, Co, kt = case
    H, W = H if isinstance(H, tuple) else (H, H)
    To, Ho, Wo = Ti - kt + 1, H // 2, W // 2
    Cip = (Ci + 3) // 4 * 4
    return dict(N=N, Ti=Ti, H=H, W=W, Ci=Ci, Cip=Cip, Co=Co, kt=kt, To=To, Ho=Ho, Wo=Wo,
                rows_f=N * To * Ho * Wo,            # output rows of fprop = GEMM rows
                rows_d=N * Ti * H * W,              # output rows of dgrad ...
                rows_class=N * Ti * Ho * Wo)        # ... a quarter of them per output-parity class = GEMM rows of a block column


def _pow2(c, lo):
    return c >= lo and c & (c - 1) == 0


def takes(pass_, tile, prec, case):
    """does the PLAIN launch of this pass / tile code / precision accept the geometry (make_geom, split_ok, dense_ok, v2_ok,
    c4_layer, dgrad_patch_ok and the branches of conv_fprop_impl / conv_dgrad_impl, restated)"""
    d = dims(case)
    Ci, Co, fam = d['Cip'], d['Co'], family_of(tile)
    if prec == 'bf16s' and (Ci % 8 or Co % 8):
        return False
    ksum = Ci if pass_ == 'fprop' else Co                      # the channel count the GEMM sums over
    if prec == 'f32x3' and (fam in ('reg', 'c4') or not _pow2(ksum, 16)):
        return False
    if fam == 'reg':
        return True
    if fam == 'c4':                                            # forward only here: the input gradient of these layers has no epilogue
        return (pass_ == 'fprop' and prec in ('f32', 'bf16') and Ci == 4 and Co == 64 and d['Wo'] in (16, 32)
                and d['Ho'] % (256 // d['Wo']) == 0)
    if fam == 'patch':
        return pass_ == 'dgrad' and prec in ('bf16s', 'f32x3') and Ci == 64 and d['Ho'] == 16 and d['Wo'] == 16 and Co % 64 == 0
    if prec == 'bf16' or (fam != 'lds' and prec != 'f32x3'):
        return False
    if prec != 'f32x3' and not _pow2(ksum, 64):
        return False
    if pass_ == 'dgrad':
        if fam in ('posmajor', 'posmajor37') or not _pow2(Ci, 64):
            return False
        if prec == 'f32' and tile == 10 and Ci == 64:          # (256x64 with two buffers is not instantiated for fp32 operands)
            return False
    if fam != 'lds' and ksum % 64:
        return False
    if fam in ('posmajor', 'posmajor37') and d['N'] * d['To'] < 2:
        return False
    return True


def form_ok(pass_, cls, out, case, groups):
    """the conditions on a form that do not depend on the kernel family (make_epi, conv_dgrad_impl): two groups need an even batch,
    the split output whole groups of 16 channels; the input gradient of a Ci = 4 layer never writes bf16 nor carries ReLU"""
    d = dims(case)
    if groups == 2 and d['N'] % 2:
        return False
    if out == 'split' and d['Co'] % 16:
        return False
    if pass_ == 'dgrad' and out == 'bf16' and d['Cip'] == 4:
        return False
    return True


def expected(pass_, tile, prec, cls, out, case, groups=1):
    """True: the fused launch must run; False: it must be refused"""
    fam = family_of(tile)
    if fam == 'lds' and out == 'bf16' and (dims(case)['Co'] if pass_ == 'fprop' else dims(case)['Cip']) % 8:
        return False                 # the row-wise bf16 store of the LDS-DMA kernels writes runs of 8 channels (conv_fprop_impl)
    return takes(pass_, tile, prec, case) and form_ok(pass_, cls, out, case, groups) and SUPPORT[(pass_, fam, prec, cls, out)]


def tiles_of(pass_, prec, case):
    """the tile codes of the families that take the case, in family order"""
    return [t for fam in FAMILIES for t in FAMILIES[fam] if takes(pass_, t, prec, case)]
