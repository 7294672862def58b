"""tests/epilogue_ref.py by hand: the float64 restatement of the fused conv epilogues on tiny arrays, the case table of
tests/test_gpu_epilogue_guard.py against the conditions it is there for (computed from N, To / Ti, Ho, Wo, C), and the support matrix
against what include/mocogan_hip.h promises."""
import numpy as np

import epilogue_ref as ER


def test_statistics_and_column_sums_by_hand():
    v = np.array([[1.0, -2.0], [3.0, 0.5], [-1.0, 4.0], [2.0, 2.0]])
    sel = ER.group_rows('fprop', 2, 1, 1, 2, 2)                     # N = 2, two rows per item
    assert [s.tolist() for s in sel] == [[True, True, False, False], [False, False, True, True]]
    s, a = ER.partial_sums('stats', v, sel)
    assert s.tolist() == [[[4.0, -1.5], [10.0, 4.25]], [[1.0, 6.0], [5.0, 20.0]]]
    assert a.tolist() == [[[4.0, 2.5], [10.0, 4.25]], [[3.0, 6.0], [5.0, 20.0]]]
    s, a = ER.partial_sums('col', v, ER.group_rows('fprop', 2, 1, 1, 2, 1))
    assert s.tolist() == [[[5.0, 4.5], [0.0, 0.0]]] and a.tolist() == [[[7.0, 8.5], [0.0, 0.0]]]


def test_batchnorm_backward_sums_by_hand():
    # one column: mean 1, inv_std 2, scale 0.5, shift -1  ->  pre = y / 2 - 1, x_hat = 2 (y - 1)
    stats = np.array([1.0, 2.0, 0.5, -1.0], np.float32)
    y = np.array([[4.0], [0.0], [3.0]])                            # pre = 1, -1, 0.5
    v = np.array([[2.0], [10.0], [-1.0]])
    sel = [np.ones(3, bool)]
    s, a = ER.partial_sums('bn_bwd', v, sel, bn=(y, 'relu'), stats=(stats,))
    # g' = 2, 0, -1;  x_hat = 6, -2, 4
    assert s.tolist() == [[[1.0], [8.0]]] and a.tolist() == [[[3.0], [16.0]]]
    s, a = ER.partial_sums('bn_bwd', v, sel, bn=(y, 'lrelu'), stats=(stats,))
    k = ER.LRELU_SLOPE
    assert np.allclose(s, [[[1.0 + 10 * k], [8.0 - 20 * k]]], rtol=0, atol=1e-15)
    assert np.allclose(a, [[[3.0 + 10 * k], [16.0 + 20 * k]]], rtol=0, atol=1e-15)
    assert k == float(np.float32(0.2)) and abs(k - 0.2) < 2.0 ** -26
    # the activation's derivative at its kink, as mcg_bn_act_bwd has it
    assert ER.act_derivative(np.array([0.0, -0.0]), 'relu').tolist() == [0.0, 0.0]
    assert ER.act_derivative(np.array([0.0, -0.0]), 'lrelu').tolist() == [1.0, 1.0]


def test_input_gradient_groups_follow_the_batch_item_in_every_parity_class():
    N, T, H, W = 4, 2, 2, 2
    sel = ER.group_rows('dgrad', N, T, H, W, 2)
    n_of_row = np.repeat(np.arange(N), T * H * W)
    assert np.array_equal(sel[0], n_of_row < 2) and np.array_equal(sel[1], n_of_row >= 2)
    # every output-parity class (h % 2, w % 2) holds rows of both groups, a quarter of each
    hw = np.arange(N * T * H * W) % (H * W)
    for ph in range(2):
        for pw in range(2):
            cls = (hw // W % 2 == ph) & (hw % W % 2 == pw)
            assert (sel[0] & cls).sum() == (sel[1] & cls).sum() == N * T * H * W // 8
    assert ER.group_rows('dgrad', 3, 1, 2, 2, 1)[0].all()


def test_mask_words_by_hand():
    pre = -np.ones((2, 40))
    pre[0, [0, 31, 32, 39]] = [0.0, 2.0, 1.0, 5.0]                 # 0.0 counts as non-negative
    pre[1, 33] = -0.0                                              # -0.0 >= 0
    w = ER.mask_words(pre)
    assert w.shape == (2, 2) and w.dtype == np.uint32
    assert w.tolist() == [[0x80000001, 0x81], [0, 0x2]]
    assert ER.valid_bits(40).tolist() == [0xffffffff, 0xff] and ER.valid_bits(64).tolist() == [0xffffffff] * 2
    assert ER.valid_bits(4).tolist() == [0xf]
    bits = ER.unpack_bits(w, 40)
    assert np.array_equal(bits, pre >= 0)
    # garbage above column C in the last word must not matter to a reader that goes through valid_bits / unpack_bits
    dirty = w.copy()
    dirty[:, 1] |= np.uint32(0xffffff00)
    assert np.array_equal(ER.unpack_bits(dirty, 40), bits) and np.array_equal(dirty & ER.valid_bits(40), w)
    m = ER.lrelu_bwd_multiplier(w, 40)
    assert m[0, 0] == 1.0 and m[0, 1] == ER.LRELU_SLOPE and m[1, 33] == 1.0
    assert ER.leaky_relu(np.array([-1.0, 0.0, 2.0])).tolist() == [-ER.LRELU_SLOPE, 0.0, 2.0]


def test_bound_is_the_derived_one():
    assert ER.sums_bound(1.0) == (256 + 8) * 2.0 ** -24
    # a row dropped from a column of equal terms moves it by 1 / rows of sum|t|: more than 100 bounds at the ragged shapes
    assert (1.0 / 288) / ER.sums_bound(1.0) > 100 and (1.0 / 96) / ER.sums_bound(1.0) > 100


def _ragged(rows, tile):
    return rows % tile != 0


def test_case_table_meets_its_stated_conditions():
    c = [ER.dims(k) for k in ER.CASES]
    # 288 rows in both passes: ragged for 64-, 128- and 256-row tiles; group boundary inside a tile, a multiple of 4; Co = 40
    for i in (0, 7):
        assert c[i]['rows_f'] == c[i]['rows_class'] == 288
        assert all(_ragged(288, t) for t in (64, 128, 256))
        half = c[i]['rows_f'] // 2
        assert half == 144 and all(half % t for t in (64, 128, 256)) and half % 4 == 0
    assert c[0]['Co'] == 40 and (40 + 31) // 32 == 2 and 40 % 32 != 0 and 40 % 64 != 0
    # 3-D, 96 forward rows, 48 per group
    assert c[1]['kt'] == 4 and c[1]['rows_f'] == 96 and c[1]['rows_f'] // 2 == 48 and 48 % 64
    # C not a multiple of 8 -> no bf16-stored operands; split operands forward only (16 | Ci; the input gradient would sum over Co = 20)
    assert c[2]['Co'] % 8 and c[2]['Co'] % 4 == 0
    assert [p for p in ER.PRECS if ER.tiles_of('fprop', p, ER.CASES[2])] == ['f32', 'bf16', 'f32x3']
    assert ER.tiles_of('fprop', 'f32x3', ER.CASES[2]) == [7, 8, 10]
    assert [p for p in ER.PRECS if ER.tiles_of('dgrad', p, ER.CASES[2])] == ['f32', 'bf16']
    # three column tiles (64 wide), the last ragged; five mask words
    assert -(-c[3]['Co'] // 64) == 3 and c[3]['Co'] % 64 and (c[3]['Co'] + 31) // 32 == 5
    # the Ci = 4 kernels: tile code 6 takes them forward, in fp32 and bf16; odd N; H != W
    for i in (4, 5, 6):
        assert c[i]['Cip'] == 4 and c[i]['Ci'] == 3 and c[i]['Co'] == 64
        for prec in ('f32', 'bf16'):
            assert ER.takes('fprop', 6, prec, ER.CASES[i]) and ER.takes('fprop', 0, prec, ER.CASES[i])
            assert not ER.takes('dgrad', 6, prec, ER.CASES[i])
        assert c[i]['Co'] % 16 == 0                                # the first-layer forms with out_split run
    assert c[5]['N'] % 2 == 1 and not ER.form_ok('fprop', 'act', 'f32', ER.CASES[5], 2)
    assert c[6]['H'] != c[6]['W'] and c[6]['Wo'] == 16
    # LDS-DMA, dense and position-major families at 288 ragged rows
    for fam in ('lds', 'dense', 'posmajor', 'posmajor37'):
        assert all(ER.takes('fprop', t, 'f32x3', ER.CASES[7]) for t in ER.FAMILIES[fam]), fam
    assert all(ER.takes('dgrad', t, 'f32x3', ER.CASES[7]) for t in ER.FAMILIES['lds'] + ER.FAMILIES['dense'])
    assert all(ER.takes('fprop', t, 'bf16s', ER.CASES[7]) and ER.takes('fprop', t, 'f32', ER.CASES[7]) for t in ER.FAMILIES['lds'])
    # a ragged column tile for 128- and 256-wide tiles
    assert c[8]['Co'] % 128 and c[8]['Co'] % 256 and c[8]['Co'] > 128
    assert all(ER.takes('fprop', t, p, ER.CASES[8]) for t in ER.FAMILIES['lds'] for p in ('f32', 'bf16s', 'f32x3'))
    # two groups on the 256x256 tile: the tile exists (Co >= 256), the group boundary lies inside a 256-row tile
    assert c[9]['Co'] >= 256 and c[9]['N'] % 2 == 0 and (c[9]['rows_f'] // 2) % 256 and c[9]['rows_f'] > 256
    assert all(ER.takes(p_, 8, 'bf16s', ER.CASES[9]) for p_ in ('fprop', 'dgrad'))
    # code 9
    assert all(ER.takes('dgrad', 9, p, ER.CASES[10]) for p in ('bf16s', 'f32x3'))
    assert not any(ER.takes('dgrad', 9, p, k) for p in ER.PRECS for k in ER.CASES[:10])
    # (added) the LDS-DMA forward takes fp32 operands with Co = 8 k + 4, and must then refuse a bf16 output, which it stores in runs of
    # 8 channels; the register-staged tiles store element by element and run it
    assert c[11]['Co'] % 8 == 4 and all(ER.takes('fprop', t, 'f32', ER.CASES[11]) for t in ER.FAMILIES['lds'])
    assert not any(ER.expected('fprop', t, 'f32', 'plain', 'bf16', ER.CASES[11]) for t in ER.FAMILIES['lds'])
    assert all(ER.expected('fprop', t, 'f32', 'stats', 'f32', ER.CASES[11]) for t in ER.FAMILIES['lds'])
    assert all(ER.expected('fprop', t, 'f32', 'plain', 'bf16', ER.CASES[11]) for t in ER.FAMILIES['reg'])
    # in-kernel noise: a row quad never straddles two groups (make_epi refuses that)
    for k, d in zip(ER.CASES, c):
        if d['N'] % 2 == 0:
            assert (d['rows_f'] // 2) % 4 == 0, k


def test_cases_reach_every_running_entry_of_the_support_matrix():
    """every (pass, family, precision, class, output) that SUPPORT says runs is expected to run at some case, tile code of the family
    and group count -- what the closing test of the GPU module then finds to have happened"""
    reached = set()
    codes = set()
    for case in ER.CASES:
        for p_ in ER.FORMS:
            for prec in ER.PRECS:
                for tile in ER.tiles_of(p_, prec, case):
                    for cls, out in ER.FORMS[p_]:
                        if ER.expected(p_, tile, prec, cls, out, case, 1):
                            reached.add((p_, ER.family_of(tile), prec, cls, out))
                            codes.add((p_, tile))
    assert reached == {k for k, v in ER.SUPPORT.items() if v}
    assert {t for p_, t in codes if p_ == 'fprop'} == {t for f in ER.FAMILIES if f != 'patch' for t in ER.FAMILIES[f]}
    assert {t for p_, t in codes if p_ == 'dgrad'} == {t for f in ('reg', 'lds', 'patch', 'dense') for t in ER.FAMILIES[f]}
    # the issue's two production combinations
    for t in (1, 2, 3, 4, 5):
        assert any(ER.expected('fprop', t, 'f32', 'bn_bwd', 'f32', k, 2) for k in ER.CASES)
    for t in (27, 40):
        assert any(ER.expected('fprop', t, 'f32x3', 'bn_bwd', 'f32', k, 2) for k in ER.CASES)


def test_support_matrix_holds_what_the_header_promises():
    S = ER.SUPPORT
    runs = lambda p_, fam, cls: any(v for (a, b, _, c, _), v in S.items() if (a, b, c) == (p_, fam, cls))
    # statistics: every GEMM family of both passes (the Ci = 4 kernels carry the activation only: c4_fprop_ok)
    for fam in ('reg', 'lds', 'dense', 'posmajor', 'posmajor37'):
        assert runs('fprop', fam, 'stats'), fam
    for fam in ('reg', 'lds', 'dense', 'patch'):
        assert runs('dgrad', fam, 'stats') and runs('dgrad', fam, 'col') and runs('dgrad', fam, 'mask'), fam
    # BatchNorm's backward sums: the register-staged tiles (fp32 tensors) and the LDS-DMA kernels, both passes; position-major 27 / 40
    for p_ in ('fprop', 'dgrad'):
        for fam in ('reg', 'lds', 'dense'):
            assert runs(p_, fam, 'bn_bwd'), (p_, fam)
    assert runs('fprop', 'posmajor', 'bn_bwd') and not runs('fprop', 'posmajor37', 'bn_bwd') and not runs('dgrad', 'patch', 'bn_bwd')
    # "MCG_SUMS_BN_BWD [with out_bf16]: LDS-DMA kernels only", bf16-stored operands
    assert [k[1:3] for k, v in S.items() if v and k[3:] == ('bn_bwd', 'bf16')] == [('lds', 'bf16s')] * 2
    # the first layer's activation epilogue: forward, register-staged and Ci = 4 kernels, fp32-stored operands, every output type
    for fam in ('reg', 'c4'):
        for prec in ('f32', 'bf16'):
            assert all(S[('fprop', fam, prec, 'act', o)] for o in ('f32', 'bf16', 'split'))
    assert not any(v for k, v in S.items() if k[3] == 'act' and (k[1] not in ('reg', 'c4') or k[2] in ('bf16s', 'f32x3')))
    # split operands never write a bf16 output; nothing but split operands runs the dense / position-major codes
    assert not any(v for k, v in S.items() if k[2] == 'f32x3' and k[4] != 'f32')
    assert not any(v for k, v in S.items() if k[1] in ('dense', 'posmajor', 'posmajor37') and k[2] != 'f32x3')
    # position-major rows are forward only; the patch kernel and the weight-stationary first layer one pass each
    assert not any(v for k, v in S.items() if k[0] == 'dgrad' and k[1] in ('posmajor', 'posmajor37', 'c4'))
    assert not any(v for k, v in S.items() if k[0] == 'fprop' and k[1] == 'patch')
    # the domain is complete: every family x precision x form of a pass has an entry
    assert len(S) == len(ER.FAMILIES) * len(ER.PRECS) * (len(ER.FORMS['fprop']) + len(ER.FORMS['dgrad']))
