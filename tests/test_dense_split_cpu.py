"""Host side of the dense LDS form of the MCG_PREC_SPLIT GEMMs (tile codes 17 / 20), checked without a GPU: which geometries and
passes admit the form, which tile codes the library takes, and that the K range of a block is a whole number of triples of
K-steps.  Nothing is launched: mcg_conv_dense_split_ok / mcg_conv_dense_split_chunk are pure functions of the geometry, and the
conv entry points validate the geometry before they look at their pointers."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def geom(hl, N, Ti, H, Ci, Co, kt, tile=0, precision='f32x3'):
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision=precision)
    g.tile = tile
    return g


# the layers of the benchmark's networks (N clips of 16 frames at 64 x 64, 64 base filters): dc2..dc4 of D_V (3-D) and D_I (2-D)
BENCH_LAYERS = [(32, 13, 32, 64, 128, 4), (32, 10, 16, 128, 256, 4), (32, 7, 8, 256, 512, 4),
                (32, 1, 32, 64, 128, 1), (32, 1, 16, 128, 256, 1), (32, 1, 8, 256, 512, 1)]


def test_which_geometries_admit_the_dense_form(hl):
    for case in BENCH_LAYERS:
        g = geom(hl, *case)
        assert hl.dense_split_ok("fprop", g) and hl.dense_split_ok("dgrad", g) and hl.dense_split_ok("wgrad", g), case
    # a triple of K-steps is 64 channels of one filter tap: 64 | Ci forward, 64 | Co in the input gradient
    for ci, want in ((16, False), (32, False), (64, True), (128, True)):
        assert hl.dense_split_ok("fprop", geom(hl, 2, 1, 16, ci, 128, 1)) == want, ci
    for co, want in ((16, False), (32, False), (64, True), (256, True)):
        assert hl.dense_split_ok("dgrad", geom(hl, 2, 1, 16, 64, co, 1)) == want, co
    # the forward only sums over Ci (a narrow Co is fine); the input gradient's tiles need >= 64 output columns, a power of two
    assert hl.dense_split_ok("fprop", geom(hl, 2, 1, 16, 64, 32, 1))
    assert not hl.dense_split_ok("dgrad", geom(hl, 2, 1, 16, 32, 64, 1))
    # the weight gradient sums over pixels: whatever the split weight gradient covers (Co >= 128, whole groups of 16 pixels)
    assert hl.dense_split_ok("wgrad", geom(hl, 3, 1, 8, 64, 128, 1))           # 48 pixels: less than one triple
    assert not hl.dense_split_ok("wgrad", geom(hl, 3, 1, 16, 128, 64, 1))      # Co = 64
    assert not hl.dense_split_ok("wgrad", geom(hl, 1, 1, 4, 64, 128, 1))       # 4 pixels
    # the first layer (3 channels padded to 4) and channel counts that are no power of two have no split form at all
    assert not hl.dense_split_ok("fprop", geom(hl, 2, 4, 16, 4, 64, 4))
    assert not hl.dense_split_ok("fprop", geom(hl, 2, 1, 16, 192, 128, 1))
    lib = hl.load()
    assert lib.mcg_conv_dense_split_ok(None, 0) == 0
    assert lib.mcg_conv_dense_split_ok(ctypes.byref(geom(hl, 2, 1, 16, 64, 128, 1)), 3) == 0
    assert lib.mcg_conv_dense_split_chunk(ctypes.byref(geom(hl, 2, 1, 16, 16, 128, 1)), 0) == 0


def test_tile_codes_around_the_dense_ones(hl):
    """17 / 20 pass the geometry check (the null pointers are then the bad argument, as for every good geometry); there is no 18
    (the 256x256 tile keeps the padded form), nothing between 10 and 17 or above 20; the dense codes belong to split operands"""
    lib = hl.load()

    def status(tile, precision='f32x3'):
        g = geom(hl, 2, 1, 16, 64, 128, 1, tile=tile, precision=precision)
        return (lib.mcg_conv_fprop(ctypes.byref(g), None, None, None, None, None),
                lib.mcg_conv_dgrad(ctypes.byref(g), None, None, None, None, 0, 0, None),
                lib.mcg_conv_wgrad(ctypes.byref(g), None, None, None, None))
    BAD, UNSUPPORTED = -1, -2
    for tile in (11, 12, 16, 18, 19, 21, 30, 99, 1018, 2019):
        assert status(tile) == (BAD, BAD, BAD), tile
    for tile in (17, 20, 1017, 2020):
        for precision in ('f32', 'bf16', 'bf16s'):
            assert status(tile, precision) == (UNSUPPORTED,) * 3, (tile, precision)
    # with split operands the same calls get as far as the pointer check: one real pointer each, and the geometry decides
    buf = ctypes.create_string_buffer(16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for tile in (17, 20):
        g = geom(hl, 2, 1, 16, 16, 128, 1, tile=tile)         # Ci = 16: no whole triple inside a tap
        assert lib.mcg_conv_fprop(ctypes.byref(g), p, p, None, p, None) == UNSUPPORTED
        g = geom(hl, 2, 1, 16, 64, 32, 1, tile=tile)          # Co = 32 in the input gradient
        assert lib.mcg_conv_dgrad(ctypes.byref(g), p, p, None, p, 0, 0, None) == UNSUPPORTED


def test_a_block_covers_whole_triples(hl):
    """fprop / dgrad: the K chunk of a block is a multiple of 256 split elements (a triple of K-steps: four groups of 16 channels x
    4 planes) for every K-split digit, at least 1024 (what the padded form's 16 K-steps of 64 are), and the chunks cover K;
    wgrad: a multiple of 64 pixels, at least 8 triples unless the layer has fewer"""
    for case in BENCH_LAYERS + [(2, 7, 16, 64, 128, 4), (3, 1, 16, 128, 64, 1), (1, 5, 8, 256, 256, 4), (5, 1, 8, 128, 512, 1), (3, 1, 8, 64, 128, 1)]:
        N, Ti, H, Ci, Co, kt = case
        K = {"fprop": kt * 16 * 4 * Ci, "dgrad": kt * 4 * 4 * Co}
        for kind in ("fprop", "dgrad"):
            chunks = []
            for digit in (0, 1000, 2000):
                for code in (17, 20):
                    c = hl.dense_split_chunk(kind, geom(hl, *case, tile=code + digit))
                    assert c > 0 and c % 256 == 0 and c >= min(1024, K[kind]), (case, kind, code + digit, c)
                    want = 1 << (digit // 1000)
                    assert (K[kind] + c - 1) // c <= want, (case, kind, digit, c)
                chunks.append(c)
            assert chunks[0] == K[kind] and chunks[0] >= chunks[1] >= chunks[2], (case, kind, chunks)
        if Co >= 128:
            mpix = N * (Ti - kt + 1) * (H // 2) ** 2
            for code in (17, 20, 1020, 2017):
                c = hl.dense_split_chunk("wgrad", geom(hl, *case, tile=code))
                assert c > 0 and c % 64 == 0, (case, code, c)
                assert c >= min(512, (mpix + 63) // 64 * 64), (case, code, c)


def test_shipped_dense_list_is_well_formed(hl):
    """mocogan-chainer_amd/dense_tiles_mi355x.json: [[key, dense code], ...]; every key is a split-operand (precision 3) entry of
    the shipped tile table, whose own code stays the padded form; every code is a dense one the library admits for that pass and
    geometry (with or without the K-split / pixel-split digit); use_pretuned_table() alone loads the padded table, and with the
    tuner switched on hiplib's table is the shipped one with exactly these entries replaced"""
    import json
    import os
    pkg = os.path.dirname(hl.__file__)
    main = {tuple(k): v for k, v in json.load(open(os.path.join(pkg, 'tuned_tiles_mi355x.json')))}
    dense = json.load(open(os.path.join(pkg, 'dense_tiles_mi355x.json')))
    assert len({tuple(k) for k, _ in dense}) == len(dense)
    for key, code in dense:
        key = tuple(key)
        assert key in main and main[key] % 100 <= 10, key
        kind, N, Ti, Hi, Wi, Ci, Co, kt, perm, prec = key[:10]
        assert kind in ("fprop", "dgrad", "wgrad") and prec == hl.PREC_SPLIT and perm == 0 and Hi == Wi
        assert isinstance(code, int) and code % 100 in (17, 20) and code // 1000 in (0, 1, 2) and (code // 100) % 10 == 0, (key, code)
        g = geom(hl, N, Ti, Hi, Ci, Co, kt, tile=code)
        assert hl.dense_split_ok(kind, g), key
        assert hl.dense_split_chunk(kind, g) % (64 if kind == "wgrad" else 256) == 0
    hl.reset_tuning()
    try:
        hl.use_pretuned_table()                        # the table alone: the padded reference
        assert hl.tile_choices() == main
        hl.reset_tuning()
        hl.set_autotune(True)                          # what bench.py and train.py do
        got = hl.tile_choices()
        for key, code in main.items():
            assert got[key] == dict((tuple(k), v) for k, v in dense).get(key, code), key
    finally:
        hl.reset_tuning()
