"""Host side of the position-major forward codes (27 / 40, 37, + 1000 / + 2000), checked without a GPU: which tile codes the
library takes and for which pass, and that the list of launches that run them (mocogan-chainer_amd/live_tiles_mi355x.json, when
the package ships one) and its loader agree with the shipped tile table.  Nothing is launched: the conv entry points validate
geometry and tile code before they look at their pointers."""
import ctypes
import json
import os

import pytest


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def _tables(hl):
    pkg = os.path.dirname(hl.__file__)
    main = {tuple(k): v for k, v in json.load(open(os.path.join(pkg, 'tuned_tiles_mi355x.json')))}
    dense = {tuple(k): v for k, v in json.load(open(os.path.join(pkg, 'dense_tiles_mi355x.json')))}
    return main, dense


def test_position_major_codes_belong_to_the_split_forward(hl):
    lib = hl.load()
    BAD_PTR, BAD, UNSUPPORTED = -1, -1, -2

    def status(tile, precision='f32x3', ci=64):
        g = hl.make_geom(2, 1, 16, 16, ci, 128, 1, precision=precision)
        g.tile = tile
        return (lib.mcg_conv_fprop(ctypes.byref(g), None, None, None, None, None),
                lib.mcg_conv_dgrad(ctypes.byref(g), None, None, None, None, 0, 0, None),
                lib.mcg_conv_wgrad(ctypes.byref(g), None, None, None, None))
    for tile in hl.LIVE_CANDIDATES + hl.LIVE_WGRAD_CANDIDATES + (37,):
        assert status(tile) == (BAD_PTR,) * 3, tile                 # a good geometry: the null pointers are the bad argument
        for precision in ('f32', 'bf16', 'bf16s'):
            assert status(tile, precision) == (UNSUPPORTED,) * 3, (tile, precision)
    for tile in (29, 38, 39, 41, 47, 3027):
        assert status(tile) == (BAD,) * 3, tile
    buf = ctypes.create_string_buffer(16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for tile in hl.LIVE_CANDIDATES + (37,):
        g = hl.make_geom(2, 1, 16, 16, 64, 128, 1, precision='f32x3')
        g.tile = tile                                               # the other passes have no position-major form
        assert lib.mcg_conv_dgrad(ctypes.byref(g), p, p, None, p, 0, 0, None) == UNSUPPORTED
        assert lib.mcg_conv_wgrad(ctypes.byref(g), p, p, p, None) == UNSUPPORTED       # (N To = 2: no whole K advance per position)
        g = hl.make_geom(2, 1, 16, 16, 16, 128, 1, precision='f32x3')
        g.tile = tile                                               # Ci = 16: no whole triple of K-steps inside a tap
        assert lib.mcg_conv_fprop(ctypes.byref(g), p, p, None, p, None) == UNSUPPORTED


def test_weight_gradient_codes_need_whole_advances_per_position(hl):
    """27 / 28 in the weight gradient: refused (before anything is launched) unless N To is a multiple of the K advance in pixels
    -- 64 for the dense 128x256 tile (27), 16 for the padded 256x256 one (28), which also needs Co >= 256; 28 is no code of the
    forward or the input gradient; 40 and 37 are the forward's alone"""
    lib = hl.load()
    UNSUPPORTED = -2
    buf = ctypes.create_string_buffer(16)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def wgrad(N, Ti, Co, kt, tile):
        g = hl.make_geom(N, Ti, 8, 8, 64, Co, kt, precision='f32x3')
        g.tile = tile
        return g
    for N, Ti, Co, kt, tile in ((3, 7, 128, 4, 27), (24, 1, 128, 1, 27), (32, 1, 128, 1, 27), (5, 1, 256, 1, 28), (8, 4, 256, 4, 1028),
                                (16, 1, 128, 1, 28), (64, 1, 256, 1, 40), (64, 1, 256, 1, 37)):
        assert lib.mcg_conv_wgrad(ctypes.byref(wgrad(N, Ti, Co, kt, tile)), p, p, p, None) == UNSUPPORTED, (N, Ti, Co, kt, tile)
    g = wgrad(64, 1, 256, 1, 28)
    assert lib.mcg_conv_fprop(ctypes.byref(g), p, p, None, p, None) == UNSUPPORTED
    assert lib.mcg_conv_dgrad(ctypes.byref(g), p, p, None, p, 0, 0, None) == UNSUPPORTED
    assert lib.mcg_conv_wgrad(ctypes.byref(g), None, None, None, None) == -1       # a good geometry: the null pointers are the bad argument


def test_the_list_loader_takes_the_codes_and_only_known_launches(hl, tmp_path):
    """every position-major code on a shipped split forward launch is taken; a key the table does not hold, another pass or another
    code is not; the list moves a launch only from its shipped or dense code; MCG_LIVE_STEPS=0 switches it off"""
    main, dense = _tables(hl)
    keys = [k for k in main if k[0] == 'fprop' and k[9] == hl.PREC_SPLIT and len(k) == 10]
    assert len(keys) >= len(hl.LIVE_CANDIDATES)
    entries = [[list(k), c] for k, c in zip(keys, hl.LIVE_CANDIDATES)]
    path = str(tmp_path / 'live.json')
    json.dump(entries, open(path, 'w'))
    assert hl.live_list(path) == {tuple(k): c for k, c in entries}
    hl.reset_tuning()
    try:
        hl.use_pretuned_table()
        hl.use_dense_list()
        before = hl.tile_choices()
        assert hl.use_live_list(path) == len(entries)
        got = hl.tile_choices()
        for k in main:
            assert got[k] == dict((tuple(a), b) for a, b in entries).get(k, before[k]), k
        # a launch tuned to something else in this process stays
        hl.reset_tuning()
        hl.use_pretuned_table()
        hl.load_tile_choices(_other(tmp_path, keys[0], 8))
        assert hl.use_live_list(path) == len(entries) - 1 and hl.tile_choices()[keys[0]] == 8
        os.environ['MCG_LIVE_STEPS'] = '0'
        hl.reset_tuning()
        hl.use_pretuned_table()
        assert hl.use_live_list(path) == 0 and hl.tile_choices() == main
    finally:
        os.environ.pop('MCG_LIVE_STEPS', None)
        hl.reset_tuning()
    unknown = list(keys[0])
    unknown[1] = 7777
    json.dump([[unknown, 27]], open(path, 'w'))
    hl.use_pretuned_table()
    try:
        assert hl.use_live_list(path) == 0                          # not a launch of the shipped table: ignored
    finally:
        hl.reset_tuning()
    for bad in ([list(keys[0]), 17], [['dgrad'] + list(keys[0][1:]), 27], [list(keys[0][:9]) + [hl.PRECISIONS['bf16s']], 27],
                [['wgrad'] + list(keys[0][1:]), 40], [list(keys[0]), 28]):
        json.dump([bad], open(path, 'w'))
        with pytest.raises(ValueError):
            hl.live_list(path)


def _other(tmp_path, key, code):
    path = str(tmp_path / 'other.json')
    json.dump([[list(key), code]], open(path, 'w'))
    return path


def test_shipped_list_is_well_formed(hl):
    """live_tiles_mi355x.json, where the package ships one: every key is a split forward launch of the shipped table, every code a
    position-major one.  set_autotune(True) leaves the table the shipped one with the dense list's entries; use_live_list(), which
    a training step built with the tuner on calls, then replaces exactly the list's entries, and a second call changes nothing"""
    main, dense = _tables(hl)
    live = hl.live_list()
    for key in live:
        assert key in main, key
    hl.reset_tuning()
    try:
        hl.set_autotune(True)
        assert hl.tile_choices() == {k: dense.get(k, c) for k, c in main.items()}
        assert hl.use_live_list() == len(live)
        got = hl.tile_choices()
        for key, code in main.items():
            assert got[key] == live.get(key, dense.get(key, code)), key
        assert hl.use_live_list() == 0 and hl.tile_choices() == got
    finally:
        hl.reset_tuning()
