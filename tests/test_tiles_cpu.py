"""mocogan-chainer_amd/tiles.py -- the candidate rules, the tile table, the shipped lists laid over it, the timing loop and the
'f32x3' split decision -- checked on the CPU without the built library: tiles imports neither torch nor ctypes, and the
measurement is a callable, so the tests script the times."""
import ctypes
import json
import os
import subprocess
import sys
import warnings

import pytest

from mocogan_chainer_amd import tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'mocogan-chainer_amd')


class Geom(ctypes.Structure):
    """the integer fields of mcg_conv_geom that tiles reads (a duck-typed stand-in for hiplib.ConvGeom)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("N", "Ti", "Hi", "Wi", "Ci", "To", "Ho", "Wo", "Co", "kt", "x_perm_n", "precision", "tile")] \
        + [("x_stride0", ctypes.c_int64)]


def geom(key, tile=0):
    """the geometry of a table key [pass, N, Ti, Hi, Wi, Ci, Co, kt, x_perm_n, precision, ...], derived as hiplib.make_geom does"""
    N, Ti, Hi, Wi, Ci, Co, kt, perm, prec = key[1:10]
    return Geom(N, Ti, Hi, Wi, Ci, Ti - kt + 1, Hi // 2, Wi // 2, Co, kt, perm, prec, tile, Ti * Hi * Wi * Ci)


def shipped(name):
    return {tuple(k): v for k, v in json.load(open(os.path.join(PKG, name)))}


def dump(path, entries):
    json.dump([[list(k), v] for k, v in entries.items()], open(str(path), 'w'))
    return str(path)


# ------------------------------------------------------------------------------------------------------------
# 1. candidate lists, pinned to what the tuner's chain gave before it became tiles.candidates
# ------------------------------------------------------------------------------------------------------------
def test_candidates_are_the_recorded_ones():
    """tests/golden/tile_candidates.json: [[key, [codes...]], ...] for every distinct (pass, geometry) of the three shipped lists and
    one synthetic geometry on each side of every branch they do not reach, recorded from the tuner's chain before it
    became tiles.candidates.  Same codes in the same order: the loop keeps the first of equal timings."""
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'tile_candidates.json')))
    keys = {tuple(k) for k, _ in golden}
    assert len(keys) == len(golden) >= 300
    for name in ('tuned_tiles_mi355x.json', 'dense_tiles_mi355x.json', 'live_tiles_mi355x.json'):
        for k in shipped(name):
            assert str(k[0]).startswith('split-') or k[:10] in keys, k
    for key, codes in golden:
        assert tiles.candidates(key[0], geom(key)) == tuple(codes), key
    assert tiles.geom_key('wgrad', geom(golden[0][0]), ('ep', 1)) == ('wgrad',) + tuple(golden[0][0][1:]) + ('ep', 1)


# ------------------------------------------------------------------------------------------------------------
# 2. the shipped lists and the overlay rule
# ------------------------------------------------------------------------------------------------------------
def test_shipped_lists_lay_over_one_another():
    main, dense, live = shipped('tuned_tiles_mi355x.json'), shipped('dense_tiles_mi355x.json'), shipped('live_tiles_mi355x.json')
    assert (len(main), len(dense), len(live)) == (443, 45, 6)
    t = tiles.TileTable()
    t.use_pretuned()                                   # the sampling path: the table alone
    assert t.as_dict() == main and not t.autotune_on()
    t.reset()
    t.set_autotune(True)                               # bench.py, train.py: exactly the dense entries replaced
    assert t.autotune_on() and t.as_dict() == {k: dense.get(k, c) for k, c in main.items()}
    assert tiles.live_list(t.live) == live
    assert t.use_live() == len(live)                   # a training step on top: exactly the live entries moved
    assert t.as_dict() == {k: live.get(k, dense.get(k, c)) for k, c in main.items()}
    assert t.use_live() == 0
    t.reset()
    assert t.as_dict() == {} and not t.autotune_on()


K = [('fprop', 8, 1, 16, 16, 64, 128, 1, 0, 3), ('dgrad', 8, 1, 16, 16, 64, 128, 1, 0, 3, 0, 0), ('wgrad', 64, 1, 16, 16, 64, 128, 1, 0, 3),
     ('fprop', 8, 1, 32, 32, 64, 128, 1, 0, 3), ('split-fprop', 8, 1, 16, 16, 64, 128, 1, 0, 0), ('split-wgrad', 8, 1, 16, 16, 64, 128, 1, 0, 0)]


@pytest.fixture
def small(tmp_path):
    """a table over three hand-made lists: main holds K[0..5]; dense moves K[0], K[1]; live moves K[0] (from its dense code),
    K[2] and K[3] (from their main codes); dense and live each name one launch that main does not hold"""
    main = {K[0]: 7, K[1]: 8, K[2]: 7, K[3]: 10, K[4]: 1, K[5]: 0}
    stranger = ('fprop', 9, 1, 16, 16, 64, 128, 1, 0, 3)
    dense = {K[0]: 17, K[1]: 1020, stranger: 17}
    live = {K[0]: 27, K[2]: 28, K[3]: 2040, stranger: 40}
    t = tiles.TileTable(main=dump(tmp_path / 'main.json', main), dense=dump(tmp_path / 'dense.json', dense),
                        live=dump(tmp_path / 'live.json', live))
    return t, main, dense, live, stranger


def test_overlay_moves_a_launch_only_from_an_earlier_layer_s_code(small, tmp_path):
    t, main, dense, live, stranger = small
    t.set_autotune(True)
    assert t.as_dict() == {**main, K[0]: 17, K[1]: 1020}                 # a key the main list lacks is not added
    assert t.use_live() == 3 and t.as_dict() == {**main, K[0]: 27, K[1]: 1020, K[2]: 28, K[3]: 2040}
    assert stranger not in t.as_dict()
    # an entry tuned to something else in this process stays, in either layer
    t.reset()
    t.set(K[0], 10)
    t.set(K[2], 8)
    t.set_autotune(True)
    assert t.get(K[0]) == 10 and t.get(K[1]) == 1020
    assert t.use_live() == 1 and t.as_dict() == {**main, K[0]: 10, K[1]: 1020, K[2]: 8, K[3]: 2040}
    # the live list over the main table alone (no dense layer applied) moves the launch from its main code too
    t.reset()
    t.use_pretuned()
    assert t.use_live() == 3 and t.get(K[0]) == 27
    # a list given by path takes the place of the live list; what is not a live-steps entry is an error
    t.reset()
    t.use_pretuned()
    assert t.use_live(dump(tmp_path / 'other.json', {K[3]: 1027})) == 1 and t.as_dict() == {**main, K[3]: 1027}
    for bad in ({K[0]: 17}, {K[1]: 27}, {K[2]: 40}, {K[0][:9] + (2,): 27}):
        with pytest.raises(ValueError):
            tiles.live_list(dump(tmp_path / 'bad.json', bad))
    # load / save / replace / merge
    t.save(str(tmp_path / 'saved.json'))
    u = tiles.TileTable(main=t.main, dense=t.dense, live=t.live)
    u.set(K[3], 7)
    u.merge([[list(K[3]), 8], [list(stranger), 9]], overwrite=False)
    assert u.as_dict() == {K[3]: 7, stranger: 9}
    u.load(str(tmp_path / 'saved.json'))
    assert u.as_dict() == {**t.as_dict(), stranger: 9}
    u.replace([[list(K[1]), 203]])
    assert u.as_dict() == {K[1]: 203} and u.tile('dgrad', geom(K[1]), (0, 0)) == 203 and u.tile('dgrad', geom(K[1])) == 0


def test_a_key_listed_twice(tmp_path):
    """the table takes the first entry of the main list (it never replaces a choice it holds); an overlay goes by the last"""
    path = str(tmp_path / 'main.json')
    json.dump([[list(K[0]), 7], [list(K[0]), 8]], open(path, 'w'))
    t = tiles.TileTable(main=path, dense=dump(tmp_path / 'dense.json', {K[0]: 17}), live=str(tmp_path / 'none.json'))
    t.use_pretuned()
    assert t.as_dict() == {K[0]: 7} and tiles.read_list(path) == {K[0]: 8}
    assert t.use_dense() == 0 and t.get(K[0]) == 7
    t.set(K[0], 8)
    assert t.use_dense() == 1 and t.get(K[0]) == 17


def test_each_switch_turns_its_layer_off(small, monkeypatch):
    t, main, dense, live, _ = small
    monkeypatch.setenv('MCG_DENSE_SPLIT', '0')
    t.set_autotune(True)
    assert t.as_dict() == main
    assert t.use_live() == 3 and t.get(K[0]) == 27                      # (the live list still moves it, from its main code)
    monkeypatch.delenv('MCG_DENSE_SPLIT')
    monkeypatch.setenv('MCG_LIVE_STEPS', '0')                           # read at the call, not at import
    t.reset()
    t.set_autotune(True)
    assert t.use_live() == 0 and t.as_dict() == {**main, K[0]: 17, K[1]: 1020}
    monkeypatch.delenv('MCG_LIVE_STEPS')
    monkeypatch.setenv('MCG_NO_PRETUNED', '1')
    t.reset()
    t.set_autotune(True)
    assert t.autotune_on() and t.as_dict() == {} and t.use_live() == 0
    monkeypatch.delenv('MCG_NO_PRETUNED')
    # tuner off: the split / fp32 decisions are loaded, and only those
    t.reset()
    t.set_autotune(False)
    assert not t.autotune_on() and t.as_dict() == {K[4]: 1, K[5]: 0}
    t.reset()
    t.set_autotune(True, use_pretuned=False)
    assert t.autotune_on() and t.as_dict() == {}


# ------------------------------------------------------------------------------------------------------------
# 3. the tuning loop and the split decision with scripted times
# ------------------------------------------------------------------------------------------------------------
class Script:
    """measure(geom) -> the scripted ms of geom.tile (None: the candidate is impossible), recording what was asked"""

    def __init__(self, ms, default=9.0):
        self.ms, self.default, self.asked = ms, default, []

    def __call__(self, g):
        self.asked.append(g.tile)
        return self.ms.get(g.tile, self.default)


def test_tuning_loop_keeps_the_first_best_possible_candidate():
    key = ('fprop', 4, 1, 16, 16, 64, 128, 1, 0, 0)
    cands = tiles.candidates('fprop', geom(key))
    assert cands.index(102) < cands.index(202) < cands.index(10)
    t = tiles.TileTable()
    t.set_autotune(True, use_pretuned=False)
    g = geom(key)
    m = Script({101: None, 102: 2.0, 202: 2.0, 10: None, 0: 3.0})     # two equal best times; the impossible ones are skipped
    got = t.tuned('fprop', g, ('ep', 1), m)
    assert got.tile == 102 and got is not g and g.tile == 0 and tuple(m.asked) == cands
    assert t.as_dict() == {tiles.geom_key('fprop', g, ('ep', 1)): 102}
    assert (got.N, got.Ci, got.Co, got.x_stride0) == (g.N, g.Ci, g.Co, g.x_stride0)
    again = Script({})
    assert t.tuned('fprop', g, ('ep', 1), again).tile == 102 and again.asked == [] and g.tile == 0     # a hit: nothing is measured
    assert t.tuned('fprop', g, (), Script({201: 1.0})).tile == 201                                      # another launch form: its own entry
    # all impossible: code 0, the caller's geometry itself comes back, and that too is remembered
    h = geom(('dgrad',) + key[1:])
    none = Script({}, default=None)
    assert t.tuned('dgrad', h, (0, 0), none) is h and h.tile == 0 and len(none.asked) == len(tiles.candidates('dgrad', h))
    assert t.get(tiles.geom_key('dgrad', h, (0, 0))) == 0
    assert t.tuned('dgrad', h, (0, 0), again) is h and again.asked == []
    # a geometry that names its tile is never tuned, nor is anything while the tuner is off
    fixed = geom(key, tile=203)
    assert t.tuned('wgrad', fixed, (), again) is fixed and again.asked == []
    t.set_autotune(False, use_pretuned=False)
    w = geom(('wgrad',) + key[1:])
    assert t.tuned('wgrad', w, (), again) is w and again.asked == [] and tiles.geom_key('wgrad', w) not in t.as_dict()
    # the tile override fills in where the geometry names none
    t.set_override(7)
    assert t.with_override(w).tile == 7 and w.tile == 0 and t.with_override(fixed) is fixed
    t.set_override(0)
    assert t.with_override(w) is w


def test_split_pays_below_97_percent_of_the_plain_time(monkeypatch):
    monkeypatch.delenv('MCG_SPLIT', raising=False)
    g = geom(('fprop', 8, 1, 16, 16, 64, 128, 1, 0, 0))
    assert tiles.split_covers('fprop', g)
    calls = []

    def best_ms(run):
        calls.append(run)
        return run()
    for ratio, want in ((0.969, True), (0.971, False)):
        t = tiles.TileTable()
        t.set_autotune(True, use_pretuned=False)
        assert not t.split_decided('fprop', g)
        assert t.split_pays('fprop', g, lambda: 10.0, lambda: 10.0 * ratio, best_ms) is want
        assert t.as_dict() == {('split-fprop', 8, 1, 16, 16, 64, 128, 1, 0, 0): int(want)}
        assert t.split_decided('fprop', g) is want
        n = len(calls)
        assert t.split_pays('fprop', g, None, None, None) is want and len(calls) == n        # decided: nothing is timed again
    # MCG_SPLIT=always / never: neither the table nor the measurement is consulted
    t = tiles.TileTable()
    t.set(tiles.geom_key('split-fprop', g), 0)
    monkeypatch.setenv('MCG_SPLIT', 'always')
    assert t.split_pays('fprop', g, None, None, None) is True and t.split_decided('fprop', g)
    t.set(tiles.geom_key('split-fprop', g), 1)
    monkeypatch.setenv('MCG_SPLIT', 'never')
    assert t.split_pays('fprop', g, None, None, None) is False and not t.split_decided('fprop', g)
    narrow = geom(('dgrad', 4, 5, 16, 16, 16, 32, 4, 0, 0))
    monkeypatch.setenv('MCG_SPLIT', 'always')
    assert not tiles.split_covers('dgrad', narrow) and not t.split_decided('dgrad', narrow)


def test_split_pays_warns_once_when_the_tuner_is_off(monkeypatch):
    monkeypatch.delenv('MCG_SPLIT', raising=False)
    t = tiles.TileTable()
    g, h = geom(('fprop', 8, 1, 16, 16, 64, 128, 1, 0, 0)), geom(('wgrad', 64, 1, 16, 16, 64, 128, 1, 0, 0))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        assert t.split_pays('fprop', g, None, None, None) is False
        assert t.split_pays('wgrad', h, None, None, None) is False
    assert len(seen) == 1 and "tile tuner is off" in str(seen[0].message)
    assert t.as_dict() == {}
    t.set(tiles.geom_key('split-wgrad', h), 1)                           # a loaded decision holds with the tuner off
    assert t.split_pays('wgrad', h, None, None, None) is True


# ------------------------------------------------------------------------------------------------------------
# 4. tiles stays importable where neither torch nor the library can be
# ------------------------------------------------------------------------------------------------------------
def test_import_pulls_in_neither_torch_nor_ctypes():
    """in a fresh process: what importing mocogan_chainer_amd.tiles adds to sys.modules holds no torch and no ctypes, and the
    library is not loaded (hiplib is not imported at all)"""
    code = ("import sys; sys.path.insert(0, %r); before = set(sys.modules); import mocogan_chainer_amd.tiles as t; "
            "added = set(sys.modules) - before; bad = sorted(m for m in added if m.split('.')[0] in ('torch', 'ctypes', '_ctypes')); "
            "assert not bad, bad; assert 'mocogan_chainer_amd.hiplib' not in sys.modules; assert 'mocogan_chainer_amd.tiles' in added; "
            "assert t.table.as_dict() == {}; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, '-S', '-c', code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr
