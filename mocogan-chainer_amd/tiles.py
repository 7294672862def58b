"""Which GEMM block tile (mcg_conv_geom.tile) a conv launch takes: the candidate rules, the per-process table of choices, the
shipped lists laid over it, the timing loop and the 'f32x3' decision whether a launch takes the split form.

Pure host logic: no torch, no ctypes, no library.  A geometry is any object with mcg_conv_geom's integer fields (copied with
type(g).from_buffer_copy), and a measurement is a callable the caller hands in -- hiplib times launches with HIP events, the CPU
tests script the times.  hiplib imports this module, never the other way round.
"""
import json
import os
import warnings

PREC_F32, PREC_BF16, PREC_BF16_STORE, PREC_SPLIT, PREC_BF16_Y16 = 0, 1, 2, 3, 4
# 'bf16': bf16 MFMA on fp32 tensors (rounded in the kernel); 'bf16s': bf16 MFMA on operands that are bf16 in memory;
# 'f32x3': fp32 values as three bf16 terms (split_planes), six bf16 products per fp32 product -- fp32 results on the bf16 pipe
# 'bf16y': as 'bf16' with the y-side tensor bf16 in memory (x, w fp32): the clip-side layers of bf16 networks (wgrad, dgrad)

# ------------------------------------------------------------------------------------------
# per-geometry choice of the GEMM block tile (mcg_conv_geom.tile).  The best of the six candidates
# depends on how the tile count of a launch divides over the 256 CUs and, for dgrad, on how many blocks
# skip dead temporal taps -- the library's closed-form heuristic misses by up to 20 % on some layers.
# With autotune on, the first launch of each (pass, geometry) times every candidate once on scratch
# tensors and the winner is used from then on.  Off by default (tests, parity runs): bench.py, train.py
# and generate_samples.py switch it on.
# ------------------------------------------------------------------------------------------
TILE_CANDIDATES = (0, 101, 102, 103, 201, 202, 203)     # (the long tiles 4 = 256x64 and 5 = 64x256 exist, but when they
                                                        # win the isolated timing they lose inside the iteration: measured)
FPROP_SPLIT_CANDIDATES = (1103, 1203, 1202, 2103, 2203, 2202)     # 2- / 4-way split-K: only when few tiles (see candidates)
WGRAD_SPLIT_CANDIDATES = (2007, 2008, 2010, 1010)      # LDS-DMA weight gradient with half / twice the pixel splits (few-tile layers)
V2_CANDIDATES = (7, 8, 10)                              # gemm_bf16_v2_kernel (bf16-stored / split / fp32 operands): 256x128 / 256x256 (wgrad 128x256 / 256x256) one block per CU; 10 = 128x128, two blocks per CU
DENSE_CANDIDATES = (17, 20)                             # MCG_PREC_SPLIT only: tiles 7 / 10 with the dense LDS form (no padding-plane slots; the library
                                                        # refuses it where a triple of K-steps would straddle a tap: channels along the sum not a multiple of 64)
LIVE_CANDIDATES = (27, 40, 1027, 2027, 1040, 2040)       # MCG_PREC_SPLIT forward only: 17 / 20 with position-major rows -- K-steps of filter taps that read zero padding for every row
                                                        # of a tile are skipped; + 1000 / + 2000: the tiles cut into blocks of equal LIVE work, one / two per resident slot (no epilogue)
LIVE_WGRAD_CANDIDATES = (27, 28, 1027, 2027, 1028, 2028)     # MCG_PREC_SPLIT weight gradient: 128x256/3 dense / 256x256/2 padded with a position-major pixel axis -- advances whose position
                                                        # reads only padding for the column tile's taps are skipped; needs N * To a multiple of 64 / 16 (the library refuses otherwise)


def candidates(kind, g):
    """the tile codes the tuner times for a launch of this pass and geometry, in the order it times them (the first of equal
    timings wins).  The shipped lists also hold a few codes placed by the A/B tools that are not in here."""
    cands = TILE_CANDIDATES
    if (kind == "dgrad" and 4 < g.Ci <= 64) or (kind == "fprop" and g.Co <= 64 and g.Ci > 4):
        cands = cands + (4,)                                # 256 x 64: the widest tile a 64-column output admits
    if kind == "wgrad" and g.Ci == 4:
        cands = cands + (6,)                                # patch-in-LDS kernel (also what tile 0 selects when it applies)
    out_elems = g.N * g.To * g.Ho * g.Wo * g.Co if kind == "fprop" else g.N * g.Ti * g.Hi * g.Wi * g.Ci
    if kind in ("fprop", "dgrad") and g.Ci > 4 and out_elems <= (1 << (23 if kind == "fprop" else 25)):
        cands = cands + FPROP_SPLIT_CANDIDATES          # <= 1024 tiles of 64x64: K splits can fill the CUs
    if g.precision == PREC_BF16_STORE and g.Ci >= 64 and g.Co >= 64:
        # the LDS-DMA kernels (the library refuses what they do not cover).  fp32 networks can run them too (tile codes
        # 7 / 8 by request), but measured on the MI355X they do not beat the register-staged fp32 kernels: 110-127
        # against 128-134 TFLOP/s on the big layers, and one 256-row block per CU quantises badly at batch 32
        if not (kind == "dgrad" and g.Ci == 64):        # (64 output columns per parity class: the 256x64 tile never wins)
            cands = cands + V2_CANDIDATES
            if kind == "wgrad" and g.Co * g.kt * 16 * g.Ci <= (1 << 21):
                cands = cands + WGRAD_SPLIT_CANDIDATES
        else:
            cands = cands + (10,)                       # ... but 256x64 with two buffers lets two blocks share a CU
            if g.Ho == 16 and g.Wo == 16:
                cands = cands + (9,)                    # ... and the patch-stationary kernel, four classes per block, is made for it
    if g.precision == PREC_F32 and g.Ci >= 64 and g.Co >= 64 and kind != "dgrad" or (g.precision == PREC_F32 and kind == "dgrad" and g.Ci >= 128 and g.Co >= 64):
        cands = cands + (10,)                           # the LDS-DMA kernel on fp32 operands, 128x128, two blocks per CU
    if g.precision == PREC_SPLIT:
        # (the LDS-DMA kernels are the only ones that multiply split operands; one 256-row block per CU: late layers need K splits)
        cands = V2_CANDIDATES + DENSE_CANDIDATES
        if kind in ("fprop", "dgrad") and out_elems <= (1 << 25):
            cands = cands + (1007, 2007, 1010, 2010, 1017, 2017, 1020, 2020)
        if kind == "fprop":
            cands = cands + LIVE_CANDIDATES
        if kind == "wgrad":
            cands = cands + LIVE_WGRAD_CANDIDATES
        if kind == "wgrad" and g.Co * g.kt * 16 * g.Ci <= (1 << 21):
            # few (Co, tap x Ci) tiles -- the 2-D layers: many pixel splits then add onto the same small dw with float
            # atomics; + 2000 halves / + 1000 doubles the number of splits (round 6)
            cands = cands + WGRAD_SPLIT_CANDIDATES + (2017, 2020, 1020)
        if kind == "dgrad" and g.Ci == 64 and g.Ho == 16 and g.Wo == 16:
            cands = cands + (9,)                        # the patch-stationary kernel (four parity classes per block)
    return cands


def geom_key(kind, g, extra=()):
    return (kind, g.N, g.Ti, g.Hi, g.Wi, g.Ci, g.Co, g.kt, g.x_perm_n, g.precision) + tuple(extra)


def ep_key(g, ep, out_bf16):
    """bf16 networks tune a geometry per launch FORM: a fused epilogue / a bf16 output change which tile wins (the LDS-DMA
    kernels' row-wise epilogue costs differently from the register-staged kernels'), so the form is part of the key and the
    candidates are timed in it.  fp32 geometries keep their single key (and the shipped table)."""
    if g.precision != PREC_BF16_STORE:
        return ()
    return ('ep', int(ep.sums) if ep is not None else 0, int(bool(ep.mask_in)) if ep is not None else 0, int(out_bf16))


def split_covers(kind, g):
    """does the MCG_PREC_SPLIT form of this pass exist for the geometry (the library's own condition, restated for callers)?
    kind 'fprop': the sum runs over Ci; 'dgrad': over Co, and the LDS-DMA input-gradient tiles need >= 64 output columns;
    'wgrad': the sum runs over pixels, x and y both in the split layout."""
    def p2(c, lo):
        return c >= lo and c & (c - 1) == 0
    x_el = max((g.N - 1) * g.x_stride0, 0) + g.Ti * g.Hi * g.Wi * g.Ci if not g.x_perm_n else None
    y_el = g.N * g.To * g.Ho * g.Wo * g.Co
    w_el = g.Co * g.kt * 16 * g.Ci
    if w_el * 8 >= 1 << 31:
        return False
    if kind == 'fprop':
        return p2(g.Ci, 16) and x_el is not None and x_el * 8 < 1 << 31
    if kind == 'wgrad':                                             # both operands split; the LDS-DMA weight-gradient tiles' own limits
        return (g.Co >= 128 and g.Co % 64 == 0 and p2(g.Ci, 64) and x_el is not None and x_el * 8 < 1 << 31 and y_el * 8 < 1 << 31
                and (y_el // g.Co) % 16 == 0)
    return p2(g.Co, 16) and p2(g.Ci, 64) and y_el * 8 < 1 << 31


def with_tile(g, code):
    """a copy of the geometry with its tile code set (the caller's geometry is never modified)"""
    gg = type(g).from_buffer_copy(g)
    gg.tile = code
    return gg


def read_entries(path):
    """[(key, code), ...] of a list in save()'s form ([[key, tile code], ...]), in file order; [] when the file does not exist"""
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [(tuple(k), int(v)) for k, v in json.load(f)]


def read_list(path):
    """{key: code} of such a list (of a key listed twice, the last entry)"""
    return dict(read_entries(path))


def live_list(path):
    """{key: code} of a live-steps list, checked: forward / weight-gradient launches of the split form, codes of LIVE_CANDIDATES / LIVE_WGRAD_CANDIDATES"""
    entries = read_list(path)
    for k, v in entries.items():
        if k[9] != PREC_SPLIT or not ((k[0] == 'fprop' and v in LIVE_CANDIDATES) or (k[0] == 'wgrad' and v in LIVE_WGRAD_CANDIDATES)):
            raise ValueError("not a live-steps entry: %r -> %r" % (k, v))
    return entries


_HERE = os.path.dirname(os.path.abspath(__file__))


class TileTable:
    """{(pass, geometry...): tile code} of one process, with the tuner's switch, the tests' tile override and the three shipped
    lists.  One instance (`table` below): the library has no process-global state, so this lives here, in the caller.

    main:  the choices the tuner made on an MI355X for the reference's layer geometries at batch 32 per GPU, refined in the step.
    dense: the 'f32x3' launches of `main` which take the DENSE LDS form instead (tile codes 17 / 20 in place of the table's padded
           7 / 8 / 9 / 10), each measured faster than its padded entry by more than the padded form's own spread (tools/
           ab_dense_split.py, profiles/dense_split_notes.md).  A list of its own, applied by set_autotune(True): `main` and
           use_pretuned() stay the padded reference that the production-batch parity test pins against float64.
    live:  the forward / weight-gradient launches among them which take position-major rows and live K-steps, measured the same
           way (tools/ab_live_steps.py, profiles/live_steps_notes.md); applied on top of the dense list where a training step is
           built with the tuner on (step.TrainStep -> use_live): set_autotune()'s table stays `main` with the dense entries."""

    def __init__(self, main=os.path.join(_HERE, 'tuned_tiles_mi355x.json'), dense=os.path.join(_HERE, 'dense_tiles_mi355x.json'),
                 live=os.path.join(_HERE, 'live_tiles_mi355x.json')):
        self.main, self.dense, self.live = main, dense, live
        self.choices = {}
        self.autotune = False
        self.override = 0
        self.warned_undecided_split = False

    def reset(self):
        """Back to the state of a fresh import: tuner off, no cached tile choices, no tile override.  (tests/conftest.py calls this
        before every test module so that no module inherits a timing-dependent tile table from an earlier one; train.main() and
        bench.py switch the tuner on for their own process.)"""
        self.autotune = False
        self.override = 0
        self.choices.clear()

    def set_autotune(self, on, use_pretuned=True):
        """on: time the tile candidates at the first launch of every (pass, geometry) not known yet.  use_pretuned: start
        from the table shipped with the package (`main`); anything else is still tuned on first use."""
        self.autotune = bool(on)
        if use_pretuned:
            # tuner off (train.py --autotune 0): the tile heuristic replaces the table's tile codes, but WHICH FORM a launch of an
            # 'f32x3' network takes (split on the bf16 pipe / fp32 MFMA) has no heuristic -- those entries are loaded either way,
            # otherwise such a network would silently run every GEMM on the fp32 kernels (round 4's advice)
            self.use_pretuned(only_split=not on)
            if on:
                self.use_dense()

    def autotune_on(self):
        return self.autotune

    def set_override(self, t):
        """Tests / tuning tools: a default for mcg_conv_geom.tile of every conv call that does not set one itself (0 = none)."""
        self.override = int(t)

    def with_override(self, g):
        return g if not self.override or g.tile else with_tile(g, self.override)

    def get(self, key, default=None):
        return self.choices.get(key, default)

    def set(self, key, code):
        self.choices[tuple(key)] = int(code)

    def tile(self, kind, g, extra=()):
        """the tile code the table holds for (pass, geometry, launch form) -- 0 when it holds none.  Never tunes."""
        return self.choices.get(geom_key(kind, g, extra), 0)

    def as_dict(self):
        """{(pass, geometry...): tile code} chosen so far (for logs / DESIGN.md tables)."""
        return dict(self.choices)

    def merge(self, entries, overwrite, only_split=False):
        """[[key, tile code], ...] (save()'s form) into the table; overwrite: an entry replaces the one the table holds"""
        for k, v in entries:
            if overwrite:
                self.choices[tuple(k)] = int(v)
            elif not only_split or str(k[0]).startswith('split-'):
                self.choices.setdefault(tuple(k), int(v))

    def save(self, path):
        """Persist the tuned choices (JSON) so that a later process -- or a profiler pass that must not see the
        tuning launches -- can start from them."""
        with open(path, 'w') as f:
            json.dump([[list(k), v] for k, v in self.choices.items()], f)

    def load(self, path):
        with open(path) as f:
            self.merge(json.load(f), overwrite=True)

    def replace(self, entries):
        """the table becomes exactly `entries` ([[key, tile code], ...]): every data-parallel rank takes rank 0's choices"""
        self.choices.clear()
        self.merge(entries, overwrite=True)

    def use_pretuned(self, only_split=False):
        """Load `main` WITHOUT switching the tuner on: what the sampling path reads (conv_dgrad_relu's tile codes, the split /
        fp32 decisions of 'f32x3'); launches that tune ignore tile codes while the tuner is off, so nothing else changes.
        MCG_NO_PRETUNED=1 loads nothing."""
        if os.environ.get('MCG_NO_PRETUNED') != '1':
            self.merge(read_entries(self.main), overwrite=False, only_split=only_split)      # (of a key listed twice, the first entry)

    def overlay(self, entries, *earlier):
        """Move the launches of `entries` to their codes -- where `main` (earlier[0]) knows the launch and the table still holds a
        code one of the earlier layers gives for it (a choice loaded from elsewhere, or tuned in this process, stays).  Returns
        the number of launches moved."""
        moved = 0
        for k, v in entries.items():
            if k in earlier[0] and self.choices.get(k, -1) in [layer[k] for layer in earlier if k in layer]:
                self.choices[k] = v
                moved += 1
        return moved

    def use_dense(self):
        """The dense list over `main`.  Part of set_autotune(True) with the shipped table; MCG_DENSE_SPLIT=0 keeps the padded
        codes (A/B timing)."""
        if os.environ.get('MCG_DENSE_SPLIT', '1') == '0':
            return 0
        return self.overlay(read_list(self.dense), read_list(self.main))

    def use_live(self, path=None):
        """The live-steps list (or the one at `path`) over `main` and the dense list.  Called by step.TrainStep when the tuner is
        on (bench.py, train.py); set_autotune() does not; MCG_LIVE_STEPS=0 leaves the table as it is (A/B timing)."""
        if not os.path.exists(self.main) or os.environ.get('MCG_LIVE_STEPS', '1') == '0':
            return 0
        return self.overlay(live_list(path or self.live), read_list(self.main), read_list(self.dense))

    def tuned(self, kind, g, extra, measure):
        """Returns g, or a copy of it with .tile set to the fastest candidate.  measure(geom) -> ms of the pass with that tile code
        (on scratch output: tuning never touches the caller's output or accumulators), None for an impossible candidate."""
        if not self.autotune or g.tile:
            return g
        key = geom_key(kind, g, extra)
        code = self.choices.get(key)
        if code is None:
            best, code = None, 0
            gg = type(g).from_buffer_copy(g)
            for cand in candidates(kind, g):
                gg.tile = cand
                ms = measure(gg)
                if ms is not None and (best is None or ms < best):
                    best, code = ms, cand
            self.choices[key] = code
        return with_tile(g, code) if code else g

    def split_decided(self, kind, g):
        """True when a launch of this pass and geometry is KNOWN to take the split form (MCG_SPLIT=always, or the table says so): the
        producers of its operands may then write the split layout only.  False while undecided."""
        if not split_covers(kind, g):
            return False
        mode = os.environ.get('MCG_SPLIT', 'auto')
        if mode != 'auto':
            return mode == 'always'
        return self.choices.get(geom_key('split-' + kind, g)) == 1

    def split_pays(self, kind, g, run_plain, run_split, best_ms):
        """Which of the two forms of a launch is faster for this geometry -- the fp32-MFMA kernels on fp32 operands (run_plain) or the
        split form on the bf16 pipe (run_split, INCLUDING whatever it takes to produce the split operands)?  Timed once (best_ms(run)
        -> ms) per (pass, geometry) like the tile candidates and kept in the same table (key 'split-<pass>', value 1 = split);
        MCG_SPLIT=always / never overrides (tests, A/B timing).  Both forms write the same output; the caller launches the winner."""
        mode = os.environ.get('MCG_SPLIT', 'auto')
        if mode != 'auto':
            return mode == 'always'
        key = geom_key('split-' + kind, g)
        c = self.choices.get(key)
        if c is None and not self.autotune:
            # tuner off (tests, train.py --autotune 0): nothing is timed -- the table's entries, else the fp32 form.
            # (Under data parallelism per-rank timing could also leave the ranks on different forms.)
            if not self.warned_undecided_split:
                self.warned_undecided_split = True
                warnings.warn("precision 'f32x3': the tile tuner is off and the table holds no decision for %s N=%d T=%d H=%d Ci=%d Co=%d -- "
                              "this launch (and every other undecided one) runs the fp32-MFMA form; hiplib.set_autotune(True), "
                              "MCG_SPLIT=always or a loaded tile table decide it" % (kind, g.N, g.Ti, g.Hi, g.Ci, g.Co))
            return False
        if c is None:
            plain_ms = best_ms(run_plain)
            self.choices[key] = c = int(best_ms(run_split) < 0.97 * plain_ms)
        return bool(c)


table = TileTable()
