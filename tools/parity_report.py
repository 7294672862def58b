#!/usr/bin/env python
"""profiles/production_parity.md from the rows the production-size parity tests write.

    MCG_PARITY_TABLE=rows.md python -m pytest tests/test_gpu_fullwidth.py -m gpu -k production -s --durations=25 > run.log
    python tools/parity_report.py rows.md [run.log] [note.md] > profiles/production_parity.md

rows.md: what tests/test_gpu_fullwidth.py appended (one markdown row per compared launch, one '(total)' row per configuration);
run.log: the pytest output (its --durations lines give the tests' run times); note.md: free text placed under the heading
(observations of the run that no row holds)."""
import re
import sys


def main(argv):
    rows = [l.rstrip("\n") for l in open(argv[1]) if l.startswith("|")]
    log = open(argv[2]).read() if len(argv) > 2 else ""
    note = open(argv[3]).read().strip() if len(argv) > 3 else ""
    cells = lambda r: [x.strip() for x in r.strip("|").split("|")]
    totals = [cells(r) for r in rows if "(total)" in r]
    body = [cells(r) for r in rows if "(total)" not in r]
    worst = {}
    for c in body:
        kind = c[2].split(" ")[0]
        store = "bf16" if "bf16 store" in c[2] else "fp32 / split"
        rel, blk = float(c[5]), float(c[6])
        w = worst.get((kind, store), (0.0, 0.0, ""))
        worst[(kind, store)] = (max(rel, w[0]), max(blk, w[1]), "%s %s %s code %s" % (c[0], c[1], c[3], c[4]) if rel > w[0] else w[2])
    dur = re.findall(r"^([\d.]+)s call\s+tests/test_gpu_fullwidth.py::(\S*(?:production|largest|clip_bytes)\S*)", log, re.M)
    out = ["# Production-size parity: every launch of the benchmarked step against float64", ""]
    out += ["Written by `tools/parity_report.py` from the rows `tests/test_gpu_fullwidth.py` appends to `$MCG_PARITY_TABLE` (the same figures",
            "are printed per launch).  Reference: `tests/ref64.py`, a tap-wise float64 convolution on the device.  `rel-L2` is global;",
            "`worst block` is the largest error of a 256-row x 64-column block of the result seen as the GEMM's [M][C] matrix, relative to",
            "the reference norm an average block of its size holds.  Conditions: rel-L2 < 1e-5 (fprop) / 1e-4 (dgrad, wgrad), worst block",
            "< 4 x that; a launch that stores bf16 is allowed 2^-9 = 1.95e-3 on top (the rms of a round-to-nearest bf16 store is 1.7e-3).",
            "`layer` is `<net>.<layer>@<N of the launch>`; `code` is the tile code of `mocogan-chainer_amd/tuned_tiles_mi355x.json` for the",
            "launch (0 also where the table holds no entry).  bf16 / bf16s / bf16y launches run on bf16-representable inputs.", ""]
    if note:
        out += [note, ""]
    out += ["## Largest figures per pass", "", "| pass | store | largest rel-L2 | launch | largest worst block |", "|---|---|---|---|---|"]
    for (kind, store), (rel, blk, where) in sorted(worst.items()):
        out.append("| %s | %s | %.2e | %s | %.2e |" % (kind, store, rel, where, blk))
    out += ["", "## Run time and peak device memory", "", "| configuration | launches compared | time | peak device memory |", "|---|---|---|---|"]
    for c in totals:
        out.append("| %s | %s | %s | %s |" % (c[0], c[2], c[5], c[6]))
    if dur:
        out += ["", "Slowest production-size tests (pytest --durations), %.0f s together:" % sum(float(d) for d, _ in dur), ""]
        out += ["* %s s  `%s`" % d for d in dur[:12]]
    out += ["", "## Per launch", "", "| configuration | layer@N | pass (variant) | form | code | rel-L2 | worst block |", "|---|---|---|---|---|---|---|"]
    out += ["| " + " | ".join(c) + " |" for c in body]
    print("\n".join(out))


if __name__ == '__main__':
    main(sys.argv)
