"""The distinct shapes of the optimizer's two 128-bit tables, as lists a test can be parametrized with.
A helper module, not a test file.

Every list is the sorted set of a column tuple over every row of tests/golden/v0_last_128_rows.json (235 rows)
and / or tests/golden/wop_pbs_last_128_rows.json (272 rows, all at k = 2, N = 1024), so a sweep over it is
complete by construction; tests/test_keygen_abi.py pins the counts, the WoP rows' acceptance and the key
formats.
"""
import json
import os

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rows(name):
    return json.load(open(os.path.join(_GOLDEN, name)))["rows"]


V0_ROWS = _rows("v0_last_128_rows.json")
WOP_ROWS = _rows("wop_pbs_last_128_rows.json")


def distinct(rows, *cols):
    return sorted({tuple(r[c] for c in cols) for r in rows})


PBS_COLS = ("k", "N", "br_l", "br_b")
V0_PBS = distinct(V0_ROWS, *PBS_COLS)
V0_KS = distinct(V0_ROWS, "ks_l", "ks_b")
WOP_BSK = distinct(WOP_ROWS, *PBS_COLS)
WOP_KS = distinct(WOP_ROWS, "ks_l", "ks_b")
WOP_CB = distinct(WOP_ROWS, "cb_l", "cb_b")  # the circuit bootstrap's output = the vertical packing's GGSWs
WOP_PP = distinct(WOP_ROWS, "pp_l", "pp_b")  # the fp-ks
PBS_SHAPES = sorted(set(V0_PBS) | set(WOP_BSK))
KS_DECOMPS = sorted(set(V0_KS) | set(WOP_KS))
WOP_RING = (2, 1024)
