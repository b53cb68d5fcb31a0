"""Extracts the parameter rows of the concrete optimizer's WoP-PBS reference table
(compilers/concrete-optimizer/v0-parameters/ref/wop_pbs_last_128: per message width and log norm2,
k, log2 N, n, br_l, br_b, ks_l, ks_b, cb_l, cb_b, pp_l, pp_b; cost and p_error are left out) into
tests/golden/wop_pbs_last_128_rows.json.  The rows are data (the table's numbers), read by
tests/table_shapes.py; this script runs where the reference tree is, not on the GPU boxes.
Usage: python tests/golden/make_wop_rows.py <reference tree>"""
import json
import os
import re
import sys

FIELDS = ("k", "N", "n", "br_l", "br_b", "ks_l", "ks_b", "cb_l", "cb_b", "pp_l", "pp_b")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    rel = "compilers/concrete-optimizer/v0-parameters/ref/wop_pbs_last_128"
    rows, width = [], None
    for line in open(os.path.join(ref, rel)):
        m = re.match(r"\s*- (\d+): # bits", line)
        if m:
            width = int(m.group(1))
            continue
        m = re.match(r"\s*- (\d+)\s*:\s*(.*)", line)
        if m and width is not None:
            cells = m.group(2).split(",")
            assert len(cells) == len(FIELDS) + 2, line  # the columns of FIELDS, then cost and p_error
            row = dict(zip(FIELDS, (int(x) for x in cells[:len(FIELDS)])))
            row["N"] = 1 << row["N"]
            rows.append({"bits": width, "log_norm2": int(m.group(1)), **row})
    assert len(rows) == 272, len(rows)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wop_pbs_last_128_rows.json")
    with open(out, "w") as fh:  # one row per line
        fh.write('{"source": "%s", "rows": [\n' % rel)
        fh.write(",\n".join(json.dumps(r) for r in rows))
        fh.write("\n]}\n")
    print(f"{len(rows)} rows -> {out}")


if __name__ == "__main__":
    main()
