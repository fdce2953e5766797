#!/usr/bin/env python3
"""What every octree level costs and buys, ring by ring: reads a `<stream>.depth.json` (encode*.py --depth_report).

    python tools/rd_depth.py out/000000_spher_12_1023_0.depth.json

Per range ring (and for the frame as a whole), for every truncation depth k of the report: the ideal bits per input point of levels
1 .. D - k, the D1 mean squared error of the input -> reconstruction direction of the cloud those levels describe, and what the deepest
level kept buys: level D - k lowers the error from mse(k + 1) to mse(k), 10 log10(mse(k + 1) / mse(k)) dB, for the bits(k) - bits(k + 1)
per point it adds - the marginal dB per bit.  The coarsest depth of the report has nothing to compare with; a level that costs a ring
nothing, or an error of 0, gives no ratio.  Host only.
"""
import argparse
import json
import math
import sys


class NotADepthReport(ValueError):
    pass


def _levels(entries):
    """[(drop, rate entry with `points` and `ideal_bits`, distortion entry with `rows` and `sum_sq`)] of one ring -> its rows."""
    rows = []
    for drop, rate, ab in entries:
        rows.append(dict(drop=drop, bits_per_point=rate["ideal_bits"] / rate["points"] if rate["points"] else 0.0,
                         mse_ab=ab["sum_sq"] / ab["rows"] if ab["rows"] else 0.0, gain_db=None, db_per_bit=None))
    for e, coarser in zip(rows, rows[1:]):
        if e["mse_ab"] > 0.0 and coarser["mse_ab"] > 0.0:
            e["gain_db"] = 10.0 * math.log10(coarser["mse_ab"] / e["mse_ab"])
            added = e["bits_per_point"] - coarser["bits_per_point"]
            e["db_per_bit"] = e["gain_db"] / added if added > 0.0 else None
    return rows


def table(doc):
    """The loaded document -> one dict per ring and one for the whole frame (plain Python)."""
    if "levels" not in doc or "edges" not in doc:
        raise NotADepthReport("no `levels` / `edges` in the document: a <stream>.depth.json written by --depth_report expected")
    edges = [float(e) for e in doc["edges"]]
    levels = doc["levels"]
    out = []
    for r, lo in enumerate(edges):
        out.append(dict(ring=r, lo=lo, hi=edges[r + 1] if r + 1 < len(edges) else None,
                        levels=_levels([(lv["drop"], lv["rate"]["rings"][r], lv["distortion"]["a_to_b"]["rings"][r]) for lv in levels])))
    out.append(dict(ring="total", lo=0.0, hi=None, levels=_levels([(lv["drop"], lv["rate"]["total"], lv["distortion"]["a_to_b"]["total"]) for lv in levels])))
    return out


def render(rows):
    out = [f"{'ring':>14} {'drop':>5} {'bits/point':>10} {'mse in->rec':>12} {'gain dB':>9} {'dB/bit':>9}"]
    for e in rows:
        name = "total" if e["ring"] == "total" else (f"{e['lo']:g} - {e['hi']:g}" if e["hi"] is not None else f"{e['lo']:g} -")
        for lv in e["levels"]:
            gain = f"{lv['gain_db']:>9.3f}" if lv["gain_db"] is not None else f"{'-':>9}"
            per = f"{lv['db_per_bit']:>9.3f}" if lv["db_per_bit"] is not None else f"{'-':>9}"
            out.append(f"{name:>14} {lv['drop']:>5d} {lv['bits_per_point']:>10.4f} {lv['mse_ab']:>12.6g} {gain} {per}")
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("depth_json")
    ap.add_argument("--json", action="store_true", help="print the rows as JSON instead of a table")
    args = ap.parse_args(argv)
    with open(args.depth_json) as f:
        doc = json.load(f)
    try:
        rows = table(doc)
    except NotADepthReport as e:
        print("rd_depth:", e, file=sys.stderr)
        return 2
    print(json.dumps(rows) if args.json else render(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
