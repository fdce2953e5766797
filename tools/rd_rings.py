#!/usr/bin/env python3
"""Rate and distortion of one frame side by side, per range ring: `<stream>.rings.json` (--rate_rings) joined with `<stream>.dist.json`
(--distortion_report) made with the same ring edges.

    python tools/rd_rings.py out/000000_spher_12_1023_0.rings.json out/000000_spher_12_1023_0.dist.json

Per ring: the reconstructed leaves and the input points in it, the ideal bits per leaf and per input point, and the D1 mean squared
error of both directions (input -> reconstruction binned by the input point's ring, reconstruction -> input binned by the
reconstructed point's ring, the rho shells taken together).  Host only; refuses two files whose edges differ.
"""
import argparse
import json
import math
import sys


class EdgesDiffer(ValueError):
    pass


def join(rings, dist):
    """The two loaded documents -> one dict per ring (plain Python)."""
    if [float(e) for e in rings["edges"]] != [float(e) for e in dist["edges"]]:
        raise EdgesDiffer(f"the ring edges differ: {rings['edges']} (rate) against {dist['edges']} (distortion) - make both reports with the same edges")
    edges = [float(e) for e in rings["edges"]]
    rows = []
    for r, lo in enumerate(edges):
        rate, ab = rings["rings"][r], dist["a_to_b"]["rings"][r]
        shells = [g[r] for g in dist["b_to_a"]["groups"]]
        ba_rows = sum(e["rows"] for e in shells)
        ba_sq = math.fsum(e["sum_sq"] for e in shells)
        rows.append(dict(ring=r, lo=lo, hi=edges[r + 1] if r + 1 < len(edges) else None, leaves=rate["leaves"], points=rate["points"],
                         ideal_bits=rate["ideal_bits"], table_bits=rate["table_bits"],
                         bits_per_leaf=rate["ideal_bits"] / rate["leaves"] if rate["leaves"] else 0.0,
                         bits_per_point=rate["ideal_bits"] / rate["points"] if rate["points"] else 0.0,
                         mse_ab=ab["sum_sq"] / ab["rows"] if ab["rows"] else 0.0, mse_ba=ba_sq / ba_rows if ba_rows else 0.0,
                         dist_rows_ab=ab["rows"], dist_rows_ba=ba_rows))
    return rows


def render(rows):
    out = [f"{'ring':>14} {'leaves':>9} {'points':>9} {'bits/leaf':>10} {'bits/point':>10} {'mse in->rec':>12} {'mse rec->in':>12}"]
    for e in rows:
        name = f"{e['lo']:g} - {e['hi']:g}" if e["hi"] is not None else f"{e['lo']:g} -"
        out.append(f"{name:>14} {e['leaves']:>9d} {e['points']:>9d} {e['bits_per_leaf']:>10.4f} {e['bits_per_point']:>10.4f} "
                   f"{e['mse_ab']:>12.6g} {e['mse_ba']:>12.6g}")
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rings_json")
    ap.add_argument("dist_json")
    ap.add_argument("--json", action="store_true", help="print the joined rows as JSON instead of a table")
    args = ap.parse_args(argv)
    with open(args.rings_json) as f:
        rings = json.load(f)
    with open(args.dist_json) as f:
        dist = json.load(f)
    try:
        rows = join(rings, dist)
    except EdgesDiffer as e:
        print("rd_rings:", e, file=sys.stderr)
        return 2
    print(json.dumps(rows) if args.json else render(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
