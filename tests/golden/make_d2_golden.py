#!/usr/bin/env python3
"""Fixtures of the D2 (point-to-plane) PSNR: tests/golden/d2_metrics.json + d2_sphere.npz + d2_lattice.npz.

Runs the MPEG `pc_error` binary the reference shells out to (data_preproc/pt.py:13-85, `-a A -b B -r peak`, A an ascii PLY with
float32 x y z nx ny nz as data_preproc/gene_normals.py writes it) on two small cloud pairs and records the numbers it prints for
p2point and p2plane.  The binary (`utils/pc_error` of the reference checkout) may come without an exec bit: a temporary copy is made
executable, as make_golden.py gen_metrics does.  Two pairs:
  sphere   2000 points on a 10 m sphere (float32) against their distinct copies rounded to 0.25: no exact distance tie anywhere
           (asserted), normals = the radial direction;
  lattice  120 points with even integer coordinates against 90 with odd ones: nearly every nearest-neighbour search ends in an exact
           tie (up to 8 equal neighbours), in any arithmetic; normals = seeded random unit vectors.
Usage: python tests/golden/make_d2_golden.py --tool <reference checkout>/utils/pc_error
"""
import argparse
import json
import os
import re
import shutil
import stat
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import d2_ref  # noqa: E402
from scp_amd.data_preproc import pt  # noqa: E402

PEAK = 59.70


def unit_f32(v):
    v = np.asarray(v, np.float64)
    return (v / np.sqrt((v * v).sum(1))[:, None]).astype(np.float32)


def sphere_pair():
    rng = np.random.default_rng(11)
    a = (unit_f32(rng.standard_normal((2000, 3))).astype(np.float64) * 10.0).astype(np.float32)
    b = np.unique(np.round(a.astype(np.float64) / 0.25) * 0.25, axis=0).astype(np.float32)
    return a, unit_f32(a), b


def lattice_pair():
    rng = np.random.default_rng(12)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing="ij"), -1).reshape(-1, 3)
    a = (2 * g).astype(np.float32)                                        # 120 even points
    h = np.stack(np.meshgrid(np.arange(3), np.arange(5), np.arange(6), indexing="ij"), -1).reshape(-1, 3)
    b = (2 * h + 1).astype(np.float32)                                    # 90 odd points
    a, b = a[rng.permutation(len(a))], b[rng.permutation(len(b))]         # no help from the index order
    return a, unit_f32(rng.standard_normal((len(a), 3))), b


def run_tool(exe, tmp, a, n_a, b):
    fa, fb = os.path.join(tmp, "a.ply"), os.path.join(tmp, "b.ply")
    pt.write_ply_normals(fa, a, n_a)
    pt.write_ply_data(fb, b)
    out = subprocess.run([exe, "-a", fa, "-b", fb, "-r", "%.2f" % PEAK], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    got = {}
    for key, pat in (("d1_mse_ab", r"mse1\s+\(p2point\)"), ("d1_mse_ba", r"mse2\s+\(p2point\)"), ("d1_psnr", r"mseF,PSNR\s+\(p2point\)"),
                     ("mse_ab", r"mse1\s+\(p2plane\)"), ("mse_ba", r"mse2\s+\(p2plane\)"), ("psnr_d2", r"mseF,PSNR\s+\(p2plane\)")):
        m = re.search(pat + r":\s*(\S+)", out)
        assert m, (key, out)
        got[key] = float(m.group(1))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tool", required=True, help="the MPEG pc_error binary (utils/pc_error of the reference checkout)")
    tool = ap.parse_args().tool
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pc_error")
        shutil.copy(tool, exe)
        os.chmod(exe, os.stat(exe).st_mode | stat.S_IXUSR)
        for name, (a, n_a, b) in (("sphere", sphere_pair()), ("lattice", lattice_pair())):
            assert len(np.unique(a, axis=0)) == len(a) and len(np.unique(b, axis=0)) == len(b)        # no fixture holds duplicates
            dab, dba = d2_ref.nn_sqdist(a, b), d2_ref.nn_sqdist(b, a)
            ties_ab = (d2_ref._sqdist_rows(a.astype(np.float64), b.astype(np.float64)) == dab[:, None]).sum(1)
            ties_ba = (d2_ref._sqdist_rows(b.astype(np.float64), a.astype(np.float64)) == dba[:, None]).sum(1)
            if name == "sphere":
                assert ties_ab.max() == 1 and ties_ba.max() == 1
            else:
                assert ties_ab.min() >= 2 or ties_ba.min() >= 2
            tool = run_tool(exe, tmp, a, n_a, b)
            ref = d2_ref.d2_psnr(a, n_a, b, PEAK)
            out[name] = dict(tool, peak=PEAK, n_a=len(a), n_b=len(b), max_ties_ab=int(ties_ab.max()), max_ties_ba=int(ties_ba.max()))
            print(name, out[name], "numpy:", ref)
            np.savez_compressed(os.path.join(HERE, f"d2_{name}.npz"), a=a, n_a=n_a, b=b)
    with open(os.path.join(HERE, "d2_metrics.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote d2_metrics.json")


if __name__ == "__main__":
    main()
