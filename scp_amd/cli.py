"""Drop-in command lines: `encode.py` (encode.py:315-339) and `encode_mullevel.py` (encode_mullevel.py:235-260).

Same flags, same output files (`<run>/test_output<ckpt-stem>/<frame>[_spher|_cylin]_<levels>_<bin_num>_<z_offset>.bin` + `.dat`),
same stdout block per frame, same summary file.  Differences, all additive:
  * `--gpus N` / torchrun: frames are sharded across ranks and the summary is all-reduced (scp_amd/distributed.py);
    the GPU is selected by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES like CUDA_VISIBLE_DEVICES in the reference;
  * the hydra run directory is read with a plain YAML loader; `--random_weights SEED` replaces the checkpoint for
    smoke runs (no trained checkpoint can be fetched offline);
  * `--test_files` accepts a glob, a directory or a list (the reference's `glob.glob(list)` cannot work, SURVEY B-3).
  * `--metrics`: chamfer distance and D1 PSNR of every frame, computed on the device (scp_amd/metrics.py; the reference
    shells out to pc_error and a CPU KD-tree for these) - they enter the per-frame block and the all-reduced summary.
  * `--rate_report`: where every frame's bits go - the model's cross-entropy (ideal bits), the cost of the coder's 16-bit tables and the
    coded size, per octree level (EHEM: per phase), computed on the device (csrc/rate.hip): one more line per frame and a
    `<stream>.rate.json` next to every stream.  The streams themselves do not change.
  * `--distortion_report [EDGES]` (EHEM): where every frame's D1 error goes - per range ring (EDGES: comma-separated ring edges starting at
    0, by default 0,5,10,15,20,30,40,60,80 m for KITTI and the same in millimetres for Ford) and per rho shell, split along the sensor's
    r / phi / theta axes, computed on the device (csrc/distreport.hip): one more line per frame and a `<stream>.dist.json` next to every
    stream.  The streams themselves do not change.
  * `--rate_rings [EDGES]` (EHEM): what every range ring costs - each node's ideal and coded-table bits handed to the points below it in
    equal parts and summed per ring (same EDGES and defaults as `--distortion_report`) and rho shell, computed on the device
    (csrc/ringrate.hip): one more line per frame (ideal bits per leaf of every ring) and a `<stream>.rings.json` next to every stream
    (tools/rd_rings.py joins it with the `.dist.json`).  Implies the rate kernels; the streams themselves do not change.
  * `--depth_report [K[:EDGES]]` (EHEM): what every octree level costs and buys, from one encode - for every truncation depth k = 0 .. K
    (default 4) the bits of levels 1 .. D - k per range ring and rho shell (csrc/ringrate.hip, on the bins of `--rate_rings`) and the D1
    error of the cloud those levels describe (the cells of size 2^k, which `decode_ehem.py --lod k` writes): one more line per frame
    (ideal bits per point and D1 PSNR for every k) and a `<stream>.depth.json` next to every stream (tools/rd_depth.py reads it).
    Implies the rate kernels; the streams themselves do not change.
  * `--temper` (EHEM) / `--temper_report`: one inverse temperature per (octree level, phase) out of a grid of 25, chosen on the frame as the
    one that costs the fewest ideal bits (csrc/temper.hip) when that saves more than the byte its index costs.  `--temper` codes the
    scaled rows: the stream's name gains `_temper` in front of the coordinate token and the side-info file the grid and the indices, which
    `decode_ehem*.py` require for such a name.  `--temper_report` alone leaves the streams as they are.  One more line per frame (ideal
    bits per point at 1 and as chosen, the side bits, the groups that moved); `--temper_report` also writes `<stream>.temper.json`.
  * `--ring_lod EDGES:DROPS` (EHEM, `--spher` / `--cylin`): a truncation depth per range ring - the points of a ring with drop k are snapped
    to cells of size 2^k before the octree is built, the rows below such a cell are forced to symbol 0 on both sides (csrc/ringlod.hip), and
    the decoder writes the cells' centres.  The stream's name gains `_ringlod` in front of `_temper` / the coordinate token and the
    side-info file the drops and the integer thresholds, which `decode_ehem*.py` require for such a name (not with `--lod` / `--streams`).
    One more line per frame; `--metrics` and the reports then describe the tree that was coded.  All drops 0: the streams of today.
  * `--attr [Q]` (EHEM, `--type kitti` / `ford`) / `--attr_scale S`: the reflectance of every frame, one 8-bit value per leaf of the octree, through an
    integer lifting transform on that octree (csrc/attr.hip) with step Q (default 1: lossless on the leaf values) into `<stream>.attr` next
    to the stream, which `decode_ehem*.py --attr` turns into `<stem>.attr.bin` (x y z r).  S = 8-bit units per unit of reflectance (default
    255 for kitti, 1 for ford).  One more line per frame (bits, bits per point, with `--metrics` the reflectance PSNR); the streams and
    every other file keep their bytes.
  * `--color [Q]` (EHEM, `--type obj`): the RGB of an object cloud, one colour per leaf of the octree - per-leaf means, a reversible YCoCg-R
    transform and the reflectance layer's integer lifting on the three planes at once (csrc/color.hip), one step Q for all channels
    (default 1: lossless on the leaf means) - into `<stream>.color` next to the stream, which `decode_ehem.py --color` turns into
    `<stem>.color.ply` (x y z red green blue).  One more line per frame (bits, bits per point, with `--metrics` the luma and RGB PSNR); the
    stream and every other file keep their bytes.
  * `--chunk [N]` (with `--attr` or `--color`): the layer's file in its version 2 - every payload cut into chunks of N symbols (64 .. 2^20,
    default 4096), each an independently terminated range-coder stream, which the device codes and `decode_ehem*.py --attr` / `--color`
    decode all at once (csrc/ac_chunks.hip); costs the length table and a flush per chunk.  The decoders take the version from the file.
    File names, the per-frame lines and every other file stay as they are.
  * `--attr_sweep [STEPS]` / `--color_sweep [STEPS]` (with `--attr` / `--color`): what every step of a grid (comma-separated, strictly ascending,
    1 .. 255, at most 16; default 1,2,3,4,6,8,12,16,24,32,48,64,96,128,192,255) costs and loses on the frame, from one pass over the octree
    (csrc/lift.h: scp_attr_sweep / scp_color_sweep).  One more line per frame (per step Q: estimated bits per point, leaf PSNR) and
    `<stream>.attr.sweep.json` / `<stream>.color.sweep.json`; every other file keeps its bytes.  The PSNR is over leaf values - what the layer
    codes against what it returns - not the point-wise PSNR of `--metrics`.
  * `--attr_target KIND=VALUE` / `--color_target KIND=VALUE` (with `--attr` / `--color` without a Q), KIND `psnr`, `bpp` or `linf`: the layer's
    file is written at the step the sweep chooses per frame - the largest whose leaf PSNR is >= VALUE, the smallest whose estimated bits are
    <= VALUE per point, the largest whose largest leaf error is <= VALUE; where no step qualifies, the smallest (the largest for `bpp`), reported
    as not met.  One more line per frame (target, chosen Q, met, estimated / written bits); with `--attr_sweep` / `--color_sweep` alongside, the
    target chooses on that grid and the table is written too.  The decoders read the chosen Q from the header as before.
  * `--normals estimate|DIR` (with `--metrics`, EHEM): the D2 (point-to-plane) PSNR as well, on normals estimated on the device or
    read from the `<DIR>/<sequence>/<frame>.ply` files `gene_normals.py` writes; one more line per frame, `PSNR_D2:` in the summary.
"""
import argparse
import glob
import json
import os
import time
from pathlib import Path

import numpy as np
import torch

from . import distributed as D
from . import native
from .data_preproc import pt as pointCloud
from .decoder import decode_file, write_sidecar
from .encoder import FrameEncoder, OctAttnFrameEncoder


class Cfg(dict):
    def __getattr__(self, k):
        v = self[k]
        return Cfg(v) if isinstance(v, dict) else v


EHEM_DEFAULT = dict(class_name="EHEM", context_size=8192, token_num=255, level_k=4, max_level=19)
OCTATTN_DEFAULT = dict(class_name="OctAttention", max_octree_level=12, context_size=1024, token_num=255, layer_num=3,
                       head_num=4, abs_pos_embed_dim=12, occ_embed_dim=128, level_embed_dim=6, octant_embed_dim=4,
                       hidden_dimension=300, pos_max_len=5000, level_k=4, pos_embed=True)


def load_cfg(ckpt_path, model_name=None):
    """encode.py:238-244: the hydra snapshot next to the checkpoint, else the reference's config defaults."""
    root = ckpt_path.split("ckpt")[0] if ckpt_path else ""
    y = Path(root, ".hydra", "config.yaml")
    if ckpt_path and y.exists():
        import yaml
        with open(y) as f:
            raw = yaml.safe_load(f)
        raw.setdefault("data", {}).setdefault("extra_pos", False)
        raw.setdefault("train", {}).setdefault("type", "kitti")
        return Cfg(raw)
    model = dict(EHEM_DEFAULT if (model_name or "EHEM") == "EHEM" else OCTATTN_DEFAULT)
    return Cfg(model=model, data=dict(extra_pos=False), train=dict(type="kitti", dropout=0.0))


def parse_edges(text, flag="--distortion_report"):
    """`--distortion_report 0,5,10`: the ring edges as a tuple of floats (native.dist_edges states what a valid list is)."""
    try:
        vals = [float(v) for v in text.split(",")]
    except ValueError:
        raise native.ScpError(f"{flag}: ring edges are comma-separated numbers starting at 0, got {text!r}")
    return native.dist_edges(vals)


def parse_ring_edges(text):
    """`--rate_rings 0,5,10`: the same syntax as --distortion_report's."""
    return parse_edges(text, "--rate_rings")


def distortion_request(args):
    """(wanted, edges) of --distortion_report: (False, None) without the flag, (True, None) for the data type's default edges."""
    v = getattr(args, "distortion_report", None)
    return (v is not None and v is not False), (None if v is None or isinstance(v, bool) else tuple(v))


def rings_request(args):
    """(wanted, edges) of --rate_rings, read like distortion_request."""
    v = getattr(args, "rate_rings", None)
    return (v is not None and v is not False), (None if v is None or isinstance(v, bool) else tuple(v))


DEPTH_REPORT_DEFAULT = 4


def parse_depth_report(text):
    """`--depth_report 3` / `--depth_report 3:0,5,10`: (K, ring edges or None); the edges in --distortion_report's syntax."""
    k, _, e = text.partition(":")
    try:
        drop = int(k) if k else DEPTH_REPORT_DEFAULT
    except ValueError:
        raise native.ScpError(f"--depth_report: K[:EDGES] with K the number of levels to drop (0 .. {native.MAX_DEPTH}), got {text!r}")
    if not 0 <= drop <= native.MAX_DEPTH:
        raise native.ScpError(f"--depth_report: K = {drop} outside 0 .. {native.MAX_DEPTH}")
    return drop, (parse_edges(e, "--depth_report") if e else None)


def depth_request(args):
    """(wanted, K, edges) of --depth_report: (False, None, None) without the flag; the flag alone asks for K = 4 and the default edges."""
    v = getattr(args, "depth_report", None)
    if v is None or v is False:
        return False, None, None
    return (True, DEPTH_REPORT_DEFAULT, None) if v is True else (True, v[0], None if v[1] is None else tuple(v[1]))


def temper_request(args):
    """--temper / --temper_report -> (the encoder's `temper` mode: None, "report" or "code"; whether <stream>.temper.json is written)."""
    code, rep = getattr(args, "temper", False), getattr(args, "temper_report", False)
    return ("code" if code else ("report" if rep else None)), bool(rep)


def parse_ring_lod(text):
    """`--ring_lod 0,10,25:2,1,0`: (ring edges in --distortion_report's syntax, one drop per ring) as FrameEncoder(ring_lod=) takes them."""
    e, sep, d = text.partition(":")
    try:
        drops = [int(v) for v in d.split(",")] if sep else None
    except ValueError:
        drops = None
    if drops is None:
        raise native.ScpError(f"--ring_lod: EDGES:DROPS expected - ring edges from 0 and one integer drop per ring, as in 0,10,25:2,1,0 - got {text!r}")
    from .encoder import parse_ring_lod as check
    edges = parse_edges(e, "--ring_lod")
    check((edges, drops))
    return edges, tuple(drops)


def ring_lod_request(args):
    """--ring_lod -> the encoder's `ring_lod` argument, None without the flag."""
    return getattr(args, "ring_lod", None)


def attr_request(args):
    """--attr [Q] / --attr_scale S -> (Q or None without the flag, S or None for the data type's default)."""
    q, s = getattr(args, "attr", None), getattr(args, "attr_scale", None)
    if q is None and s is not None:
        raise native.ScpError("--attr_scale sets the scale of the reflectance layer: give --attr as well")
    if q is not None and not 1 <= int(q) <= 255:
        raise native.ScpError(f"--attr {q}: the step Q is 1 (lossless) .. 255")
    if s is not None and not 1 <= int(s) <= 1 << 20:
        raise native.ScpError(f"--attr_scale {s}: 1 .. 2^20 8-bit units per unit of reflectance expected")
    return (None if q is None else int(q)), (None if s is None else int(s))


def color_request(args):
    """--color [Q] -> Q, or None without the flag."""
    q = getattr(args, "color", None)
    if q is not None and not 1 <= int(q) <= 255:
        raise native.ScpError(f"--color {q}: the step Q is 1 (lossless on the leaf means) .. 255")
    return None if q is None else int(q)


def sweep_request(args, layer):
    """--<layer>_sweep [STEPS] / --<layer>_target KIND=VALUE (layer: "attr" or "color") -> (steps: numpy int32 [G] or None without
    --<layer>_sweep, target: (kind, value) or None without --<layer>_target).  Refused with the reason: either option without --<layer>, a
    step Q other than 1 together with a target, an unknown kind, a value that is not finite or negative, a grid that is empty, longer
    than 16, not strictly ascending or outside 1 .. 255."""
    from . import attr
    sw, tg, q = getattr(args, layer + "_sweep", None), getattr(args, layer + "_target", None), getattr(args, layer, None)
    what = "the reflectance layer" if layer == "attr" else "the colour layer"
    if q is None and (sw is not None or tg is not None):
        opt = f"--{layer}_sweep" if sw is not None else f"--{layer}_target"
        raise native.ScpError(f"{opt} measures or sets the step of {what}: give --{layer} as well")
    steps = target = None
    if sw is not None:
        if isinstance(sw, str):
            try:
                sw = None if sw == "" else [int(t) for t in sw.split(",")]
            except ValueError:
                raise native.ScpError(f"--{layer}_sweep {sw}: comma-separated integer steps expected, e.g. 1,2,4,8") from None
        try:
            steps = native.sweep_steps(sw)
        except native.ScpError as e:
            raise native.ScpError(f"--{layer}_sweep: {e}") from None
    if tg is not None:
        kind, sep, val = str(tg).partition("=")
        try:
            value = float(val)
        except ValueError:
            raise native.ScpError(f"--{layer}_target {tg}: KIND=VALUE expected, KIND one of {', '.join(attr.TARGET_KINDS)}") from None
        if not sep:
            raise native.ScpError(f"--{layer}_target {tg}: KIND=VALUE expected, KIND one of {', '.join(attr.TARGET_KINDS)}")
        target = attr.check_target((kind, value), f"--{layer}_target")
        if int(q) != 1:
            raise native.ScpError(f"--{layer} {q} with --{layer}_target: the target chooses the step - give --{layer} without a Q")
    return steps, target


def chunk_request(args):
    """--chunk [N] -> N, or None without the flag; refused without --attr / --color and outside 64 .. 2^20."""
    n = getattr(args, "chunk", None)
    if n is None:
        return None
    if getattr(args, "attr", None) is None and getattr(args, "color", None) is None:
        raise native.ScpError("--chunk cuts the payloads of an attribute layer into chunks: give --attr or --color as well")
    return native.check_chunk(n, "--chunk")


def ply_has_colors(path):
    """Whether the first point line of an ascii PLY holds six tokens that parse (x y z and three colour columns)."""
    if not str(path).endswith(".ply") or not os.path.exists(path):
        return False
    with open(path) as f:
        for line in f:
            w = line.split(" ")
            try:
                float(w[0]), float(w[1]), float(w[2])
            except (ValueError, IndexError):
                continue
            try:
                float(w[3]), float(w[4]), float(w[5])
            except (ValueError, IndexError):
                return False
            return True
    return False


def get_args(argv=None, mullevel=False):
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt_path", type=str, default="", help="example: outputs/obj/2023-04-28/10-43-45/ckpt/epoch=7-step=64088.ckpt")
    p.add_argument("--test_files", nargs="*", default=["data/obj/mpeg/8iVLSF_910bit/boxer_viewdep_vox9.ply"])
    p.add_argument("--sequential", action="store_true")
    p.add_argument("--type", type=str, default="obj", choices=["obj", "kitti", "ford"])
    p.add_argument("--lidar_level", type=int, default=12)
    p.add_argument("--level_wise", action="store_true")
    p.add_argument("--cylin", action="store_true")
    p.add_argument("--spher", action="store_true")
    if not mullevel:
        p.add_argument("--spher_circle", action="store_true")
    p.add_argument("--preproc_path", type=str, default="")
    # additions
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--model", type=str, default=None, choices=[None, "EHEM", "OctAttention"])
    p.add_argument("--random_weights", type=int, default=None)
    p.add_argument("--out_dir", type=str, default=None)
    p.add_argument("--metrics", action="store_true", help="chamfer distance + D1 PSNR per frame (computed on the device)")
    p.add_argument("--normals", type=str, default=None, metavar="estimate|DIR",
                   help="with --metrics (EHEM): also the D2 (point-to-plane) PSNR, on normals estimated on the device (`estimate`) or read "
                        "from <DIR>/<sequence>/<frame>.ply as written by gene_normals.py")
    p.add_argument("--decodable", action="store_true",
                   help="OctAttention only: code under the decodable numeric profile (octattn/1d) so that decode.py can rebuild the stream; "
                        "EHEM streams are decodable already")
    # (absent from the namespace unless given, like the fields hand-made namespaces leave out: read it with getattr(args, "rate_report", False))
    p.add_argument("--rate_report", action="store_true", default=argparse.SUPPRESS,
                   help="per frame: ideal (cross-entropy), coded-table and coded bits per point on one more line, and <stream>.rate.json next to "
                        "the stream with the same figures per octree level (EHEM: per phase); the streams do not change")
    # (absent from the namespace unless given, like --rate_report: read it with distortion_request(args))
    p.add_argument("--distortion_report", nargs="?", const=True, type=parse_edges, default=argparse.SUPPRESS, metavar="EDGES",
                   help="per frame (EHEM): the D1 error per range ring and rho shell, split along r / phi / theta, on one more line and in "
                        "<stream>.dist.json next to the stream (the line: MSE and shares of the direction with the larger MSE, as D1's mseF takes it, "
                        "and the largest error of both directions); EDGES = comma-separated ring edges from 0 (default: 0,5,10,15,20,30,40,60,80 m "
                        "for kitti, x 1000 for ford); the streams do not change")
    # (absent from the namespace unless given: read it with rings_request(args))
    p.add_argument("--rate_rings", nargs="?", const=True, type=parse_ring_edges, default=argparse.SUPPRESS, metavar="EDGES",
                   help="per frame (EHEM): ideal bits per leaf of every range ring on one more line, and <stream>.rings.json next to the stream "
                        "with ideal / coded-table bits and leaves per ring and rho shell (every node's bits shared equally among the points "
                        "below it); EDGES as for --distortion_report, with the same defaults; implies the rate kernels; the streams do not change")
    # (absent from the namespace unless given: read it with depth_request(args))
    p.add_argument("--depth_report", nargs="?", const=True, type=parse_depth_report, default=argparse.SUPPRESS, metavar="K[:EDGES]",
                   help="per frame (EHEM): for every truncation depth k = 0 .. K (default 4) the ideal bits per point of octree levels 1 .. D - k "
                        "and the D1 PSNR of the cloud they describe on one more line, and <stream>.depth.json next to the stream with both per "
                        "range ring and rho shell (what decode_ehem*.py --lod k would write); EDGES as for --rate_rings, with the same defaults; "
                        "implies the rate kernels; the streams do not change")
    # (absent from the namespace unless given, like --rate_report: read them with temper_request(args))
    p.add_argument("--temper", action="store_true", default=argparse.SUPPRESS,
                   help="EHEM: code every (octree level, phase) under the inverse temperature - out of a grid of 25 from 0.354 to 2.83 - that "
                        "costs the fewest ideal bits on this frame, when that saves more than the byte its index costs; the stream's name gains "
                        "`_temper`, its side-info file the grid and the indices, and decode_ehem*.py reads them; one more line per frame")
    p.add_argument("--temper_report", action="store_true", default=argparse.SUPPRESS,
                   help="per frame: what --temper would choose and save in ideal bits, on one more line and in <stream>.temper.json next to the "
                        "stream with the bits of every group at every grid value; the streams do not change (with --temper: the same report, "
                        "columns included, of the choice that was coded)")
    # (absent from the namespace unless given: read it with ring_lod_request(args))
    p.add_argument("--ring_lod", type=parse_ring_lod, default=argparse.SUPPRESS, metavar="EDGES:DROPS",
                   help="EHEM, with --spher or --cylin: every range ring leaves out its own number of octree levels - EDGES as for "
                        "--distortion_report (the last ring open), DROPS one integer 0 .. 8 per ring, e.g. 0,10,25:2,1,0; the stream's name gains "
                        "`_ringlod`, its side-info file the drops and the integer thresholds, and decode_ehem*.py writes the centres of the "
                        "cells; one more line per frame (points snapped per drop, implied rows, leaves)")
    # (absent from the namespace unless given: read them with attr_request(args))
    p.add_argument("--attr", nargs="?", const=1, type=int, default=argparse.SUPPRESS, metavar="Q",
                   help="EHEM, --type kitti / ford: code the frame's reflectance as well - one 8-bit value per octree leaf, integer lifting "
                        "transform with step Q (1 .. 255, default 1: lossless on the leaf values) - into <stream>.attr next to the stream, "
                        "which decode_ehem*.py --attr reads; one more line per frame (bits, bits per point, with --metrics the reflectance "
                        "PSNR); the streams do not change")
    p.add_argument("--attr_scale", type=int, default=argparse.SUPPRESS, metavar="S",
                   help="with --attr: 8-bit units per unit of reflectance (default 255 for kitti, whose files hold 0 .. 1, and 1 for ford)")
    # (absent from the namespace unless given: read it with color_request(args))
    p.add_argument("--color", nargs="?", const=1, type=int, default=argparse.SUPPRESS, metavar="Q",
                   help="EHEM, --type obj: code the cloud's RGB as well - one colour per octree leaf, YCoCg-R and the integer lifting transform "
                        "of --attr on the three planes with step Q (1 .. 255, default 1: lossless on the leaf means) - into <stream>.color next "
                        "to the stream, which decode_ehem.py --color reads; one more line per frame (bits, bits per point, with --metrics "
                        "the luma and RGB PSNR); the streams do not change")
    # (absent from the namespace unless given: read them with sweep_request(args, "attr") / sweep_request(args, "color"))
    for layer, noun in (("attr", "reflectance"), ("color", "colour")):
        p.add_argument(f"--{layer}_sweep", nargs="?", const="", default=argparse.SUPPRESS, metavar="STEPS",
                       help=f"with --{layer}: what every step of a grid costs and loses on this frame's {noun}, from one pass over the octree - "
                            "STEPS comma-separated, strictly ascending, 1 .. 255, at most 16 (default 1,2,3,4,6,8,12,16,24,32,48,64,96,128,192,255); "
                            f"one more line per frame (per step: estimated bits per point, leaf PSNR) and <stream>.{layer}.sweep.json; the PSNR "
                            "is over leaf values, not the point-wise PSNR of --metrics; every other file keeps its bytes")
        p.add_argument(f"--{layer}_target", default=argparse.SUPPRESS, metavar="KIND=VALUE",
                       help=f"with --{layer} (without a Q): choose the step per frame from the sweep - psnr=DB: the largest step whose leaf PSNR is "
                            "at least DB; bpp=B: the smallest step whose estimated bits stay within B bits per point; linf=E: the largest step "
                            "whose largest leaf error is at most E; one more line per frame (target, chosen Q, met, estimated against written bits)")
    # (absent from the namespace unless given: read it with chunk_request(args))
    p.add_argument("--chunk", nargs="?", const=native.CHUNK_DEFAULT, type=int, default=argparse.SUPPRESS, metavar="N",
                   help="with --attr or --color: write the layer's file in its version 2 - every payload in chunks of N symbols (64 .. 2^20, "
                        "default 4096), each an independently terminated range-coder stream, coded and decoded all at once on the device; "
                        "decode_ehem*.py take the version from the file; file names and the per-frame lines do not change")
    p.add_argument("--host_transform", action="store_true",
                   help="strict identity with the reference from the frame on: the coordinate transform + quantiser run in numpy float32 on the "
                        "host exactly as data_preprocess.py:42-70 does (the device transform is more accurate, hence not bit-identical); "
                        "also SCP_XFORM=numpy")
    return p.parse_args(argv)


def expand_files(specs):
    out = []
    for s in specs:
        if os.path.isdir(s):
            out += sorted(glob.glob(os.path.join(s, "**", "*.bin"), recursive=True) + glob.glob(os.path.join(s, "**", "*.ply"), recursive=True))
        elif "*" in s:
            out += sorted(glob.glob(s))
        else:
            out.append(s)
    return out


MVUB_NAMES = ("andrew10", "david10", "phil10", "phil9", "ricardo10", "ricardo9", "sarah10")   # data_preprocess.py:242


def obj_ints(xyz, name, dev):
    """`--type obj` (encode_dataset.py:69-77 -> proc_pc defaults, data_preprocess.py:13-70): optional MVUB axis swap, offset = per-axis
    minimum, qs = 1, round half to even.  float32 subtraction then the float64 round of numpy, as index plumbing on the device."""
    p = torch.from_numpy(np.ascontiguousarray(xyz[:, :3], np.float32)).to(dev)
    if any(m in name for m in MVUB_NAMES):
        p = torch.stack((p[:, 0], p[:, 2], -p[:, 1]), 1)
    off = p.min(0)[0]
    return torch.round((p - off).double()).to(torch.int32).contiguous(), [float(v) for v in off.cpu()]


def refuse_unsupported(args, name, mullevel):
    """Flag combinations the reference accepts on its command line but cannot execute (or executes wrongly) are refused loudly
    instead of silently encoding something else."""
    if getattr(args, "spher_circle", False):
        raise native.ScpError("--spher_circle: the reference passes circle= to proc_pc, which has no such parameter "
                              "(encode_dataset_ehem.py:159-169 -> TypeError); there is no behaviour to reproduce")
    if name == "OctAttention" and args.level_wise and not mullevel:
        raise native.ScpError("--level_wise with OctAttention in encode.py stacks the padded per-level tables without removing the 1023 "
                              "pad rows (encode.py:59), so symbols are coded with the wrong rows; encode_mullevel.py has the fixed form "
                              "(encode_mullevel.py:60) - use it")
    if name == "OctAttention" and args.preproc_path:
        raise native.ScpError("--preproc_path with OctAttention is not supported (records are rebuilt on the device from the frame)")
    if name == "OctAttention" and args.metrics:
        raise native.ScpError("--metrics is available for the EHEM encoders only")
    if getattr(args, "normals", None) and (name == "OctAttention" or not args.metrics):
        raise native.ScpError("--normals adds the D2 PSNR to --metrics, which the EHEM encoders have: give --metrics as well, with an EHEM model")
    if temper_request(args)[0] == "code" and name == "OctAttention":
        raise native.ScpError("--temper is available for the EHEM encoders only: OctAttention's decodable profile decodes one node per step, and "
                              "a tempered form of it is not part of this library (--temper_report measures what it would save)")
    if ring_lod_request(args) is not None:
        if name == "OctAttention":
            raise native.ScpError("--ring_lod is available for the EHEM encoders only: OctAttention's decoder has no forced rows")
        if args.type == "obj":
            raise native.ScpError("--ring_lod cuts rings by the range from a LiDAR sensor at the origin: --type obj has none")
        if not (args.spher or args.cylin):
            raise native.ScpError("--ring_lod: Cartesian coordinates have no radial axis to cut rings on - encode with --spher or --cylin")
        if args.preproc_path:
            raise native.ScpError("--ring_lod with --preproc_path: the record files hold a finished octree, and the option snaps the points "
                                  "before the tree is built")
    chunk_request(args)
    sweep_request(args, "attr")
    sweep_request(args, "color")
    if attr_request(args)[0] is not None:
        if name == "OctAttention":
            raise native.ScpError("--attr is available for the EHEM encoders only: the OctAttention readers keep no reflectance and their "
                                  "decoders return no leaf list to hang it on")
        if args.type == "obj":
            raise native.ScpError("--attr codes a LiDAR frame's reflectance: --type obj files have points only")
        if args.preproc_path:
            raise native.ScpError("--attr with --preproc_path: the record files hold a finished octree and no points, so there is nothing to "
                                  "average per leaf")
        if ring_lod_request(args) is not None:
            raise native.ScpError("--attr with --ring_lod: the leaves of such a tree are snapped cells of mixed sizes, and an attribute layer "
                                  "for them is not part of this library")
    if color_request(args) is not None:
        if name == "OctAttention":
            raise native.ScpError("--color is available for the EHEM encoders only: the OctAttention decoders return no leaf list to hang "
                                  "a colour on")
        if args.type != "obj":
            raise native.ScpError(f"--color codes the RGB of an object cloud: --type {args.type} frames have no colour - their reflectance is "
                                  "what --attr codes")
        if args.preproc_path:
            raise native.ScpError("--color with --preproc_path: the record files hold a finished octree and no points, so there is nothing to "
                                  "average per leaf")
        if not mullevel:
            for f in expand_files(args.test_files):
                if not ply_has_colors(f):
                    raise native.ScpError(f"--color: {f} has no colour columns (an ascii PLY with x y z red green blue per point is expected)")
    want_dist, dist_edges = distortion_request(args)
    if want_dist:
        if name == "OctAttention":
            raise native.ScpError("--distortion_report is available for the EHEM encoders only (like --metrics: the OctAttention encoders "
                                  "keep no reconstructed cloud)")
        if args.type == "obj":
            raise native.ScpError("--distortion_report splits the error in the frame of a LiDAR sensor at the origin: --type obj has none")
        if args.preproc_path:
            raise native.ScpError("--distortion_report with --preproc_path: no geometry of the frame is built there, only its records are coded")
        if dist_edges is None:
            from . import metrics
            metrics.default_edges(args.type)
    want_rings, ring_edges = rings_request(args)
    if want_rings:
        if name == "OctAttention":
            raise native.ScpError("--rate_rings is available for the EHEM encoders only (like --distortion_report: the OctAttention encoders "
                                  "keep no reconstructed cloud)")
        if args.type == "obj":
            raise native.ScpError("--rate_rings bins the points by their range from a LiDAR sensor at the origin: --type obj has none")
        if args.preproc_path:
            raise native.ScpError("--rate_rings with --preproc_path: no geometry of the frame is built there, only its records are coded")
        if ring_edges is None:
            from . import metrics
            metrics.default_edges(args.type)
    want_depth, _, depth_edges = depth_request(args)
    if want_depth:
        if name == "OctAttention":
            raise native.ScpError("--depth_report is available for the EHEM encoders only (like --rate_rings: the OctAttention encoders "
                                  "keep no reconstructed cloud)")
        if args.type == "obj":
            raise native.ScpError("--depth_report bins the points by their range from a LiDAR sensor at the origin: --type obj has none")
        if args.preproc_path:
            raise native.ScpError("--depth_report with --preproc_path: no geometry of the frame is built there, only its records are coded")
        if depth_edges is None:
            from . import metrics
            metrics.default_edges(args.type)
    if args.type == "obj" and (args.spher or args.cylin or mullevel and name != "OctAttention"):
        raise native.ScpError("--type obj is Cartesian and single-level in the reference (proc_pc defaults); drop --spher/--cylin/mullevel")
    if args.sequential and name != "OctAttention":
        raise native.ScpError("--sequential is an OctAttention mode (encode.py:38-41)")
    decodable = getattr(args, "decodable", False)
    if decodable and name != "OctAttention":
        raise native.ScpError("--decodable is an OctAttention option: EHEM streams are decodable already")
    if decodable and mullevel:
        raise native.ScpError("--decodable: multi-level OctAttention streams (encode_mullevel.py) have no decoder; use encode.py")
    if decodable and args.sequential:
        raise native.ScpError("--decodable with --sequential: each node's window slides, so a decoder has no cache to keep")


def spawn_ranks(n, argv0, argv):
    """`--gpus N` outside torchrun: start N ranks (one per GPU) as a child launcher and hand back its exit code.  Runs before
    anything touches the GPU."""
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), argv0] + list(argv)
    return subprocess.call(cmd)


def normals_file(root, ori):
    """The file gene_normals.py writes for the original file `ori`: `<root>/<sequence>/<frame>.ply`, the sequence being the third path
    component from the end (KITTI: <sequence>/velodyne/<frame>.bin; gene_normals.py:36-39)."""
    parts = str(ori).split("/")
    return os.path.join(root, parts[-3] if len(parts) >= 3 else "", Path(ori).stem + ".ply")


def frame_normals(source, ori, x_dev):
    """`--normals`: one normal per input point, float32 values on the device.  `estimate`: the device estimator with gene_normals.py's
    parameters, rounded to the float32 its file would carry - so both sources give the same D2.  Otherwise the file of `normals_file`,
    whose points must be the frame's, in the frame's order."""
    from . import metrics
    if source == "estimate":
        return metrics.estimate_normals(x_dev).float()
    path = normals_file(source, ori)
    if not os.path.exists(path):
        raise native.ScpError(f"--normals {source}: no {path} for {ori} (gene_normals.py --ori_dir ... --out_dir {source} writes it)")
    pts, nrm = pointCloud.load_ply_normals(path)
    if pts.shape[0] != x_dev.shape[0] or not np.array_equal(pts, x_dev.cpu().numpy()):
        raise native.ScpError(f"{path} does not hold the points of {ori} in its order: normals belong to points by position")
    return torch.from_numpy(nrm).to(x_dev.device)


def gene_normals_main(argv=None):
    """Drop-in for data_preproc/gene_normals.py: for every KITTI `.bin` matching `--ori_dir` (a glob; `--parts i/n` takes the i-th of n
    slices) write `<out_dir>/<sequence>/<frame>.ply`, ascii x y z nx ny nz declared float32, with normals from the device estimator
    (radius 1.0, at most 30 neighbours, turned towards the sensor at the origin) where the reference calls open3d."""
    from . import metrics
    p = argparse.ArgumentParser()
    p.add_argument("--ori_dir", type=str, required=True)
    p.add_argument("--out_dir", type=str, required=True)
    p.add_argument("--parts", type=str, default="-1/-1")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise native.ScpError("gene_normals needs an MI355X: the normal estimator has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    native.lib()
    files = sorted(glob.glob(args.ori_dir))
    part, total = (0, 1) if args.parts.startswith("-1") else (int(args.parts.split("/")[0]), int(args.parts.split("/")[1]))
    start, end = len(files) * part // total, len(files) * (part + 1) // total
    written = []
    for i, ori in enumerate(files[start:end]):
        print(f"part {part}/{total}: {i}/{end - start}")
        out = normals_file(args.out_dir, ori)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        pc = pointCloud.loadbin(ori)[0]
        nrm = metrics.estimate_normals(torch.from_numpy(np.ascontiguousarray(pc, np.float32)).to(dev))
        pointCloud.write_ply_normals(out, pc, nrm.float().cpu().numpy())
        written.append(out)
    return written


def frame_attr(enc, path, xyz, res, dev, Q, scale, want_psnr, chunk=None, steps=None, target=None):
    """--attr: the reflectance column of the frame file `path` through FrameEncoder.encode_attr, on the octree `enc` has just coded ->
    encode_attr's report with `bytes` (the attribute file) and, with want_psnr, `psnr` / `mse_ab` / `mse_ba` (attr.reflectance_psnr
    of the cloud decode_ehem*.py --attr will write: the kept leaves through the decoder's own de-quantiser, with the decoded values).
    steps / target: sweep_request's - the step from the target, and with steps alone the table of FrameEncoder.attr_sweep as `sweep`."""
    from . import attr
    from .decoder import dequantise_leaves, shell_qs
    refl = pointCloud.pcread(path)[1]
    if refl is None or len(refl) != len(xyz):
        raise native.ScpError(f"--attr: {path} has no reflectance column (KITTI / Ford .bin frames hold x y z r)")
    x_dev = torch.from_numpy(np.ascontiguousarray(xyz[:, :3], np.float32)).to(dev)
    r_dev = torch.from_numpy(np.ascontiguousarray(refl, np.float32).reshape(-1)).to(dev)
    data, rep = enc.encode_attr(x_dev, r_dev, Q, scale, chunk=chunk, target=target, steps=steps if target is not None else None)
    if steps is not None and target is None:
        rep["sweep"] = enc.attr_sweep(x_dev, r_dev, scale, steps)
    rep["bytes"] = data
    if want_psnr:
        qs = shell_qs(enc.data_type, enc.lidar_level, enc.mullevel)
        pts = [dequantise_leaves(lv.long(), q, b, float(res["z_offset"]), enc.spher, enc.cylin, enc.data_type)
               for lv, q, b in zip(enc.attr_leaves(), qs, res.get("bin_nums", [res["bin_num"]]))]
        rep.update(attr.reflectance_psnr(x_dev, r_dev, torch.cat(pts), torch.cat(rep["decoded"]), rep["scale"]))
    return rep


def frame_color(enc, path, xyz, q, res, dev, Q, want_psnr, chunk=None, steps=None, target=None):
    """--color: the colour columns of the object file `path` through FrameEncoder.encode_color, on the octree `enc` has just coded from the
    integers q -> encode_color's report with `bytes` (the colour file) and, with want_psnr, color.color_psnr of the cloud
    decode_ehem.py --color will write (the leaves through the decoder's own de-quantiser, with the decoded colours) against the
    file's points (MVUB files: in the swapped axes the stream is coded in).  steps / target: as for frame_attr."""
    from . import color, metrics
    rgb = pointCloud.pcread(path, "rgb")[1]
    if rgb is None or len(rgb) != len(xyz):
        raise native.ScpError(f"--color: {path} has no colour columns (an ascii PLY with x y z red green blue per point is expected)")
    c_dev = color.point_colors(torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).to(dev))
    data, rep = enc.encode_color(q, c_dev, Q, chunk=chunk, target=target, steps=steps if target is not None else None)
    if steps is not None and target is None:
        rep["sweep"] = enc.color_sweep(q, c_dev, steps)
    rep["bytes"] = data
    if want_psnr:
        x = torch.from_numpy(np.ascontiguousarray(xyz[:, :3], np.float32)).to(dev)
        if any(m in path for m in MVUB_NAMES):
            x = torch.stack((x[:, 0], x[:, 2], -x[:, 1]), 1).contiguous()
        qd = res["quant"][0]
        pts = metrics.dequantize(enc.attr_leaves()[0].long(), qd["qs"], qd["offset"], spher=False, cylin=False)
        rep.update(color.color_psnr(x, c_dev, pts, rep["decoded"][0]))
    return rep


def sweep_lines(layer, rep, path, want_table):
    """The lines and the file of --<layer>_sweep / --<layer>_target for a frame whose layer file is `path`: with a target one line (the
    target, the chosen Q, met, estimated against written bits); with want_table one line (per step Q: estimated bits per point, leaf
    PSNR) and `<path>.sweep.json`.  The PSNR is over leaf values - what the layer codes against what it returns."""
    table = rep.get("sweep")
    if table is None:
        return
    if "target" in rep:
        row = table["rows"][[r["Q"] for r in table["rows"]].index(rep["chosen_Q"])]
        print(f"{layer} target, chosen Q, met, estimated / written bits :", "%s=%g" % rep["target"], rep["chosen_Q"], rep["met"], row["est_bits"],
              rep["bits"])
    if want_table:
        n = max(table["points"], 1)
        print(f"{layer} sweep Q:est bpp:leaf PSNR (over leaf values, not the point-wise PSNR of --metrics) :",
              *["%d:%.4f:%.2f" % (r["Q"], r["est_bits"] / n, r["psnr"]) for r in table["rows"]])
        extra = {k: rep[k] for k in ("target", "chosen_Q", "met") if k in rep}
        with open(path + ".sweep.json", "w") as f:
            json.dump(dict(table, layer=layer, psnr_over="leaf values", bits=rep["bits"], **extra), f, indent=1)


class Prefetch:
    """File reads (and the ascii PLY parse) one frame ahead on a reader thread, so the launch thread only enqueues GPU work.
    `post` (strict-identity mode: the host transform + quantiser) runs on the reader thread too; get() then returns (xyz, post(xyz))."""

    def __init__(self, files, depth=2, post=None):
        from concurrent.futures import ThreadPoolExecutor
        self.files = files
        self.pool = ThreadPoolExecutor(max_workers=1)
        self.depth = depth
        self.futs = {}
        self.next = 0
        self.post = post

    def _read(self, path):
        xyz = pointCloud.ptread(path)
        return xyz if self.post is None else (xyz, self.post(xyz))

    def get(self, k):
        while self.next < len(self.files) and self.next <= k + self.depth:
            self.futs[self.next] = self.pool.submit(self._read, self.files[self.next][1])
            self.next += 1
        return self.futs.pop(k).result()


def main(argv=None, mullevel=False):
    import sys
    args = get_args(argv, mullevel)
    rank, world, local = D.env_rank()
    if args.gpus > 1 and world == 1 and "RANK" not in os.environ:
        script = os.path.abspath(sys.argv[0])
        raise SystemExit(spawn_ranks(args.gpus, script, sys.argv[1:] if argv is None else argv))
    rank, world, local = D.init()
    if not torch.cuda.is_available():
        raise native.ScpError("encode needs an MI355X: the SCP hot path has no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    native.lib()
    D.pin_rank_threads(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))

    from .models import EHEM, OctAttention
    cfg = load_cfg(args.ckpt_path, args.model)
    name = cfg.model.class_name
    refuse_unsupported(args, name, mullevel)
    rate_report = getattr(args, "rate_report", False)
    temper, temper_report = temper_request(args)
    want_dist, dist_edges = distortion_request(args)
    want_rings, ring_edges = rings_request(args)
    want_depth, depth_drop, depth_edges = depth_request(args)
    attr_q, attr_scale = attr_request(args)
    color_q = color_request(args)
    chunk = chunk_request(args)
    (attr_steps, attr_target), (color_steps, color_target) = sweep_request(args, "attr"), sweep_request(args, "color")
    cls = OctAttention if name == "OctAttention" else EHEM
    if args.random_weights is not None or not args.ckpt_path:
        from .weights import fill_weights
        model = fill_weights(cls(cfg), args.random_weights or 0)
    else:
        model = cls.load_from_checkpoint(args.ckpt_path, cfg=cfg)
    model = model.to(dev).eval()

    if args.out_dir:
        out_root = args.out_dir.rstrip("/") + "/"
    else:
        root = args.ckpt_path.split("ckpt")[0] if args.ckpt_path else "./"
        out_root = root + "test_output" + (args.ckpt_path.split("ckpt")[1][:-1] if args.ckpt_path else "") + "/"
    os.makedirs(out_root, exist_ok=True)

    files = expand_files(args.test_files)
    combine = len(files) > 1
    obj = args.type == "obj"
    if name == "OctAttention":
        mul = mullevel and args.spher and not obj       # encode_dataset_mullevel.py:76: the three-shell form exists for --spher
        enc = OctAttnFrameEncoder(model, args.type, args.lidar_level, spher=args.spher and not obj, cylin=args.cylin and not obj, device=dev,
                                  mullevel=mul, level_wise=args.level_wise and mullevel, named=mullevel,
                                  host_transform=True if args.host_transform else None, decodable=args.decodable, rate=rate_report, temper=temper)
    else:
        enc = FrameEncoder(model, args.type, args.lidar_level, spher=args.spher, cylin=args.cylin, mullevel=mullevel, device=dev,
                           host_transform=True if args.host_transform else None, rate=rate_report or want_rings or want_depth,
                           rate_rows=want_rings or want_depth, temper=temper, ring_lod=ring_lod_request(args))
    if temper_report:
        enc.temper_sums = True                 # the columns of <stream>.temper.json, under --temper as well

    mine = D.shard(files, rank, world)
    # fast path: frames are enqueued with encode_async (stage G on a side stream, two model lanes, range coder on a worker thread)
    # and finished three frames later - what bench.py measures.  Flows that need the frame's octree after the encode (--metrics, --distortion_report,
    # --rate_rings, --depth_report),
    # come from record files, or run the one-window-per-node mode stay on the synchronous call.
    pipelined = not (args.preproc_path or args.metrics or want_dist or want_rings or want_depth or args.sequential or obj or attr_q is not None)
    DEPTH = 3
    host_ints = enc.host_ints if (pipelined and name != "OctAttention" and enc.host_transform) else None
    reader = Prefetch(mine, post=host_ints)
    pending = []
    sums = [0.0, 0.0, 0.0, 0.0, 0.0] + ([0.0] if args.normals else [])      # --normals: one more number in the reduced summary
    rate_sums = [0.0, 0.0, 0.0, 0]            # --rate_report: this rank's own frames (the reduced summary stays as it is)
    last_done = [time.time()]

    def stem_of(cur):
        return (cur.split("/")[-2] + Path(cur).stem) if (args.type == "kitti" and name != "OctAttention" and "/" in cur.rstrip("/")
                                                          and len(cur.split("/")) >= 2) else Path(cur).stem

    def report(cur, res, t_submit, dist=None, drep=None, rrep=None, lrep=None, arep=None, crep=None):
        now = time.time()
        elapsed = now - max(last_done[0], t_submit)      # wall time this frame added to the run (frames overlap in the pipeline)
        last_done[0] = now
        outfile = enc.outfile(out_root + stem_of(cur), res)
        with open(outfile, "wb") as f:
            f.write(res["bytes"])
        if name != "OctAttention":
            torch.save(torch.Tensor(res["pos_mm"].astype(np.float32)), outfile + ".dat")     # encode.py:150
            write_sidecar(outfile, enc, res, name)
        elif args.decodable:
            write_sidecar(outfile, enc, res, name)                                            # what decode.py reads besides the stream
        print("outputfile                  :", outfile)
        print("time(s)                     :", elapsed)
        print("pt num                      :", res["n_points"])
        print("oct num                     :", res["n_nodes"])
        print("total binsize               :", res["bits"])
        print("bit per oct                 :", res["bits"] / res["n_nodes"])
        print("bit per pixel               :", res["bpp"])
        if dist:
            print("chamfer distance            :", dist["chamfer"])
            print("PSNR (D1)                   :", dist["psnr"])
            if "psnr_d2" in dist:
                print("PSNR (D2)                   :", dist["psnr_d2"])
                sums[5] += dist["psnr_d2"]
        if rate_report:
            rate = res["rate"]
            print("bpp ideal / table / coded   :", rate["bpp_ideal"], rate["bpp_table"], res["bpp"])
            with open(outfile[:-len(".bin")] + ".rate.json", "w") as f:
                json.dump(dict(rate, model=name, profile=enc.profile_string(), lidar_level=args.lidar_level, bits=res["bits"],
                               n_points=res["n_points"], n_nodes=res["n_nodes"]), f, indent=1)
            rate_sums[0] += rate["bpp_ideal"]; rate_sums[1] += rate["bpp_table"]; rate_sums[2] += res["bpp"]; rate_sums[3] += 1
        if temper:
            tp = res["temper"]
            print("temper bpp unit / chosen, side bits, moved :", tp["ideal_bits_unit"] / res["n_points"], tp["ideal_bits_chosen"] / res["n_points"],
                  tp["side_bits"], tp["moved"])
            if temper_report:
                with open(outfile[:-len(".bin")] + ".temper.json", "w") as f:
                    json.dump(dict(tp, model=name, profile=enc.profile_string(), lidar_level=args.lidar_level, bits=res["bits"],
                                   n_points=res["n_points"], n_nodes=res["n_nodes"]), f, indent=1)
        if res.get("ring_lod"):
            rl = res["ring_lod"]
            print("ring LOD snapped per drop, implied rows, leaves :", rl["snapped"], rl["implied_rows"], sum(rl["leaves"]))
        if arep:
            with open(outfile + ".attr", "wb") as f:
                f.write(arep["bytes"])
            print("attr bits, bits per point" + (", PSNR (refl) :" if "psnr" in arep else "  :"), arep["bits"], arep["bits_per_point"],
                  *([arep["psnr"]] if "psnr" in arep else []))
            sweep_lines("attr", arep, outfile + ".attr", attr_steps is not None)
        if crep:
            with open(outfile + ".color", "wb") as f:
                f.write(crep["bytes"])
            print("color bits, bits per point" + (", PSNR (Y), PSNR (RGB) :" if "psnr_y" in crep else "  :"), crep["bits"], crep["bits_per_point"],
                  *([crep["psnr_y"], crep["psnr_rgb"]] if "psnr_y" in crep else []))
            sweep_lines("color", crep, outfile + ".color", color_steps is not None)
        if drep:
            worse = max((drep["a_to_b"]["total"], drep["b_to_a"]["total"]), key=lambda e: e["mse"])     # the direction D1's mseF takes
            share = [worse[k] / worse["mse"] if worse["mse"] > 0 else 0.0 for k in ("mse_r", "mse_phi", "mse_theta")]
            print("D1 mse, r/phi/theta, max    :", worse["mse"], *share, max(drep["a_to_b"]["total"]["max"], drep["b_to_a"]["total"]["max"]))
            with open(outfile[:-len(".bin")] + ".dist.json", "w") as f:
                json.dump(dict(drep, lidar_level=args.lidar_level, type=args.type, n_points=res["n_points"]), f, indent=1)
        if rrep:
            print("ideal bits per leaf by ring :", *[e["ideal_bits_per_leaf"] for e in rrep["rings"]])
            with open(outfile[:-len(".bin")] + ".rings.json", "w") as f:
                json.dump(dict(rrep, lidar_level=args.lidar_level, type=args.type, n_points=res["n_points"], bits=res["bits"]), f, indent=1)
        if lrep:
            print("depth k: ideal bpp, D1 PSNR :", *[v for lv in lrep["levels"] for v in (lv["rate"]["total"]["ideal_bits_per_point"], lv["d1"]["psnr"])])
            with open(outfile[:-len(".bin")] + ".depth.json", "w") as f:
                json.dump(dict(lrep, lidar_level=args.lidar_level, type=args.type, n_points=res["n_points"], bits=res["bits"]), f, indent=1)
        sums[0] += res["bpp"]; sums[1] += dist["psnr"] if dist else 0.0; sums[2] += dist["chamfer"] if dist else 0.0
        sums[3] += elapsed; sums[4] += 1

    if rank == 0:
        print("Encoding with", name)
    def fetch(k):
        d = reader.get(k)
        return d if host_ints is not None else (d, None)

    # the front part (stage G + window plans) of frame k + 1 runs on the encoder's front thread while this thread enqueues the model part of
    # frame k (FrameEncoder.front_async: the front part blocks its host thread for most of a frame time)
    front_ahead = pipelined and hasattr(enc, "front_async")
    nxt = None
    for k, (i, cur) in enumerate(mine):
        print("Encoding ", cur, i, "/", len(files))
        if front_ahead:
            xyz, ints, fr = nxt if nxt is not None else (*fetch(k), None)
            if fr is None:
                fr = enc.front_async(xyz, ints)
            nxt = None
            if k + 1 < len(mine):
                x2, i2 = fetch(k + 1)
                nxt = (x2, i2, enc.front_async(x2, i2))
        else:
            xyz, ints = fetch(k)
        t0 = time.time()
        if pipelined:
            pending.append((cur, enc.encode_async(xyz, ints, front=fr) if front_ahead else enc.encode_async(xyz), t0))
            if len(pending) > DEPTH:
                c0, h0, ts = pending.pop(0)
                report(c0, enc.finish(h0), ts)
            continue
        dist = drep = rrep = lrep = arep = crep = None
        if args.preproc_path:
            # encode_dataset_ehem.py:149-157 / ..._mullevel.py:147-155: records + meta written by the test-set generator
            pp = args.preproc_path + ((cur.split("/")[-2] + Path(cur).stem) if args.type == "kitti" else Path(cur).stem)
            meta = np.load(pp + "_meta.npy")
            recs = [np.load(pp + sfx + ".npy") for sfx in (("_0_0", "_0_1", "_1") if mullevel else ("",))]
            res = enc.encode_records(recs, float(meta[0]), float(meta[2]) if len(meta) > 2 else 0.0, len(xyz))
        elif obj:
            q, off = obj_ints(xyz, cur, dev)
            res = enc.encode_ints(q, 0, len(xyz), sequential=args.sequential) if name == "OctAttention" else enc.encode_ints([q], 0, 0.0, len(xyz))
            res["quant"] = [dict(qs=[1.0, 1.0, 1.0], offset=off)]     # the sidecar is the only carrier of the per-axis minimum
            if color_q is not None:
                crep = frame_color(enc, cur, xyz, q, res, dev, color_q, args.metrics, chunk, color_steps, color_target)
        elif name == "OctAttention":
            res = enc.encode(xyz, sequential=args.sequential)
        else:
            res = enc.encode(xyz)
            if args.metrics or want_dist or want_rings or want_depth:
                x_dev = torch.from_numpy(np.ascontiguousarray(xyz[:, :3], np.float32)).to(dev)
            if args.metrics:
                dist = enc.distortion(x_dev, normals=frame_normals(args.normals, cur, x_dev) if args.normals else None)
            if want_dist:
                drep = enc.distortion_report(x_dev, dist_edges)
            if want_rings:
                rrep = enc.ring_rate(x_dev, ring_edges)
            if want_depth:
                lrep = enc.depth_report(x_dev, depth_drop, depth_edges)
            if attr_q is not None:
                arep = frame_attr(enc, cur, xyz, res, dev, attr_q, attr_scale, args.metrics, chunk, attr_steps, attr_target)
        report(cur, res, t0, dist, drep, rrep, lrep, arep, crep)
    for c0, h0, ts in pending:
        report(c0, enc.finish(h0), ts)
    total = D.reduce_summary(sums, dev)
    m = D.summary_means(total)
    if rank == 0:
        print("sample number:", m["count"])
        print("times:", m["time"])
        print("bpp:", m["bpp"])
        if args.normals:
            print("PSNR_D2:", m["psnr_d2"])
        if rate_report and world == 1 and rate_sums[3]:
            print("bpp ideal / table / coded (mean):", *[v / rate_sums[3] for v in rate_sums[:3]])
        if combine and args.type in ("kitti", "ford"):
            tag = "mul" if mullevel else "same"
            out = (f"{tag} {args.lidar_level} {args.test_files} {args.ckpt_path}\nsample number: {m['count']}\ntimes: {m['time']}\n"
                   f"bpp: {m['bpp']}\nchamfer_dist: {m['chamfer']}\nPSNR: {m['psnr']}\n" + (f"PSNR_D2: {m['psnr_d2']}\n" if args.normals else "") + "\n")
            with open(f"test_results_{tag}_{args.type}_{args.lidar_level}.txt", "a") as f:
                f.write(out)
    D.finalize()
    return m


# ---------------------------------------------------------------------------------------------------------------- decode
def get_decode_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt_path", type=str, default="", help="example: outputs/obj/2023-04-28/10-43-45/ckpt/epoch=7-step=64088.ckpt")
    p.add_argument("--test_files", nargs="*", default=["data/obj/mpeg/8iVLSF_910bit/boxer_viewdep_vox9.ply"])
    p.add_argument("--preproc_path", type=str, default="")
    p.add_argument("--sequential_enc", action="store_true")
    p.add_argument("--level_wise", action="store_true")
    # additions
    p.add_argument("--random_weights", type=int, default=None)
    p.add_argument("--out_dir", type=str, default=None)
    p.add_argument("--lidar_level", type=int, default=None, help="overrides the side-info file / the reference's level-count rule")
    p.add_argument("--type", type=str, default=None, choices=[None, "obj", "kitti", "ford"])
    p.add_argument("--streams", type=_streams_arg, default=1,
                   help="decode this many files at a time in lockstep, one packed forward serving one level of each (1 .. 64; default 1: one "
                        "file after the other).  With more than one, the time printed per file is the total over the number of files")
    p.add_argument("--attr", action="store_true",
                   help="also decode <stream>.attr (written by encode*.py --attr) and write <stem>.attr.bin next to the .ply: float32 [U,4], "
                        "x y z r in the KITTI layout, rows in the order of the .ply; works with --streams (the attribute stage runs per file "
                        "after the geometry), not with --lod above 0")
    p.add_argument("--color", action="store_true",
                   help="also decode <stream>.color (written by encode.py --type obj --color) and write <stem>.color.ply next to the .ply: "
                        "x y z red green blue, rows in the order of the .ply; works with --streams (the colour stage runs per file after the "
                        "geometry), not with --lod above 0")
    p.add_argument("--lod", type=int, default=0, metavar="K",
                   help="preview: stop every tree after its level D - K and write the centres of the cells of size 2^K those levels describe "
                        "(what encode*.py --depth_report measures at k = K); 0 (default): the full decode.  A multi-level stream codes its "
                        "shells one after the other, so the first two are decoded in full - the range decoder has to pass them - and only "
                        "the last one stops early.  K <= the shallowest shell's depth - 1; not with --streams above 1")
    return p.parse_args(argv)


def get_decode_octattn_args(argv=None):
    """decode.py's flags (the reference's decode.py:157-172) plus the repository's additions."""
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt_path", type=str, default="", help="example: outputs/obj/2023-04-28/10-43-45/ckpt/epoch=7-step=64088.ckpt")
    p.add_argument("--test_files", nargs="*", default=["data/obj/mpeg/8iVLSF_910bit/boxer_viewdep_vox9.ply"])
    p.add_argument("--sequential_enc", action="store_true")
    p.add_argument("--level_wise", action="store_true")
    # additions
    p.add_argument("--random_weights", type=int, default=None)
    p.add_argument("--out_dir", type=str, default=None)
    p.add_argument("--lidar_level", type=int, default=None, help="checked against the side-info file")
    p.add_argument("--type", type=str, default=None, choices=[None, "obj", "kitti", "ford"])
    p.add_argument("--preproc_path", type=str, default="")
    p.add_argument("--streams", type=_streams_arg, default=1,
                   help="decode this many files at a time in lockstep, one model step serving one node of each (1 .. 64; default 1: one "
                        "file after the other).  With more than one, the time printed per file is the total over the number of files")
    return p.parse_args(argv)


def _streams_arg(v):
    n = int(v)
    if not 1 <= n <= 64:
        raise argparse.ArgumentTypeError(f"--streams {v}: 1 .. 64 expected")
    return n


def decode_octattn_main(argv=None):
    """Drop-in for the reference's decode.py (decodeOct): for every original file, its `<stem>.bin` (`find_stream`) written by
    `encode.py --decodable` is decoded (scp_amd/decoder.py: OctAttnFrameDecoder), checked against the record file `<stem>.npy` when it
    exists, and written as `<stem>.ply`.  The stream's side-info file carries the window length, level-wise flag, depth and profile;
    streams of the default profile, --sequential and multi-level streams are refused with the reason.  `--streams S` (S > 1) decodes
    the files S at a time in lockstep (decoder.decode_octattn_files): the same checks, files and printed lines per file."""
    from .decoder import decode_octattn_file, decode_octattn_files, read_sidecar
    args = get_decode_octattn_args(argv)
    if not torch.cuda.is_available():
        raise native.ScpError("decode needs an MI355X: the SCP hot path has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    native.lib()
    from .models import OctAttention
    cfg = load_cfg(args.ckpt_path, "OctAttention")
    if cfg.model.class_name != "OctAttention":
        raise native.ScpError("decode.py decodes OctAttention streams; EHEM streams: decode_ehem.py / decode_ehem_mullevel.py")
    if args.random_weights is not None or not args.ckpt_path:
        from .weights import fill_weights
        model = fill_weights(OctAttention(cfg), args.random_weights or 0)
    else:
        model = OctAttention.load_from_checkpoint(args.ckpt_path, cfg=cfg)
    model = model.to(dev).eval()
    if args.out_dir:
        out_root = args.out_dir.rstrip("/") + "/"
    else:
        root = args.ckpt_path.split("ckpt")[0] if args.ckpt_path else "./"
        out_root = root + "test_output" + (args.ckpt_path.split("ckpt")[1][:-1] if args.ckpt_path else "") + "/"
    files = expand_files(args.test_files)
    elapsed, results = 0.0, []

    def locate(ori):
        name, stem = find_stream(out_root, ori)
        binfile = out_root + name
        side = read_sidecar(binfile)
        if side is not None:     # the flags describe the stream; the side-info file is what it was coded with
            if args.sequential_enc != bool(side.get("sequential", False)) or args.level_wise != bool(side.get("level_wise", False)):
                print("note: --sequential_enc / --level_wise differ from the stream's side-info file; the side-info file wins")
            if args.lidar_level is not None and args.lidar_level != side.get("lidar_level"):
                raise native.ScpError(f"{binfile}: coded at lidar level {side.get('lidar_level')}, --lidar_level {args.lidar_level} given")
            if args.type is not None and args.type != side.get("type"):
                raise native.ScpError(f"{binfile}: coded as --type {side.get('type')}, --type {args.type} given")
        return binfile, stem

    def report(ori, stem, out, t):
        npy = (args.preproc_path.rstrip("/") + "/" + Path(ori).stem) if args.preproc_path else str(ori).rsplit(".")[0]
        if os.path.exists(npy + ".npy"):                       # the reference asserts every node against it (decode.py:99)
            want = np.load(npy + ".npy")[:, -1, 0]
            got = out["codes"][0].cpu().numpy().astype(np.int64)
            assert np.array_equal(got[:len(want)], want) and len(got) == len(want), f"decoded occupancy differs from {npy}.npy"
            print("checked against", npy + ".npy")
        print("decode succee,time:", t)
        print("oct len:", int(out["codes"][0].numel()))
        ply = out_root + stem + ".ply"
        pointCloud.write_ply_data(ply, out["points"].cpu().numpy())
        print(ply)
        results.append((ply, out))

    if args.streams > 1:
        # every stream is located and its side-info checked first; then the files are decoded `streams` at a time in lockstep
        found = [locate(ori) for ori in files]
        t0 = time.time()
        outs = decode_octattn_files([b for b, _ in found], model, streams=args.streams, device=dev)
        torch.cuda.synchronize()
        elapsed = time.time() - t0
        for i, (ori, (_, stem), out) in enumerate(zip(files, found, outs)):
            print(f"{i}/{len(files)}")
            report(ori, stem, out, elapsed / len(files))
    else:
        for i, ori in enumerate(files):
            print(f"{i}/{len(files)}")
            binfile, stem = locate(ori)
            t0 = time.time()
            out = decode_octattn_file(binfile, model, dev)
            torch.cuda.synchronize()
            t = time.time() - t0
            elapsed += t
            report(ori, stem, out, t)
    print(elapsed / max(len(files), 1))
    return results


def find_stream(out_root, ori):
    """The stream the encode CLIs wrote for the original file `ori`: `<stem>[_ringlod][_temper][_spher|_cylin]_<levels>_<bin_num>_<z_offset>.bin` with
    stem = `<sequence dir><frame>` for KITTI EHEM runs (encode.py:140-144 via the dataset's file name) or the plain file stem.  The
    reference takes the first name that merely CONTAINS the frame number (decode_ehem.py:206-214), which picks the wrong sequence's
    stream as soon as two sequences hold the same frame number; here the name must match exactly, and 0 or several candidates are
    an error.  Returns (file name, the stem that matched) - the stem names the decoder's `.ply`."""
    import re
    p = Path(ori)
    names = [f for f in os.listdir(out_root) if f.endswith(".bin")]
    tried = []
    for stem in ([p.parent.name + p.stem] if p.parent.name else []) + [p.stem]:
        pat = re.compile("^" + re.escape(stem) + r"((_ringlod)?(_temper)?(_spher|_cylin)?_\d+_-?\d+_-?\d+)?\.bin$")
        c = sorted(f for f in names if pat.match(f))
        if len(c) == 1:
            return c[0], stem
        if len(c) > 1:
            raise native.ScpError(f"{len(c)} streams match {ori} in {out_root}: {c}")
        tried.append(stem)
    raise native.ScpError(f"no stream for {ori} in {out_root} (looked for {tried})")


def decode_main(argv=None, mullevel=False):
    """Drop-in for decode_ehem.py:191-255 / decode_ehem_mullevel.py:209-277: for every original file, find its stream in the
    test_output directory (`find_stream`: the exact name the encoder wrote, sequence included), decode it with the side info of `extract_info`,
    check the occupancy codes against the `--preproc_path` record files when they exist (the reference asserts this window by
    window, decode_ehem.py:184), rebuild the points (DeOctree -> de-quantise -> spher2cart / cylin2cart) and write
    `<test_output>/<stream stem>.ply` (KITTI: `<sequence><frame>.ply`, so two sequences never overwrite each other).  `--streams S` (S > 1)
    decodes the files S at a time in lockstep (decoder.decode_files): the same checks, files and printed lines per file."""
    args = get_decode_args(argv)
    if not torch.cuda.is_available():
        raise native.ScpError("decode needs an MI355X: the SCP hot path has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    native.lib()
    from .models import EHEM
    cfg = load_cfg(args.ckpt_path, "EHEM")
    if cfg.model.class_name != "EHEM":
        raise native.ScpError("decode_ehem*.py decode EHEM streams; OctAttention streams written with --decodable: decode.py")
    if args.lod < 0:
        raise native.ScpError(f"--lod {args.lod}: 0 (the full decode) or the number of levels to leave out expected")
    if args.attr and args.lod:
        raise native.ScpError(f"--attr with --lod {args.lod}: a preview has cells, not leaves, and the attribute layer codes one value per leaf")
    if args.color and args.lod:
        raise native.ScpError(f"--color with --lod {args.lod}: a preview has cells, not leaves, and the weights of a cut tree are unknown to the decoder")
    if args.lod and args.streams > 1:
        raise native.ScpError("--lod with --streams above 1: the lockstep decoder decodes every level of every stream; decode previews one "
                              "file after the other (--streams 1)")
    if args.random_weights is not None or not args.ckpt_path:
        from .weights import fill_weights
        model = fill_weights(EHEM(cfg), args.random_weights or 0)
    else:
        model = EHEM.load_from_checkpoint(args.ckpt_path, cfg=cfg)
    model = model.to(dev).eval()
    if args.out_dir:
        out_root = args.out_dir.rstrip("/") + "/"
    else:
        root = args.ckpt_path.split("ckpt")[0] if args.ckpt_path else "./"
        out_root = root + "test_output" + (args.ckpt_path.split("ckpt")[1][:-1] if args.ckpt_path else "") + "/"
    files = args.test_files
    if files and os.path.isdir(files[0]):      # decode_ehem.py:202-203
        files = sorted(os.path.join(files[0], f) for f in os.listdir(files[0]) if f.endswith((".ply", ".bin")))
    else:
        files = expand_files(files)
    elapsed, results = 0.0, []
    outs = None
    if args.streams > 1:
        # every stream is located first; then the files are decoded `streams` at a time in lockstep (every side-info file checked before the
        # first is decoded), and the loop below reports them one by one
        from .decoder import decode_files
        found = [find_stream(out_root, ori) for ori in files]
        t0 = time.time()
        outs = decode_files([out_root + name for name, _ in found], model, args.streams, args.lidar_level, args.type, mullevel, dev)
        torch.cuda.synchronize()
        each = (time.time() - t0) / max(len(files), 1)
    for i, ori in enumerate(files):
        print(f"{i}/{len(files)}")
        if outs is not None:
            (name, stem), out, t = found[i], outs[i], each
            if args.attr:
                from .decoder import decode_attr
                decode_attr(out_root + name, out, mullevel)
            if args.color:
                from .decoder import decode_color
                decode_color(out_root + name, out, mullevel)
        else:
            name, stem = find_stream(out_root, ori)            # the stem that matched, not string surgery on the stream name
            binfile = out_root + name
            t0 = time.time()
            out = decode_file(binfile, model, args.lidar_level, args.type, mullevel, dev, lod=args.lod, attr=args.attr, color=args.color)
            torch.cuda.synchronize()
            t = time.time() - t0
        elapsed += t
        # the reference needs the record files (their length drives its loop and every window is asserted against them); here
        # they are an optional check
        npy = (args.preproc_path.rstrip("/") + "/" + Path(ori).stem) if args.preproc_path else str(ori).rsplit(".")[0]
        cands_npy = [npy + s + ".npy" for s in (("_0_0", "_0_1", "_1") if mullevel else ("",))]
        if not all(os.path.exists(c) for c in cands_npy) and args.preproc_path:
            alt = args.preproc_path.rstrip("/") + "/" + Path(ori).parent.name + Path(ori).stem       # kitti: <sequence><frame>
            cands_npy = [alt + s + ".npy" for s in (("_0_0", "_0_1", "_1") if mullevel else ("",))]
        if all(os.path.exists(c) for c in cands_npy):
            for codes, c in zip(out["codes"], cands_npy):
                want = np.load(c)[:, -1, 0]
                got = codes.cpu().numpy()[:len(want)]
                want = want[:len(got)] if args.lod else want          # --lod: the decoded levels only
                assert np.array_equal(got.astype(np.int64), want), f"decoded occupancy differs from {c}"
            print("checked against", ", ".join(cands_npy))
        print("decode succeeded, time:", t)
        print("oct len:", int(sum(len(c) for c in out["codes"])))
        print("avg dec time:", elapsed / (i + 1))
        ply = out_root + stem + ".ply"
        pointCloud.write_ply_data(ply, out["points"].cpu().numpy())
        print(ply)
        if args.attr:
            rows = np.concatenate([out["points"].cpu().numpy().astype(np.float32), out["reflectance"].cpu().numpy().reshape(-1, 1)], 1)
            rows.astype(np.float32).tofile(out_root + stem + ".attr.bin")
            print(out_root + stem + ".attr.bin")
        if args.color:
            pointCloud.write_ply_colors(out_root + stem + ".color.ply", out["points"].cpu().numpy(), out["colors"].cpu().numpy())
            print(out_root + stem + ".color.ply")
        results.append((ply, out))
    print(elapsed / max(len(files), 1))
    return results
