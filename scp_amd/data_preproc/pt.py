"""Point-cloud readers / writers of the encode path (drop-in for the input half of data_preproc/pt.py).

Only the formats the encode CLI touches: KITTI `.bin` (pt.py:190), ascii `.ply` (pt.py:224, the reference parses it line
by line and skips every line that does not start with three floats), the ascii PLY writer used for `_quant.ply`, and the
ascii PLY with normals that data_preproc/gene_normals.py leaves behind (x y z nx ny nz, declared float32) for the D2 PSNR.
The metrics themselves (chamfer, D1, D2) run on the device: scp_amd/metrics.py; no pc_error subprocess, no KD-tree.
"""
import os

import numpy as np


def loadbin(file):
    """KITTI: float32 [P,4] -> (xyz [P,3], reflectance [P,1])."""
    points = np.fromfile(file, dtype=np.float32).reshape(-1, 4)
    return points[:, 0:3], points[:, 3:4]


def loadply(filedir, color_format="geometry"):
    """ascii PLY: every line whose first three tokens parse as floats is a point (header lines fail the parse).  color_format "rgb": tokens
    3 .. 5 of those lines as well (pt.py:224-246) -> (xyz float32 [P,3], rgb float32 [P,3]); a point line with fewer than six tokens
    means the file has no colour columns, and the whole file falls back to (xyz, None).  Any other format returns (xyz, None)."""
    coords, colors = [], []
    want = color_format == "rgb"
    with open(filedir) as f:
        for line in f:
            w = line.split(" ")
            try:
                coords.append((float(w[0]), float(w[1]), float(w[2])))
            except (ValueError, IndexError):
                continue
            if want:
                try:
                    colors.append((float(w[3]), float(w[4]), float(w[5])))
                except (ValueError, IndexError):
                    want = False
    xyz = np.array(coords).astype("float32").reshape(-1, 3)
    return xyz, (np.array(colors).astype("float32").reshape(-1, 3) if want and color_format == "rgb" else None)


def pcread(path, color_format="geometry"):
    if not os.path.exists(path):
        raise Exception("no such file:" + path)
    if path.endswith(".ply"):
        return loadply(path, color_format)
    if path.endswith(".bin"):
        return loadbin(path)
    raise ValueError("unsupported point cloud format: " + path)


def ptread(path):
    return pcread(path, "geometry")[0]


def write_ply_data(filename, points):
    """ascii PLY with x y z float columns (what test_gene.py writes as `<name>_quant.ply`)."""
    points = np.asarray(points)
    with open(filename, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                % len(points))
        for p in points:
            f.write("%s %s %s\n" % (repr(float(p[0])), repr(float(p[1])), repr(float(p[2]))))


def write_ply_colors(filename, points, rgb):
    """ascii PLY with x y z as `write_ply_data` prints them, followed by uchar red green blue."""
    points, rgb = np.asarray(points), np.asarray(rgb)
    if rgb.shape != (len(points), 3) or points.ndim != 2 or points.shape[1] < 3:
        raise ValueError(f"points {points.shape} [n,3] and rgb {rgb.shape} [n,3] expected")
    with open(filename, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(points))
        for p, c in zip(points, rgb):
            f.write("%s %s %s %d %d %d\n" % (repr(float(p[0])), repr(float(p[1])), repr(float(p[2])), int(c[0]), int(c[1]), int(c[2])))


def write_ply_normals(filename, points, normals):
    """ascii PLY with x y z nx ny nz, every property declared `float32` (gene_normals.py:46-52 rewrites open3d's `double` header that
    way).  Values are rounded to float32 and written with the digits that read back to the same float32."""
    points, normals = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    if points.shape != normals.shape or points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points {points.shape} and normals {normals.shape} must both be [n,3]")
    with open(filename, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\n" % len(points))
        f.write("".join("property float32 %s\n" % c for c in ("x", "y", "z", "nx", "ny", "nz")) + "end_header\n")
        for row in np.hstack((points, normals)):
            f.write(" ".join(str(v) for v in row) + "\n")            # str(np.float32): the shortest text that reads back exactly


def load_ply_normals(filename):
    """-> (xyz float32 [n,3], normals float32 [n,3]) of an ascii PLY whose vertex lines hold x y z nx ny nz."""
    rows = []
    with open(filename) as f:
        for line in f:
            w = line.split()
            try:
                rows.append([float(t) for t in w[:6]])
            except ValueError:
                continue
            if len(rows[-1]) < 6:
                rows.pop()
    a = np.array(rows, dtype=np.float64).reshape(-1, 6).astype(np.float32)
    return a[:, :3].copy(), a[:, 3:].copy()
