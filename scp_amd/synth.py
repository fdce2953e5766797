"""Synthetic LiDAR frames (test-input spec of SURVEY.md Appendix G / §8d).

No dataset is available offline, so every parity test, fixture and bench line in this
repo uses this generator: a 64-beam x 1875-azimuth HDL-64-like sweep over a flat ground
plane plus uniformly distributed obstacles.  P = 120 000 points per frame.
"""
import numpy as np


def synth_frame(seed=0, beams=64, az=1875):
    """xyz float32 [beams*az, 3]; RNG numpy PCG64 (default_rng)."""
    rng = np.random.default_rng(seed)
    el = np.deg2rad(np.linspace(2.0, -24.8, beams))
    phi = np.linspace(0, 2 * np.pi, az, endpoint=False)
    E, P = np.meshgrid(el, phi, indexing="ij")
    r_ground = np.where(E < 0, 1.73 / np.maximum(np.sin(-E), 1e-6), 120.0)
    r_obj = rng.uniform(5, 80, size=E.shape)
    r = np.minimum(r_ground, r_obj) + rng.normal(0, 0.02, size=E.shape)
    r = np.clip(r, 2.0, 120.0)
    x = r * np.cos(E) * np.cos(P)
    y = r * np.cos(E) * np.sin(P)
    z = r * np.sin(E)
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)


def write_kitti_bin(path, xyz):
    """KITTI .bin layout: float32 [P,4] (x, y, z, reflectance=0)."""
    p = np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], 1).astype(np.float32)
    p.tofile(path)


def ford_like(xyz):
    """Ford-like frame: same cloud in integer millimetres (float32 values)."""
    return np.round(xyz.astype(np.float64) * 1000).astype(np.float32)


def synth_reflectance(xyz, seed=0):
    """A reflectance for the points of a frame, float32 [P] in [0, 1]: smooth in azimuth, an offset on the ground plane, noise of sigma
    0.03; rounded to multiples of 1/255, as KITTI files hold them.  It says nothing about the statistics of a real sensor."""
    rng = np.random.default_rng(seed)
    x, y, z = (xyz[:, i].astype(np.float64) for i in range(3))
    phi = np.arctan2(y, x)
    r = 0.35 + 0.15 * np.sin(2.0 * phi) + 0.08 * np.cos(5.0 * phi + 0.7) + np.where(z < -1.5, 0.2, 0.0) + rng.normal(0, 0.03, size=len(xyz))
    return (np.round(np.clip(r, 0.0, 1.0) * 255.0) / 255.0).astype(np.float32)


def write_kitti_bin4(path, xyz, refl):
    """KITTI .bin layout with the reflectance kept: float32 [P,4] (x, y, z, r)."""
    p = np.concatenate([np.asarray(xyz, np.float32)[:, :3], np.asarray(refl, np.float32).reshape(-1, 1)], 1).astype(np.float32)
    p.tofile(path)


def synth_object(seed=0, n=4096):
    """An object cloud as `--type obj` files hold them: int64 [n,3] distinct integer points on the surface of a bumpy sphere inside a 2^10
    cube (centre 512, radius 380 +- 60 in smooth bumps), in no particular order."""
    rng = np.random.default_rng(seed)
    out = np.zeros((0, 3), np.int64)
    while len(out) < n:
        d = rng.normal(size=(2 * n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = 380.0 + 40.0 * np.sin(5.0 * d[:, 0] + 1.0) * np.cos(4.0 * d[:, 1]) + 20.0 * np.sin(9.0 * d[:, 2] + 0.3)
        p = np.clip(np.round(512.0 + d * r[:, None]), 0, 1023).astype(np.int64)
        out = np.concatenate([out, p])
        out = out[np.sort(np.unique(out, axis=0, return_index=True)[1])]
    return np.ascontiguousarray(out[:n])


def synth_colors(xyz, seed=0):
    """Colours for the points of an object cloud, uint8 [P,3]: a smooth gradient along the axes, a texture term (stripes of period ~ 40
    cells) and noise of sigma 4.  It says nothing about the statistics of a captured 8i / MVUB cloud."""
    rng = np.random.default_rng(seed)
    p = np.asarray(xyz, np.float64)[:, :3]
    u = (p - p.min(0)) / np.maximum(p.max(0) - p.min(0), 1.0)
    tex = 30.0 * np.sin(2.0 * np.pi * (p[:, 0] + 0.5 * p[:, 1]) / 40.0)
    c = np.stack([40.0 + 170.0 * u[:, 0] + tex, 60.0 + 120.0 * u[:, 1] - 0.5 * tex, 200.0 - 150.0 * u[:, 2] + 0.25 * tex], 1)
    return np.clip(np.round(c + rng.normal(0.0, 4.0, size=c.shape)), 0, 255).astype(np.uint8)
