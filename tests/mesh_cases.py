"""Inputs and checks shared by tests/test_mesh_cpu.py and tests/test_mesh_gpu.py: volumes written straight into a ``fusion.TsdfHost`` (the sphere
of the closed-surface test, seeded noise, the volumes without a cell and with one), bit equality of two meshes, and the edge counts of a
triangle list."""
from collections import Counter

import numpy as np

from endodav_amd.fusion import TsdfHost, Volume
from tests import fusion_cases as fc

NO_CELL = [(1, 1, 1), (1, 5, 5), (5, 1, 5)]     # no voxel has a +x, +y and +z neighbour

SPHERE_N, SPHERE_R, SPHERE_C = 14, 4.3, (7.1, 6.8, 7.3)    # voxels; the volume has origin 0 and voxel 1, so world units are voxels


def filled(dims, tsdf, weight=None, color=None, **kw):
    """A TsdfHost of ``dims`` = (nx, ny, nz) whose arrays [nz, ny, nx] are set by hand; weight 1 everywhere unless given."""
    nx, ny, nz = dims
    kw.setdefault("origin", (0.0, 0.0, 0.0))
    kw.setdefault("voxel", 1.0)
    host = TsdfHost(Volume(dims=dims, **kw), coloured=color is not None)
    host.tsdf[:] = np.asarray(tsdf, np.float32).reshape(nz, ny, nx)
    host.weight[:] = 1.0 if weight is None else np.asarray(weight, np.float32).reshape(nz, ny, nx)
    if color is not None:
        host.color[:] = np.asarray(color, np.float32).reshape(nz, ny, nx, 3)
    return host


def sphere(holes=0.0, seed=0, coloured=False):
    """tsdf = clip((|c - centre| - r) / trunc, -1, 1) with trunc = 4 voxels in a 14^3 grid; a seeded share ``holes`` of the voxels unobserved."""
    n = SPHERE_N
    g = np.arange(n) + 0.5
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    dist = np.sqrt((X - SPHERE_C[0]) ** 2 + (Y - SPHERE_C[1]) ** 2 + (Z - SPHERE_C[2]) ** 2)
    rng = np.random.default_rng(700 + seed)
    weight = (rng.random((n, n, n)) >= holes).astype(np.float32)
    color = rng.random((n, n, n, 3)) * 255.0 if coloured else None
    return filled((n, n, n), np.clip((dist - SPHERE_R) / 4.0, -1.0, 1.0), weight, color)


def noise(dims, seed=0, unobserved=0.1, coloured=True):
    """Random tsdf in (-1, 1), weight 0 for a share ``unobserved`` of the voxels, 1 for a tenth of the rest and 2 otherwise, so that cells stay
    valid at min_weight 1 and 2 alike; colours partly outside 0..255."""
    nx, ny, nz = dims
    rng = np.random.default_rng(800 + seed)
    tsdf = rng.uniform(-1.0, 1.0, (nz, ny, nx))
    weight = np.where(rng.random((nz, ny, nx)) < unobserved, 0.0, np.where(rng.random((nz, ny, nx)) < 0.1, 1.0, 2.0))
    color = rng.random((nz, ny, nx, 3)) * 300.0 - 20.0 if coloured else None
    return filled(dims, tsdf, weight, color, origin=(-1.0, 0.25, 3.0), voxel=0.03)


def one_cell(name):
    """A (2, 2, 2) volume, one cell, with the named corner pattern; corner c is voxel c."""
    mag = np.array([0.3, 0.7, 0.45, 0.9, 0.25, 0.6, 0.8, 0.35])
    inside = {"corner-0": [0], "corner-5": [5], "all-but-3": [0, 1, 2, 4, 5, 6, 7], "half-x": [0, 2, 4, 6], "checker": [0, 3, 5, 6], "diagonal": [0, 7],
              "all-in": list(range(8)), "all-out": [], "zero-corner": [1, 2, 3, 4, 5, 6, 7]}[name]
    tsdf = np.where(np.isin(np.arange(8), inside), -mag, mag)
    if name == "zero-corner":
        tsdf[0] = 0.0                            # outside, and t = 0 on every edge out of it: its seven vertices coincide at the voxel centre
    color = np.random.default_rng(900).random((8, 3)) * 255.0
    return filled((2, 2, 2), tsdf, None, color)


ONE_CELL = ["corner-0", "corner-5", "all-but-3", "half-x", "checker", "diagonal", "all-in", "all-out", "zero-corner"]


def same_mesh(got, want):
    """Two host meshes equal bit for bit, with the dtypes and shapes of fusion.Mesh."""
    for name, dtype in (("vertices", np.float32), ("normals", np.float32), ("colors", np.uint8), ("triangles", np.int32)):
        g, w = getattr(got, name), getattr(want, name)
        if w is None:
            assert g is None, name
            continue
        assert isinstance(g, np.ndarray) and g.dtype == dtype and g.shape == w.shape and g.ndim == 2 and g.shape[1] == 3, (name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32) if dtype == np.float32 else g, w.view(np.uint32) if dtype == np.float32 else w), name


def edge_counts(triangles):
    """(directed, undirected): how often each directed edge (a, b) and each undirected edge {a, b} occurs in the triangle list."""
    directed = Counter()
    for a, b, c in np.asarray(triangles).tolist():
        directed.update(((a, b), (b, c), (c, a)))
    undirected = Counter()
    for (a, b), k in directed.items():
        undirected[(min(a, b), max(a, b))] += k
    return directed, undirected


def integrated(dims, shape, seed=0, coloured=True, **kw):
    """A TsdfHost after one seeded clip of fusion_cases, and the case it came from."""
    case = fc.case(dims, shape, seed=seed, **kw)
    vol, spec, depth, frames = case
    host = TsdfHost(vol, coloured=coloured)
    host.integrate(depth, spec, frames if coloured else None)
    return host, case
