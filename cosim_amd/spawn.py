"""Spawn tables: base poses spread over the terrain instead of one ``init_qpos`` for the whole fleet.

A table row is ``(x, y, yaw)``.  The engine (``cosim_spawn_set``, ``csrc/cosim_spawn.hip``) lifts each row onto the
heightfield and every reset takes the base pose ``qpos[0:7]`` from a row; this module holds the host side of that:

* ``footprint(cm)`` -- one bounding sphere per ground geom at ``init_qpos``, the table the placement kernel walks;
* ``grid_poses`` / ``uniform_poses`` -- pose generators, pure functions of their arguments (``uniform_poses``: of
  ``(seed, row)`` through the counter-based RNG, purpose 6, so every rank of a distributed run builds the same table);
* ``place_reference`` -- the float64 numpy twin of the kernel's rule, written out independently of the engine;
* ``episode_row`` -- the host prediction of the row a per-episode reset draws on the device (purpose 5).

Placement rule, for a row with ``c, s = cos yaw, sin yaw`` and a footprint geom ``(ox, oy, r, free)``:
``g_xy = (x, y) + R(yaw) (ox, oy)``; ``hmax_g`` = the highest heightfield sample over the vertices ``cmin..cmax`` x
``rmin..rmax``, ``cmin = floor((lx - r + sx) / dx)``, ``cmax = ceil((lx + r + sx) / dx)``, ``lx = g_x - ground_pos.x``,
``dx = 2 sx / (ncol - 1)`` (rows alike); ``dz = max(0, max_g(sz hmax_g - free_g)) + clearance``; ``z = init_qpos[2] + dz``.
The prism surface inside a cell never exceeds the cell's corner heights, so no point of geom g ends closer to the terrain
than it was to ``z = 0`` at the nominal pose; where the field is 0, ``dz = clearance`` exactly.

Limits: only yaw orientations; position-mode commands stay world-frame targets; the CPU twins of ``oracle/fleet.py`` reset
to ``init_qpos`` (they do not know about spawn tables).
"""
from __future__ import annotations

from typing import Optional, Union

import numpy as np

from . import rng as crng
from .compile import CompiledModel, forward_kinematics
from .model import DEFINES, get_field


def _is_plane(cm: CompiledModel) -> bool:
    return cm.blob.ground_type == DEFINES["CS_GEOM_PLANE"]


def footprint(cm: CompiledModel) -> np.ndarray:
    """float32 ``[G, 4]`` = ``(ox, oy, r, free)`` per geom that can touch the ground, at ``init_qpos``: horizontal offset of the
    geom's bounding-sphere centre (``geom_rcenter`` through the body pose) from the base, ``r = geom_rbound``, and
    ``free = max(cz - r, 0)`` with ``cz`` the centre's world height."""
    b = cm.blob
    ng = b.ngeom
    q0 = np.array(get_field(b, "init_qpos")[:b.nq], dtype=np.float64)
    fk = forward_kinematics(cm.const["m"], q0)
    body = np.array(get_field(b, "geom_bodyid")[:ng])
    ground = np.array(get_field(b, "geom_ground")[:ng])
    rc = np.array(get_field(b, "geom_rcenter")[:ng], dtype=np.float64).reshape(ng, 3)
    rb = np.array(get_field(b, "geom_rbound")[:ng], dtype=np.float64)
    rows = []
    for g in range(ng):
        if ground[g] == 0:
            continue
        ctr = fk["xpos"][body[g]] + fk["xmat"][body[g]] @ rc[g]
        rows.append([ctr[0] - q0[0], ctr[1] - q0[1], rb[g], max(ctr[2] - rb[g], 0.0)])
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)


def footprint_radius(cm: CompiledModel) -> float:
    """Radius of the disc about the base that holds every footprint sphere at any yaw."""
    fp = footprint(cm).astype(np.float64)
    return float((np.hypot(fp[:, 0], fp[:, 1]) + fp[:, 2]).max()) if len(fp) else 0.0


def default_extent(cm: CompiledModel) -> float:
    """Half-size of the square of base positions the generators fill by default: the field's half-size minus the footprint
    radius (every footprint then lies on the field at any yaw); 10 m on plane ground."""
    if _is_plane(cm):
        return 10.0
    b = cm.blob
    return float(min(b.hfield_size[0], b.hfield_size[1])) - footprint_radius(cm) - 1e-3


def _yaw_column(yaw, count: int, draw) -> np.ndarray:
    if isinstance(yaw, str):
        if yaw != "random":
            raise ValueError(f"yaw must be 'random' or a number, got {yaw!r}")
        return draw()
    y = np.broadcast_to(np.asarray(yaw, dtype=np.float64), (count,)).copy()
    if not np.all(np.isfinite(y)):
        raise ValueError("yaw must be finite")
    return y


def _centre(cm: CompiledModel) -> np.ndarray:
    return np.array(cm.blob.ground_pos[:2], dtype=np.float64)


def grid_poses(cm: CompiledModel, count: int, extent: Optional[float] = None, spacing: Optional[float] = None,
               yaw: Union[float, str, np.ndarray] = 0.0) -> np.ndarray:
    """``count`` poses ``[count, 3]`` on a square grid centred on the terrain, row-major from the (-x, -y) corner.  The grid
    has ``ceil(sqrt(count))`` points per side; ``spacing`` sets their distance, else they span ``[-extent, extent]``
    (default: ``default_extent``).  ``yaw``: one angle, an array of ``count``, or "random" (row-indexed draws, seed 0)."""
    count = int(count)
    if count < 1:
        raise ValueError("count must be >= 1")
    ext = default_extent(cm) if extent is None else float(extent)
    side = int(np.ceil(np.sqrt(count)))
    half = ext if spacing is None else 0.5 * float(spacing) * (side - 1)
    if half > ext:
        raise ValueError(f"a {side} x {side} grid at spacing {spacing} does not fit the extent {ext:.3f}")
    ticks = np.linspace(-half, half, side) if side > 1 else np.zeros(1)
    i = np.arange(count)
    ctr = _centre(cm)
    out = np.empty((count, 3), dtype=np.float64)
    out[:, 0] = ctr[0] + ticks[i % side]
    out[:, 1] = ctr[1] + ticks[i // side]
    out[:, 2] = _yaw_column(yaw, count, lambda: (2.0 * crng.uniform(0, i, 0, crng.PURPOSE_SPAWN_POSE, 2).astype(np.float64) - 1.0) * np.pi)
    return out.astype(np.float32)


def uniform_poses(cm: CompiledModel, count: int, seed: int, extent: Optional[float] = None,
                  yaw: Union[float, str, np.ndarray] = "random") -> np.ndarray:
    """``count`` poses ``[count, 3]`` uniform over ``[-extent, extent]^2`` about the terrain centre; row ``i`` is a pure
    function of ``(seed, i)`` (``rng.uniform`` with the row as env id, purpose 6, index 0 / 1 / 2 = x / y / yaw)."""
    count = int(count)
    if count < 1:
        raise ValueError("count must be >= 1")
    ext = default_extent(cm) if extent is None else float(extent)
    i = np.arange(count)
    u = [crng.uniform(int(seed), i, 0, crng.PURPOSE_SPAWN_POSE, k).astype(np.float64) for k in range(3)]
    ctr = _centre(cm)
    out = np.empty((count, 3), dtype=np.float64)
    out[:, 0] = ctr[0] + (2.0 * u[0] - 1.0) * ext
    out[:, 1] = ctr[1] + (2.0 * u[1] - 1.0) * ext
    out[:, 2] = _yaw_column(yaw, count, lambda: (2.0 * u[2] - 1.0) * np.pi)
    return out.astype(np.float32)


def windows(cm: CompiledModel, xyyaw: np.ndarray):
    """Per (row, footprint geom): local centre ``lx, ly`` ``[M, G]`` and the unclamped window bounds as reals
    ``(cmin, cmax, rmin, rmax)`` before floor / ceil -- what the placement rule rounds (float64)."""
    b = cm.blob
    fp = footprint(cm).astype(np.float64)
    p = np.asarray(xyyaw, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    c, s = np.cos(p[:, 2])[:, None], np.sin(p[:, 2])[:, None]
    gx, gy = float(np.float32(b.ground_pos[0])), float(np.float32(b.ground_pos[1]))
    lx = p[:, 0:1] + (c * fp[None, :, 0] - s * fp[None, :, 1]) - gx
    ly = p[:, 1:2] + (s * fp[None, :, 0] + c * fp[None, :, 1]) - gy
    if _is_plane(cm):
        return lx, ly, None
    sx, sy = float(np.float32(b.hfield_size[0])), float(np.float32(b.hfield_size[1]))
    dx, dy = 2.0 * sx / (b.hfield_ncol - 1), 2.0 * sy / (b.hfield_nrow - 1)
    r = fp[None, :, 2]
    return lx, ly, ((lx - r + sx) / dx, (lx + r + sx) / dx, (ly - r + sy) / dy, (ly + r + sy) / dy)


def check_rows(cm: CompiledModel, xyyaw: np.ndarray):
    """``ValueError`` naming the first row that is not finite or puts a footprint sphere off the field (``|l| + r > s``)."""
    p = np.asarray(xyyaw, dtype=np.float32).reshape(-1, 3)
    bad = np.flatnonzero(~np.isfinite(p).all(axis=1))
    if len(bad):
        raise ValueError(f"spawn row {int(bad[0])} is not finite")
    if _is_plane(cm):
        return
    b = cm.blob
    lx, ly, _ = windows(cm, p)
    r = footprint(cm).astype(np.float64)[None, :, 2]
    off = (np.abs(lx) + r > float(np.float32(b.hfield_size[0]))) | (np.abs(ly) + r > float(np.float32(b.hfield_size[1])))
    bad = np.flatnonzero(off.any(axis=1))
    if len(bad):
        raise ValueError(f"spawn row {int(bad[0])} puts footprint geom {int(np.argmax(off[bad[0]]))} off the heightfield")


def place_reference(cm: CompiledModel, xyyaw: np.ndarray, clearance: float = 0.0) -> np.ndarray:
    """float64 ``[M, 7]`` = ``x, y, z, qw, qx, qy, qz``: the placement rule of the module docstring in numpy, independent of
    the engine.  Inputs are taken at the precision the engine receives them (float32 rows and footprint)."""
    b = cm.blob
    p32 = np.asarray(xyyaw, dtype=np.float32).reshape(-1, 3)
    check_rows(cm, p32)
    p = p32.astype(np.float64)
    M = len(p)
    q0 = np.array(get_field(b, "init_qpos")[:7], dtype=np.float64)
    fp = footprint(cm).astype(np.float64)
    dz = np.zeros(M)
    if not _is_plane(cm) and len(fp):
        _, _, (c0, c1, r0, r1) = windows(cm, p32)
        nrow, ncol = cm.hfield.shape
        cmin = np.clip(np.floor(c0).astype(np.int64), 0, ncol - 1); cmax = np.clip(np.ceil(c1).astype(np.int64), 0, ncol - 1)
        rmin = np.clip(np.floor(r0).astype(np.int64), 0, nrow - 1); rmax = np.clip(np.ceil(r1).astype(np.int64), 0, nrow - 1)
        sz = float(np.float32(b.hfield_size[2]))
        h = cm.hfield.astype(np.float64)
        for i in range(M):
            lift = -np.inf
            for g in range(len(fp)):
                hmax = h[rmin[i, g]:rmax[i, g] + 1, cmin[i, g]:cmax[i, g] + 1].max()
                lift = max(lift, sz * hmax - fp[g, 3])
            dz[i] = max(0.0, lift)
    out = np.empty((M, 7), dtype=np.float64)
    out[:, 0:2] = p[:, 0:2]
    out[:, 2] = q0[2] + (dz + float(clearance))
    hw, hz = np.cos(0.5 * p[:, 2]), np.sin(0.5 * p[:, 2])   # q_yaw (x) init_quat
    out[:, 3] = hw * q0[3] - hz * q0[6]
    out[:, 4] = hw * q0[4] - hz * q0[5]
    out[:, 5] = hw * q0[5] + hz * q0[4]
    out[:, 6] = hw * q0[6] + hz * q0[3]
    return out


def episode_row(seed: int, env_ids, step_count, rows: int) -> np.ndarray:
    """Row a reset draws in per-episode mode: ``min(rows - 1, floor(u01(philox(seed, gid, step_count, 5, 0)) * rows))`` in
    float32, as the device computes it; ``step_count`` is the env's meta word 1 before the launch that resets."""
    u = crng.uniform(int(seed), env_ids, step_count, crng.PURPOSE_SPAWN, 0)
    return np.minimum(int(rows) - 1, np.floor(u * np.float32(rows)).astype(np.int64))


def resolve(cm: CompiledModel, spawn, seed: int = 0):
    """``(xyyaw float32 [M, 3], clearance, per_episode)`` from what ``BatchedEnv(spawn=...)`` / ``config["engine"]["spawn"]``
    accept: an ``[M, 3]`` array, or a dict ``{"pattern": "grid" | "uniform" | "poses", "count", "extent", "spacing", "yaw",
    "per_episode", "clearance", "poses"}``.  Poses of 7 numbers (x, y, z, quaternion) are accepted when the orientation is a
    pure yaw (z is recomputed); any other orientation raises ``ValueError``."""
    clearance, per_episode = 0.0, False
    if isinstance(spawn, dict):
        known = {"pattern", "count", "extent", "spacing", "yaw", "per_episode", "clearance", "poses", "seed"}
        if set(spawn) - known:
            raise ValueError(f"unknown spawn keys {sorted(set(spawn) - known)}")
        clearance = float(spawn.get("clearance", 0.0) or 0.0)
        per_episode = bool(spawn.get("per_episode", False))
        pattern = spawn.get("pattern", "poses" if spawn.get("poses") is not None else "uniform")
        seed = int(spawn.get("seed", seed))
        if pattern == "poses":
            if spawn.get("poses") is None:
                raise ValueError("spawn pattern 'poses' needs 'poses'")
            poses = spawn["poses"]
        elif pattern in ("grid", "uniform"):
            count = spawn.get("count")
            if count is None:
                raise ValueError(f"spawn pattern '{pattern}' needs 'count'")
            if pattern == "grid":
                poses = grid_poses(cm, count, spawn.get("extent"), spawn.get("spacing"), spawn.get("yaw", 0.0) if spawn.get("yaw") is not None else 0.0)
            else:
                poses = uniform_poses(cm, count, seed, spawn.get("extent"), spawn.get("yaw", "random") if spawn.get("yaw") is not None else "random")
        else:
            raise ValueError(f"unknown spawn pattern {pattern!r}")
    else:
        poses = spawn
    a = np.asarray(poses, dtype=np.float64)
    if a.ndim == 1 and a.size == 0:
        a = a.reshape(0, 3)
    if a.ndim != 2 or a.shape[1] not in (3, 7):
        raise ValueError(f"spawn poses must be [M, 3] (x, y, yaw) or [M, 7] with a yaw-only quaternion, got {a.shape}")
    if a.shape[1] == 7:
        q = a[:, 3:7]
        if np.any(np.abs(q[:, 1]) > 1e-6) or np.any(np.abs(q[:, 2]) > 1e-6) or np.any(np.abs(np.linalg.norm(q, axis=1) - 1.0) > 1e-5):
            raise ValueError("only yaw spawns are supported: the quaternion must be a unit (w, 0, 0, z)")
        a = np.column_stack([a[:, 0], a[:, 1], 2.0 * np.arctan2(q[:, 3], q[:, 0])])
    if not (clearance >= 0.0 and np.isfinite(clearance)):
        raise ValueError("spawn clearance must be finite and >= 0")
    xy = a.astype(np.float32)
    check_rows(cm, xy)
    return xy, clearance, per_episode
