"""Fall rules: end an episode on tilt, height or body contact, per cause (``cosim_fall_set``, the rule itself is in ``env_body`` of
csrc/cosim_kernels.hip).

The reference ends an episode early only through a robot's own ``_is_done``: an empty body list for ``flamingo_light_v1``
(the intended list is commented out, flamingo_light_v1.py:191), ``False`` for ``w4_p_v2`` and ``humanoid_p_v0``.  A ``FallRule``
gives every robot a notion of "fell": the step kernel tests the pose a control step ends in and, if a rule fires, ends the episode
there -- ``terminated``, the info row of the fallen step, the auto-reset, the ledger record -- and keeps the cause:

    TILT (1)     up = 1 - 2 (qx^2 + qy^2) < cos(tilt)        up: world-z component of the base's z axis, quaternion as stored
    HEIGHT (2)   qpos[2] - ground < height                   ground: the plane's z, or the heightfield under the base
    CONTACT (4)  cfrc_ext of a listed body has a signed component > 1.0   (the ``_is_done`` rule of ``flamingo_p_v3``)

Tilt and height hold from episode step ``grace + 1`` on; the body rule is the model's block and knows no grace.
``reference_fall`` is the numpy twin of the two posture rules.  No torch, no GPU in this module.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

TILT, HEIGHT, CONTACT = 1, 2, 4
CAUSE_NAMES = {TILT: "tilt", HEIGHT: "height", CONTACT: "contact"}


def min_up(tilt: Optional[float]) -> float:
    """The fp32 threshold of the tilt rule: ``cos(tilt)`` rounded to float32; ``-1.0``, which the engine reads as "off", for
    ``None``.  The one place that turns the angle into what the kernel compares against."""
    if tilt is None:
        return -1.0
    return float(np.float32(math.cos(float(tilt))))


class FallRule:
    """``tilt``: largest tilt of the base from upright, radians in (0, pi) (``None``: no tilt rule).  ``height``: smallest height
    of the base above the ground under it, metres > 0 (``None``: no height rule).  ``grace``: control steps at the start of every
    episode during which the two posture rules are not tested.  ``bodies``: names of the bodies whose contact force ends the
    episode; ``None`` leaves the robot's own ``_is_done`` list alone, ``[]`` switches the body rule off."""

    def __init__(self, tilt: Optional[float] = None, height: Optional[float] = None, grace: int = 0,
                 bodies: Optional[Sequence[str]] = None):
        if tilt is not None:
            if isinstance(tilt, bool) or not isinstance(tilt, (int, float, np.floating, np.integer)) or not math.isfinite(float(tilt)):
                raise ValueError(f"FallRule: tilt must be a finite angle in radians, got {tilt!r}")
            if not 0.0 < float(tilt) < math.pi:
                raise ValueError(f"FallRule: tilt must lie in (0, pi) radians, got {tilt!r}")
            tilt = float(tilt)
        if height is not None:
            if isinstance(height, bool) or not isinstance(height, (int, float, np.floating, np.integer)) or not math.isfinite(float(height)):
                raise ValueError(f"FallRule: height must be a finite length in metres, got {height!r}")
            if not float(height) > 0.0:
                raise ValueError(f"FallRule: height must be > 0 metres, got {height!r}")
            height = float(height)
        if isinstance(grace, bool) or not isinstance(grace, (int, np.integer)):
            raise ValueError(f"FallRule: grace must be a whole number of control steps, got {grace!r}")
        if int(grace) < 0:
            raise ValueError(f"FallRule: grace must be >= 0 control steps, got {grace!r}")
        if bodies is not None:
            if isinstance(bodies, str):
                raise ValueError(f"FallRule: bodies must be a list of body names, got the string {bodies!r}")
            bodies = [str(b) for b in bodies]
            if len(set(bodies)) != len(bodies):
                raise ValueError(f"FallRule: bodies lists a name twice: {bodies}")
        self.tilt, self.height, self.grace, self.bodies = tilt, height, int(grace), bodies

    @classmethod
    def build(cls, rule) -> Optional["FallRule"]:
        """``None``, a ``FallRule`` or a dict of its arguments."""
        if rule is None or isinstance(rule, FallRule):
            return rule
        if isinstance(rule, dict):
            unknown = set(rule) - {"tilt", "height", "grace", "bodies"}
            if unknown:
                raise ValueError(f"FallRule: unknown keys {sorted(unknown)}")
            return cls(**rule)
        raise ValueError(f"FallRule: expected a FallRule, a dict or None, got {type(rule).__name__}")

    def is_off(self) -> bool:
        return self.tilt is None and self.height is None and self.bodies is None

    @property
    def min_up(self) -> float:
        return min_up(self.tilt)

    @property
    def min_height(self) -> float:
        return 0.0 if self.height is None else float(np.float32(self.height))

    def posture_mask(self) -> int:
        return (TILT if self.tilt is not None else 0) | (HEIGHT if self.height is not None else 0)

    def body_ids(self, body_names: Sequence[str]) -> Optional[np.ndarray]:
        """Body ids of ``bodies`` in a model's body list (``None``: the model's own list stays).  The world body and names the
        model does not have raise ``ValueError`` naming them."""
        if self.bodies is None:
            return None
        ids = []
        for b in self.bodies:
            if b not in body_names:
                raise ValueError(f"FallRule: bodies: the model has no body {b!r} (it has {', '.join(body_names[1:])})")
            if body_names.index(b) == 0:
                raise ValueError(f"FallRule: bodies: {b!r} is the world body")
            ids.append(body_names.index(b))
        return np.asarray(ids, dtype=np.int32)

    def as_dict(self) -> dict:
        return {"tilt": self.tilt, "height": self.height, "grace": self.grace, "bodies": None if self.bodies is None else list(self.bodies)}

    def __repr__(self):
        return f"FallRule(tilt={self.tilt}, height={self.height}, grace={self.grace}, bodies={self.bodies})"


class Terrain:
    """The ground the height rule measures from.  Plane: ``Terrain(pos)`` (only ``pos[2]`` matters).  Heightfield: elevation samples
    ``data`` float32 ``[nrow, ncol]`` in [0, 1], half sizes and elevation scale ``size = (sx, sy, sz, .)``, centre ``pos``."""

    def __init__(self, pos=(0.0, 0.0, 0.0), size=None, data=None):
        self.pos = np.asarray(pos, dtype=np.float32).reshape(-1)[:3]
        self.size = None if size is None else np.asarray(size, dtype=np.float32).reshape(-1)
        self.data = None if data is None else np.ascontiguousarray(data, dtype=np.float32)
        if (self.size is None) != (self.data is None):
            raise ValueError("Terrain: a heightfield needs both size and data")
        if self.data is not None and (self.data.ndim != 2 or min(self.data.shape) < 2):
            raise ValueError("Terrain: data must be [nrow, ncol] with at least 2 rows and columns")

    @classmethod
    def of(cls, cm) -> "Terrain":
        """The ground of a compiled model."""
        from .model import DEFINES
        b = cm.blob
        pos = [b.ground_pos[k] for k in range(3)]
        if b.ground_type == DEFINES["CS_GEOM_PLANE"]:
            return cls(pos)
        return cls(pos, [b.hfield_size[k] for k in range(4)], cm.hfield)


def terrain_height(terrain: Terrain, x, y):
    """Numpy twin of the kernel's ``terrain_height`` at world ``(x, y)`` (float32 arrays): elevation on the ray triangulation (every
    cell split along (r, c)-(r + 1, c + 1), as ``mj_rayHfield`` sees it) with the kernel's casts -- cell coordinates in double,
    the in-cell fractions and the interpolation in float32.  Returns ``(height float32 [n], inside bool [n])``; off the field the
    height is 0 and ``inside`` False."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    if terrain.data is None:
        return np.full(x.shape, terrain.pos[2], dtype=np.float32), np.ones(x.shape, dtype=bool)
    f32 = np.float32
    nrow, ncol = terrain.data.shape
    sx, sy, sz, gz = float(terrain.size[0]), float(terrain.size[1]), f32(terrain.size[2]), f32(terrain.pos[2])
    dx, dy = 2.0 * sx / (ncol - 1), 2.0 * sy / (nrow - 1)
    lx = 0.0 + (x.astype(np.float64) - float(terrain.pos[0]))   # the kernel's frame: origin under the base, looked up at (0, 0)
    ly = 0.0 + (y.astype(np.float64) - float(terrain.pos[1]))
    with np.errstate(invalid="ignore"):
        inside = ~((lx < -sx) | (lx > sx) | (ly < -sy) | (ly > sy))
    fx, fy = (np.where(inside, lx, 0.0) + sx) / dx, (np.where(inside, ly, 0.0) + sy) / dy
    fx, fy = np.nan_to_num(fx), np.nan_to_num(fy)
    c = np.clip(np.floor(fx).astype(np.int64), 0, ncol - 2)
    r = np.clip(np.floor(fy).astype(np.int64), 0, nrow - 2)
    u, v = (fx - c).astype(f32), (fy - r).astype(f32)
    d = terrain.data
    h00, h01, h10, h11 = d[r, c], d[r, c + 1], d[r + 1, c], d[r + 1, c + 1]
    hh = np.where(u >= v, h00 + u * (h01 - h00) + v * (h11 - h01), h00 + v * (h10 - h00) + u * (h11 - h10))
    assert hh.dtype == f32
    out = (gz + sz * hh).astype(f32)
    return np.where(inside, out, f32(0.0)), inside


def up_component(qpos) -> np.ndarray:
    """``1 - 2 (qx^2 + qy^2)`` of ``qpos[:, 3:7]`` in float32, operation by operation as the kernel rounds it."""
    q = np.asarray(qpos, dtype=np.float32)
    qx, qy = q[..., 4], q[..., 5]
    with np.errstate(all="ignore"):
        return (np.float32(1.0) - np.float32(2.0) * (qx * qx + qy * qy)).astype(np.float32)


def base_height(qpos, terrain: Optional[Terrain] = None):
    """``(qpos[2] - ground float32 [n], inside bool [n])``."""
    q = np.asarray(qpos, dtype=np.float32)
    terrain = terrain if terrain is not None else Terrain()
    ground, inside = terrain_height(terrain, q[..., 0], q[..., 1])
    with np.errstate(all="ignore"):
        return (q[..., 2] - ground).astype(np.float32), inside


def reference_fall(qpos, sim_step, rule, terrain: Optional[Terrain] = None) -> np.ndarray:
    """Numpy twin of the kernel's posture rules: the cause bits (``TILT | HEIGHT``) per env from float32 ``qpos`` rows ``[N, nq]``
    -- the state a control step ended in -- and the episode clock ``sim_step`` of that step (scalar or ``[N]``; 1 on the first step
    after a reset).  ``terrain``: ``Terrain.of(compiled)``; ``None`` is the plane at z = 0.  The body rule is a function of the
    contact forces, not of the pose: it has no twin here (its bit, 4, is what ``terminated`` says beyond these two)."""
    rule = FallRule.build(rule)
    q = np.asarray(qpos, dtype=np.float32)
    if q.ndim == 1:
        q = q[None]
    n = q.shape[0]
    cause = np.zeros(n, dtype=np.int32)
    if rule is None:
        return cause
    live = np.broadcast_to(np.asarray(sim_step), (n,)) > rule.grace
    with np.errstate(invalid="ignore"):
        if rule.tilt is not None:
            cause |= np.where(live & (up_component(q) < np.float32(rule.min_up)), TILT, 0).astype(np.int32)
        if rule.height is not None:
            hgt, inside = base_height(q, terrain)
            cause |= np.where(live & inside & (hgt < np.float32(rule.min_height)), HEIGHT, 0).astype(np.int32)
    return cause
