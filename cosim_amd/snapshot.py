"""``Snapshot`` — a fleet's complete state at one control step (``BatchedEnv.snapshot`` / ``restore`` / ``fork`` / ``history``).

What it holds:

* ``rows`` ``[M, snapshot_floats]`` float32: the engine's opaque rows (``cosim_snapshot``, include/cosim.h): per env the whole state
  record -- physics state, action-delay line, last action, the 16 meta words with ``sim_step`` and the Philox step counter,
  frequency cache, observation stack -- and the parameter record (masses, inverse weights, friction, gains);
* ``obs`` ``[M, state_dim]`` and ``command`` ``[M, max(command_dim, 1)]``: the last observation and the command buffer, which a
  resumed loop needs to compute its first action and to keep its command.  ``None`` in snapshots that come out of the history ring
  (``BatchedEnv.history``): the ring keeps the engine rows only;
* ``steps``: control steps taken since the last whole-fleet reset;
* ``meta``: what the rows were taken from (``META_FIELDS``) -- rows do not carry the model, the terrain or the spawn table, so
  ``check_compatible`` refuses to restore into an env built differently, naming the first field that disagrees;
* ``policy_state``: optional dict of the policy's own state (``LSTMPolicy.state()`` / ``SinusoidPolicy.state()``).

``save`` / ``load`` use one ``.npz`` with the metadata as JSON bytes; no pickle.  Arrays are device tensors while a snapshot is in
use and numpy arrays after ``load(path)`` without a device; the float32 words are moved bit for bit (meta words are int32 bits).
"""
from __future__ import annotations

import json
from typing import Optional

import numpy as np

# compared by check_compatible, in this order (n_envs only when rows map one to one); env_id0 and seed are recorded, not compared:
# a fork into a fleet with another seed is legitimate
META_FIELDS = ("env_id", "terrain", "precision", "snapshot_floats", "state_stride", "param_stride", "state_dim")
FORMAT = 1


def check_compatible(snap_meta: dict, env_meta: dict, need_n_envs: bool) -> None:
    """Raise ``ValueError`` naming the first metadata field of a snapshot that disagrees with the env it is restored into."""
    for key in META_FIELDS + (("n_envs",) if need_n_envs else ()):
        if key not in snap_meta:
            raise ValueError(f"snapshot metadata has no field '{key}'")
        if snap_meta[key] != env_meta[key]:
            raise ValueError(f"snapshot does not fit this env: {key} is {snap_meta[key]!r} in the snapshot, {env_meta[key]!r} here")


def _host(x):
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x)


class Snapshot:
    def __init__(self, rows, obs=None, command=None, steps: int = 0, meta: Optional[dict] = None, policy_state: Optional[dict] = None):
        self.rows, self.obs, self.command = rows, obs, command
        self.steps = int(steps)
        self.meta = dict(meta or {})
        self.policy_state = policy_state
        self.steps_ago = None            # history() captures: how many step() calls ago the capture was taken

    @property
    def num_rows(self) -> int:
        return int(self.rows.shape[0])

    def save(self, path: str) -> None:
        arrays = {"rows": _host(self.rows).astype(np.float32, copy=False)}
        if self.obs is not None:
            arrays["obs"] = _host(self.obs)
        if self.command is not None:
            arrays["command"] = _host(self.command)
        for k, v in (self.policy_state or {}).items():
            arrays["policy." + k] = _host(v) if hasattr(v, "detach") else np.asarray(v)
        head = {"format": FORMAT, "steps": self.steps, "meta": self.meta}
        arrays["header_json"] = np.frombuffer(json.dumps(head).encode("utf-8"), dtype=np.uint8)
        with open(path, "wb") as f:          # (a file object: numpy appends no ".npz" to the name it is given)
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path: str, device=None) -> "Snapshot":
        with np.load(path, allow_pickle=False) as z:
            if "header_json" not in z.files or "rows" not in z.files:
                raise ValueError(f"{path}: not a snapshot file")
            head = json.loads(bytes(z["header_json"].tobytes()).decode("utf-8"))
            if head.get("format") != FORMAT:
                raise ValueError(f"{path}: snapshot format {head.get('format')!r}, this version reads {FORMAT}")
            arrays = {k: z[k] for k in z.files if k != "header_json"}
        if device is not None:
            import torch
            arrays = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in arrays.items()}
        pol = {k[len("policy."):]: v for k, v in arrays.items() if k.startswith("policy.")}
        return cls(arrays["rows"], arrays.get("obs"), arrays.get("command"), head["steps"], head["meta"], pol or None)
