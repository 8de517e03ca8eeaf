"""Failure traces: every env's last control steps before an episode ended (``cosim_ftrace_set`` / ``cosim_ftrace_get``,
csrc/cosim_ftrace.hip).

The engine keeps a window of the last ``frames`` control steps of every env on the device -- one ``(state, action, outcome)`` frame
per step, plain copies -- and freezes it as a trace when an episode ends with a selected cause (no host read per step).
``FailureTraces`` is those traces on the host: one row per kept trace, sorted by (env, episode), the frames unrolled into time
order.  ``reference_traces`` is the numpy twin of the three kernels: the same writes in the same order on per-step host arrays, so
its buffers, counters and headers equal the device's bit for bit.  No torch, no GPU in this module.
"""
from __future__ import annotations

import json
from typing import Optional, Sequence

import numpy as np

from . import records as rc
from .records import FELL_CONTACT, FELL_HEIGHT, FELL_TILT, NO_RESET, NONFINITE, OPEN, TERMINATED, TRUNCATED

HDR, FRAME_HDR, NCNT = 16, 4, 16
MAX_FRAMES, MAX_KEEP = 1024, 64
ON_NAMES = {"terminated": TERMINATED, "truncated": TRUNCATED, "nonfinite": NONFINITE, "tilt": FELL_TILT, "height": FELL_HEIGHT,
            "contact": FELL_CONTACT}
ON_ALL = sum(ON_NAMES.values())
DEFAULT_ON = ("terminated", "nonfinite")                               # everything but a plain time limit
HEADER_FIELDS = {"episode": 0, "length": 1, "flags": 2, "frames": 3, "oldest": 4, "spawn_row": 5, "steps_seen": 7}
SCENARIO_WORD = 6                                                      # scenario row + 1 (0: no scenario table)
DIMS = ("nq", "nv", "nu", "command_dim", "info_dim")


def frame_words(nq: int, nv: int, nu: int, command_dim: int, info_dim: int) -> int:
    """F: 32-bit words of a frame, padded to a multiple of 4 (``cosim_query "ftrace_frame_words"``)."""
    return (FRAME_HDR + int(nq) + int(nv) + int(nu) + int(command_dim) + int(info_dim) + 3) & ~3


def on_mask(on) -> int:
    """The ledger-flag mask of the causes that freeze a window: ``on`` is a mask (int) or names out of ``ON_NAMES``.  Raises
    ``ValueError`` naming an unknown name, an empty selection or a bit outside ``1|2|4|32|64|128``."""
    if on is None:
        on = DEFAULT_ON
    if isinstance(on, (int, np.integer)) and not isinstance(on, bool):
        mask = int(on)
        if mask == 0 or mask & ~ON_ALL:
            raise ValueError(f"failure_traces: on mask {mask} must be a non-empty subset of 1|2|4|32|64|128")
        return mask
    if isinstance(on, str):
        on = (on,)
    names = list(on)
    if not names:
        raise ValueError(f"failure_traces: 'on' is empty: name at least one of {sorted(ON_NAMES)}")
    mask = 0
    for n in names:
        if n not in ON_NAMES:
            raise ValueError(f"failure_traces: unknown 'on' name {n!r}: expected one of {sorted(ON_NAMES)}")
        mask |= ON_NAMES[n]
    return mask


def on_names(mask: int) -> list:
    return [n for n, b in ON_NAMES.items() if int(mask) & b]


def resolve(spec, on=None):
    """``(frames, keep, mask)`` from ``(frames, keep)`` or ``{"frames", "keep", "on"}``.  Raises ``ValueError`` naming the value
    that is out of range (frames 1..1024, keep 1..64) or the key it does not know."""
    if isinstance(spec, dict):
        unknown = sorted(set(spec) - {"frames", "keep", "on"})
        if unknown:
            raise ValueError(f"failure_traces: unknown key {unknown[0]!r}: expected 'frames', 'keep', 'on'")
        if "frames" not in spec or "keep" not in spec:
            raise ValueError("failure_traces: a mapping needs 'frames' and 'keep'")
        frames, keep = spec["frames"], spec["keep"]
        on = spec.get("on") if on is None else on
    else:
        try:
            frames, keep = spec
        except (TypeError, ValueError):
            raise ValueError(f"failure_traces: expected (frames, keep) or a mapping, got {spec!r}") from None
    for name, v in (("frames", frames), ("keep", keep)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"failure_traces: {name} {v!r} is not an integer")
    frames, keep = int(frames), int(keep)
    if not 1 <= frames <= MAX_FRAMES:
        raise ValueError(f"failure_traces: frames {frames} outside 1..{MAX_FRAMES}")
    if not 1 <= keep <= MAX_KEEP:
        raise ValueError(f"failure_traces: keep {keep} outside 1..{MAX_KEEP}")
    return frames, keep, on_mask(on)


class FailureTraces:
    """Kept traces of a fleet, one row per trace, sorted by (global env id, episode).

    ``headers`` int32 ``[M, 16]`` is each trace's header as the engine wrote it (include/cosim.h); ``words`` int32 ``[M, T, F]`` its
    frames in time order (oldest first, left-aligned, rows beyond ``frames[m]`` zero), ``T`` the window size.  Per trace: ``env``
    int64 (global id), ``episode``, ``flags``, ``length``, ``frames`` (valid frames), ``spawn_row``, ``scenario`` (row, -1: no
    table), ``steps_seen``.  Per frame, padded with -1 (integers) / NaN (floats) beyond ``frames[m]``: ``t`` ``[M, T]`` (1-based
    episode step), ``terminated``, ``truncated``, ``qpos`` ``[M, T, nq]``, ``qvel``, ``action``, ``command``, ``info``.  ``lost``
    int64 ``[N]``: per env, the traces that newer ones overwrote.  Rows with flag 16 (``include_open``) are windows still running;
    ``summary`` leaves them out.  ``meta``: ``nq, nv, nu, command_dim, info_dim, window, keep, on_mask, env_id0``."""

    def __init__(self, headers, words, env, lost, meta: dict):
        self.meta = {k: int(v) for k, v in meta.items()}
        for k in DIMS + ("window", "keep", "on_mask", "env_id0"):
            if k not in self.meta:
                raise ValueError(f"FailureTraces: meta lacks {k!r}")
        nq, nv, nu, cd, ni = (self.meta[k] for k in DIMS)
        T, F = self.meta["window"], frame_words(nq, nv, nu, cd, ni)
        self.headers = np.ascontiguousarray(headers, dtype=np.int32).reshape(-1, HDR)
        M = len(self.headers)
        self.words = np.ascontiguousarray(words, dtype=np.int32).reshape(M, T, F)
        self.env = np.ascontiguousarray(env, dtype=np.int64).reshape(-1)
        self.lost = np.ascontiguousarray(lost, dtype=np.int64).reshape(-1)
        if len(self.env) != M:
            raise ValueError(f"FailureTraces: {M} traces but {len(self.env)} env ids")
        for name, w in HEADER_FIELDS.items():
            setattr(self, name, self.headers[:, w])
        self.scenario = self.headers[:, SCENARIO_WORD] - 1
        valid = np.arange(T)[None, :] < self.frames[:, None]                      # [M, T]
        self.valid = valid
        self.t = np.where(valid, self.words[:, :, 0], -1)
        self.terminated = np.where(valid, self.words[:, :, 1] & 1, -1)
        self.truncated = np.where(valid, (self.words[:, :, 1] >> 1) & 1, -1)
        o = FRAME_HDR
        for name, n in (("qpos", nq), ("qvel", nv), ("action", nu), ("command", cd), ("info", ni)):
            x = self.words[:, :, o:o + n].view(np.float32).copy()
            x[~valid] = np.nan
            setattr(self, name, x)
            o += n

    def __len__(self):
        return len(self.headers)

    @classmethod
    def from_raw(cls, buffers, counts, open_rows, dims: dict, on: int, env_id0: int = 0) -> "FailureTraces":
        """From what ``cosim_ftrace_get`` copies: buffers ``[N, keep + 1, 16 + frames * F]``, counters ``[N, 3]`` (working buffer,
        triggered, lost), open headers ``[N, 16]`` or ``None``.  The kept traces of an env are the ``min(triggered, keep)`` buffers
        behind its working one; an open row takes its frames from the working buffer.  ``dims``: ``nq, nv, nu, command_dim,
        info_dim``."""
        F = frame_words(*(dims[k] for k in DIMS))
        buffers = np.asarray(buffers, dtype=np.int32)
        N, nbuf = buffers.shape[0], buffers.shape[1]
        keep, T = nbuf - 1, (buffers.shape[2] - HDR) // F
        if buffers.shape[2] != HDR + T * F or T < 1:
            raise ValueError(f"FailureTraces.from_raw: buffers of {buffers.shape[2]} words are not 16 + frames * {F}")
        counts = np.asarray(counts, dtype=np.int64).reshape(N, 3)
        work, trig = counts[:, 0], counts[:, 1]
        env, k, kept = rc.kept_rows(trig, keep)
        b = (work[env] - (kept[env] - k)) % nbuf                                  # oldest first: age kept - 1 - k behind the working buffer
        headers = buffers[env, b, :HDR]
        if open_rows is not None:
            headers, env, order = rc.merge_open(headers, env, np.asarray(open_rows, dtype=np.int32).reshape(N, HDR))
            b = np.concatenate([b, work])[order]
        rings = buffers[env, b, HDR:].reshape(len(env), T, F)
        pos = (headers[:, 4:5].astype(np.int64) + np.arange(T)[None, :]) % T
        words = np.take_along_axis(rings, pos[:, :, None], axis=1)
        words = np.where((np.arange(T)[None, :] < headers[:, 3:4])[:, :, None], words, 0)
        meta = {**{k: int(dims[k]) for k in DIMS}, "window": T, "keep": keep, "on_mask": int(on), "env_id0": int(env_id0)}
        out = cls(headers, words, env + int(env_id0), counts[:, 2], meta)
        out.buffers, out.counts = buffers, counts.astype(np.int32)                # the raw copies, for bit-for-bit comparisons
        out.open_headers = None if open_rows is None else np.asarray(open_rows, dtype=np.int32).reshape(N, HDR)
        return out

    def ended(self) -> np.ndarray:
        """Mask of the rows that are frozen traces (not flag 16)."""
        return (self.flags & OPEN) == 0

    def select(self, flags=None, env=None) -> "FailureTraces":
        """The traces with any of ``flags`` (a mask or ``on`` names) set and / or of the global env ids ``env``."""
        m = np.ones(len(self), dtype=bool)
        if flags is not None:
            m &= (self.flags & on_mask(flags)) != 0
        if env is not None:
            m &= np.isin(self.env, np.atleast_1d(np.asarray(env, dtype=np.int64)))
        return FailureTraces(self.headers[m], self.words[m], self.env[m], self.lost, self.meta)

    def summary(self) -> dict:
        """Traces per cause (a trace with several flags counts under each), open windows and traces lost."""
        m = self.ended()
        f = self.flags[m]
        out = {"traces": int(m.sum())}
        for name, bit in ON_NAMES.items():
            out[name] = int(((f & bit) != 0).sum())
        out["no_reset_start"] = int(((f & NO_RESET) != 0).sum())
        out["open"] = int((~m).sum())
        out["lost"] = int(self.lost.sum())
        return out

    def join(self, ledger) -> np.ndarray:
        """Per trace, the row of ``ledger`` (an ``EpisodeLedger``) with the same (env, episode), or -1 (the ledger's ring has
        overwritten it, or the two were not set together).  The ordinals agree when traces and ledger are set together."""
        return rc.join(self, ledger)

    def save(self, path: str):
        """One ``.npz`` of plain arrays, the metadata as JSON bytes (no pickle)."""
        np.savez(path, headers=self.headers, words=self.words, env=self.env, lost=self.lost,
                 meta=np.frombuffer(json.dumps(self.meta, sort_keys=True).encode(), dtype=np.uint8))

    @classmethod
    def load(cls, path: str) -> "FailureTraces":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["headers"], z["words"], z["env"], z["lost"], json.loads(z["meta"].tobytes().decode()))


def same_traces(a: FailureTraces, b: FailureTraces) -> Optional[str]:
    """``None`` if two sets hold the same rows, word for word (floats as bits), else a sentence naming the first difference."""
    head = rc.same_rows(a, b, "traces", meta=True)
    if head is not None:
        return head
    for name, x, y in (("header", a.headers, b.headers), ("frame", a.words.reshape(len(a), -1), b.words.reshape(len(b), -1))):
        bad = rc.first_difference(x, y)
        if bad is not None:
            r, w = bad
            return f"{name} word {w} of row {r} (env {a.env[r]}, episode {a.headers[r, 0]}): {x[r, w]} against {y[r, w]}"
    return None


def reference_traces(qpos, qvel, actions, commands, info, term, trunc, meta4, meta14, meta15, frames: int, keep: int,
                     on=None, include_open: bool = False, initial_flags: int = 0, begins: Sequence = (), env_id0: int = 0,
                     scenario_rows=None, open_scenario_rows=None) -> FailureTraces:
    """Numpy twin of ``ftrace_step_kernel`` / ``ftrace_begin_kernel`` / ``ftrace_open_kernel``: the same words written in the same
    order, so ``buffers``, ``counts`` and ``open_headers`` of the result equal what ``cosim_ftrace_get`` copies.

    K control steps of N envs.  ``qpos`` ``[K + 1, N, nq]`` / ``qvel`` ``[K + 1, N, nv]``: the state record BEFORE step k in row k
    (after any host cut ahead of it) and after the last step in row K.  ``actions`` ``[K, N, nu]``, ``commands`` ``[K, N, cd]`` (or
    ``[N, cd]``; the applied command), ``info`` ``[K, N, info_dim]``, ``term`` / ``trunc`` ``[K, N]``: what step k was given and
    returned.  ``meta4`` / ``meta14`` ``[K + 1, N]``: the engine's meta words 4 / 14 with the rows of ``qpos`` (``None``: no
    non-finite reset / no spawn table, -1).  ``meta15`` ``[K, N]``: meta word 15 after step k while a fall rule is set (``None``:
    no rule).  ``on``: names or a mask.  ``initial_flags``: 8 if the traces were set on a stepped fleet.  ``begins``: ``(k, mask or
    None, flag)`` -- a host reset (flag 0) or restore / set (flag 8) of the masked envs before step k (k = K: after the last step).
    ``scenario_rows`` ``[K, N]``: the row each env ran in step k (header word 6 = row + 1); ``open_scenario_rows`` ``[N]``: the rows
    of the open windows."""
    frames, keep, mask_on = resolve((frames, keep), on)
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.int32)   # noqa: E731
    qp, qv, act, inf = u32(qpos), u32(qvel), u32(actions), u32(info)
    K, N = act.shape[0], act.shape[1]
    nq, nv, nu, ni = qp.shape[2], qv.shape[2], act.shape[2], inf.shape[2]
    cm = None if commands is None else u32(commands)
    cd = 0 if cm is None else cm.shape[-1]
    te_all, tr_all = np.asarray(term).reshape(K, N) != 0, np.asarray(trunc).reshape(K, N) != 0
    nan_all = np.zeros((K + 1, N), dtype=np.int32) if meta4 is None else np.asarray(meta4, dtype=np.int32).reshape(K + 1, N)
    spawn_all = np.full((K + 1, N), -1, dtype=np.int32) if meta14 is None else np.asarray(meta14, dtype=np.int32).reshape(K + 1, N)
    cause_all = None if meta15 is None else np.asarray(meta15, dtype=np.int32).reshape(K, N)
    scn_all = None if scenario_rows is None else np.asarray(scenario_rows, dtype=np.int32).reshape(K, N)
    F = frame_words(nq, nv, nu, cd, ni)
    o_act = FRAME_HDR + nq + nv
    buf = np.zeros((N, keep + 1, HDR + frames * F), dtype=np.int32)
    work, trig, lost, cursor, length, episode, oflags, seen = (np.zeros(N, dtype=np.int64) for _ in range(8))
    nan0, spawn = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    ar = np.arange(N)

    def state_part(k, i):
        base = HDR + cursor[i] * F + FRAME_HDR
        for w in range(nq):
            buf[i, work[i], base + w] = qp[k, i, w]
        for w in range(nv):
            buf[i, work[i], base + nq + w] = qv[k, i, w]

    def begin(k, mask, flag):
        i = ar if mask is None else np.nonzero(np.asarray(mask).reshape(N))[0]
        cursor[i], length[i], oflags[i] = 0, 0, int(flag)
        spawn[i], nan0[i] = spawn_all[k][i], nan_all[k][i]
        state_part(k, i)

    begin(0, None, initial_flags)                                                 # cosim_ftrace_set
    for k in range(K + 1):
        for kb, mask, flag in begins:
            if kb == k:
                begin(k, mask, flag)
        if k == K:
            break
        te, tr = te_all[k], tr_all[k]
        length += 1
        seen += 1
        base = HDR + cursor * F
        buf[ar, work, base] = length
        buf[ar, work, base + 1] = te * TERMINATED | tr * TRUNCATED
        buf[ar, work, base + 2] = 0
        buf[ar, work, base + 3] = 0
        for w in range(nu):
            buf[ar, work, base + o_act + w] = act[k, :, w]
        for w in range(cd):
            buf[ar, work, base + o_act + nu + w] = cm[:, w] if cm.ndim == 2 else cm[k, :, w]
        for w in range(ni):
            buf[ar, work, base + o_act + nu + cd + w] = inf[k, :, w]
        done = te | tr
        flags = te * TERMINATED | tr * TRUNCATED | (nan_all[k + 1] != nan0) * NONFINITE | oflags
        if cause_all is not None:
            flags = flags | ((cause_all[k] & 7) << 5)
        fire = done & ((flags & mask_on) != 0)
        i = np.nonzero(fire)[0]
        if len(i):
            hdr = np.zeros((len(i), HDR), dtype=np.int32)
            hdr[:, 0], hdr[:, 1], hdr[:, 2] = episode[i], length[i], flags[i]
            hdr[:, 3] = np.minimum(length[i], frames)
            hdr[:, 4] = np.where(length[i] <= frames, 0, (cursor[i] + 1) % frames)
            hdr[:, 5], hdr[:, 7] = spawn[i], seen[i]
            hdr[:, 6] = 0 if scn_all is None else scn_all[k][i] + 1
            buf[i, work[i], :HDR] = hdr
            work[i] = (work[i] + 1) % (keep + 1)
            trig[i] += 1
            lost[i] += trig[i] > keep
        d = np.nonzero(done)[0]
        episode[d] += 1
        cursor[d], length[d], oflags[d] = 0, 0, 0
        spawn[d], nan0[d] = spawn_all[k + 1][d], nan_all[k + 1][d]
        nd = np.nonzero(~done)[0]
        cursor[nd] = (cursor[nd] + 1) % frames
        state_part(k + 1, ar)
    open_rows = None
    if include_open:
        open_rows = np.zeros((N, HDR), dtype=np.int32)
        open_rows[:, 0], open_rows[:, 1] = episode, length
        open_rows[:, 2] = OPEN | oflags | (nan_all[K] != nan0) * NONFINITE
        open_rows[:, 3] = np.minimum(length, frames - 1)
        open_rows[:, 4] = np.where(length <= frames - 1, 0, (cursor + 1) % frames)
        open_rows[:, 5], open_rows[:, 7] = spawn, seen
        open_rows[:, 6] = 0 if open_scenario_rows is None else np.asarray(open_scenario_rows, dtype=np.int32) + 1
    counts = np.stack([work, trig, lost], axis=1)
    dims = {"nq": nq, "nv": nv, "nu": nu, "command_dim": cd, "info_dim": ni}
    return FailureTraces.from_raw(buf, counts, open_rows, dims, mask_on, env_id0)
