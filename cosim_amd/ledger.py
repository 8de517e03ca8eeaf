"""Episode ledger: per-episode outcomes of a fleet (``cosim_ledger_set`` / ``cosim_ledger_get``, csrc/cosim_ledger.hip).

The engine closes every episode of every env into one 16-word record on the device (no host read per step); ``EpisodeLedger`` is
those records on the host -- one numpy array per field, rows sorted by (env, episode) -- with the summaries a fleet tester asks
for: how many robots fell and after how long, which, from which spawn row, how well each episode tracked its command.
``reference_ledger`` is the numpy twin of the kernel: the same operations in the same order on recorded step outputs, so its
records equal the device's bit for bit.  No torch, no GPU in this module.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import records as rc
from .records import (FELL, FELL_CONTACT, FELL_HEIGHT, FELL_TILT, NO_RESET, NONFINITE, OPEN, TERMINATED, TRUNCATED,  # noqa: F401
                      policy_of_records)

WORDS = 16
INT_FIELDS = {"episode": 0, "length": 1, "flags": 2, "spawn_row": 3, "steps_seen": 4}
FLOAT_FIELDS = {"mean_action_diff_RMSE": 5, "mean_tracking_err_0": 6, "mean_tracking_err_1": 7, "mean_tracking_err_2": 8,
                "mean_abs_torque": 9, "peak_abs_torque": 10, "mean_lin_vel_x": 11, "peak_tracking_err_0": 12}
SCENARIO_WORD = 13   # scenario row + 1 (0: no scenario table)
NSUM = 6   # action_diff_RMSE, lin_vel_x, tracking error 0..2, mean abs torque


class EpisodeLedger:
    """Records of a fleet's episodes.  ``words`` int32 ``[R, 16]`` is the record as the engine wrote it (include/cosim.h); every name
    in ``INT_FIELDS`` / ``FLOAT_FIELDS`` is an attribute holding that column (int32 / float32 ``[R]``).  ``env`` int64 ``[R]``: the
    global env id of each row; ``lost`` int64 ``[N]``: per env, how many ended episodes the ring of ``slots`` records overwrote
    before they were read.  Rows with flag 16 (``include_open``) are episodes still running; the summaries leave them out."""

    def __init__(self, words, env, lost, slots: int = 0, env_id0: int = 0):
        self.words = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, WORDS)
        self.env = np.ascontiguousarray(env, dtype=np.int64).reshape(-1)
        self.lost = np.ascontiguousarray(lost, dtype=np.int64).reshape(-1)
        self.slots, self.env_id0 = int(slots), int(env_id0)
        if len(self.env) != len(self.words):
            raise ValueError(f"EpisodeLedger: {len(self.words)} records but {len(self.env)} env ids")
        for name, w in INT_FIELDS.items():
            setattr(self, name, self.words[:, w])
        for name, w in FLOAT_FIELDS.items():
            setattr(self, name, self.words[:, w].view(np.float32))
        self.scenario = self.words[:, SCENARIO_WORD] - 1   # scenario-table row of the episode; -1: no table was set

    def __len__(self):
        return len(self.words)

    @classmethod
    def from_raw(cls, records, counts, open_rows=None, env_id0: int = 0) -> "EpisodeLedger":
        """From what ``cosim_ledger_get`` copies: rings ``[N, slots, 16]``, ended-episode counts ``[N]``, open rows ``[N, 16]`` or
        ``None``.  Episode ``o`` of an env lies in slot ``o mod slots``; the ring holds the last ``min(count, slots)``."""
        words, env, lost = rc.unroll_rings(records, counts, open_rows)
        return cls(words, env + int(env_id0), lost, np.shape(records)[1], env_id0)

    def ended(self) -> np.ndarray:
        """Mask of the rows that are ended episodes (not flag 16)."""
        return (self.flags & OPEN) == 0

    def counts(self) -> dict:
        """The integer sums a distributed run all-reduces (``cli.py``): every value adds over ranks."""
        m = self.ended()
        f, n = self.flags[m], self.length[m].astype(np.int64)
        return {"episodes": int(m.sum()), "terminated": int(((f & TERMINATED) != 0).sum()), "truncated": int(((f & TRUNCATED) != 0).sum()),
                "non_finite": int(((f & NONFINITE) != 0).sum()), "no_reset_start": int(((f & NO_RESET) != 0).sum()),
                "length_sum": int(n.sum()), "lost": int(self.lost.sum()),
                "fell": int(((f & FELL) != 0).sum()), "fell_tilt": int(((f & FELL_TILT) != 0).sum()),
                "fell_height": int(((f & FELL_HEIGHT) != 0).sum()), "fell_contact": int(((f & FELL_CONTACT) != 0).sum())}

    def summary(self) -> dict:
        """Episodes, how they ended, length quantiles (control steps) and the means over episodes of the record means (non-finite
        records, which only a non-finite state produces, are left out of those means and counted)."""
        m = self.ended()
        out = self.counts()
        n = self.length[m].astype(np.float64)
        e = out["episodes"]
        out["length"] = ({"mean": float(n.mean()), "min": int(n.min()), "p25": float(np.quantile(n, 0.25)), "p50": float(np.quantile(n, 0.5)),
                          "p75": float(np.quantile(n, 0.75)), "max": int(n.max())} if e else None)
        out["terminated_share"] = out["terminated"] / e if e else None
        out["fell_share"] = out["fell"] / e if e else None
        means, skipped = {}, 0
        for name in FLOAT_FIELDS:
            v = getattr(self, name)[m].astype(np.float64)
            ok = np.isfinite(v)
            skipped = max(skipped, int((~ok).sum()))
            means[name] = float(v[ok].mean()) if ok.any() else None
        out["means"] = means
        out["non_finite_records"] = skipped
        return out

    def _with_fell(self, fell: Optional[bool]) -> bool:
        """Whether the per-row tables carry the ``fell`` columns: asked for, or (``None``) some ended record has a fall flag.  A
        ledger kept without a fall rule so keeps the tables it had before there were rules."""
        return bool(fell) if fell is not None else bool(((self.flags[self.ended()] & FELL) != 0).any())

    def by_spawn_row(self, fell: Optional[bool] = None) -> dict:
        """Per spawn-table row (``-1``: no table): ended episodes that started there and the share of them that terminated; with
        ``fell`` (default: if any record has a fall flag) also the count and share a fall rule ended (flags 32 / 64 / 128)."""
        with_fell = self._with_fell(fell)
        m = self.ended()
        rows, term, fallen = self.spawn_row[m], (self.flags[m] & TERMINATED) != 0, (self.flags[m] & FELL) != 0
        out = {}
        for r in np.unique(rows):
            sel = rows == r
            out[int(r)] = {"episodes": int(sel.sum()), "terminated": int(term[sel].sum()), "terminated_share": float(term[sel].mean())}
            if with_fell:
                out[int(r)].update({"fell": int(fallen[sel].sum()), "fell_share": float(fallen[sel].mean())})
        return out

    def by_scenario(self, fell: Optional[bool] = None) -> dict:
        """Per scenario-table row (``-1``: no table): ended episodes that ran it, the share of them that terminated -- with ``fell``
        (default: if any record has a fall flag) also the count and share a fall rule ended --, length
        quantiles (control steps) and the means over those episodes of the record means (non-finite records left out)."""
        m = self.ended()
        with_fell = self._with_fell(fell)
        return {int(r): self._cell(m & (self.scenario == r), with_fell) for r in np.unique(self.scenario[m])}

    def _cell(self, sel, with_fell: bool) -> dict:
        """The columns of ``by_scenario()`` / ``by_policy()`` over the records under mask ``sel`` (at least one, all ended)."""
        term, n, fallen = (self.flags[sel] & TERMINATED) != 0, self.length[sel].astype(np.float64), (self.flags[sel] & FELL) != 0
        means = {}
        for name in FLOAT_FIELDS:
            v = getattr(self, name)[sel].astype(np.float64)
            ok = np.isfinite(v)
            means[name] = float(v[ok].mean()) if ok.any() else None
        return {"episodes": int(sel.sum()), "terminated": int(term.sum()), "terminated_share": float(term.mean()),
                **({"fell": int(fallen.sum()), "fell_share": float(fallen.mean())} if with_fell else {}),
                "length": {"mean": float(n.mean()), "min": int(n.min()), "p50": float(np.quantile(n, 0.5)), "max": int(n.max())},
                "means": means}

    def by_policy(self, table, scenario: bool = False, fell: Optional[bool] = None) -> dict:
        """Per policy of a ``policy.PolicyTable`` (or of an int array: the policy of each LOCAL env, named "0", "1", ...): the columns
        of ``by_scenario()`` over the ended episodes of the envs that policy drives, keyed by the policy's name -- with ``scenario``
        by ``(name, scenario row)``, the checkpoint x scenario matrix.  An env's policy is looked up from its global id; a policy
        (or a cell) without an ended episode has no entry.  Under a ROTATING table a record belongs to the policy that drove that episode,
        ``table.policy_of(env, episode ordinal)``: the ordinals are the table's counters when the ledger was armed in the env's
        constructor and the table drove the env from its first step."""
        with_fell = self._with_fell(fell)
        return {key: self._cell(sel, with_fell) for key, sel in rc.policy_cells(self, table, scenario)}

    def save(self, path: str):
        """One ``.npz`` of plain arrays (no pickle)."""
        np.savez(path, words=self.words, env=self.env, lost=self.lost, header=rc.header(self.slots, self.env_id0))

    @classmethod
    def load(cls, path: str) -> "EpisodeLedger":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["words"], z["env"], z["lost"], *rc.read_header(z))


def _records(episode, length, flags, spawn, seen, s, peak, scenario=None) -> np.ndarray:
    """``ledger_store``: the 16 words of one record per column of the accumulators."""
    n = len(episode)
    w = np.zeros((n, WORDS), dtype=np.int32)
    w[:, 0], w[:, 1], w[:, 2], w[:, 3], w[:, 4] = episode, length, flags, spawn, seen
    f = w.view(np.float32)
    with np.errstate(all="ignore"):
        mean = np.where(length[None, :] > 0, s / np.maximum(length, 1).astype(np.float64)[None, :], 0.0).astype(np.float32)
    f[:, 5], f[:, 6], f[:, 7], f[:, 8], f[:, 9], f[:, 11] = mean[0], mean[2], mean[3], mean[4], mean[5], mean[1]
    f[:, 10], f[:, 12] = peak[0], peak[1]
    if scenario is not None:
        w[:, SCENARIO_WORD] = np.asarray(scenario, dtype=np.int32) + 1
    return w


def reference_ledger(info_rows, terminated, truncated, commands, nan_resets, spawn_rows, slots: int, nu: int, command_dim: int,
                     include_open: bool = False, initial_flags: int = 0, begins: Sequence = (), env_id0: int = 0, scenario_rows=None,
                     open_scenario_rows=None, causes=None) -> EpisodeLedger:
    """Numpy twin of ``ledger_step_kernel`` / ``ledger_begin_kernel`` / ``ledger_open_kernel``: sequential float64 adds of float32
    values, float32 subtraction / sum / divide where the kernel does them in float32, ``np.fmax`` for the peaks.

    ``info_rows`` ``[K, N, info_dim]``, ``terminated`` / ``truncated`` ``[K, N]``: what K control steps returned.  ``commands``:
    the raw user commands ``[N, >= command_dim]`` (or ``[K, N, .]``, one per step).  ``nan_resets`` / ``spawn_rows`` ``[K + 1, N]``:
    the engine's meta words 4 / 14 BEFORE step k in row k and after the last step in row K (``None``: no non-finite reset / no
    spawn table, -1); step k's record logic reads row k + 1, which is what the kernel finds behind step k.  ``initial_flags``: 8 if
    the ledger was set on a stepped fleet.  ``begins``: ``(k, mask or None, flag)`` -- a host reset (flag 0) or restore / set (flag
    8) of the masked envs before step k (k = K: after the last step).  ``scenario_rows`` ``[K, N]`` (a scenario table was set): the
    row each env ran in step k (``BatchedEnv.scenario_rows()`` after the step) -- word 13 of a record that step k closes is that
    row + 1; ``commands`` is then the per-step applied command.  ``open_scenario_rows`` ``[N]``: the rows of the open records (the
    table's rule at the meta words after the last step).  ``causes`` ``[K, N]`` (a fall rule was set, cosim_amd/fall.py): the
    engine's meta word 15 after step k (``BatchedEnv.end_cause()``) -- a record that step k closes gets ``(cause & 7) << 5`` in
    its flags; ``None`` (no rule): the records of a ledger without fall rules, bit for bit."""
    info = np.asarray(info_rows, dtype=np.float32)
    K, N = info.shape[0], info.shape[1]
    te_all, tr_all = np.asarray(terminated).reshape(K, N), np.asarray(truncated).reshape(K, N)
    ncmd = min(int(command_dim), 3)
    cmd = None if ncmd == 0 else np.asarray(commands, dtype=np.float32)
    nan_all = np.zeros((K + 1, N), dtype=np.int32) if nan_resets is None else np.asarray(nan_resets, dtype=np.int32).reshape(K + 1, N)
    spawn_all = np.full((K + 1, N), -1, dtype=np.int32) if spawn_rows is None else np.asarray(spawn_rows, dtype=np.int32).reshape(K + 1, N)
    slots = int(slots)
    scn_all = None if scenario_rows is None else np.asarray(scenario_rows, dtype=np.int32).reshape(K, N)
    cause_all = None if causes is None else np.asarray(causes, dtype=np.int32).reshape(K, N)
    s = np.zeros((NSUM, N), dtype=np.float64)
    peak = np.zeros((2, N), dtype=np.float32)
    length, seen, episode = (np.zeros(N, dtype=np.int32) for _ in range(3))
    oflags = np.full(N, int(initial_flags), dtype=np.int32)
    spawn, nan0 = spawn_all[0].copy(), nan_all[0].copy()
    ring = np.zeros((N, slots, WORDS), dtype=np.int32)

    def begin(k):
        for kb, mask, flag in begins:
            if kb != k:
                continue
            m = np.ones(N, dtype=bool) if mask is None else np.asarray(mask).astype(bool).reshape(N)
            s[:, m] = 0.0
            peak[:, m] = 0.0
            length[m] = 0
            oflags[m] = int(flag)
            spawn[m] = spawn_all[k][m]
            nan0[m] = nan_all[k][m]

    f32 = np.float32
    with np.errstate(all="ignore"):
        for k in range(K):
            begin(k)
            row = info[k]
            length += 1
            seen += 1
            s[0] += row[:, 0].astype(np.float64)
            s[1] += row[:, 1].astype(np.float64)
            e0 = np.zeros(N, dtype=f32)
            c = None if cmd is None else (cmd if cmd.ndim == 2 else cmd[k])
            for q in range(ncmd):
                d = np.abs(c[:, q] - row[:, 1 + q])
                assert d.dtype == f32
                s[2 + q] += d.astype(np.float64)
                if q == 0:
                    e0 = d
            tq, tmax = np.zeros(N, dtype=f32), np.zeros(N, dtype=f32)
            for j in range(int(nu)):
                t = np.abs(row[:, 4 + j])
                tq = tq + t
                tmax = np.fmax(tmax, t)
            s[5] += (tq / f32(nu)).astype(np.float64)
            peak[0] = np.fmax(peak[0], tmax)
            if ncmd > 0:
                peak[1] = np.fmax(peak[1], e0)
            te, tr = te_all[k] != 0, tr_all[k] != 0
            done = te | tr
            if done.any():
                i = np.nonzero(done)[0]
                flags = (te[i] * TERMINATED) | (tr[i] * TRUNCATED) | ((nan_all[k + 1][i] != nan0[i]) * NONFINITE) | oflags[i]
                if cause_all is not None:
                    flags = flags | ((cause_all[k][i] & 7) << 5)
                ring[i, episode[i] % slots] = _records(episode[i], length[i], flags.astype(np.int32), spawn[i], seen[i], s[:, i], peak[:, i],
                                                         None if scn_all is None else scn_all[k][i])
                episode[i] += 1
                s[:, i] = 0.0
                peak[:, i] = 0.0
                length[i] = 0
                oflags[i] = 0
                spawn[i] = spawn_all[k + 1][i]
                nan0[i] = nan_all[k + 1][i]
        begin(K)
        open_rows = None
        if include_open:
            flags = OPEN | oflags | ((nan_all[K] != nan0) * NONFINITE)
            open_rows = _records(episode, length, flags.astype(np.int32), spawn, seen, s, peak, open_scenario_rows)
    return EpisodeLedger.from_raw(ring, episode, open_rows, env_id0)


def same_records(a: EpisodeLedger, b: EpisodeLedger) -> Optional[str]:
    """``None`` if two ledgers hold the same rows -- ints as ints, floats as float32 bits, two non-finite floats count as equal --,
    else a sentence naming the first difference."""
    head = rc.same_rows(a, b)
    if head is not None:
        return head
    for name, w in list(INT_FIELDS.items()) + [("scenario + 1", SCENARIO_WORD), ("padding", 14), ("padding", 15)]:
        bad = np.nonzero(a.words[:, w] != b.words[:, w])[0]
        if len(bad):
            r = bad[0]
            return f"{name}: row {r} (env {a.env[r]}, episode {a.words[r, 0]}): {a.words[r, w]} against {b.words[r, w]}"
    for name, w in FLOAT_FIELDS.items():
        x, y = a.words[:, w], b.words[:, w]
        fx, fy = x.view(np.float32), y.view(np.float32)
        bad = np.nonzero((x != y) & ~(~np.isfinite(fx) & ~np.isfinite(fy)))[0]
        if len(bad):
            r = bad[0]
            return f"{name}: row {r} (env {a.env[r]}, episode {a.words[r, 0]}): {fx[r]!r} against {fy[r]!r}"
    return None
