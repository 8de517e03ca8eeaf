"""Scenario checks: per-scenario pass / fail criteria judged on the device (``cosim_scenario_checks_set`` /
``cosim_scenario_checks_get``, csrc/cosim_checks.hip).

A scenario of a ``ScenarioTable`` may hold checks (``cosim_amd/scenario.py``): timed criteria on a signal of the step.  The engine
evaluates them behind every control step and closes them, when an episode ends, into one verdict record per episode on the device (no
host read per step).  ``Verdicts`` is those records on the host -- one numpy array per field, rows sorted by (env, episode) -- with
the summaries a sweep asks for; ``(env, episode)`` joins a row to the ledger's and the failure traces'.  ``reference_checks`` is the
numpy twin of the three kernels: the same operations in the same order on recorded step outputs, so its records equal the device's
bit for bit.  No torch, no GPU in this module.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import records as rc
from .records import NO_RESET, OPEN, TERMINATED, TRUNCATED  # noqa: F401

HDR = 8
NONE_BITS = 0x7FC00000          # value word with no sample behind it
INFO, ABS_INFO, TRACKING_ERROR, TORQUE_MAX, UP, QPOS, QVEL, ABS_QVEL = range(8)
ALWAYS, SETTLE, MEAN = range(3)
LT, GT = 0, 1


def items_per_record(table) -> int:
    """I: the largest item count of any scenario, rounded up to even."""
    return (max(len(c) for c in table._resolved_checks()) + 1) & ~1


class Verdicts:
    """Verdict records of a fleet's episodes.  ``words`` int32 ``[R, 8 + 2 I]`` is the record as the engine wrote it (include/cosim.h).
    Per row: ``env`` (global id), ``episode``, ``length``, ``flags`` (1 terminated | 2 truncated | 8 did not begin at a reset | 16
    open), ``scenario`` (table row); per row and item ``[R, I]``: ``valid`` (the scenario has that item), ``failed``,
    ``incomplete``, ``passed`` (valid, complete and not failed), ``value`` float32 (always / settle: the sample furthest on the failing
    side; mean: the mean; NaN with no sample), ``aux`` (always: step of the first violation or -1; settle: step of the last violation
    or -1; mean: samples) and ``settle_time`` (settle items: ``aux + 1 - t0``, 0 if never bad; -1 for other modes).  ``names[s][k]``:
    the name of item k of scenario s.  ``lost`` int64 ``[N]``: per env, how many ended episodes the ring overwrote."""

    def __init__(self, words, env, lost, names, item_mode, item_t, slots: int = 0, env_id0: int = 0):
        self.item_mode = np.ascontiguousarray(item_mode, dtype=np.int32)          # [S, I], -1: no such item
        self.item_t = np.ascontiguousarray(item_t, dtype=np.int32)                # [S, I, 2]
        S, I = self.item_mode.shape
        self.words = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, HDR + 2 * I)
        self.env = np.ascontiguousarray(env, dtype=np.int64).reshape(-1)
        self.lost = np.ascontiguousarray(lost, dtype=np.int64).reshape(-1)
        self.names = [list(n) for n in names]
        self.slots, self.env_id0 = int(slots), int(env_id0)
        if len(self.env) != len(self.words):
            raise ValueError(f"Verdicts: {len(self.words)} records but {len(self.env)} env ids")
        w = self.words
        self.episode, self.length, self.flags, self.scenario = w[:, 0], w[:, 1], w[:, 2], w[:, 3] - 1
        bits = lambda lo, hi: (((w[:, lo].astype(np.int64) & 0xFFFFFFFF) | ((w[:, hi].astype(np.int64) & 0xFFFFFFFF) << 32)).astype(np.uint64)[:, None]  # noqa: E731
                               >> np.arange(I, dtype=np.uint64)[None, :]) & np.uint64(1)
        self.failed, self.incomplete = bits(4, 5) != 0, bits(6, 7) != 0
        row = np.clip(self.scenario, 0, S - 1)
        self.mode = self.item_mode[row]                                            # [R, I]
        self.valid = self.mode >= 0
        self.passed = self.valid & ~self.failed & ~self.incomplete
        self.value = np.ascontiguousarray(w[:, HDR::2]).view(np.float32)
        self.aux = w[:, HDR + 1::2]
        t0 = self.item_t[row][:, :, 0]
        self.settle_time = np.where(self.mode == SETTLE, np.where(self.aux < 0, 0, self.aux + 1 - t0), -1).astype(np.int64)

    def __len__(self):
        return len(self.words)

    @classmethod
    def from_raw(cls, records, counts, open_rows, table, env_id0: int = 0) -> "Verdicts":
        """From what ``cosim_scenario_checks_get`` copies: rings ``[N, slots, W]``, ended-episode counts ``[N]``, open rows ``[N, W]`` or
        ``None``; ``table``: the ``ScenarioTable`` whose checks were set."""
        words, env, lost = rc.unroll_rings(records, counts, open_rows)
        names, mode, t = item_tables(table)
        return cls(words, env + int(env_id0), lost, names, mode, t, np.shape(records)[1], env_id0)

    def ended(self) -> np.ndarray:
        """Mask of the rows that are ended episodes (not flag 16)."""
        return (self.flags & OPEN) == 0

    def _shares(self, m) -> dict:
        """Counts over the rows under mask ``m``: episodes by their worst item, and items."""
        v, f, i, p = self.valid[m], self.failed[m] & self.valid[m], self.incomplete[m] & self.valid[m], self.passed[m]
        ep_failed = f.any(axis=1)
        ep_incomplete = ~ep_failed & i.any(axis=1)
        return {"episodes": int(m.sum()), "episodes_failed": int(ep_failed.sum()), "episodes_incomplete": int(ep_incomplete.sum()),
                "episodes_passed": int((~ep_failed & ~ep_incomplete).sum()), "items": int(v.sum()), "items_passed": int(p.sum()),
                "items_failed": int(f.sum()), "items_incomplete": int((i & ~f).sum())}

    def counts(self) -> dict:
        """The integer sums a distributed run all-reduces (``cli.py``): every value adds over ranks.  An episode counts as failed if
        any of its items failed, as incomplete if none failed and one was incomplete, as passed otherwise."""
        out = self._shares(self.ended())
        out["lost"] = int(self.lost.sum())
        return out

    @staticmethod
    def with_shares(c: dict) -> dict:
        """``counts()`` (possibly summed over ranks) with the shares derived from it."""
        out = dict(c)
        e, n = c["episodes"], c["items"]
        for k in ("passed", "failed", "incomplete"):
            out[f"episodes_{k}_share"] = c[f"episodes_{k}"] / e if e else None
            out[f"items_{k}_share"] = c[f"items_{k}"] / n if n else None
        return out

    def _by_name(self, m) -> dict:
        out = {}
        rows = np.nonzero(m)[0]
        for r in rows:
            s = int(self.scenario[r])
            for k, name in enumerate(self.names[s] if 0 <= s < len(self.names) else []):
                d = out.setdefault(name, {"items": 0, "passed": 0, "failed": 0, "incomplete": 0, "_settle": []})
                d["items"] += 1
                d["passed"] += int(self.passed[r, k])
                d["failed"] += int(self.failed[r, k])
                d["incomplete"] += int(self.incomplete[r, k] and not self.failed[r, k])
                if self.mode[r, k] == SETTLE and not self.incomplete[r, k]:
                    d["_settle"].append(int(self.settle_time[r, k]))
        for d in out.values():
            st = d.pop("_settle")
            n = d["items"]
            d.update({"passed_share": d["passed"] / n, "failed_share": d["failed"] / n, "incomplete_share": d["incomplete"] / n})
            if st:
                q = np.asarray(st, dtype=np.float64)
                d["settle_time"] = {"min": int(q.min()), "p50": float(np.quantile(q, 0.5)), "p90": float(np.quantile(q, 0.9)), "max": int(q.max())}
        return out

    def summary(self) -> dict:
        """Ended episodes and the share of them (and of their items) that passed / failed / were incomplete, overall and per named
        check (``checks``: name -> counts, shares and, for settle items with a complete window, settle-time quantiles in steps)."""
        out = self.with_shares(self.counts())
        out["checks"] = self._by_name(self.ended())
        return out

    def by_scenario(self) -> dict:
        """``summary()`` per scenario-table row."""
        m = self.ended()
        out = {}
        for r in np.unique(self.scenario[m]):
            sel = m & (self.scenario == r)
            out[int(r)] = {**self.with_shares(self._shares(sel)), "checks": self._by_name(sel)}
        return out

    def by_policy(self, table, scenario: bool = False) -> dict:
        """``summary()`` per policy of a ``policy.PolicyTable`` (or of an int array with the policy of each local env), keyed by the
        policy's name, with ``scenario`` by ``(name, scenario row)``: as ``EpisodeLedger.by_policy``, a rotating table included (a
        record belongs to the policy of its episode ordinal)."""
        return {key: {**self.with_shares(self._shares(sel)), "checks": self._by_name(sel)} for key, sel in rc.policy_cells(self, table, scenario)}

    def join(self, ledger) -> np.ndarray:
        """Per verdict row, the row of ``ledger`` (an ``EpisodeLedger``, or anything with ``env`` and ``episode`` columns such as
        ``FailureTraces``) with the same (env, episode), or -1: int64 ``[R]``.  The ordinals agree when both were set together."""
        return rc.join(self, ledger)

    def save(self, path: str):
        """One ``.npz`` of plain arrays (no pickle)."""
        S, I = self.item_mode.shape
        names = np.array([[(n[k] if k < len(n) else "") for k in range(I)] for n in self.names], dtype=np.str_).reshape(S, I)
        np.savez(path, words=self.words, env=self.env, lost=self.lost, names=names, item_mode=self.item_mode, item_t=self.item_t,
                 header=rc.header(self.slots, self.env_id0))

    @classmethod
    def load(cls, path: str) -> "Verdicts":
        with np.load(path, allow_pickle=False) as z:
            mode = z["item_mode"]
            names = [[str(z["names"][s, k]) for k in range(mode.shape[1]) if mode[s, k] >= 0] for s in range(mode.shape[0])]
            return cls(z["words"], z["env"], z["lost"], names, mode, z["item_t"], *rc.read_header(z))


def item_tables(table):
    """``(names [S][k], mode int32 [S, I] (-1: no such item), t int32 [S, I, 2])`` of a table's resolved checks."""
    C = table._resolved_checks()
    S, I = len(C), items_per_record(table)
    mode, t = np.full((S, I), -1, dtype=np.int32), np.zeros((S, I, 2), dtype=np.int32)
    for s, items in enumerate(C):
        for k, it in enumerate(items):
            mode[s, k], t[s, k] = it[4], (it[0], it[1])
    return table.check_item_names(), mode, t


def same_verdicts(a: Verdicts, b: Verdicts) -> Optional[str]:
    """``None`` if two sets of verdicts hold the same rows word for word (floats as their bits), else a sentence naming the first
    difference."""
    head = rc.same_rows(a, b, lost_values=True)
    if head is not None:
        return head
    if a.words.shape != b.words.shape:
        return f"record words {a.words.shape[1]} against {b.words.shape[1]}"
    bad = rc.first_difference(a.words, b.words)
    if bad is not None:
        r, w = bad
        return f"row {r} (env {a.env[r]}, episode {a.words[r, 0]}), word {w}: {a.words[r, w]} against {b.words[r, w]}"
    return None


def _signal(sig, idx, info, cmd, qpos, qvel, nu):
    """``checks_signal`` for one env: float32, operation by operation."""
    f32 = np.float32
    if sig == INFO:
        return f32(info[idx])
    if sig == ABS_INFO:
        return np.abs(f32(info[idx]))
    if sig == TRACKING_ERROR:
        return np.abs(f32(cmd[idx]) - f32(info[1 + idx]))
    if sig == TORQUE_MAX:
        m = f32(0.0)
        for j in range(nu):
            m = np.fmax(m, np.abs(f32(info[4 + j])))
        return f32(m)
    if sig == UP:
        from .fall import up_component
        return f32(up_component(qpos[None, :])[0])
    if sig == QPOS:
        return f32(qpos[idx])
    if sig == QVEL:
        return f32(qvel[idx])
    return np.abs(f32(qvel[idx]))


def _cmp(op, v, bound) -> bool:
    return bool(v < bound) if op == LT else bool(v > bound)


class _Acc:
    __slots__ = ("ext", "aux", "n", "sum")

    def __init__(self):
        self.ext, self.aux, self.n, self.sum = None, -1, 0, np.float64(0.0)


def _verdict(x: _Acc, item):
    """``checks_verdict``: ``(value bits, aux, failed, incomplete)``."""
    t0, t1, _, _, mode, op, bound = item[:7]
    inc = x.n < t1 - t0
    with np.errstate(all="ignore"):
        if mode == MEAN:
            if x.n == 0:
                return NONE_BITS, 0, False, inc
            m = np.float32(x.sum / np.float64(x.n))
            return (NONE_BITS if np.isnan(m) else int(m.view(np.int32))), x.n, not _cmp(op, m, bound), inc
        value = NONE_BITS if x.ext is None else int(np.float32(x.ext).view(np.int32))
        return value, x.aux, (x.aux >= 0 if mode == ALWAYS else (not inc and x.aux == t1 - 1)), inc


def _record(I, items, accs, episode, length, flags, row):
    w = np.zeros(HDR + 2 * I, dtype=np.int64)
    fail = inc = 0
    for k, it in enumerate(items):
        value, aux, f, n = _verdict(accs[k], it)
        fail |= int(f) << k
        inc |= int(n) << k
        w[HDR + 2 * k], w[HDR + 2 * k + 1] = value, aux
    w[:HDR] = [episode, length, flags, row + 1, fail & 0xFFFFFFFF, fail >> 32, inc & 0xFFFFFFFF, inc >> 32]
    return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def reference_checks(table, info_rows, terminated, truncated, commands, qpos, qvel, clock, scenario_rows, slots: int, nu: int,
                     include_open: bool = False, initial_flags: int = 0, begins: Sequence = (), env_id0: int = 0,
                     open_scenario_rows=None) -> Verdicts:
    """Numpy twin of ``checks_step_kernel`` / ``checks_begin_kernel`` / ``checks_open_kernel``.

    ``table``: the ``ScenarioTable`` with resolved checks.  ``info_rows`` ``[K, N, info_dim]``, ``terminated`` / ``truncated`` ``[K,
    N]``, ``commands`` ``[K, N, >= command_dim]`` (or ``[N, .]``): what K control steps returned and the command they applied;
    ``qpos`` ``[K, N, nq]`` / ``qvel`` ``[K, N, nv]``: the state record read back behind step k.  ``clock`` ``[K + 1, N]``: the
    engine's meta word 0 before step k in row k (after whatever the host did ahead of it) and after the last step in row K.  The twin
    keeps the kernel's clock word: set to ``clock[k]`` by a begin ahead of step k and to ``clock[k + 1]`` behind step k; step k's
    ``t`` is the word it finds.  ``scenario_rows`` ``[K, N]``: the row each env ran in step k (``BatchedEnv.scenario_rows()`` after
    the step); ``open_scenario_rows`` ``[N]``: the rows of the open records.  ``initial_flags``: 8 if the checks were set on a
    stepped fleet.  ``begins``: ``(k, mask or None, flag)`` -- a host reset (flag 0) or restore / set / checks rewrite (flag 8) of
    the masked envs before step k (k = K: after the last step)."""
    C = table._resolved_checks()
    I = items_per_record(table)
    info = np.asarray(info_rows, dtype=np.float32)
    K, N = info.shape[0], info.shape[1]
    te_all, tr_all = np.asarray(terminated).reshape(K, N) != 0, np.asarray(truncated).reshape(K, N) != 0
    cmd = None if commands is None else np.asarray(commands, dtype=np.float32)
    qpos, qvel = np.asarray(qpos, dtype=np.float32), np.asarray(qvel, dtype=np.float32)
    clock_all = np.asarray(clock, dtype=np.int64).reshape(K + 1, N)
    rows_all = np.asarray(scenario_rows, dtype=np.int64).reshape(K, N)
    slots = int(slots)
    W = HDR + 2 * I
    ring = np.zeros((N, slots, W), dtype=np.int32)
    episode, length = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    oflags = np.full(N, int(initial_flags), dtype=np.int64)
    clk = clock_all[0].copy()
    accs = [[_Acc() for _ in range(I)] for _ in range(N)]

    def begin(k):
        for kb, mask, flag in begins:
            if kb != k:
                continue
            m = np.ones(N, dtype=bool) if mask is None else np.asarray(mask).astype(bool).reshape(N)
            for i in np.nonzero(m)[0]:
                accs[i] = [_Acc() for _ in range(I)]
                length[i], oflags[i], clk[i] = 0, int(flag), clock_all[k][i]

    with np.errstate(all="ignore"):
        for k in range(K):
            begin(k)
            for i in range(N):
                te, tr = bool(te_all[k, i]), bool(tr_all[k, i])
                done = te or tr
                t, row = int(clk[i]), int(rows_all[k, i])
                items = C[row]
                c = None if cmd is None else (cmd[i] if cmd.ndim == 2 else cmd[k, i])
                for j, it in enumerate(items):
                    t0, t1, sig, idx, mode, op, bound = it[:7]
                    if not (t0 <= t < t1) or (done and sig >= UP):
                        continue
                    x = accs[i][j]
                    v = _signal(sig, idx, info[k, i], c, qpos[k, i], qvel[k, i], int(nu))
                    x.n += 1
                    if mode == MEAN:
                        x.sum = x.sum + np.float64(v)
                        continue
                    if not np.isnan(v) and (x.ext is None or (v > x.ext if op == LT else v < x.ext)):
                        x.ext = v
                    if not _cmp(op, v, bound) and (mode == SETTLE or x.aux < 0):
                        x.aux = t
                length[i] += 1
                if done:
                    flags = (TERMINATED if te else 0) | (TRUNCATED if tr else 0) | int(oflags[i])
                    ring[i, episode[i] % slots] = _record(I, items, accs[i], int(episode[i]), int(length[i]), flags, row)
                    accs[i] = [_Acc() for _ in range(I)]
                    episode[i] += 1
                    length[i], oflags[i] = 0, 0
                clk[i] = clock_all[k + 1][i]
        begin(K)
        open_rows = None
        if include_open:
            orow = np.asarray(open_scenario_rows, dtype=np.int64).reshape(N)
            open_rows = np.stack([_record(I, C[int(orow[i])], accs[i], int(episode[i]), int(length[i]), OPEN | int(oflags[i]), int(orow[i]))
                                  for i in range(N)])
    return Verdicts.from_raw(ring, episode, open_rows, table, env_id0)
