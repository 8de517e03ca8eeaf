"""Limit search: a per-env staircase on a scenario's push, command, parameter-window and fault scale, kept on the device (``cosim_set_param "search"``,
csrc/cosim_search.hip).

"What is the hardest push this checkpoint survives?"  A scenario of a ``ScenarioTable`` may hold one search item
(``cosim_amd/scenario.py``).  Every env of such a row keeps a LEVEL in ``[lo, hi]`` that the scenario kernel multiplies into the
row's pushes and / or command keyframes, and the parameter-window and fault kernels into the values of the row's marked items; when an
episode of the env ends, a small rule on the device moves the level down after a failure and up after a pass (``harder="down"``: the
other way round) -- no host read, no re-planning between runs.  A failure is a ledger flag of the item's ``fail_on`` or a selected
check of the ended episode that did not pass.  ``SearchResult`` is the per-env records and the trial rings
on the host, with the summaries a sweep asks for; ``(env, episode)`` joins a trial to the ledger's record of the same episode.
``SearchTwin`` / ``reference_search`` are the numpy twin of the three kernels: the same float32 operations in the same order, so its
words equal the device's bit for bit.  No torch, no GPU in this module.

Record words (int32 ``[N, 16]``): 0 level, 1 step, 2 trials, 3 fails, 4 last_dir, 5 reversals, 6 rev_sum, 7 rev_n, 8 hi_pass, 9
lo_fail, 10 status (1 the open episode began at a reset | 2 done | 4 has a pass | 8 has a fail | 16 the row has an item), 11 episodes
ended since arming, 12 length of the open episode, 13 meta word 4 at its start, 14 ended episodes that were no trials, 15 zero.
Trial words (int32 ``[N, slots, 4]``, episode ``o`` in slot ``o mod slots``): episode, the level it RAN at, flags | 256 counted | 512
failed | 1024 reversal | 2048 failed by a check, length.  With ``harder="down"`` word 8 holds the LOWEST pass and word 9 the HIGHEST failure.
"""
from __future__ import annotations

import json
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np

from . import records as rc
from .scenario import SEARCH_RULES, scenario_rows, search_fail_mask

NCNT, TRIAL_WORDS = 16, 4
LEVEL, STEP, TRIALS, FAILS, LAST_DIR, REVERSALS, REV_SUM, REV_N, HI_PASS, LO_FAIL, STATUS, EPISODE, LENGTH, NAN0, UNCOUNTED = range(15)
AT_RESET, DONE, HAS_PASS, HAS_FAIL, HAS_ITEM = 1, 2, 4, 8, 16
COUNTED, FAILED, REVERSAL, BY_CHECK = 256, 512, 1024, 2048
_F32 = np.float32


def _bits(x) -> int:
    return int(np.float32(x).view(np.int32))


def _float(w) -> np.float32:
    return np.int32(w).view(np.float32)


def ledger_flags(te: bool, tr: bool, nan_now: int, nan0: int, at_reset: bool, fall: bool, meta15: int) -> int:
    """An ended episode's flags as ``ledger_step_kernel`` builds them (``search_flags``, csrc/cosim_search.h)."""
    return ((rc.TERMINATED if te else 0) | (rc.TRUNCATED if tr else 0) | (rc.NONFINITE if int(nan_now) != int(nan0) else 0)
            | (0 if at_reset else rc.NO_RESET) | (((int(meta15) & 7) << 5) if fall else 0))


class SearchTwin:
    """The numpy twin of ``search_init_kernel`` / ``search_step_kernel`` / ``search_begin_kernel``, advanced call by call.

    ``table``: the ``ScenarioTable`` with the search items; ``rows`` int ``[N]``: the table row of every env (mode ``env``: it never
    changes); ``fall``: a fall rule is set (meta word 15 is read); ``flag``: 8 if the search was armed on a stepped fleet; ``meta4``
    ``[N]``: meta word 4 when the search was armed.  ``state`` int32 ``[N, 16]`` and ``ring`` int32 ``[N, slots, 4]`` are the
    device's buffers, ``remaining`` its one word."""

    def __init__(self, table, slots: int, rows, fall: bool = False, flag: int = 0, meta4=None):
        self.table, self.slots, self.fall = table, int(slots), bool(fall)
        self.rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        N = len(self.rows)
        self.state = np.zeros((N, NCNT), dtype=np.int32)
        self.ring = np.zeros((N, self.slots, TRIAL_WORDS), dtype=np.int32)
        meta4 = np.zeros(N, dtype=np.int64) if meta4 is None else np.asarray(meta4, dtype=np.int64).reshape(N)
        self.remaining = 0
        for i in range(N):
            it = table.search[int(self.rows[i])]
            if it is not None:
                self.state[i, LEVEL], self.state[i, STEP] = _bits(it["start"]), _bits(it["step"])
                self.remaining += 1
            self.state[i, STATUS] = (HAS_ITEM if it is not None else 0) | (AT_RESET if int(flag) == 0 else 0)
            self.state[i, NAN0] = int(meta4[i])

    def levels(self) -> np.ndarray:
        """float32 ``[N]``: the level each env's next step runs at (0 for an env without an item)."""
        return np.ascontiguousarray(self.state[:, LEVEL]).view(np.float32).copy()

    def begin(self, mask, flag: int, meta4):
        """Behind a reset (``flag`` 0) or a restore / set_state (8) of the masked envs (``None``: all): the open episode is discarded,
        the level does not move."""
        N = len(self.rows)
        m = np.ones(N, dtype=bool) if mask is None else np.asarray(mask).astype(bool).reshape(N)
        meta4 = np.asarray(meta4, dtype=np.int64).reshape(N)
        for i in np.nonzero(m)[0]:
            s = self.state[i]
            s[STATUS] = (int(s[STATUS]) & ~AT_RESET) | (AT_RESET if int(flag) == 0 else 0)
            s[LENGTH], s[NAN0] = 0, int(meta4[i])

    def _trial(self, s, it, fail: bool) -> int:
        """``search_trial``: one counted trial, float32 operation by operation."""
        x, step = _float(s[LEVEL]), _float(s[STEP])
        lo, hi, d_min = _F32(it["lo"]), _F32(it["hi"]), _F32(it["min_step"])
        status, last = int(s[STATUS]), int(s[LAST_DIR])
        down = it["harder"] == "down"
        d = -1 if fail != down else 1
        if fail:
            s[LO_FAIL] = _bits((np.fmax if down else np.fmin)(_float(s[LO_FAIL]), x) if status & HAS_FAIL else x)
            status |= HAS_FAIL
        else:
            s[HI_PASS] = _bits((np.fmin if down else np.fmax)(_float(s[HI_PASS]), x) if status & HAS_PASS else x)
            status |= HAS_PASS
        rev = last != 0 and d != last
        if rev:
            s[REVERSALS] += 1
            if int(s[REVERSALS]) > it["rev_skip"]:
                s[REV_SUM] = _bits(_F32(_float(s[REV_SUM]) + x))
                s[REV_N] += 1
        if SEARCH_RULES[it["rule"]] == 1:
            if rev:
                step = np.fmax(_F32(step * _F32(0.5)), d_min)
            xn = _F32(x + (step if d > 0 else -step))
        else:
            xn = _F32(x + (step if d > 0 else -step))
            step = np.fmax(_F32(step * _F32(0.5)), d_min)
        s[LEVEL], s[STEP] = _bits(np.fmin(np.fmax(xn, lo), hi)), _bits(step)
        s[LAST_DIR] = d
        s[TRIALS] += 1
        s[FAILS] += int(fail)
        if int(s[TRIALS]) >= it["trials"]:
            status |= DONE
        s[STATUS] = status
        return COUNTED | (FAILED if fail else 0) | (REVERSAL if rev else 0)

    def step(self, terminated, truncated, meta4, meta15=None, check_fail=None, check_incomplete=None):
        """Behind one control step: the done flags it returned and meta words 4 and 15 of every env as it left them.  ``check_fail`` /
        ``check_incomplete`` (uint64 ``[N]``, read only where the step ended an episode): the two masks of the verdict record the
        checks closed for that episode; needed only where an item fails on a check."""
        N = len(self.rows)
        te_all, tr_all = np.asarray(terminated).reshape(N) != 0, np.asarray(truncated).reshape(N) != 0
        meta4 = np.asarray(meta4, dtype=np.int64).reshape(N)
        meta15 = np.zeros(N, dtype=np.int64) if meta15 is None else np.asarray(meta15, dtype=np.int64).reshape(N)
        bad = np.zeros(N, dtype=np.uint64)
        for m in (check_fail, check_incomplete):
            if m is not None:
                bad |= np.asarray(m).astype(np.uint64).reshape(N)
        with np.errstate(all="ignore"):
            for i in range(N):
                s = self.state[i]
                te, tr = bool(te_all[i]), bool(tr_all[i])
                length = int(s[LENGTH]) + 1
                if not (te or tr):
                    s[LENGTH] = length
                    continue
                status = int(s[STATUS])
                flags = ledger_flags(te, tr, meta4[i], s[NAN0], bool(status & AT_RESET), self.fall, meta15[i])
                level, episode = int(s[LEVEL]), int(s[EPISODE])
                it = self.table.search[int(self.rows[i])]
                extra = 0
                if it is not None and not status & DONE and status & AT_RESET:
                    by_check = (int(bad[i]) & it["check_mask"]) != 0
                    extra = self._trial(s, it, (flags & search_fail_mask(it)) != 0 or by_check) | (BY_CHECK if by_check else 0)
                    if int(s[STATUS]) & DONE:
                        self.remaining -= 1
                else:
                    s[UNCOUNTED] += 1
                self.ring[i, episode % self.slots] = (episode, level, flags | extra, length)
                s[EPISODE], s[LENGTH], s[NAN0] = episode + 1, 0, int(meta4[i])
                s[STATUS] = int(s[STATUS]) | AT_RESET


def reference_search(table, slots: int, rows, events: Sequence, fall: bool = False, flag: int = 0, meta4=None):
    """``SearchTwin`` run over ``events``: ``("step", terminated [N], truncated [N], meta4 [N], meta15 [N] or None[, check_fail [N],
    check_incomplete [N]])`` for a control step,
    ``("begin", mask or None, flag, meta4 [N])`` for a reset (flag 0) or a restore / set_state (8) ahead of the next one.  Returns
    ``(state int32 [N, 16], ring int32 [N, slots, 4], remaining)``."""
    twin = SearchTwin(table, slots, rows, fall, flag, meta4)
    for ev in events:
        if ev[0] == "step":
            twin.step(*ev[1:])
        elif ev[0] == "begin":
            twin.begin(*ev[1:])
        else:
            raise ValueError(f"reference_search: unknown event {ev[0]!r}")
    return twin.state, twin.ring, twin.remaining


class SearchResult:
    """The search of a fleet.  ``state`` int32 ``[N, 16]`` and ``trial_words`` int32 ``[R, 4]`` are the words as the engine wrote them.
    Per env ``[N]``: ``env`` (global id), ``scenario`` (table row), ``has_item``, ``level``, ``step`` float32, ``trials``, ``fails``,
    ``reversals``, ``done``, ``bracket`` float32 ``[N, 2]`` (``hi_pass``, ``lo_fail``; NaN where none), ``threshold`` float32
    (``rev_sum / rev_n`` where ``rev_n > 0``, else the middle of the bracket where both ends exist, else NaN), ``episodes`` (ended since
    arming), ``uncounted``.  Per trial ``[R]``, sorted by (env, episode): ``trial_env``, ``episode``, ``trial_level`` (the level the
    episode ran at), ``flags``, ``counted``, ``failed``, ``reversal``, ``length``.  ``lost`` int64 ``[N]``: trials the ring overwrote.
    Without the rings (``include_trials=False``) there are no trial rows and ``lost`` is zero.  ``harder`` int ``[N]``: 0 where a
    higher level is harder (the default), 1 where a lower one is (the item's ``harder="down"``): there ``bracket`` is (the LOWEST pass,
    the HIGHEST failure) -- column 0 is the pass end and column 1 the failure end for both signs, and the threshold lies between
    them.  ``items``: per scenario row with an item, ``{"harder", "targets", "fail_on"}`` as the table states them (empty if unknown)."""

    def __init__(self, state, scenario, trial_words, trial_env, lost, slots: int = 0, env_id0: int = 0, harder=None, items: dict = None):
        self.state = np.ascontiguousarray(state, dtype=np.int32).reshape(-1, NCNT)
        N = len(self.state)
        self.scenario = np.ascontiguousarray(scenario, dtype=np.int64).reshape(N)
        self.trial_words = np.ascontiguousarray(trial_words, dtype=np.int32).reshape(-1, TRIAL_WORDS)
        self.trial_env = np.ascontiguousarray(trial_env, dtype=np.int64).reshape(-1)
        self.lost = np.ascontiguousarray(lost, dtype=np.int64).reshape(N)
        self.slots, self.env_id0 = int(slots), int(env_id0)
        self.harder = np.zeros(N, dtype=np.int64) if harder is None else np.ascontiguousarray(harder, dtype=np.int64).reshape(N)
        self.items = {int(r): dict(v) for r, v in (items or {}).items()}
        if len(self.trial_env) != len(self.trial_words):
            raise ValueError(f"SearchResult: {len(self.trial_words)} trial records but {len(self.trial_env)} env ids")
        s = self.state
        f32 = lambda w: np.ascontiguousarray(s[:, w]).view(np.float32)  # noqa: E731
        self.env = np.arange(N, dtype=np.int64) + self.env_id0
        status = s[:, STATUS]
        self.has_item, self.done = (status & HAS_ITEM) != 0, (status & DONE) != 0
        self.level, self.step = f32(LEVEL), f32(STEP)
        self.trials, self.fails, self.reversals = s[:, TRIALS], s[:, FAILS], s[:, REVERSALS]
        self.episodes, self.uncounted = s[:, EPISODE], s[:, UNCOUNTED]
        nan = np.float32(np.nan)
        hi_pass = np.where((status & HAS_PASS) != 0, f32(HI_PASS), nan).astype(np.float32)
        lo_fail = np.where((status & HAS_FAIL) != 0, f32(LO_FAIL), nan).astype(np.float32)
        self.bracket = np.stack([hi_pass, lo_fail], axis=1)
        with np.errstate(all="ignore"):
            mean = f32(REV_SUM) / s[:, REV_N].astype(np.float32)
            mid = (hi_pass + lo_fail) * np.float32(0.5)
        self.threshold = np.where(s[:, REV_N] > 0, mean, mid).astype(np.float32)
        w = self.trial_words
        self.episode = w[:, 0]
        self.trial_level = np.ascontiguousarray(w[:, 1]).view(np.float32)
        self.flags, self.length = w[:, 2], w[:, 3]
        self.counted, self.failed, self.reversal = (w[:, 2] & COUNTED) != 0, (w[:, 2] & FAILED) != 0, (w[:, 2] & REVERSAL) != 0

    def __len__(self):
        return len(self.trial_words)

    @classmethod
    def from_raw(cls, state, ring, scenario, env_id0: int = 0, table=None) -> "SearchResult":
        """From what ``cosim_get "search_state"`` / ``"search_trials"`` copy: records ``[N, 16]``, rings ``[N, slots, 4]`` or ``None``;
        ``scenario`` ``[N]``: the table row of every env; ``table``: the ``ScenarioTable`` whose items ran (``harder`` and ``items``
        come from it; without it every row reads as ``harder="up"``)."""
        state = np.asarray(state, dtype=np.int32).reshape(-1, NCNT)
        scenario = np.asarray(scenario, dtype=np.int64).reshape(len(state))
        harder, items = None, None
        if table is not None:
            items = {r: {"harder": it["harder"], "targets": list(it["targets"]), "fail_on": list(it["fail_on"])}
                     for r, it in enumerate(table.search) if it is not None}
            harder = np.array([int(r in items and items[r]["harder"] == "down") for r in scenario], dtype=np.int64)
        if ring is None:
            return cls(state, scenario, np.zeros((0, TRIAL_WORDS), np.int32), np.zeros(0, np.int64), np.zeros(len(state), np.int64), 0, env_id0,
                       harder, items)
        words, env, lost = rc.unroll_rings(ring, state[:, EPISODE])
        return cls(state, scenario, words, env + int(env_id0), lost, np.shape(ring)[1], env_id0, harder, items)

    def ended(self) -> np.ndarray:
        """Mask of the trial rows that are ended episodes: all of them (the rings hold no open episode)."""
        return np.ones(len(self), dtype=bool)

    def counts(self) -> dict:
        """The integer sums a distributed run all-reduces (``cli.py``): every value adds over ranks."""
        m = self.has_item
        return {"envs": int(m.sum()), "done": int((m & self.done).sum()), "trials": int(self.trials[m].sum()), "fails": int(self.fails[m].sum()),
                "reversals": int(self.reversals[m].sum()), "uncounted": int(self.uncounted.sum()), "lost": int(self.lost.sum())}

    @staticmethod
    def _quantiles(x) -> Optional[dict]:
        x = np.asarray(x, dtype=np.float64)
        x = x[~np.isnan(x)]
        if not len(x):
            return None
        return {"n": int(len(x)), "min": float(x.min()), "p10": float(np.quantile(x, 0.1)), "p50": float(np.quantile(x, 0.5)),
                "p90": float(np.quantile(x, 0.9)), "max": float(x.max()), "mean": float(x.mean())}

    def _cell(self, m) -> dict:
        n, t = int(m.sum()), int(self.trials[m].sum())
        return {"envs": n, "done": int(self.done[m].sum()), "done_share": float(self.done[m].mean()) if n else None, "trials": t,
                "fail_share": int(self.fails[m].sum()) / t if t else None, "threshold": self._quantiles(self.threshold[m])}

    def summary(self) -> dict:
        """Envs with an item, how many are done, counted trials, their fail share and the quantiles of the per-env thresholds."""
        return {**self.counts(), **self._cell(self.has_item)}

    def by_scenario(self) -> dict:
        """Per scenario row with an item: threshold quantiles over its envs, done share, fail share, and the row's ``harder``,
        ``targets`` and ``fail_on`` where the table is known."""
        return {int(r): {**self._cell(self.has_item & (self.scenario == r)), **self.items.get(int(r), {})} for r in np.unique(self.scenario[self.has_item])}

    def by_policy(self, table) -> dict:
        """``by_scenario`` cells per policy of a static ``policy.PolicyTable`` (or of an int array with the policy of each local env),
        keyed by the policy's name.  A rotating table is refused: an env's level belongs to no single policy."""
        if getattr(table, "rotate_every", None) is not None:
            raise ValueError("SearchResult.by_policy: the table rotates: an env's level is the outcome of several policies' episodes")
        pol, names = rc.policy_of_records(table, self.env, self.env_id0)
        return {names[int(k)]: self._cell(self.has_item & (pol == k)) for k in np.unique(pol[self.has_item])}

    def survival(self, bins) -> dict:
        """The empirical psychometric curve: per scenario row, the pass share of its counted trials per level bin.  ``bins``: the bin
        edges (ascending, as ``numpy.histogram`` takes them) or a bin count over each row's observed level range.  Returns ``{row:
        {"edges", "trials", "passed", "pass_share" (NaN for an empty bin), "harder"}}``: with ``harder`` ``"up"`` the share falls as the
        level rises, with ``"down"`` it rises."""
        out = {}
        loc = self.trial_env - self.env_id0
        row_of = self.scenario[loc] if len(loc) else np.zeros(0, dtype=np.int64)
        for r in np.unique(row_of[self.counted]):
            m = self.counted & (row_of == r)
            lv = self.trial_level[m].astype(np.float64)
            edges = np.histogram_bin_edges(lv, bins=bins)
            n, _ = np.histogram(lv, bins=edges)
            p, _ = np.histogram(lv[~self.failed[m]], bins=edges)
            with np.errstate(all="ignore"):
                share = np.where(n > 0, p / np.maximum(n, 1), np.nan)
            down = bool(self.harder[self.scenario == r].any())
            out[int(r)] = {"edges": edges, "trials": n, "passed": p, "pass_share": share, "harder": "down" if down else "up"}
        return out

    def join(self, ledger) -> np.ndarray:
        """Per trial row, the row of ``ledger`` (an ``EpisodeLedger``, or anything with ``env`` and ``episode`` columns) with the same
        (env, episode), or -1: int64 ``[R]``.  The ordinals agree when both were set together."""
        return rc.join(SimpleNamespace(env=self.trial_env, episode=self.episode), ledger)

    def merge(self, other: "SearchResult") -> "SearchResult":
        """The concatenation of two results over DISJOINT env sets (two shards of a fleet), sorted by global env id."""
        if np.intersect1d(self.env, other.env).size:
            raise ValueError("SearchResult.merge: the two results share env ids")
        if self.slots != other.slots:
            raise ValueError(f"SearchResult.merge: trial rings of {self.slots} slots against {other.slots}")
        lo, hi = (self, other) if self.env_id0 <= other.env_id0 else (other, self)
        if lo.env_id0 + len(lo.state) != hi.env_id0:
            raise ValueError("SearchResult.merge: the env ranges are not adjacent (a result holds one contiguous range of global ids)")
        return SearchResult(np.concatenate([lo.state, hi.state]), np.concatenate([lo.scenario, hi.scenario]),
                            np.concatenate([lo.trial_words, hi.trial_words]), np.concatenate([lo.trial_env, hi.trial_env]),
                            np.concatenate([lo.lost, hi.lost]), max(lo.slots, hi.slots), lo.env_id0, np.concatenate([lo.harder, hi.harder]),
                            {**lo.items, **hi.items})

    def save(self, path: str):
        """One ``.npz`` of plain arrays (no pickle)."""
        np.savez(path, state=self.state, scenario=self.scenario, trial_words=self.trial_words, trial_env=self.trial_env, lost=self.lost,
                 header=rc.header(self.slots, self.env_id0), harder=self.harder, items=np.array(json.dumps({str(r): v for r, v in self.items.items()})))

    @classmethod
    def load(cls, path: str) -> "SearchResult":
        with np.load(path, allow_pickle=False) as z:
            harder = z["harder"] if "harder" in z.files else None
            items = {int(r): v for r, v in json.loads(str(z["items"])).items()} if "items" in z.files else None
            return cls(z["state"], z["scenario"], z["trial_words"], z["trial_env"], z["lost"], *rc.read_header(z), harder, items)


def same_search(a: SearchResult, b: SearchResult) -> Optional[str]:
    """``None`` if two results hold the same records and trials word for word (floats as their bits), else a sentence naming the
    first difference."""
    if a.state.shape != b.state.shape:
        return f"{len(a.state)} envs against {len(b.state)}"
    bad = rc.first_difference(a.state, b.state)
    if bad is not None:
        return f"env {a.env[bad[0]]}, record word {bad[1]}: {a.state[bad]} against {b.state[bad]}"
    if len(a) != len(b):
        return f"{len(a)} trials against {len(b)}"
    if not np.array_equal(a.trial_env, b.trial_env):
        return "trial env ids differ"
    if not np.array_equal(a.lost, b.lost):
        return f"lost counts differ: {a.lost.tolist()} against {b.lost.tolist()}"
    bad = rc.first_difference(a.trial_words, b.trial_words)
    if bad is not None:
        r, w = bad
        return f"trial {r} (env {a.trial_env[r]}, episode {a.trial_words[r, 0]}), word {w}: {a.trial_words[r, w]} against {b.trial_words[r, w]}"
    return None


def search_rows(table, mode, gid) -> np.ndarray:
    """The table row of every env of global ids ``gid`` (mode ``env``, the only one a search runs in)."""
    return scenario_rows(len(table), mode, gid, np.zeros(len(np.asarray(gid).reshape(-1)), dtype=np.int64)).astype(np.int64)

