"""Response curves: per-scenario ensemble time series of a signal over the episode clock, split by outcome, kept on the device
(``cosim_scenario_curves_set`` / ``cosim_scenario_curves_get``, csrc/cosim_curves.hip).

A scenario of a ``ScenarioTable`` may hold curve items (``cosim_amd/scenario.py``).  The engine samples them behind every control step
into a per-env stage and, when an episode ends, folds the episode's samples into the cells of (scenario, item, outcome class) with
integer atomics -- no host read per step, and the cells are a function of the set of ended episodes alone.  ``Curves`` is those cells
on the host: per (scenario, item) the sample times, and per outcome class and time bin the count, the mean, the extremes, a histogram
and the quantiles read off it.  ``reference_curves`` is the numpy twin of the kernels: the same operations on recorded step outputs, so
its cells equal the device's word for word.  No torch, no GPU in this module.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .checks import UP, _signal

NONE_BITS, NONFINITE_BITS = 0x7FC00000, 0x7FC00001
MAX_GROUPS = 64                                   # planes of grouped cells (cosim_scenario_curves_groups)
TRUNCATED, TERMINATED = 0, 1                       # outcome classes
OUTCOMES = {None: None, "truncated": TRUNCATED, "terminated": TERMINATED}
FIX = 1 << 20                                     # the sum is in units of 2^-20, samples clamped to +-2^20


def cell_words(T: int, B: int) -> int:
    """32-bit words of the cells of one (item, class): count[T] | nan[T] | min[T] | max[T] | sum[T] (int64) | hist[B + 2][T], rounded up
    to even."""
    return ((B + 8) * T + 1) & ~1


def layout(csr) -> dict:
    """Where the engine keeps the items of ``ScenarioTable.pack_curves()``: per item ``T``, ``soff`` (first stage word in an env's
    row), ``coff`` (first cell word of class 0) and ``cw`` (cell words of one class); ``words`` (all cells) and ``stage_words`` (per
    env)."""
    adr, t, _, _, _, _, bins = csr
    n = len(bins)
    T = np.array([-(-(int(t[i, 1]) - int(t[i, 0])) // int(t[i, 2])) for i in range(n)], dtype=np.int64)
    cw = np.array([cell_words(int(T[i]), int(bins[i])) for i in range(n)], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum(2 * cw)])[:n].astype(np.int64)
    soff = np.zeros(n, dtype=np.int64)
    stage = 0
    for s in range(len(adr) - 1):
        w = 0
        for i in range(int(adr[s]), int(adr[s + 1])):
            soff[i] = w
            w += int(T[i])
        stage = max(stage, w)
    return {"T": T, "soff": soff, "coff": coff, "cw": cw, "words": int(2 * cw.sum()), "stage_words": int(stage)}


def key_of(bits) -> np.ndarray:
    """The order-preserving uint32 key of float32 bits."""
    b = np.asarray(bits).astype(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def float_of_key(key) -> np.ndarray:
    k = np.asarray(key).astype(np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


class Curve:
    """The cells of one (scenario, item): ``t`` int64 ``[T]`` the sample times; ``count`` / ``nan`` int64 ``[2, T]``, ``sum`` int64 ``[2,
    T]`` (units of 2^-20), ``min_key`` / ``max_key`` uint32 ``[2, T]``, ``hist`` int64 ``[2, B + 2, T]`` (row 0: below ``lo``, row B + 1:
    at or above ``hi``); axis 0 is the outcome class (0 truncated only, 1 terminated).  The methods take ``outcome=None | "truncated"
    | "terminated"``; ``None`` merges the two classes."""

    def __init__(self, name, t0, t1, every, lo, hi, bins, count, nan, sum_, min_key, max_key, hist):
        self.name, self.t0, self.t1, self.every, self.lo, self.hi, self.bins = name, int(t0), int(t1), int(every), float(lo), float(hi), int(bins)
        self.t = np.arange(self.t0, self.t1, self.every, dtype=np.int64)
        self._count, self._nan, self._sum, self._min, self._max, self._hist = count, nan, sum_, min_key, max_key, hist

    @staticmethod
    def _cls(outcome):
        if outcome not in OUTCOMES:
            raise ValueError(f"outcome must be None, 'truncated' or 'terminated', got {outcome!r}")
        return OUTCOMES[outcome]

    def _pick(self, a, outcome, how="sum"):
        c = self._cls(outcome)
        if c is not None:
            return a[c]
        return a.sum(axis=0) if how == "sum" else (a.min(axis=0) if how == "min" else a.max(axis=0))

    def count(self, outcome=None) -> np.ndarray:
        """Finite samples per time bin."""
        return self._pick(self._count, outcome)

    def nan(self, outcome=None) -> np.ndarray:
        """Non-finite samples per time bin (they are in no other cell)."""
        return self._pick(self._nan, outcome)

    def mean(self, outcome=None) -> np.ndarray:
        """Mean of the finite samples (each clamped to +-2^20 and rounded to 2^-20), float64; NaN where ``count == 0``."""
        n, s = self.count(outcome), self._pick(self._sum, outcome)
        with np.errstate(all="ignore"):
            return np.where(n > 0, s.astype(np.float64) / FIX / np.maximum(n, 1), np.nan)

    def min(self, outcome=None) -> np.ndarray:
        """Smallest finite sample, float32 (exact); NaN where ``count == 0``."""
        return np.where(self.count(outcome) > 0, float_of_key(self._pick(self._min, outcome, "min")), np.float32(np.nan))

    def max(self, outcome=None) -> np.ndarray:
        return np.where(self.count(outcome) > 0, float_of_key(self._pick(self._max, outcome, "max")), np.float32(np.nan))

    def hist(self, outcome=None) -> np.ndarray:
        """``[B + 2, T]``: row 0 below ``lo``, rows 1 .. B equal bins over ``[lo, hi)``, row B + 1 at or above ``hi``."""
        return self._pick(self._hist, outcome)

    def both(self, name: str) -> np.ndarray:
        """``count`` / ``nan`` / ``mean`` / ``min`` / ``max`` as ``[2, T]`` and ``hist`` as ``[2, B + 2, T]``: axis 0 is the outcome class."""
        if name not in ("count", "nan", "mean", "min", "max", "hist"):
            raise ValueError(f"both: unknown array {name!r}")
        return np.stack([getattr(self, name)("truncated"), getattr(self, name)("terminated")])

    def quantile(self, q: float, outcome=None) -> np.ndarray:
        """The q-quantile of the finite samples per time bin, read off the histogram: linear inside a bin, the underflow row counts
        as ``lo`` and the overflow row as ``hi`` (so the result is clamped to ``[lo, hi]``); NaN where ``count == 0``."""
        if self.bins < 1:
            raise ValueError(f"curve '{self.name}': bins = 0 keeps no histogram, so there are no quantiles")
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"quantile: q must be in [0, 1], got {q!r}")
        h = self.hist(outcome).astype(np.float64)
        n = h.sum(axis=0)
        cum = np.cumsum(h, axis=0)
        target = q * n
        row = np.argmax((cum >= target[None, :]) & (cum > 0), axis=0)            # the first non-empty row that reaches the rank
        before = np.where(row > 0, np.take_along_axis(cum, np.maximum(row - 1, 0)[None, :], axis=0)[0], 0.0)
        inside = np.take_along_axis(h, row[None, :], axis=0)[0]
        with np.errstate(all="ignore"):
            frac = np.where(inside > 0, (target - before) / np.maximum(inside, 1.0), 0.0)
            v = self.lo + (row - 1 + np.clip(frac, 0.0, 1.0)) * ((self.hi - self.lo) / self.bins)
        v = np.where(row == 0, self.lo, np.where(row == self.bins + 1, self.hi, v))
        return np.where(n > 0, np.clip(v, self.lo, self.hi), np.nan)

    def band(self, q_lo: float = 0.05, q_hi: float = 0.95, outcome=None):
        """``(quantile(q_lo), quantile(0.5), quantile(q_hi))``."""
        return self.quantile(q_lo, outcome), self.quantile(0.5, outcome), self.quantile(q_hi, outcome)


class Curves:
    """The cells of a table's curve items.  ``cells`` uint32 ``[words]`` is what the engine keeps (include/cosim.h); ``adr`` int64 ``[S
    + 1]`` the items of every scenario; ``spec`` int64 ``[n, 5]`` (t0, t1, every, signal, index) + ``bins`` ``[n]``, ``lohi`` float32
    ``[n, 2]``, ``names[s][k]``.  ``curves[s, k]`` (k: an item's position or name) is that item's ``Curve``.

    With ``groups=G`` (``cosim_scenario_curves_groups``) ``cells`` is ``[G * W]``: G planes, each a whole cell image of W words, plane g
    the episodes whose env carried group word g when they ended; ``group_names`` names the planes (default ``"0" .. "G-1"``) and
    ``ungrouped`` counts the episodes whose word was outside ``[0, G)`` (they are in no plane).  ``curves[s, k]`` stays the curve over
    ALL groups -- the planes merged, exactly -- so code written for ungrouped curves reads the same numbers; ``curves[s, k, g]`` (g: a
    plane's index or name) is one group's curve, ``group(g)`` that plane as a plain ``Curves``, ``by_group()`` all of them by name."""

    def __init__(self, cells, adr, spec, lohi, bins, names, groups=1, group_names=None, ungrouped=0):
        self.adr = np.ascontiguousarray(adr, dtype=np.int64).reshape(-1)
        self.spec = np.ascontiguousarray(spec, dtype=np.int64).reshape(-1, 5)
        self.lohi = np.ascontiguousarray(lohi, dtype=np.float32).reshape(-1, 2)
        self.bins = np.ascontiguousarray(bins, dtype=np.int64).reshape(-1)
        self.names = [list(n) for n in names]
        self._lay = layout((self.adr, self.spec[:, :3], None, None, None, None, self.bins))
        self.cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1)
        if isinstance(groups, bool) or not isinstance(groups, (int, np.integer)) or not 1 <= int(groups) <= MAX_GROUPS:
            raise ValueError(f"Curves: groups {groups!r}: an integer 1..{MAX_GROUPS}")
        self.groups, self.ungrouped = int(groups), int(ungrouped)
        self.grouped = self.groups > 1 or group_names is not None    # a group axis: ``summary`` and ``save`` carry it
        self.group_names = [str(g) for g in range(self.groups)] if group_names is None else [str(x) for x in group_names]
        if len(self.group_names) != self.groups or len(set(self.group_names)) != self.groups:
            raise ValueError(f"Curves: group_names must be {self.groups} different strings, got {self.group_names}")
        if self.cells.size != self.groups * self._lay["words"]:
            raise ValueError(f"Curves: {self.cells.size} cell words, the items need {self._lay['words']}" +
                             (f" in each of {self.groups} planes" if self.groups > 1 else ""))

    @property
    def plane_words(self) -> int:
        """W: the cell words of one plane."""
        return int(self._lay["words"])

    @classmethod
    def from_raw(cls, cells, table, groups=1, group_names=None, ungrouped=0) -> "Curves":
        """From what ``cosim_scenario_curves_get`` copies and the ``ScenarioTable`` whose curves were set."""
        adr, t, signal, index, lo, hi, bins = table.pack_curves()
        return cls(cells, adr, np.concatenate([t.astype(np.int64), signal[:, None].astype(np.int64), index[:, None].astype(np.int64)], axis=1),
                   np.stack([lo, hi], axis=1), bins, table.curve_item_names(), groups=groups, group_names=group_names, ungrouped=ungrouped)

    @classmethod
    def empty(cls, table, groups=1, group_names=None) -> "Curves":
        c = cls.from_raw(np.zeros(groups * layout(table.pack_curves())["words"], dtype=np.uint32), table, groups, group_names)
        for _, _, base, T, _ in c._blocks():
            for g in range(c.groups):
                c.cells[g * c.plane_words + base + 2 * T:g * c.plane_words + base + 3 * T] = 0xFFFFFFFF
        return c

    def _blocks(self):
        """``(flat item, class, first word, T, B)`` of every block of cells of ONE plane."""
        L = self._lay
        for i in range(len(self.bins)):
            for c in (0, 1):
                yield i, c, int(L["coff"][i] + c * L["cw"][i]), int(L["T"][i]), int(self.bins[i])

    def word_kinds(self) -> np.ndarray:
        """Per cell word how two fleets' cells merge: 0 add as uint32, 1 unsigned min, 2 unsigned max, 3 half of an int64 that adds
        (the two halves are neighbours).  With groups: one plane's kinds tiled over the planes."""
        kind = np.zeros(self.plane_words, dtype=np.int8)
        for _, _, b, T, _ in self._blocks():
            kind[b + 2 * T:b + 3 * T], kind[b + 3 * T:b + 4 * T], kind[b + 4 * T:b + 6 * T] = 1, 2, 3
        return np.tile(kind, self.groups)

    def _group_index(self, g) -> int:
        if isinstance(g, str):
            if g not in self.group_names:
                raise KeyError(f"Curves: no group '{g}' (the groups are {self.group_names})")
            return self.group_names.index(g)
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= int(g) < self.groups:
            raise KeyError(f"Curves: no group {g!r} (there are {self.groups})")
        return int(g)

    def group(self, g) -> "Curves":
        """Plane ``g`` (an index or a name) as a plain ungrouped ``Curves`` (a copy of its words)."""
        g = self._group_index(g)
        W = self.plane_words
        return Curves(self.cells[g * W:(g + 1) * W].copy(), self.adr, self.spec, self.lohi, self.bins, self.names)

    def by_group(self) -> dict:
        """``{group name: that plane as a plain Curves}``, in plane order."""
        return {name: self.group(g) for g, name in enumerate(self.group_names)}

    def merged(self) -> "Curves":
        """The planes merged into one by ``merge``'s rule, as a plain ungrouped ``Curves``: the cells the same episodes give without
        groups (when ``ungrouped == 0``).  Of ungrouped curves: a copy."""
        out = self.group(0)
        for g in range(1, self.groups):
            out = out.merge(self.group(g))
        return out

    @property
    def n_scenarios(self) -> int:
        return len(self.adr) - 1

    def items(self):
        """``(scenario, k)`` of every item."""
        return [(s, k) for s in range(self.n_scenarios) for k in range(int(self.adr[s + 1] - self.adr[s]))]

    def __getitem__(self, key) -> Curve:
        if len(key) == 3:
            return self.group(key[2])[key[0], key[1]]
        if self.groups > 1:
            return self.merged()[key]
        s, k = key
        if not 0 <= s < self.n_scenarios:
            raise KeyError(f"Curves: no scenario {s}")
        if isinstance(k, str):
            if k not in self.names[s]:
                raise KeyError(f"Curves: scenario {s} has no item '{k}' (it has {self.names[s]})")
            k = self.names[s].index(k)
        if not 0 <= k < int(self.adr[s + 1] - self.adr[s]):
            raise KeyError(f"Curves: scenario {s} has no item {k}")
        i = int(self.adr[s]) + k
        T, B = int(self._lay["T"][i]), int(self.bins[i])
        parts = []
        for c in (0, 1):
            w = self.cells[int(self._lay["coff"][i] + c * self._lay["cw"][i]):][:(B + 8) * T]
            parts.append((w[:T].astype(np.int64), w[T:2 * T].astype(np.int64), w[2 * T:3 * T], w[3 * T:4 * T],
                          np.ascontiguousarray(w[4 * T:6 * T]).view(np.int64), w[6 * T:].astype(np.int64).reshape(B + 2, T)))
        st = lambda j: np.stack([parts[0][j], parts[1][j]])   # noqa: E731
        t0, t1, every = (int(x) for x in self.spec[i, :3])
        return Curve(self.names[s][k], t0, t1, every, self.lohi[i, 0], self.lohi[i, 1], B, st(0), st(1), st(4), st(2), st(3), st(5))

    def _same_items(self, other) -> bool:
        return (np.array_equal(self.adr, other.adr) and np.array_equal(self.spec, other.spec) and np.array_equal(self.bins, other.bins)
                and np.array_equal(self.lohi.view(np.uint32), other.lohi.view(np.uint32)))

    def _same_groups(self, other) -> bool:
        return self.groups == other.groups and self.group_names == other.group_names

    def merge(self, other: "Curves") -> "Curves":
        """The curves of both fleets together, exact: counts, sums and histograms add as integers, the extremes merge on their keys.
        Grouped curves merge plane by plane (the same G and names on both sides) and their ``ungrouped`` counts add."""
        if not self._same_items(other):
            raise ValueError("Curves.merge: the two sets of curves were taken with different items")
        if not self._same_groups(other):
            raise ValueError(f"Curves.merge: the two sets of curves were taken with different groups: {self.groups} {self.group_names} "
                             f"against {other.groups} {other.group_names}")
        out = self.cells.copy()
        W = self.plane_words
        for _, _, b0, T, B in self._blocks():
            for g in range(self.groups):
                b = g * W + b0
                a, o = out[b:b + (B + 8) * T], other.cells[b:b + (B + 8) * T]
                for lo, hi in ((0, 2 * T), (6 * T, (B + 8) * T)):
                    a[lo:hi] += o[lo:hi]
                a[2 * T:3 * T] = np.minimum(a[2 * T:3 * T], o[2 * T:3 * T])
                a[3 * T:4 * T] = np.maximum(a[3 * T:4 * T], o[3 * T:4 * T])
                s = np.ascontiguousarray(a[4 * T:6 * T]).view(np.int64) + np.ascontiguousarray(o[4 * T:6 * T]).view(np.int64)
                a[4 * T:6 * T] = s.view(np.uint32)
        return Curves(out, self.adr, self.spec, self.lohi, self.bins, self.names, groups=self.groups,
                      group_names=self.group_names if self.grouped else None, ungrouped=self.ungrouped + other.ungrouped)

    def episodes(self) -> np.ndarray:
        """int64 ``[S, 2]``: per scenario and outcome class, the samples (finite or not) of its fullest time bin -- the ended episodes
        that reached that bin; an episode that ended ahead of every window is in none.  With groups: of the planes merged."""
        if self.groups > 1:
            return self.merged().episodes()
        out = np.zeros((self.n_scenarios, 2), dtype=np.int64)
        for s, k in self.items():
            c = self[s, k]
            out[s] = np.maximum(out[s], (c._count + c._nan).max(axis=1))
        return out

    def summary(self) -> dict:
        """Item count, episodes folded (``episodes()``, summed over the scenarios) and samples, by outcome class.  Grouped curves add
        ``groups``, ``ungrouped`` and ``by_group``: per group name that plane's own summary."""
        if self.grouped:                                               # the planes merged, as without groups, and every plane's own
            out = self.merged().summary()
            out.update({"groups": self.groups, "ungrouped": self.ungrouped, "by_group": {name: p.summary() for name, p in self.by_group().items()}})
            return out
        e = self.episodes().sum(axis=0)
        n = np.zeros(2, dtype=np.int64)
        bad = 0
        for s, k in self.items():
            c = self[s, k]
            n += c._count.sum(axis=1)
            bad += int(c._nan.sum())
        return {"items": int(len(self.bins)), "episodes": int(e.sum()), "episodes_truncated": int(e[0]), "episodes_terminated": int(e[1]),
                "samples": int(n.sum()), "samples_truncated": int(n[0]), "samples_terminated": int(n[1]), "nonfinite": bad}

    def save(self, path: str):
        """One ``.npz`` of plain arrays (no pickle)."""
        I = max([len(n) for n in self.names] + [1])
        names = np.array([[(n[k] if k < len(n) else "") for k in range(I)] for n in self.names], dtype=np.str_).reshape(len(self.names), I)
        more = {}
        if self.grouped:                     # ungrouped curves keep the file of before there were groups
            more = {"groups": np.int64(self.groups), "group_names": np.array(self.group_names, dtype=np.str_), "ungrouped": np.int64(self.ungrouped)}
        np.savez(path, cells=self.cells, adr=self.adr, spec=self.spec, lohi=self.lohi, bins=self.bins, names=names, **more)

    @classmethod
    def load(cls, path: str) -> "Curves":
        with np.load(path, allow_pickle=False) as z:
            adr = z["adr"]
            names = [[str(z["names"][s, k]) for k in range(int(adr[s + 1] - adr[s]))] for s in range(len(adr) - 1)]
            if "groups" not in z.files:                                # a file without a group axis
                return cls(z["cells"], adr, z["spec"], z["lohi"], z["bins"], names)
            return cls(z["cells"], adr, z["spec"], z["lohi"], z["bins"], names, groups=int(z["groups"]),
                       group_names=[str(x) for x in z["group_names"]], ungrouped=int(z["ungrouped"]))


def same_curves(a: Curves, b: Curves) -> Optional[str]:
    """``None`` if two sets of curves hold the same items and the same cells word for word, else a sentence naming the first
    difference."""
    if not a._same_items(b):
        return "the items differ"
    if not a._same_groups(b):
        return f"the groups differ: {a.groups} {a.group_names} against {b.groups} {b.group_names}"
    if a.ungrouped != b.ungrouped:
        return f"ungrouped episodes: {a.ungrouped} against {b.ungrouped}"
    bad = np.nonzero(a.cells != b.cells)[0]
    if len(bad):
        w = int(bad[0])
        if a.groups > 1:
            g = w // a.plane_words
            return f"{len(bad)} words differ in all; group {g} ('{a.group_names[g]}'): {same_curves(a.group(g), b.group(g))}"
        for i, c, base, T, B in a._blocks():
            if base <= w < base + int(a._lay["cw"][i]):
                r = w - base
                part = ("count", "nan", "min", "max", "sum", "sum")[r // T] if r < 6 * T else f"hist row {r // T - 6}"
                return f"{len(bad)} words differ; the first: flat item {i}, class {c}, {part}, word {r} (time bin {r % T if r // T != 4 and r // T != 5 else (r - 4 * T) // 2}): {a.cells[w]} against {b.cells[w]}"
        return f"word {w}: {a.cells[w]} against {b.cells[w]}"
    return None


def hist_row(v, lo, hi, inv_w, B: int) -> int:
    """``curves_hist_row``: float32, one rounded operation at a time."""
    f32 = np.float32
    v, lo, hi = f32(v), f32(lo), f32(hi)
    if v < lo:
        return 0
    if v >= hi:
        return B + 1
    with np.errstate(all="ignore"):
        x = f32(f32(v - lo) * f32(inv_w))
    return 1 + (int(x) if x < f32(B) else B - 1)


def reference_curves(table, info_rows, terminated, truncated, commands, qpos, qvel, clock, scenario_rows, nu: int, begins: Sequence = (),
                     clears: Sequence = (), groups=None, n_groups: int = 0, group_names=None) -> Curves:
    """Numpy twin of ``curves_step_kernel`` / ``curves_step_grouped_kernel`` / ``curves_begin_kernel`` (and of
    ``cosim_scenario_curves_clear``).

    The per-step records are ``reference_checks``'s (``cosim_amd/checks.py``): ``info_rows`` ``[K, N, info_dim]``, ``terminated`` /
    ``truncated`` ``[K, N]``, ``commands`` ``[K, N, >= command_dim]`` (or ``[N, .]``), ``qpos`` / ``qvel`` read back behind step k,
    ``clock`` ``[K + 1, N]`` (meta word 0 before step k, row K: after the last step), ``scenario_rows`` ``[K, N]``.  ``begins``: ``(k,
    mask or None, flag)`` -- the host cut the masked envs' episodes before step k (the flag is ignored: a curve keeps no flags).
    ``clears``: steps k before which the cells were emptied and every env's episode begun anew.

    ``groups`` int ``[K, N]`` with ``n_groups = G >= 1``: each env's group word as the fold of step k reads it; the result is the grouped
    twin -- an episode that ends in step k goes into plane ``groups[k, e]``, a word outside ``[0, G)`` into none (its stage is emptied and
    ``ungrouped`` counts it; a clear zeroes the count)."""
    G = int(n_groups)
    if (groups is None) != (G == 0):
        raise ValueError("reference_curves: groups ([K, N] ints) and n_groups (>= 1) go together")
    C = table._resolved_curves()
    csr = table.pack_curves()
    L = layout(csr)
    adr, inv_w = csr[0], [np.float32(0)] * len(csr[6])
    for i, (lo, hi, B) in enumerate(zip(csr[4], csr[5], csr[6])):
        if B > 0:
            inv_w[i] = np.float32(np.float64(B) / (np.float64(hi) - np.float64(lo)))
    info = np.asarray(info_rows, dtype=np.float32)
    K, N = info.shape[0], info.shape[1]
    te_all, tr_all = np.asarray(terminated).reshape(K, N) != 0, np.asarray(truncated).reshape(K, N) != 0
    cmd = None if commands is None else np.asarray(commands, dtype=np.float32)
    qpos, qvel = np.asarray(qpos, dtype=np.float32), np.asarray(qvel, dtype=np.float32)
    clock_all = np.asarray(clock, dtype=np.int64).reshape(K + 1, N)
    rows_all = np.asarray(scenario_rows, dtype=np.int64).reshape(K, N)
    out = Curves.empty(table, max(G, 1), group_names)
    cells = out.cells
    grp = None if groups is None else np.asarray(groups, dtype=np.int64).reshape(K, N)
    stage = np.full((N, max(L["stage_words"], 1)), NONE_BITS, dtype=np.int64)
    clk = clock_all[0].copy()

    def begin(k):
        if k in clears:
            cells[:] = Curves.empty(table, max(G, 1)).cells
            out.ungrouped = 0
            stage[:] = NONE_BITS
            clk[:] = clock_all[k]
        for kb, mask, _ in begins:
            if kb != k:
                continue
            m = np.ones(N, dtype=bool) if mask is None else np.asarray(mask).astype(bool).reshape(N)
            stage[m] = NONE_BITS
            clk[m] = clock_all[k][m]

    with np.errstate(all="ignore"):
        for k in range(K):
            begin(k)
            for e in range(N):
                te, tr = bool(te_all[k, e]), bool(tr_all[k, e])
                done = te or tr
                t, row = int(clk[e]), int(rows_all[k, e])
                c = None if cmd is None else (cmd[e] if cmd.ndim == 2 else cmd[k, e])
                for j, it in enumerate(C[row]):
                    t0, t1, every, sig, idx = it[:5]
                    if not (t0 <= t < t1) or (t - t0) % every or (done and sig >= UP):
                        continue
                    bits = int(np.float32(_signal(sig, idx, info[k, e], c, qpos[k, e], qvel[k, e], int(nu))).view(np.uint32))
                    stage[e, L["soff"][adr[row] + j] + (t - t0) // every] = bits if (bits & 0x7F800000) != 0x7F800000 else NONFINITE_BITS
                plane = 0
                if done and grp is not None:
                    plane = int(grp[k, e])
                    if not 0 <= plane < G:                              # in no plane: the stage is emptied, the episode counted
                        for j, it in enumerate(C[row]):
                            i = int(adr[row]) + j
                            stage[e, int(L["soff"][i]):int(L["soff"][i]) + int(L["T"][i])] = NONE_BITS
                        out.ungrouped += 1
                        done = False
                if done:
                    cls = 1 if te else 0
                    for j, it in enumerate(C[row]):
                        i = int(adr[row]) + j
                        T, B = int(L["T"][i]), int(it[7])
                        base = plane * int(L["words"]) + int(L["coff"][i] + cls * L["cw"][i])
                        st = stage[e, int(L["soff"][i]):int(L["soff"][i]) + T]
                        for b in np.nonzero(st != NONE_BITS)[0]:
                            bits = int(st[b])
                            st[b] = NONE_BITS
                            if (bits & 0x7F800000) == 0x7F800000:
                                cells[base + T + b] += 1
                                continue
                            v = np.array([bits], dtype=np.uint32).view(np.float32)[0]
                            cells[base + b] += 1
                            q = int(np.rint(np.float64(np.clip(v, np.float32(-FIX), np.float32(FIX))) * np.float64(FIX)))
                            s = cells[base + 4 * T + 2 * b:base + 4 * T + 2 * b + 2]
                            s[:] = np.array([int(s.copy().view(np.int64)[0]) + q], dtype=np.int64).view(np.uint32)
                            key = int(key_of(bits))
                            cells[base + 2 * T + b] = min(int(cells[base + 2 * T + b]), key)
                            cells[base + 3 * T + b] = max(int(cells[base + 3 * T + b]), key)
                            if B > 0:
                                cells[base + (6 + hist_row(v, it[5], it[6], inv_w[i], B)) * T + b] += 1
                clk[e] = clock_all[k + 1][e]
        begin(K)
    return out
