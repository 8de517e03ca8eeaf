"""The record core under ``EpisodeLedger`` (ledger.py), ``Verdicts`` (checks.py) and ``FailureTraces`` (ftrace.py).

All three observers keep, per env, a ring of fixed-size int32 records on the device, word 0 of a record being the episode ordinal,
word 2 its flags.  What they share on the host stands here once: the flag values, the unrolling of the rings into rows sorted by
(env, episode), the merge of the open rows, the ``(env, episode)`` join, the comparison of two containers and the walk over policy x
scenario cells.  No torch, no GPU in this module.
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import numpy as np

# episode flags (include/cosim.h): word 2 of a ledger record, a verdict record and a trace header
TERMINATED, TRUNCATED, NONFINITE, NO_RESET, OPEN = 1, 2, 4, 8, 16
FELL_TILT, FELL_HEIGHT, FELL_CONTACT = 32, 64, 128   # a fall rule ended the episode (cosim_amd/fall.py): (cause & 7) << 5
FELL = FELL_TILT | FELL_HEIGHT | FELL_CONTACT


def kept_rows(counts, slots: int):
    """``(env, k, kept)``: an env that closed ``counts[i]`` records into ``slots`` slots still holds ``kept[i] = min(counts[i],
    slots)``; one row per kept record, env by env, ``k`` = 0 (oldest kept) .. ``kept - 1`` within the env.  All int64."""
    kept = np.minimum(counts, slots)
    env = np.repeat(np.arange(len(counts), dtype=np.int64), kept)
    k = np.arange(len(env), dtype=np.int64) - np.repeat(np.cumsum(kept) - kept, kept)
    return env, k, kept


def merge_open(words, env, open_rows):
    """Rows sorted by (env, ordinal) plus one open row per env: ``(words, env, order)`` sorted again, ``order`` being the
    permutation applied to the concatenation (for columns the caller carries along)."""
    words = np.concatenate([words, open_rows])
    env = np.concatenate([env, np.arange(len(open_rows), dtype=np.int64)])
    order = np.lexsort((words[:, 0], env))   # an env's open episode carries the next ordinal: it sorts last
    return words[order], env[order], order


def unroll_rings(records, counts, open_rows=None):
    """``(words int32 [R, W], env int64 [R], lost int64 [N])`` from rings ``[N, slots, W]``, ended-episode counts ``[N]`` and open
    rows ``[N, W]`` or ``None``.  Episode ``o`` of an env lies in slot ``o mod slots``; the ring holds the last ``min(count,
    slots)``, ``lost`` counts the ones it overwrote.  Rows are sorted by (local env index, ordinal)."""
    records = np.asarray(records, dtype=np.int32)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    N, slots, W = records.shape
    env, k, kept = kept_rows(counts, slots)
    words = records[env, (np.repeat(counts - kept, kept) + k) % max(slots, 1)]
    if open_rows is not None:
        words, env, _ = merge_open(words, env, np.asarray(open_rows, dtype=np.int32).reshape(N, W))
    return words, env, counts - kept


def join(rows, other) -> np.ndarray:
    """Per row of ``rows``, the row of ``other`` with the same (env, episode), or -1: int64 ``[R]``.  Both have ``env`` and
    ``episode`` columns."""
    at = {(int(e), int(o)): i for i, (e, o) in enumerate(zip(other.env, other.episode))}
    return np.array([at.get((int(e), int(o)), -1) for e, o in zip(rows.env, rows.episode)], dtype=np.int64)


def same_rows(a, b, noun: str = "records", meta: bool = False, lost_values: bool = False) -> Optional[str]:
    """The head of every container comparison: ``None`` if ``a`` and ``b`` hold as many rows of the same envs (and the same ``meta``)
    and lost as many, else the sentence naming the first difference."""
    if len(a) != len(b):
        return f"{len(a)} {noun} against {len(b)}"
    if meta and a.meta != b.meta:
        return f"metadata differs: {a.meta} against {b.meta}"
    if not np.array_equal(a.env, b.env):
        return "env ids differ"
    if not np.array_equal(a.lost, b.lost):
        return f"lost counts differ: {a.lost.tolist()} against {b.lost.tolist()}" if lost_values else "lost counts differ"
    return None


def first_difference(x, y) -> Optional[Tuple[int, int]]:
    """``(row, word)`` of the first word in which two int32 ``[R, W]`` blocks differ (floats compare as their bits), or ``None``."""
    bad = np.argwhere(x != y)
    return (int(bad[0][0]), int(bad[0][1])) if len(bad) else None


def header(slots: int, env_id0: int) -> np.ndarray:
    """The ``header`` array of a container's ``.npz``."""
    return np.array([slots, env_id0], dtype=np.int64)


def read_header(z) -> Tuple[int, int]:
    """``(slots, env_id0)`` back from a loaded ``.npz``."""
    return int(z["header"][0]), int(z["header"][1])


def policy_of_records(table, env, env_id0: int, episode=None):
    """``(policy index int64 [R], names)`` for records of the global env ids ``env``: ``table`` is a ``policy.PolicyTable`` (its
    ``policy_of`` and ``names``) or an int array holding the policy of each local env (env ``env_id0 + i`` is entry ``i``).
    ``episode``: the records' episode ordinals, which a rotating table (``rotate_every``) attributes by; others ignore them."""
    env = np.asarray(env, dtype=np.int64)
    if hasattr(table, "policy_of"):
        if getattr(table, "rotate_every", None) is not None:
            if episode is None:
                raise ValueError("by_policy: the table rotates, so a record is attributed by (env, episode ordinal): pass the records' ordinals")
            return np.asarray(table.policy_of(env, np.asarray(episode, dtype=np.int64)), dtype=np.int64), list(table.names)
        return np.asarray(table.policy_of(env), dtype=np.int64), list(table.names)
    a = np.asarray(table, dtype=np.int64).reshape(-1)
    loc = env - int(env_id0)
    if loc.size and (loc.min() < 0 or loc.max() >= len(a)):
        raise ValueError(f"by_policy: the array names the policy of {len(a)} local envs, the records hold env ids "
                         f"{int(env.min())}..{int(env.max())} (first id {env_id0})")
    return a[loc], [str(k) for k in range(int(a.max()) + 1 if a.size else 0)]


def policy_cells(rows, table, scenario: bool = False) -> Iterator[tuple]:
    """The walk under every ``by_policy``: ``(key, mask)`` per policy of ``table`` that has an ended row in ``rows`` -- ``key`` the
    policy's name -- or with ``scenario`` per (policy, scenario row) cell that has one, ``key = (name, row)``.  ``rows`` has
    ``env``, ``env_id0``, ``episode``, ``scenario`` and ``ended()``."""
    pol, names = policy_of_records(table, rows.env, rows.env_id0, rows.episode)
    m = rows.ended()
    for k in np.unique(pol[m]):
        mk = m & (pol == k)
        if not scenario:
            yield names[int(k)], mk
            continue
        for s in np.unique(rows.scenario[mk]):
            yield (names[int(k)], int(s)), mk & (rows.scenario == s)
