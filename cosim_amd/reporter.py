"""Fleet reporter: what the reference's ``Reporter`` distils from the ``info`` stream (core/reporter.py:210-218 write_info,
:257 dt, :380-382 set_points vs state, :429-442 torque / action_diff_RMSE, :506-508 command tracking), reduced over N envs.

``write_info(info)`` takes the batched ``info`` dict of ``BatchedEnv.step`` and keeps sufficient statistics on the device
(``distributed.MetricsAccumulator``: one small all-reduce across GPUs when ``summary()`` is called); ``trace_env`` keeps
the full per-step series of one env as plain numpy / floats — the dict stream the reference's single-env ``Reporter``
consumes, so its PDF code can be fed from it unchanged.
"""
from __future__ import annotations

import json
from typing import Optional

import numpy as np

from .distributed import MetricsAccumulator


NBINS = 512


class FleetReporter:
    def __init__(self, env, trace_env: Optional[int] = None, percentiles: bool = False):
        """``percentiles``: also keep one 512-bin histogram per metric column (magnitudes over [0, range): action-RMSE 0..2, base
        velocities 0..8, |torque| 0..max torque of the actuator, tracking error 0..8), summed over the sampled steps and, in
        ``summary()``, over ranks: p5 / p50 / p95 of tracking error, |torque| and action-RMSE come out of it to one bin width."""
        self.env, self.trace_env = env, trace_env
        nu, cd = env.action_dim, env.command_dim
        self.names = (["action_diff_RMSE", "lin_vel_x", "lin_vel_y", "ang_vel_yaw"] + [f"abs_torque_{i}" for i in range(nu)] +
                      [f"tracking_err_{i}" for i in range(min(cd, 3))])
        self.acc = MetricsAccumulator(self.names, device=env.device)
        self.trace = []
        self._row = None
        self._fast = hasattr(env, "info_buf") and hasattr(env, "user_command")   # BatchedEnv: the info dict is views of these
        self._lib = None
        if self._fast and str(env.device).startswith("cuda") and len(self.names) <= 32:
            from .engine import load_library
            self._lib = load_library()                                # (typed there: engine.ABI)
        self.steps = 0
        self.episodes_ended = 0
        self.policy_table = None      # a policy.PolicyTable (Runner sets it): summary() then breaks episodes and checks down by policy (a rotating one: by the policy of each record's episode ordinal)
        self.hist = None
        if percentiles:
            if self._lib is None:
                raise RuntimeError("FleetReporter(percentiles=True) needs the BatchedEnv GPU path (libcosim_hip.so)")
            from .model import get_field
            t = env.torch
            blob = env.cm.blob
            maxtq = [float(x) for x in get_field(blob, "ctl_maxtq")[:nu]]
            self.hist_hi = np.array([2.0, 8.0, 8.0, 8.0] + [max(1e-3, m) for m in maxtq] + [8.0] * min(cd, 3), dtype=np.float32)
            self._hist_hi_dev = t.tensor(self.hist_hi, device=env.device)
            self.hist = t.zeros((len(self.names), NBINS), dtype=t.float64, device=env.device)

    def write_info_range(self, first: int, count: int):
        """GPU fast path for a fleet stepped as several ranges on streams of their own (``BatchedEnv.step_range``): reduce the info
        rows of envs [first, first + count) on the CURRENT stream -- the stream that range's step was launched on -- into the shared
        accumulator (double atomics), so sampling a step needs no cross-stream wait.  Call once per range; ``steps`` counts one
        sampled step when the last range (first + count == num_envs) is written."""
        if not (self._fast and self._lib is not None):
            raise RuntimeError("write_info_range needs the BatchedEnv GPU path (libcosim_hip.so)")
        t = self.env.torch
        e = self.env
        nu, cd = e.action_dim, min(e.command_dim, 3)
        if first < 0 or count <= 0 or first + count > e.num_envs:
            raise ValueError("write_info_range: range outside the fleet")
        rc = self._lib.cosim_fleet_stats(e.info_buf.data_ptr() + first * e.info_buf.shape[1] * 4, count, e.info_buf.shape[1], nu,
                                         e.applied_command.data_ptr() + first * e.user_command.shape[1] * 4, e.user_command.shape[1], cd,
                                         self.acc.buf.data_ptr(), t.cuda.current_stream(e.device).cuda_stream)
        if rc != 0:
            raise RuntimeError(self._lib.cosim_last_error().decode())
        self._hist_rows(first, count)
        if first + count == e.num_envs:
            self.steps += 1

    def _hist_rows(self, first: int, count: int):
        if self.hist is None:
            return
        e, t = self.env, self.env.torch
        rc = self._lib.cosim_fleet_hist(e.info_buf.data_ptr() + first * e.info_buf.shape[1] * 4, count, e.info_buf.shape[1], e.action_dim,
                                        e.applied_command.data_ptr() + first * e.user_command.shape[1] * 4, e.user_command.shape[1],
                                        min(e.command_dim, 3), self._hist_hi_dev.data_ptr(), NBINS, self.hist.data_ptr(),
                                        t.cuda.current_stream(e.device).cuda_stream)
        if rc != 0:
            raise RuntimeError(self._lib.cosim_last_error().decode())

    def percentiles(self, qs=(0.05, 0.5, 0.95)) -> dict:
        """p5 / p50 / p95 (or ``qs``) per metric column from the histograms, all-reduced over ranks; linear inside a bin."""
        import torch.distributed as dist
        h = self.hist.clone()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
        h = h.cpu().numpy()
        out = {}
        for i, name in enumerate(self.names):
            c = np.cumsum(h[i])
            n = c[-1]
            width = float(self.hist_hi[i]) / NBINS
            row = {}
            for q in qs:
                if n <= 0:
                    row[f"p{int(round(100 * q))}"] = float("nan")
                    continue
                b = int(np.searchsorted(c, q * n, side="left"))
                b = min(b, NBINS - 1)
                below = c[b - 1] if b > 0 else 0.0
                frac = (q * n - below) / max(h[i, b], 1e-300)
                row[f"p{int(round(100 * q))}"] = (b + min(max(frac, 0.0), 1.0)) * width
            row["bin_width"] = width
            out[name] = row
        return out

    def write_info(self, info):
        """``info``: the dict of ``BatchedEnv.step`` (on the GPU fast path it is only a token: the statistics are reduced from
        the env's own ``info_buf`` / ``applied_command`` buffers, which the dict's entries are views of)."""
        t = self.env.torch
        nu, cd = self.env.action_dim, min(self.env.command_dim, 3)
        # one row per env: [action_diff_RMSE, lin_vel_x, lin_vel_y, ang_vel_yaw, |torque|..., |command - measured|...]
        # (command tracking as in reporter.py:506-508: applied command 0, 1 vs base linear velocity, 2 vs yaw rate)
        if self._fast and self._lib is not None:
            # BatchedEnv on a GPU: the info dict is views of info_buf / applied_command -> one launch of the engine's reducer
            e = self.env
            rc = self._lib.cosim_fleet_stats(e.info_buf.data_ptr(), e.num_envs, e.info_buf.shape[1], nu, e.applied_command.data_ptr(),
                                             e.user_command.shape[1], cd, self.acc.buf.data_ptr(),
                                             t.cuda.current_stream(e.device).cuda_stream)
            if rc != 0:
                raise RuntimeError(self._lib.cosim_last_error().decode())
            self._hist_rows(0, e.num_envs)
        else:
            if self._row is None:
                self._row = t.empty((self.env.num_envs, len(self.names)), dtype=t.float32, device=self.env.device)
            self._row[:, :4] = t.cat([info["action_diff_RMSE"][:, None], info["lin_vel_x"][:, None], info["lin_vel_y"][:, None],
                                      info["ang_vel_yaw"][:, None]], dim=1)
            t.abs(info["torque"], out=self._row[:, 4:4 + nu])
            if cd:
                cmd = t.stack([info[f"user_command_{i}"] for i in range(cd)], dim=1)
                t.abs(cmd - self._row[:, 1:1 + cd], out=self._row[:, 4 + nu:4 + nu + cd])
            self.acc.update(self._row)
        self.steps += 1
        if self.trace_env is not None:
            i = self.trace_env
            row = {}
            for k, v in info.items():
                if hasattr(v, "shape") and len(v.shape) >= 1 and v.shape[0] == self.env.num_envs:
                    x = v[i].detach().cpu().numpy()
                    row[k] = x.astype(np.float64) if x.ndim else float(x)
                else:
                    row[k] = v
            self.trace.append(row)

    def note_done(self, terminated, truncated):
        self.episodes_ended += int((terminated | truncated).sum().item())

    def summary(self) -> dict:
        out = {"control_steps": self.steps, "envs": self.env.num_envs, "episodes_ended": self.episodes_ended, "metrics": self.acc.reduce()}
        if self.hist is not None:
            out["percentiles"] = self.percentiles()
        if getattr(self.env, "ledger_slots", 0) > 0:
            out["episodes"] = self.episodes()
        if getattr(self.env, "check_slots", 0) > 0:
            out.setdefault("episodes", {})["checks"] = self.checks()
        if getattr(self.env, "curves_armed", False):
            cs = self.fleet_curves().summary()
            if "by_group" in cs:                                       # set_curve_groups(policy table): the planes are the policies
                cs["by_policy"] = cs.pop("by_group")
            out.setdefault("episodes", {})["curves"] = cs
        if getattr(self.env, "search_slots", 0) > 0:
            out.setdefault("episodes", {})["search"] = self.search()
        return out

    def fleet_curves(self):
        """The env's response curves (``BatchedEnv(scenarios=TABLE, curves=True)``) as a ``Curves``.  Under ``torch.distributed`` the
        cells are all-reduced -- SUM for the counts, the fixed-point sums and the histograms, MIN / MAX for the extremes' keys -- so
        ranks that set the same table hold one fleet's curves, exactly.  With groups set (``env.set_curve_groups``) the reduction
        covers all G planes (one plane's word kinds, tiled) and the ``ungrouped`` count; ``summary()`` then reports ``by_policy``: per
        group name that plane's own summary."""
        import torch.distributed as dist
        from .curves import Curves
        cv = self.env.curves()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = self.env.torch
            kind = cv.word_kinds()
            cells = cv.cells.copy()
            for k, op, view in ((0, dist.ReduceOp.SUM, None), (3, dist.ReduceOp.SUM, np.int64), (1, dist.ReduceOp.MIN, None), (2, dist.ReduceOp.MAX, None)):
                w = cells[kind == k]
                x = t.tensor((w.view(view) if view is not None else w).astype(np.int64), dtype=t.int64, device=self.env.device)
                dist.all_reduce(x, op=op)
                y = x.cpu().numpy()
                cells[kind == k] = y.view(np.uint32) if view is not None else y.astype(np.uint32)
            lost = t.tensor([cv.ungrouped], dtype=t.int64, device=self.env.device)
            dist.all_reduce(lost, op=dist.ReduceOp.SUM)
            cv = Curves(cells, cv.adr, cv.spec, cv.lohi, cv.bins, cv.names, groups=cv.groups, group_names=cv.group_names if cv.grouped else None,
                        ungrouped=int(lost.item()))
        return cv

    def search(self) -> dict:
        """The env's limit search (``BatchedEnv(scenarios=TABLE, search=SLOTS)``) summarised: ``SearchResult.summary()`` plus
        ``by_scenario``.  Under ``torch.distributed`` the integer counts are all-reduced (``fleet``); the thresholds stay this rank's."""
        import torch.distributed as dist
        r = self.env.search(include_trials=False)
        out = r.summary()
        out["by_scenario"] = {str(k): x for k, x in r.by_scenario().items()}
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            out["fleet"] = self._allreduce_counts(r.counts())
        return out

    def checks(self) -> dict:
        """The verdicts of the env's scenario checks (``BatchedEnv(scenarios=TABLE, check_slots=SLOTS)``) summarised:
        ``Verdicts.summary()`` plus ``by_scenario``.  Under ``torch.distributed`` the integer counts are all-reduced (``fleet``, with the
        shares of the whole fleet); the records, and so the per-check tables, stay this rank's."""
        import torch.distributed as dist
        from .checks import Verdicts
        v = self.env.verdicts()
        out = v.summary()
        out["by_scenario"] = {str(k): x for k, x in v.by_scenario().items()}
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            out["fleet"] = Verdicts.with_shares(self._allreduce_counts(v.counts()))
        if self.policy_table is not None:
            out["by_policy"] = self._by_policy(v.by_policy(self.policy_table), v.by_policy(self.policy_table, scenario=True),
                                               [k for k in v.counts() if k != "lost"], Verdicts.with_shares)
        return out

    def _allreduce_counts(self, counts: dict) -> dict:
        """A dict of integer counts summed over the ranks of ``torch.distributed`` (one all-reduce; every rank holds the same keys),
        in sorted key order."""
        import torch.distributed as dist
        t = self.env.torch
        keys = sorted(counts)
        x = t.tensor([counts[k] for k in keys], dtype=t.int64, device=self.env.device)
        dist.all_reduce(x, op=dist.ReduceOp.SUM)
        return {k: int(y) for k, y in zip(keys, x.cpu().tolist())}

    def _by_policy(self, per_policy: dict, per_cell: dict, count_keys, finish) -> dict:
        """The report's ``by_policy``: name -> that policy's columns, its ``by_scenario`` rows (the checkpoint x scenario matrix) where
        the records name a scenario, and under ``torch.distributed`` ``fleet``: the integer counts ``count_keys`` all-reduced over
        ranks (every rank holds the same names in the same order) and finished by ``finish``."""
        import torch.distributed as dist
        names = list(self.policy_table.names)
        out = {name: dict(per_policy[name]) for name in names if name in per_policy}
        for (name, s), cell in per_cell.items():
            if s >= 0:
                out[name].setdefault("by_scenario", {})[str(s)] = cell
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            fleet = self._allreduce_counts({(name, k): per_policy.get(name, {}).get(k, 0) for name in names for k in count_keys})
            for name in names:
                out.setdefault(name, {})["fleet"] = finish({k: fleet[(name, k)] for k in count_keys})
        return out

    def episodes(self) -> dict:
        """The env's episode ledger (``BatchedEnv(ledger=SLOTS)``) summarised: ``EpisodeLedger.summary()`` -- the ``fell`` counts per cause of a
        fall rule among it -- plus the per-spawn-row counts.  Under ``torch.distributed`` the integer counts and the length sum are all-reduced (``fleet``); the records, and so
        the quantiles and the means of record means, stay this rank's."""
        import torch.distributed as dist
        led = self.env.ledger()
        out = led.summary()
        fell = True if getattr(self.env, "fall_rule", None) is not None else None   # a fall rule is set: the fell columns, zeros included
        out["by_spawn_row"] = {str(k): v for k, v in led.by_spawn_row(fell).items()}
        if getattr(self.env, "scenario_table", None) is not None:
            out["by_scenario"] = {str(k): v for k, v in led.by_scenario(fell).items()}
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            fleet = self._allreduce_counts(led.counts())
            fleet["length_mean"] = fleet["length_sum"] / fleet["episodes"] if fleet["episodes"] else None
            out["fleet"] = fleet
        if self.policy_table is not None:
            def shares(c):
                e = c["episodes"]
                return {**c, "terminated_share": c["terminated"] / e if e else None, **({"fell_share": c["fell"] / e if e else None} if "fell" in c else {})}
            out["by_policy"] = self._by_policy(led.by_policy(self.policy_table, fell=fell), led.by_policy(self.policy_table, scenario=True, fell=fell),
                                               ["episodes", "terminated"] + (["fell"] if fell else []), shares)
        return out

    def save(self, path: str, extra: Optional[dict] = None):
        out = self.summary()
        if extra:
            out.update(extra)
        if self.trace:
            out["trace_env"] = self.trace_env
            out["trace"] = {k: np.asarray([r[k] for r in self.trace]).tolist() for k in self.trace[0]}
        with open(path, "w") as f:
            json.dump(out, f)
        return out
