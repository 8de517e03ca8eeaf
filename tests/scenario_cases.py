"""The hand-written scenario table shared by tests/test_scenario_host.py and tests/test_gpu_scenario.py (no test in this file).

Five scenarios for a 4-value command (flamingo_light_v1); with max_duration = 0.5 an episode's pre-step clock runs 0 .. 24:
  0  empty: the caller's command passes through, never a push
  1  first keyframe at t = 3 (the caller's command before it), a second at t = 10
  2  keyframes at t = 0, t = 24 (the episode's last step) and t = 25 (never reached under the time limit)
  3  overlapping push windows: [5, 12) and, listed after it, [8, 10): in 8, 9 the last listed wins; one keyframe at 0
  4  a push window across the time limit, [22, 30): held in 22 .. 24, gone after the auto-reset
"""
import numpy as np

CD = 4
NEVER = [9.0, 9.0, 9.0, 9.0]   # the keyframe at t = 25
TABLE5 = [
    {},
    {"commands": [[3, 1.0, 0.0, 0.0, 0.0], [10, 0.2, 0.0, 0.3, 0.0]]},
    {"commands": [[0, 0.4, 0.0, 0.0, 0.0], [24, 0.8, 0.0, 0.0, 0.0], [25] + NEVER]},
    {"commands": [[0, 0.3, 0.1, 0.0, 0.0]], "pushes": [[5, 12, 0.5, 0.0, 0.0], [8, 10, 0.0, 0.4, 0.1]]},
    {"pushes": [[22, 30, -0.3, 0.2, 0.0]]},
]
BASE = np.array([0.5, 0.0, 0.0, 0.0], dtype=np.float32)   # the caller's command


def table5():
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable(TABLE5, CD)


def table5_variant():
    """The same sizes (S, keyframes, windows) with other values: what an in-place rewrite uploads."""
    from cosim_amd.scenario import ScenarioTable
    t = [dict(s) for s in TABLE5]
    t[1] = {"commands": [[2, 0.7, 0.0, 0.0, 0.0], [6, 0.1, 0.0, -0.2, 0.0]]}
    t[4] = {"pushes": [[1, 4, 0.2, -0.3, 0.0]]}
    return ScenarioTable(t, CD)
