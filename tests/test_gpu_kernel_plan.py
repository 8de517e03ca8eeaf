"""Which kernel runs when: what the engine reports (``cosim_query``) and which switches it refuses (``cosim_set_param``), fresh
and after each switch sequence, for every robot on the plane, on a coarse heightfield (rocky_easy) and on 1 cm cells (stairs_up_easy).

The expected rows were recorded from the engine as it stood before its kernel choice moved into one launch plan (csrc/cosim_plan.h):
they pin that behaviour, accidents included (DESIGN 4.17 lists those).  After every switch the fleet is reset and stepped twice, and
``rollout()`` must raise exactly where ``rollout`` answers 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROBOTS = ("flamingo_light_v1", "flamingo_p_v3", "w4_p_v2", "humanoid_p_v0")
TERRAINS = ("flat", "rocky_easy", "stairs_up_easy")
QUERIES = ("lds_bytes", "contact_slots", "pair_slots", "fixup_contact_slots", "rollout", "step_kernel", "split")
SEQUENCES = {
    "contact_twist": (("contact_twist", 1), ("contact_twist", 0), ("envs_per_wave", 2)),
    "fixup": (("fixup", 0), ("fixup", 1), ("hfield_fixup", 1)),
    "hfield_fixup": (("hfield_fixup", 1), ("hfield_fixup", 0)),
    "envs_per_wave": (("envs_per_wave", 2), ("envs_per_wave", 1)),
    "split": (("hfield_fixup", 1), ("split", 0), ("split", 1)),   # split 0 / 1 with the heightfield fix-up on (where there is one)
    "step_kernel": (("step_kernel", 0), ("step_kernel", 1)),
}

# per case: "fresh": the seven answers of QUERIES; per sequence, one row per call: [1 if the call raised ValueError, then the seven
# answers after it]; "odd": 1 if "envs_per_wave" 2 raised with 3 envs
EXPECTED = {
    "flamingo_light_v1/flat": {
        "fresh": [10232, 14, 1, 40, 1, 1, 0],
        "contact_twist": [[0, 9408, 32, 1, 0, 0, 0, 0], [0, 9408, 32, 1, 0, 0, 0, 0], [1, 9408, 32, 1, 0, 0, 0, 0]],
        "fixup": [[0, 10232, 14, 1, 0, 0, 1, 0], [0, 10232, 14, 1, 0, 0, 1, 0], [1, 10232, 14, 1, 0, 0, 1, 0]],
        "hfield_fixup": [[1, 10232, 14, 1, 40, 1, 1, 0], [1, 10232, 14, 1, 40, 1, 1, 0]],
        "envs_per_wave": [[0, 10232, 14, 1, 40, 0, 0, 0], [0, 10232, 14, 1, 40, 1, 1, 0]],
        "split": [[1, 10232, 14, 1, 40, 1, 1, 0], [0, 10232, 14, 1, 40, 1, 1, 0], [1, 10232, 14, 1, 40, 1, 1, 0]],
        "step_kernel": [[0, 10232, 14, 1, 40, 1, 0, 0], [0, 10232, 14, 1, 40, 1, 1, 0]],
        "odd": 1,
    },
    "flamingo_light_v1/rocky_easy": {
        "fresh": [12656, 48, 0, 0, 0, 0, 0],
        "contact_twist": [[1, 12656, 48, 0, 0, 0, 0, 0], [0, 12656, 48, 0, 0, 0, 0, 0], [1, 12656, 48, 0, 0, 0, 0, 0]],
        "fixup": [[0, 12656, 48, 0, 0, 0, 0, 0], [0, 12656, 48, 0, 0, 0, 0, 0], [1, 12656, 48, 0, 0, 0, 0, 0]],
        "hfield_fixup": [[0, 12656, 48, 0, 650, 0, 0, 0], [0, 12656, 48, 0, 0, 0, 0, 0]],
        "envs_per_wave": [[1, 12656, 48, 0, 0, 0, 0, 0], [0, 12656, 48, 0, 0, 0, 0, 0]],
        "split": [[0, 12656, 48, 0, 650, 0, 0, 0], [0, 12656, 48, 0, 650, 0, 0, 0], [1, 12656, 48, 0, 650, 0, 0, 0]],
        "step_kernel": [[0, 12656, 48, 0, 0, 0, 0, 0], [0, 12656, 48, 0, 0, 0, 0, 0]],
        "odd": 1,
    },
    "flamingo_light_v1/stairs_up_easy": {
        "fresh": [17456, 128, 0, 0, 0, 0, 0],
        "contact_twist": [[1, 17456, 128, 0, 0, 0, 0, 0], [0, 17456, 128, 0, 0, 0, 0, 0], [1, 17456, 128, 0, 0, 0, 0, 0]],
        "fixup": [[0, 17456, 128, 0, 0, 0, 0, 0], [0, 17456, 128, 0, 0, 0, 0, 0], [1, 17456, 128, 0, 0, 0, 0, 0]],
        "hfield_fixup": [[0, 17456, 128, 0, 650, 0, 0, 0], [0, 17456, 128, 0, 0, 0, 0, 0]],
        "envs_per_wave": [[1, 17456, 128, 0, 0, 0, 0, 0], [0, 17456, 128, 0, 0, 0, 0, 0]],
        "split": [[0, 17456, 128, 0, 650, 0, 0, 0], [0, 17456, 128, 0, 650, 0, 0, 0], [1, 17456, 128, 0, 650, 0, 0, 0]],
        "step_kernel": [[0, 17456, 128, 0, 0, 0, 0, 0], [0, 17456, 128, 0, 0, 0, 0, 0]],
        "odd": 1,
    },
    "flamingo_p_v3/flat": {
        "fresh": [8072, 16, 0, 32, 1, 0, 0],
        "contact_twist": [[0, 9024, 32, 8, 0, 0, 0, 0], [0, 9024, 32, 8, 0, 0, 0, 0], [1, 9024, 32, 8, 0, 0, 0, 0]],
        "fixup": [[0, 8072, 16, 0, 0, 0, 0, 0], [0, 8072, 16, 0, 0, 0, 0, 0], [1, 8072, 16, 0, 0, 0, 0, 0]],
        "hfield_fixup": [[1, 8072, 16, 0, 32, 1, 0, 0], [1, 8072, 16, 0, 32, 1, 0, 0]],
        "envs_per_wave": [[1, 8072, 16, 0, 32, 1, 0, 0], [0, 8072, 16, 0, 32, 1, 0, 0]],
        "split": [[1, 8072, 16, 0, 32, 1, 0, 0], [0, 8072, 16, 0, 32, 1, 0, 0], [1, 8072, 16, 0, 32, 1, 0, 0]],
        "step_kernel": [[0, 8072, 16, 0, 32, 1, 0, 0], [0, 8072, 16, 0, 32, 1, 0, 0]],
        "odd": 1,
    },
    "flamingo_p_v3/rocky_easy": {
        "fresh": [13232, 64, 8, 0, 0, 0, 0],
        "contact_twist": [[1, 13232, 64, 8, 0, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0], [1, 13232, 64, 8, 0, 0, 0, 0]],
        "fixup": [[0, 13232, 64, 8, 0, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0], [1, 13232, 64, 8, 0, 0, 0, 0]],
        "hfield_fixup": [[0, 13232, 64, 8, 400, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0]],
        "envs_per_wave": [[1, 13232, 64, 8, 0, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0]],
        "split": [[0, 13232, 64, 8, 400, 0, 0, 0], [0, 13232, 64, 8, 400, 0, 0, 0], [1, 13232, 64, 8, 400, 0, 0, 0]],
        "step_kernel": [[0, 13232, 64, 8, 0, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0]],
        "odd": 1,
    },
    "flamingo_p_v3/stairs_up_easy": {
        "fresh": [13232, 64, 8, 0, 0, 0, 0],
        "contact_twist": [[1, 13232, 64, 8, 0, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0], [1, 13232, 64, 8, 0, 0, 0, 0]],
        "fixup": [[0, 13232, 64, 8, 0, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0], [1, 13232, 64, 8, 0, 0, 0, 0]],
        "hfield_fixup": [[0, 13232, 64, 8, 400, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0]],
        "envs_per_wave": [[1, 13232, 64, 8, 0, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0]],
        "split": [[0, 13232, 64, 8, 400, 0, 0, 0], [0, 13232, 64, 8, 400, 0, 0, 0], [1, 13232, 64, 8, 400, 0, 0, 0]],
        "step_kernel": [[0, 13232, 64, 8, 0, 0, 0, 0], [0, 13232, 64, 8, 0, 0, 0, 0]],
        "odd": 1,
    },
    "w4_p_v2/flat": {
        "fresh": [18784, 80, 12, 0, 0, 0, 0],
        "contact_twist": [[1, 18784, 80, 12, 0, 0, 0, 0], [0, 18784, 80, 12, 0, 0, 0, 0], [1, 18784, 80, 12, 0, 0, 0, 0]],
        "fixup": [[0, 18784, 80, 12, 0, 0, 0, 0], [0, 18784, 80, 12, 0, 0, 0, 0], [1, 18784, 80, 12, 0, 0, 0, 0]],
        "hfield_fixup": [[1, 18784, 80, 12, 0, 0, 0, 0], [1, 18784, 80, 12, 0, 0, 0, 0]],
        "envs_per_wave": [[1, 18784, 80, 12, 0, 0, 0, 0], [0, 18784, 80, 12, 0, 0, 0, 0]],
        "split": [[1, 18784, 80, 12, 0, 0, 0, 0], [0, 18784, 80, 12, 0, 0, 0, 0], [1, 18784, 80, 12, 0, 0, 0, 0]],
        "step_kernel": [[0, 18784, 80, 12, 0, 0, 0, 0], [0, 18784, 80, 12, 0, 0, 0, 0]],
        "odd": 1,
    },
    "w4_p_v2/rocky_easy": {
        "fresh": [19728, 48, 12, 0, 0, 0, 0],
        "contact_twist": [[1, 19728, 48, 12, 0, 0, 0, 0], [0, 19728, 48, 12, 0, 0, 0, 0], [1, 19728, 48, 12, 0, 0, 0, 0]],
        "fixup": [[0, 19728, 48, 12, 0, 0, 0, 0], [0, 19728, 48, 12, 0, 0, 0, 0], [1, 19728, 48, 12, 0, 0, 0, 0]],
        "hfield_fixup": [[0, 19728, 48, 12, 850, 0, 0, 0], [0, 19728, 48, 12, 0, 0, 0, 0]],
        "envs_per_wave": [[1, 19728, 48, 12, 0, 0, 0, 0], [0, 19728, 48, 12, 0, 0, 0, 0]],
        "split": [[0, 19728, 48, 12, 850, 0, 0, 0], [0, 19728, 48, 12, 850, 0, 0, 0], [1, 19728, 48, 12, 850, 0, 0, 0]],
        "step_kernel": [[0, 19728, 48, 12, 0, 0, 0, 0], [0, 19728, 48, 12, 0, 0, 0, 0]],
        "odd": 1,
    },
    "w4_p_v2/stairs_up_easy": {
        "fresh": [24528, 128, 12, 0, 0, 0, 0],
        "contact_twist": [[1, 24528, 128, 12, 0, 0, 0, 0], [0, 24528, 128, 12, 0, 0, 0, 0], [1, 24528, 128, 12, 0, 0, 0, 0]],
        "fixup": [[0, 24528, 128, 12, 0, 0, 0, 0], [0, 24528, 128, 12, 0, 0, 0, 0], [1, 24528, 128, 12, 0, 0, 0, 0]],
        "hfield_fixup": [[0, 24528, 128, 12, 850, 0, 0, 0], [0, 24528, 128, 12, 0, 0, 0, 0]],
        "envs_per_wave": [[1, 24528, 128, 12, 0, 0, 0, 0], [0, 24528, 128, 12, 0, 0, 0, 0]],
        "split": [[0, 24528, 128, 12, 850, 0, 0, 0], [0, 24528, 128, 12, 850, 0, 0, 0], [1, 24528, 128, 12, 850, 0, 0, 0]],
        "step_kernel": [[0, 24528, 128, 12, 0, 0, 0, 0], [0, 24528, 128, 12, 0, 0, 0, 0]],
        "odd": 1,
    },
    "humanoid_p_v0/flat": {
        "fresh": [25280, 96, 12, 0, 0, 0, 0],
        "contact_twist": [[1, 25280, 96, 12, 0, 0, 0, 0], [0, 25280, 96, 12, 0, 0, 0, 0], [1, 25280, 96, 12, 0, 0, 0, 0]],
        "fixup": [[0, 25280, 96, 12, 0, 0, 0, 0], [0, 25280, 96, 12, 0, 0, 0, 0], [1, 25280, 96, 12, 0, 0, 0, 0]],
        "hfield_fixup": [[1, 25280, 96, 12, 0, 0, 0, 0], [1, 25280, 96, 12, 0, 0, 0, 0]],
        "envs_per_wave": [[1, 25280, 96, 12, 0, 0, 0, 0], [0, 25280, 96, 12, 0, 0, 0, 0]],
        "split": [[1, 25280, 96, 12, 0, 0, 0, 0], [0, 25280, 96, 12, 0, 0, 0, 0], [1, 25280, 96, 12, 0, 0, 0, 0]],
        "step_kernel": [[0, 25280, 96, 12, 0, 0, 0, 0], [0, 25280, 96, 12, 0, 0, 0, 0]],
        "odd": 1,
    },
    "humanoid_p_v0/rocky_easy": {
        "fresh": [38192, 256, 12, 0, 0, 0, 6],
        "contact_twist": [[1, 38192, 256, 12, 0, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6], [1, 38192, 256, 12, 0, 0, 0, 6]],
        "fixup": [[0, 38192, 256, 12, 0, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6], [1, 38192, 256, 12, 0, 0, 0, 6]],
        "hfield_fixup": [[0, 38192, 256, 12, 1100, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6]],
        "envs_per_wave": [[1, 38192, 256, 12, 0, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6]],
        "split": [[0, 38192, 256, 12, 1100, 0, 0, 6], [0, 38192, 256, 12, 1100, 0, 0, 0], [0, 38192, 256, 12, 1100, 0, 0, 6]],
        "step_kernel": [[0, 38192, 256, 12, 0, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6]],
        "odd": 1,
    },
    "humanoid_p_v0/stairs_up_easy": {
        "fresh": [38192, 256, 12, 0, 0, 0, 6],
        "contact_twist": [[1, 38192, 256, 12, 0, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6], [1, 38192, 256, 12, 0, 0, 0, 6]],
        "fixup": [[0, 38192, 256, 12, 0, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6], [1, 38192, 256, 12, 0, 0, 0, 6]],
        "hfield_fixup": [[0, 38192, 256, 12, 1100, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6]],
        "envs_per_wave": [[1, 38192, 256, 12, 0, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6]],
        "split": [[0, 38192, 256, 12, 1100, 0, 0, 6], [0, 38192, 256, 12, 1100, 0, 0, 0], [0, 38192, 256, 12, 1100, 0, 0, 6]],
        "step_kernel": [[0, 38192, 256, 12, 0, 0, 0, 6], [0, 38192, 256, 12, 0, 0, 0, 6]],
        "odd": 1,
    },
}


def _answers(env):
    return [int(env.engine.query(q)) for q in QUERIES]


def _exercise(env):
    """One reset and two steps with finite outputs; rollout() raises exactly where the engine says it has none."""
    torch = env.torch
    state, _ = env.reset()
    assert torch.isfinite(state).all()
    t = np.arange(env.num_envs * env.action_dim, dtype=np.float32).reshape(env.num_envs, env.action_dim)
    for k in range(2):
        state, _, _, _ = env.step(torch.tensor(0.2 * np.sin(t + k), device=env.device))
        assert torch.isfinite(state).all()
    d = env.get_data()
    assert torch.isfinite(d.qpos).all() and torch.isfinite(d.qvel).all()
    table = torch.zeros((2, env.num_envs, env.action_dim), device=env.device)
    if env.engine.query("rollout"):
        states, _, _, _ = env.rollout(table)
        assert torch.isfinite(states).all()
    else:
        with pytest.raises(ValueError, match="no rollout kernel"):
            env.rollout(table)


def observe(robot, terrain):
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    cfg = make_config(robot, terrain=terrain, random=PARITY_RANDOM, num_envs=4)
    cm = compile_model(cfg)

    def make(n=4):
        return BatchedEnv(cfg, num_envs=n, auto_reset=False, compiled=cm)

    env = make()
    out = {"fresh": _answers(env)}
    _exercise(env)
    env.close()
    for name, calls in SEQUENCES.items():
        env = make()
        rows = []
        for param, value in calls:
            raised = 0
            try:
                env.engine.set_param(param, np.array([float(value)]))
            except ValueError:
                raised = 1
            rows.append([raised] + _answers(env))
            _exercise(env)
        env.close()
        out[name] = rows
    env = make(3)
    try:
        env.engine.set_param("envs_per_wave", np.array([2.0]))
        out["odd"] = 0
    except ValueError:
        out["odd"] = 1
    _exercise(env)
    env.close()
    return out


@pytest.mark.parametrize("terrain", TERRAINS)
@pytest.mark.parametrize("robot", ROBOTS)
def test_kernel_plan_answers_and_refusals(robot, terrain):
    got, want = observe(robot, terrain), EXPECTED[robot + "/" + terrain]
    for key in want:
        assert got[key] == want[key], f"{robot}/{terrain} {key}: calls {SEQUENCES.get(key)}, columns [raised] + {QUERIES}"
    assert got.keys() == want.keys()
