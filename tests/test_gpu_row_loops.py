"""The Newton iteration's row loops (J^T f in update_constraint, the Hessian tile) read their dense rows in batches of eight and wait
once per batch.  The FMAs and MFMAs still run in row order on one accumulator, so not a bit of a step may differ from the
one-row-per-trip loops: the reference is tests/golden/row_loops_{light_v1,p_v3}.npz, recorded on the GPU by
tools/gpu_row_loops_golden.py at the commit before the change (named inside the files).

The fleets' poses (in the files) are picked by dense-row count: flamingo_light_v1 has 6 equality rows + 4 per contact -- 6, 10, 14 and
18 rows (below one batch, both remainders 2 and 6 mod 8), counts above 32 and the full 62; flamingo_p_v3 has 4 per contact -- 0 and 4
mod 8.  Its kernels keep the one-row loops (KTraits::ROWB = 1), as does the large-capacity kernel that redoes the steps with more
than 14 contacts: the same comparison holds them to the bits as well."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARRAYS = ("state", "terminated", "info", "qpos", "qvel", "qacc_warmstart")


def _golden(name):
    with np.load(os.path.join(GOLDEN, f"row_loops_{name}.npz")) as z:
        G = {k: z[k] for k in z.files}
    assert len(str(G["commit"])) >= 7                                # the commit the bits are from
    return G


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_golden(G, rows, out, what):
    assert rows.tolist() == G["dense_rows"].tolist(), what
    for k in ARRAYS:
        assert out[k].dtype == G[k].dtype and out[k].shape == G[k].shape, (what, k)
        for t in range(G[k].shape[0]):
            same = _bits(out[k][t]) == _bits(G[k][t])
            assert same.all(), f"{what}: {k} after step {t} differs from the recorded bits in envs {sorted(set(np.argwhere(~same)[:, 0].tolist()))}"


def test_light_v1_fleet_steps_to_the_recorded_bits_with_both_kernels():
    from tools.gpu_row_loops_golden import STEPS, model, run_fleet
    G = _golden("light_v1")
    cfg, cm = model("light_v1")
    assert G["pose_qpos"].shape == (32, cm.blob.nq) and G["actions"].shape == (STEPS, 32, cm.blob.nu) and (G["actions"] != 0).all()
    res = {}
    for sk in (1, 0):
        rows, out = run_fleet(cfg, cm, G["pose_qpos"], G["actions"], step_kernel=sk)
        res[sk] = out
        # below one batch, remainders 2 and 6 mod 8 (one and two batches, with and without the batch of four), all 14 contact slots
        have = set(rows.tolist())
        assert {6, 10, 14, 18, 62} <= have and any(32 < r < 62 for r in have), sorted(have)
        assert {r % 8 for r in have} == {2, 6}
        assert (G["oracle_contacts"] > 14).any()                     # steps the large-capacity kernel redoes are in the fleet too
        _assert_golden(G, rows, out, f"step_kernel {sk}")
    for k in ARRAYS:                                                 # (implied by the above; said once directly)
        assert np.array_equal(_bits(res[1][k]), _bits(res[0][k])), f"{k} differs between step_kernel 1 and 0"
    assert np.isfinite(G["state"]).all() and (G["qpos"][-1] != G["pose_qpos"][None]).any()


def test_p_v3_fleet_steps_to_the_recorded_bits():
    from tools.gpu_row_loops_golden import STEPS, model, run_fleet
    G = _golden("p_v3")
    cfg, cm = model("p_v3")
    assert G["pose_qpos"].shape == (16, cm.blob.nq) and G["actions"].shape == (STEPS, 16, cm.blob.nu) and (G["actions"] != 0).all()
    rows, out = run_fleet(cfg, cm, G["pose_qpos"], G["actions"])
    pos = [r for r in rows.tolist() if r > 0]
    assert any(r % 8 == 0 for r in pos) and any(r % 8 == 4 for r in pos) and max(pos) > 32, rows.tolist()
    _assert_golden(G, rows, out, "flamingo_p_v3")
