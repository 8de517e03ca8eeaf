"""Episode ledger, host side (cosim_amd/ledger.py): the numpy twin of the ledger kernels on hand-written rows with known answers,
the .npz round trip and the arithmetic of summary() / by_spawn_row().  No GPU.  The EXPORTS agreement of the new entry points is
enforced by test_host_logic.test_abi_library_exports_and_layouts."""
import numpy as np

from cosim_amd.ledger import (FLOAT_FIELDS, INT_FIELDS, NONFINITE, NO_RESET, OPEN, TERMINATED, TRUNCATED, EpisodeLedger,
                              reference_ledger, same_records)

NU, CD = 2, 4
INFO_DIM = 4 + 2 * NU + 1


def _rows(K, N):
    """Hand-made step outputs with exactly representable values: env n at step k has action_diff_RMSE = k + 1, lin_vel_x = n,
    lin_vel_y = 0.5, ang_vel_yaw = -0.25, torques (k + n, -(k + 2))."""
    info = np.zeros((K, N, INFO_DIM), dtype=np.float32)
    for k in range(K):
        for n in range(N):
            info[k, n, :4] = [k + 1, n, 0.5, -0.25]
            info[k, n, 4:6] = [k + n, -(k + 2)]
            info[k, n, 6:] = 99.0          # set points / state columns: never read
    return info


def test_twin_on_hand_written_rows():
    K, N = 5, 3
    info = _rows(K, N)
    term, trunc = np.zeros((K, N), dtype=np.uint8), np.zeros((K, N), dtype=np.uint8)
    trunc[2, :] = 1                      # every env's first episode: steps 0..2
    term[3, 1] = 1                       # env 1: a one-step second episode, after a non-finite reset
    nan = np.zeros((K + 1, N), dtype=np.int32)
    nan[4:, 1] = 1                       # meta word 4 of env 1 advanced in step 3
    spawn = np.tile(np.array([4, 5, 6], dtype=np.int32), (K + 1, 1))
    spawn[3:, 2] = 7                     # env 2's auto-reset in step 2 drew row 7
    cmd = np.array([[1.0, 0.0, 0.0, 0.0]] * N, dtype=np.float32)
    led = reference_ledger(info, term, trunc, cmd, nan, spawn, slots=4, nu=NU, command_dim=CD)
    assert led.env.tolist() == [0, 1, 1, 2] and led.episode.tolist() == [0, 0, 1, 0] and led.lost.tolist() == [0, 0, 0]
    assert led.length.tolist() == [3, 3, 1, 3] and led.steps_seen.tolist() == [3, 3, 4, 3]
    assert led.flags.tolist() == [TRUNCATED, TRUNCATED, TERMINATED | NONFINITE, TRUNCATED]
    assert led.spawn_row.tolist() == [4, 5, 5, 6]
    # env 0, steps 0..2: RMSE 1, 2, 3; lin_vel_x 0; tracking |1 - 0|, |0 - 0.5|, |0 + 0.25|; torques (0, -2), (1, -3), (2, -4)
    assert led.mean_action_diff_RMSE[0] == 2.0 and led.mean_lin_vel_x[0] == 0.0
    assert (led.mean_tracking_err_0[0], led.mean_tracking_err_1[0], led.mean_tracking_err_2[0]) == (1.0, 0.5, 0.25)
    assert led.mean_abs_torque[0] == np.float32((1.0 + 2.0 + 3.0) / 3) and led.peak_abs_torque[0] == 4.0 and led.peak_tracking_err_0[0] == 1.0
    # env 1's second episode is step 3 alone: RMSE 4, lin_vel_x 1 -> tracking 0, torques (4, -5)
    assert led.mean_action_diff_RMSE[2] == 4.0 and led.mean_tracking_err_0[2] == 0.0 and led.mean_abs_torque[2] == 4.5
    assert led.peak_abs_torque[2] == 5.0 and led.peak_tracking_err_0[2] == 0.0
    assert (led.words[:, 13:] == 0).all()
    # open rows: env 0 and 2 have run steps 3, 4 of episode 1; env 1 step 4 of episode 2; env 2 started it from row 7
    opn = reference_ledger(info, term, trunc, cmd, nan, spawn, slots=4, nu=NU, command_dim=CD, include_open=True)
    o = opn.flags & OPEN != 0
    assert o.sum() == N and opn.env[o].tolist() == [0, 1, 2] and opn.episode[o].tolist() == [1, 2, 1]
    assert opn.length[o].tolist() == [2, 1, 2] and opn.spawn_row[o].tolist() == [4, 5, 7] and opn.flags[o].tolist() == [OPEN] * 3
    assert opn.mean_action_diff_RMSE[o].tolist() == [4.5, 5.0, 4.5] and opn.steps_seen[o].tolist() == [5, 5, 5]
    assert same_records(EpisodeLedger(opn.words[~o], opn.env[~o], opn.lost, 4), led) is None


def test_twin_order_of_operations_and_nan():
    """Sums are float64 adds of float32 values in step order; the tracking error is an fp32 subtraction; the torque mean an fp32 sum
    and one fp32 divide; the peaks ignore NaN while the sums carry it."""
    K, N = 4, 1
    info = np.zeros((K, N, 4 + 2 * 3), dtype=np.float32)
    vals = np.array([1e8, 1.0, -1e8, 0.3], dtype=np.float32)
    info[:, 0, 0] = vals
    info[:, 0, 1] = np.float32(0.1)
    info[:, 0, 4:7] = np.array([[0.1, 0.2, 0.3], [1e-3, 3.0, -7.5], [np.nan, 1.0, 2.0], [0.5, 0.25, 0.125]], dtype=np.float32)
    trunc = np.zeros((K, N), dtype=np.uint8)
    trunc[3] = 1
    cmd = np.array([[0.3]], dtype=np.float32)
    led = reference_ledger(info, np.zeros_like(trunc), trunc, cmd, None, None, slots=1, nu=3, command_dim=1)
    acc = 0.0
    for v in vals:
        acc += float(v)
    assert led.mean_action_diff_RMSE[0] == np.float32(acc / 4.0)
    d = np.abs(np.float32(0.3) - np.float32(0.1))                      # fp32, not the float64 difference rounded
    assert led.mean_tracking_err_0[0] == np.float32((float(d) * 4) / 4.0) and led.peak_tracking_err_0[0] == d
    assert np.isnan(led.mean_abs_torque[0]) and led.peak_abs_torque[0] == 7.5
    assert led.mean_tracking_err_1[0] == 0.0 and led.mean_tracking_err_2[0] == 0.0 and led.spawn_row[0] == -1
    # the torque mean of one clean step: ((0.1f + 0.2f) + 0.3f) / 3f in float32
    one = reference_ledger(info[:1], np.zeros((1, 1)), np.ones((1, 1)), cmd, None, None, slots=1, nu=3, command_dim=1)
    f = np.float32
    assert one.mean_abs_torque[0] == ((f(0.1) + f(0.2)) + f(0.3)) / f(3)


def test_twin_ring_overflow_begins_and_initial_flags():
    K, N = 7, 2
    info = _rows(K, N)
    term = np.zeros((K, N), dtype=np.uint8)
    term[[1, 3, 5], 0] = 1               # env 0: three two-step episodes; env 1: none ends
    cmd = np.zeros((N, CD), dtype=np.float32)
    led = reference_ledger(info, term, np.zeros_like(term), cmd, None, None, slots=2, nu=NU, command_dim=CD, initial_flags=NO_RESET)
    assert led.env.tolist() == [0, 0] and led.episode.tolist() == [1, 2] and led.lost.tolist() == [1, 0]
    assert led.flags.tolist() == [TERMINATED, TERMINATED]                 # flag 8 was on episode 0 only, which the ring lost
    one = reference_ledger(info, term, np.zeros_like(term), cmd, None, None, slots=4, nu=NU, command_dim=CD, initial_flags=NO_RESET)
    assert one.flags.tolist() == [TERMINATED | NO_RESET, TERMINATED, TERMINATED] and one.lost.tolist() == [0, 0]
    # a host reset of env 0 before step 3 discards its open one-step episode: the next record has length 1 (step 3 alone) and the
    # ordinal the discarded one would have had; a restore of env 1 before step 6 flags its open episode
    spawn = np.full((K + 1, N), 2, dtype=np.int32)
    spawn[3:, 0] = 9
    cut = reference_ledger(info, term, np.zeros_like(term), cmd, None, spawn, slots=4, nu=NU, command_dim=CD, include_open=True,
                           begins=[(3, np.array([1, 0]), 0), (6, np.array([0, 1]), NO_RESET)])
    e0 = cut.env == 0
    assert cut.episode[e0].tolist() == [0, 1, 2, 3] and cut.length[e0].tolist() == [2, 1, 2, 1] and cut.spawn_row[e0].tolist() == [2, 9, 9, 9]
    assert cut.steps_seen[e0].tolist() == [2, 4, 6, 7]
    assert cut.flags[~e0].tolist() == [OPEN | NO_RESET] and cut.length[~e0].tolist() == [1] and cut.steps_seen[~e0].tolist() == [7]


def _ledger():
    n = 6
    words = np.zeros((n, 16), dtype=np.int32)
    words[:, INT_FIELDS["episode"]] = [0, 1, 0, 0, 1, 2]
    words[:, INT_FIELDS["length"]] = [10, 20, 25, 4, 6, 3]
    words[:, INT_FIELDS["flags"]] = [TERMINATED, TRUNCATED, TRUNCATED | NO_RESET, TERMINATED | NONFINITE, TERMINATED, OPEN]
    words[:, INT_FIELDS["spawn_row"]] = [0, 1, 1, 0, 0, 1]
    words[:, INT_FIELDS["steps_seen"]] = [10, 30, 25, 4, 10, 13]
    f = words.view(np.float32)
    f[:, FLOAT_FIELDS["mean_tracking_err_0"]] = [0.1, 0.3, 0.2, np.nan, 0.4, 9.0]
    f[:, FLOAT_FIELDS["peak_abs_torque"]] = [1.0, 2.0, 3.0, np.inf, 4.0, 100.0]
    return EpisodeLedger(words, [7, 7, 8, 9, 9, 9], [0, 0, 3], slots=2, env_id0=7)


def test_summary_arithmetic():
    led = _ledger()
    s = led.summary()
    assert s["episodes"] == 5 and s["terminated"] == 3 and s["truncated"] == 2 and s["non_finite"] == 1 and s["no_reset_start"] == 1
    assert s["lost"] == 3 and s["length_sum"] == 65 and s["terminated_share"] == 0.6
    L = s["length"]
    assert (L["min"], L["max"], L["mean"], L["p50"]) == (4, 25, 13.0, 10.0) and L["p25"] == 6.0 and L["p75"] == 20.0
    # the open row (9.0 / 100.0) and the non-finite record stay out of the means
    assert abs(s["means"]["mean_tracking_err_0"] - np.mean(np.float32([0.1, 0.3, 0.2, 0.4]).astype(np.float64))) < 1e-15
    assert s["means"]["peak_abs_torque"] == 2.5 and s["non_finite_records"] == 1
    by = led.by_spawn_row()
    assert by == {0: {"episodes": 3, "terminated": 3, "terminated_share": 1.0}, 1: {"episodes": 2, "terminated": 0, "terminated_share": 0.0}}
    empty = EpisodeLedger(np.zeros((0, 16), dtype=np.int32), [], [0, 0], slots=2)
    assert empty.summary()["episodes"] == 0 and empty.summary()["length"] is None and empty.by_spawn_row() == {}


def test_npz_round_trip(tmp_path):
    led = _ledger()
    path = str(tmp_path / "episodes.npz")
    led.save(path)
    with np.load(path, allow_pickle=False) as z:                        # plain arrays only
        assert sorted(z.files) == ["env", "header", "lost", "words"]
    back = EpisodeLedger.load(path)
    assert same_records(back, led) is None and back.slots == 2 and back.env_id0 == 7
    np.testing.assert_array_equal(back.words, led.words)                # NaN payloads included
    assert back.summary() == led.summary()


def test_same_records_names_the_difference():
    a, b = _ledger(), _ledger()
    assert same_records(a, b) is None
    b.words[1, INT_FIELDS["length"]] += 1
    assert "length" in same_records(a, b) and "row 1" in same_records(a, b)
    c = _ledger()
    c.words.view(np.float32)[3, FLOAT_FIELDS["mean_tracking_err_0"]] = np.inf     # non-finite against non-finite: equal
    assert same_records(a, c) is None
    c.words.view(np.float32)[0, FLOAT_FIELDS["mean_tracking_err_0"]] = np.nextafter(np.float32(0.1), np.float32(1))
    assert "mean_tracking_err_0" in same_records(a, c)


def test_from_raw_reads_the_ring_in_episode_order():
    rec = np.zeros((2, 3, 16), dtype=np.int32)
    for o in range(5):                                                   # env 0 ended 5 episodes: the ring holds 2, 3, 4
        rec[0, o % 3, 0], rec[0, o % 3, 1] = o, 10 + o
    rec[1, 0, 0], rec[1, 0, 1] = 0, 50                                   # env 1 ended one
    led = EpisodeLedger.from_raw(rec, [5, 1], env_id0=100)
    assert led.env.tolist() == [100, 100, 100, 101] and led.episode.tolist() == [2, 3, 4, 0] and led.length.tolist() == [12, 13, 14, 50]
    assert led.lost.tolist() == [2, 0]
