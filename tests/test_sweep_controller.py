"""DenseExactAdam's sweep-width controller (two_tower_models_amd/sweep_controller.py) on stub events: no GPU, no library.
The controller only ever sees (step time, sweep time, level, step number) of steps that have completed, with the host
an arbitrary number of steps ahead -- which is exactly what the stubs model."""
import json
import os
import threading

import pytest
import torch

from two_tower_models_amd.sweep_controller import GroupSweepController, SweepController

# the decisions of the controller as it was while it lived inside DenseExactAdam, scenario by scenario
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_controller_traces.json")) as _f:
    TRACES = json.load(_f)

MS = {0: 1.30, 640: 1.31, 512: 1.18, 384: 1.21, 256: 1.41, 128: 2.3}
NO_GAP = {lv: 0.0 for lv in SweepController._SWEEP_LEVELS}


class _Ev:
    def __init__(self, t, done=lambda: True):
        self.t, self.done = t, done

    def query(self):
        return self.done()

    def synchronize(self):
        pass

    def elapsed_time(self, other):
        return other.t - self.t


def _run_steps(ctl, ms, gap, sweep, n_steps, lag=0, first_step=1):
    """n_steps host steps the way the optimiser reports them; the GPU completes step k when the host is at step k + lag.
    ms / gap: a step's begin-to-end time and the time from its end to the next begin, per level."""
    host = [first_step - 1]  # steps enqueued so far
    history, now = [], 0.0  # now: GPU time at which the step begins
    for _ in range(n_steps):
        k = host[0] + 1
        ctl.tune(k)
        done = (lambda k=k: host[0] >= k + lag)
        ctl.began(_Ev(now, done), k)
        host[0] = k
        lv = ctl.level
        ctl.swept(_Ev(now, done), _Ev(now + sweep, done))
        ctl.ended(_Ev(now + ms[lv], done))
        now = now + ms[lv] + gap[lv]
        history.append(lv)
    return history


def _drive(step_ms_of, sweep_ms, lag, n_steps):
    ctl = SweepController()
    return ctl, _run_steps(ctl, {lv: step_ms_of(lv) for lv in ctl._SWEEP_LEVELS}, NO_GAP, sweep_ms, n_steps, lag)


@pytest.mark.parametrize("lag", [0, 2, 40])
def test_sweep_bound_step_keeps_full_width(lag):
    ctl, hist = _drive(lambda lv: 5.3, 5.0, lag, 200)
    assert set(hist) == {0} and ctl.phase == "locked"


@pytest.mark.parametrize("lag", [0, 3, 40])
def test_chain_bound_step_scans_every_level_once_and_keeps_the_fastest(lag):
    ctl, hist = _drive(lambda lv: MS[lv], 1.0, lag, 300)
    assert ctl.phase == "locked" and ctl.level == 512
    for lv in (640, 512, 384, 256, 128):  # one block per level while scanning, the winner for the rest
        assert hist.count(lv) >= SweepController._SCAN_BLOCK
        if lv != 512:
            assert hist.count(lv) == SweepController._SCAN_BLOCK
    assert all(lv == 512 for lv in hist[-100:])


def test_rescan_after_the_interval():
    ctl, hist = _drive(lambda lv: MS[lv], 1.0, 1, SweepController._RESCAN_STEPS + 200)
    assert hist.count(128) == 2 * SweepController._SCAN_BLOCK and ctl.level == 512


def _drive_group(local_ms, sweep_ms, n_steps, gap=NO_GAP):
    """Two simulated ranks of a row-sharded group run GroupSweepController in lockstep (one thread each; the all-reduce
    is a barrier + a shared mailbox, in float32 like the real one).  local_ms[r][level] = rank r's step time at that level."""
    world = len(local_ms)
    barrier, mailbox = threading.Barrier(world), {}
    hist, ctls, errors = [None] * world, [None] * world, []

    def run(r):
        def all_reduce(values, op):
            mailbox[r] = torch.tensor(values, dtype=torch.float32)
            barrier.wait()
            stacked = torch.stack([mailbox[q] for q in range(world)])
            out = stacked.min(0).values if op == "min" else stacked.max(0).values
            barrier.wait()
            return [float(v) for v in out]

        try:
            ctls[r] = GroupSweepController(all_reduce)
            hist[r] = _run_steps(ctls[r], local_ms[r], gap, sweep_ms, n_steps)
        except Exception as e:  # a dead thread must not leave the other one waiting on the barrier
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors, errors
    return ctls, hist


def test_group_tuner_takes_the_level_whose_worst_rank_is_fastest_at_the_same_step_on_every_rank():
    """Row-sharded group (GroupSweepController): the sweep level is chosen ONCE for the group, at a step number
    every rank reaches (ranks locking different levels on local timing noise drag each other).  Two ranks whose
    local measurements favour different levels end on the level whose MAX over ranks is smallest, and hold the same level
    at every step, including the step the decision lands on."""
    local_ms = [{0: 4.40, 640: 4.38, 512: 4.20, 384: 4.45, 256: 4.60, 128: 5.0},   # rank 0 alone would take 512
                {0: 4.50, 640: 4.45, 512: 4.70, 384: 4.30, 256: 4.40, 128: 5.2}]   # rank 1 alone 384; group (max): 640
    ctls, hist = _drive_group(local_ms, 1.2, 400)
    assert hist[0] == hist[1]
    assert ctls[0].level == ctls[1].level == 640
    assert ctls[0].phase == "locked" and "group" in ctls[0].why
    for lv in (512, 384, 256, 128):  # every level exactly two blocks while scanning
        assert hist[0].count(lv) == 2 * SweepController._GROUP_SCAN_BLOCK  # down the levels and back up


def test_group_tuner_keeps_full_width_only_if_the_sweep_is_the_step_on_every_rank():
    sweep = 5.0
    bound = {lv: 5.3 for lv in SweepController._SWEEP_LEVELS}
    ctls, hist = _drive_group([bound, bound], sweep, 200)
    assert set(hist[0]) == {0} and ctls[0].phase == "locked"
    # one rank whose step is much longer than its sweep: the group scans
    chain = {0: 7.0, 640: 6.9, 512: 6.5, 384: 6.6, 256: 6.8, 128: 7.5}
    ctls, hist = _drive_group([bound, chain], sweep, 400)
    assert hist[0] == hist[1] and ctls[0].level == 512


def _by_level(table):
    return {int(lv): v for lv, v in table.items()}


def _expanded(runs):
    return [lv for lv, n in runs for _ in range(n)]


@pytest.mark.parametrize("name", sorted(TRACES["single"]))
def test_single_process_decisions_are_the_recorded_ones(name):
    """Every step's level, the final phase and the reason, equal to what the controller decided before it became a class
    (tests/golden/sweep_controller_traces.json; `gap` is there so that begin-to-next-begin timing would decide otherwise)."""
    sc = TRACES["single"][name]
    ctl = SweepController(resume_step=sc["resume"])
    hist = _run_steps(ctl, _by_level(sc["ms"]), _by_level(sc["gap"]), sc["sweep"], sc["steps"], sc["lag"], sc["resume"] + 1)
    assert hist == _expanded(sc["levels_rle"])
    assert (ctl.phase, ctl.why, len(ctl.pending)) == (sc["phase"], sc["why"], sc["pending"])


@pytest.mark.parametrize("name", sorted(TRACES["group"]))
def test_group_decisions_are_the_recorded_ones(name):
    sc = TRACES["group"][name]
    ctls, hist = _drive_group([_by_level(m) for m in sc["local_ms"]], sc["sweep"], sc["steps"], _by_level(sc["gap"]))
    for ctl, h, want in zip(ctls, hist, sc["ranks"]):
        assert h == _expanded(want["levels_rle"])
        assert (ctl.phase, ctl.why, len(ctl.pending)) == (want["phase"], want["why"], want["pending"])


def test_pending_records_are_capped_and_the_new_one_is_dropped():
    ctl = SweepController()
    _run_steps(ctl, MS, NO_GAP, 1.0, 1100, lag=10 ** 6)
    assert [r.step for r in ctl.pending] == list(range(1, 1025))
    assert ctl.pending[0].next_begin is ctl.pending[1].begin and ctl.pending[-1].next_begin is not None


def test_pin_holds_a_level():
    ctl = SweepController()
    ctl.pin(256, "pinned to 256")
    hist = _run_steps(ctl, MS, NO_GAP, 1.0, 50)
    assert set(hist) == {256} and ctl.note() == "pinned to 256" and ctl.phase == "locked"


def _table_optimizer():
    from two_tower_models_amd.optim import DenseExactAdam
    table = torch.nn.Parameter(torch.zeros(8, 4))
    table._tt_is_table = True
    return DenseExactAdam([table])


def test_optimizer_exposes_the_controllers_level_and_note(monkeypatch):
    monkeypatch.delenv("TT_SWEEP_WGS", raising=False)
    opt = _table_optimizer()
    assert opt._sweep_wgs == 0
    opt._sweep_wgs = 384
    assert opt._sweep_wgs == 384
    assert opt.sweep_level_note() == "not measured yet"
    monkeypatch.setenv("TT_SWEEP_WGS", "256")
    assert opt.sweep_level_note() == "fixed by TT_SWEEP_WGS"
    opt._tune_sweep()  # inert: neither the level nor the phase moves
    assert opt._sweep_wgs == 384 and opt._sweep_ctl.phase is None
