"""How many persistent workgroups DenseExactAdam's table sweep gets: the closed-loop controller, host logic only.

The optimiser records the events (step begin, sweep start / end, step end) and hands them over; nothing here creates,
records or enqueues anything.  The single-process policy only ever ``query()``s an event, the row-sharded group's waits
(``synchronize()``) at its two decision steps per scan.

    ctl.tune(step)              a step is about to be enqueued as host step `step`: the only place the level changes
    ctl.began(ev, step)         ... it began: a record is opened at the current level
    ctl.swept(start, end)       ... its sweep launch was bracketed by these two events
    ctl.ended(ev)               ... it ended: the record is filed until its events have completed
    ctl.level                   workgroups for the sweep launches, 0 = library default
    ctl.note(), ctl.pin(level, why)
"""
from __future__ import annotations

import os
import sys
from typing import Callable, Dict, List, Optional, Sequence


class StepRecord:
    """The timing events of one optimiser step and the sweep level it ran at."""

    __slots__ = ("begin", "sweep_start", "sweep_end", "end", "level", "step", "next_begin")

    def __init__(self, begin, level: int, step: int):
        self.begin, self.level, self.step = begin, level, step
        self.sweep_start = self.sweep_end = self.end = None
        self.next_begin = None  # the NEXT step's begin event, once that step has begun

    def last_event(self):
        # a step's time = begin to the NEXT step's begin where that is known: what lies between a step's end and
        # the next one's begin (routing the next batch's lookups) waits for more or less of the sweep's tail
        # depending on the level -- begin-to-end under-read the slowest level by 0.13 ms and picked it (round 5)
        return self.next_begin if self.next_begin is not None else self.end

    def step_ms(self) -> float:
        return self.begin.elapsed_time(self.last_event())

    def sweep_ms(self) -> float:
        return self.sweep_start.elapsed_time(self.sweep_end)


# The sweep saturates HBM for as long as it lasts, and everything that runs next to it is stretched 2-3x.  When the
# sweep IS the step (headline shape: 5.0 of 5.3 ms) that is free; when the forward/backward chain is as long as the
# sweep or longer, a thinner sweep (fewer persistent workgroups) that ends with the chain instead of well before it
# is faster overall -- C2: 1.27 ms at 768 workgroups, 1.14 at 512, 1.43 at 256; history model: best at 128-256.
# The best level depends on the shapes, so it is MEASURED, on the events of steps that have already completed
# (queried, never waited on: no host synchronisation is added):
#   probe   full width until two steps have been seen; sweep > 0.9 of the step -> keep full width, done
#   scan    otherwise the next len(levels) * SCAN_BLOCK steps run the levels one block each, enqueued OPEN LOOP (the
#           host may be dozens of steps ahead of the GPU: waiting for each level's verdict before trying the next
#           would stretch the scan over hundreds of steps)
#   wait    full width until the last scan step's events are in, then the level with the fastest step is kept
# and the whole thing repeats every RESCAN_STEPS steps.  Results do not depend on the level: the sweep's chunks
# are handed out dynamically either way.
class SweepController:
    _SWEEP_LEVELS = (0, 640, 512, 384, 256, 128)  # workgroups; 0 = library default (3 per CU = 768)
    _SCAN_BLOCK = 6  # steps per level; the first one of a block overlaps the previous level's tail and is not counted
    # row-sharded group: every level TWICE (down the list and back up), 16-step blocks, the first 4 steps of a block not
    # counted, the median of a level's 24 steps kept; the first scan of an optimiser starts after 40 steps.  Pinned levels
    # at the emulated W = 8 step (tools/bench_emulated_world.py, EMU_FORCE_LEVELS): 4.54 / 4.42 / 4.58 / 4.21 / 4.18 / 4.47
    # ms for 768 / 512 / 384 / 256 / 192 / 128 workgroups, the same within 0.02 ms at once after every switch.  But the
    # first ~150 steps of a process run 0.1 - 0.3 ms slower than the steady state and speed up as they go, so a one-way
    # scan right at the start read its LAST level (128) as the best and kept it: 4.5 instead of 4.2 ms (round 5).
    _GROUP_SCAN_BLOCK = 16
    _GROUP_SCAN_SKIP = 4
    _GROUP_SCAN_DELAY = 40
    _RESCAN_STEPS = 4000

    def __init__(self, resume_step: int = 0) -> None:
        self.level = 0  # 0 = library default (3 workgroups per CU)
        self.resume_step = resume_step  # step count adopted from a checkpoint: the first steps after it are not counted
        self.record: Optional[StepRecord] = None  # the step in flight
        self.pending: List[StepRecord] = []  # finished steps whose events may still be pending on the GPU
        self.phase: Optional[str] = None  # None (nothing measured yet), "probe", "scan", "wait", "locked"
        self.why: Optional[str] = None  # what the latest lock was decided on
        self.obs: Dict[int, list] = {}  # level -> [(step ms, sweep ms)]
        self.plan: List[int] = []  # the levels of the scan's steps
        self.skip: set = set()  # steps that are not counted (the first of a scan block)
        self.last = 0  # the scan's last step
        self.since = 0  # steps since the lock

    # ---- what the optimiser tells the controller
    def tune(self, step: int) -> None:
        """Host step `step` is about to be enqueued: choose its level."""
        if os.environ.get("TT_SWEEP_WGS") is not None:
            return
        self._tune(step)

    def began(self, begin, step: int) -> None:
        if self.pending and self.pending[-1].step == step - 1 and self.pending[-1].next_begin is None:
            self.pending[-1].next_begin = begin  # the previous step's record: its full period ends where this step begins
        self.record = StepRecord(begin, self.level, step)

    def swept(self, start, end) -> None:
        self.record.sweep_start, self.record.sweep_end = start, end

    def ended(self, end) -> None:
        self.record.end = end
        if len(self.pending) < 1024:  # never drop a PENDING measurement: when the host runs many steps ahead the
            self.pending.append(self.record)  # oldest one is the next to complete (new ones are skipped meanwhile)
        self.record = None

    def note(self) -> str:
        """How the sweep's width was chosen (bench.py prints it)."""
        if os.environ.get("TT_SWEEP_WGS") is not None:
            return "fixed by TT_SWEEP_WGS"
        if self.phase is None:
            return "not measured yet"
        return self.why if self.why is not None else self.phase

    def pin(self, level: int, why: str) -> None:
        """Hold `level` as if a scan had decided on it (a measurement aid: the next rescan is RESCAN_STEPS steps away)."""
        self._settle(level, why)
        self.pending.clear()

    # ---- the policy
    def _settle(self, level: int, why: str) -> None:
        self.level = level
        self.phase, self.why = "locked", why
        self.obs, self.plan, self.skip, self.since = {}, [], set(), 0

    def _lock(self, level: int, why: str) -> None:
        self._settle(level, f"{level or 768} workgroups: {why}")
        if os.environ.get("TT_TUNE_DEBUG"):
            print(f"[tt] sweep level: {level or 768} workgroups ({why})", file=sys.stderr)

    def _tune(self, step: int) -> None:
        if self.phase is None:
            self.phase = "probe"
        levels = self._SWEEP_LEVELS
        newest = 0
        while self.pending and self.pending[0].sweep_end.query() and self.pending[0].end.query():
            rec = self.pending.pop(0)
            newest = rec.step
            if rec.step - self.resume_step <= 4 or rec.step in self.skip:
                continue  # the first steps SINCE CONSTRUCTION OR RESUME (allocations, first-use set-up) / the first step of a scan block
            # begin to END: the next step's begin event is not known to have completed, and nothing here waits
            self.obs.setdefault(rec.level, []).append((rec.begin.elapsed_time(rec.end), rec.sweep_ms()))
        if self.phase == "probe":
            seen = self.obs.get(0, [])
            if len(seen) >= 2:
                if all(sweep > 0.9 * st for st, sweep in seen[-2:]):
                    self._lock(0, "the sweep is the step")
                else:
                    nxt = step
                    for lv in levels[1:]:
                        self.skip.add(nxt)
                        self.plan += [lv] * self._SCAN_BLOCK
                        nxt += self._SCAN_BLOCK
                    self.skip.add(nxt)  # back to full width: its first step overlaps the thinnest level's tail
                    self.last = nxt - 1
                    self.phase = "scan"
        if self.phase == "scan":
            if self.plan:
                self.level = self.plan.pop(0)
            else:
                self.level = levels[0]
                self.phase = "wait"
        elif self.phase == "wait":
            if newest >= self.last:
                ms = {lv: min(st for st, _ in o) for lv, o in self.obs.items() if len(o) >= 2}
                self._lock(min(ms, key=ms.get) if ms else 0, str({(lv or 768): round(v, 3) for lv, v in ms.items()}))
        elif self.phase == "locked":
            self.since += 1
            if self.since >= self._RESCAN_STEPS:
                self.level = levels[0]
                self.phase, self.obs, self.plan, self.skip, self.since = "probe", {}, [], {step}, 0


class GroupSweepController(SweepController):
    """Row-sharded group: the steps of all ranks are synchronised by the collectives, so the best level is a property of
    the GROUP, and ranks that locked different levels on local timing noise would drag each other.  Same probe / scan /
    decide as above, but every decision is taken at a step number all ranks reach, from the MAX over the ranks of each
    level's median step time (two host waits per scan, i.e. per 4000 steps).
    `all_reduce(values, op) -> list of floats`, op "min" or "max": the group's element-wise reduction."""

    def __init__(self, all_reduce: Callable[[Sequence[float], str], List[float]], resume_step: int = 0) -> None:
        super().__init__(resume_step)
        self.all_reduce = all_reduce
        self.t0 = 0  # the step the probe starts at
        self.scan_start = 0

    def _collect(self) -> Dict[int, list]:
        obs: Dict[int, list] = {}
        for rec in self.pending:
            rec.last_event().synchronize()
            if rec.step < self.t0 + 4 or rec.step in self.skip:
                continue
            obs.setdefault(rec.level, []).append((rec.step_ms(), rec.sweep_ms()))
        self.pending.clear()
        return obs

    def _tune(self, step: int) -> None:
        levels = self._SWEEP_LEVELS
        if self.phase is None:  # (the first probe waits: see _GROUP_SCAN_DELAY)
            self.phase, self.t0 = "probe", step + self._GROUP_SCAN_DELAY
        if self.phase == "probe":
            self.level = levels[0]
            if step == self.t0 + 8:
                seen = self._collect().get(0, [])
                mine = 1.0 if (len(seen) >= 2 and all(sweep > 0.9 * st for st, sweep in seen[-2:])) else 0.0
                if self.all_reduce([mine], "min")[0] > 0.5:
                    self._lock(0, "the sweep is the step on every rank")
                else:
                    self.plan, self.skip, nxt = [], set(), step
                    for lv in levels[1:] + levels[:0:-1]:  # down the levels and back up: a drift over the scan cancels
                        self.skip.update(range(nxt, nxt + self._GROUP_SCAN_SKIP))  # a block's first steps are not the level's steady state
                        self.plan += [lv] * self._GROUP_SCAN_BLOCK
                        nxt += self._GROUP_SCAN_BLOCK
                    self.skip.add(nxt)
                    self.phase, self.scan_start = "scan", step
        if self.phase == "scan":
            k = step - self.scan_start
            self.level = self.plan[k] if k < len(self.plan) else levels[0]
            if k == len(self.plan) + 3:
                obs = self._collect()
                # the MEDIAN step of each level's block (the single-GPU controller keeps the fastest step; here one lucky step
                # decided between levels 7 % apart in steady state: emulated W = 8, 4.19 vs 4.51 ms, round 5)
                def median(v):
                    v = sorted(v)
                    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])

                local = [median([st for st, _ in obs.get(lv, [])]) if len(obs.get(lv, [])) >= 3 else 1.0e9 for lv in levels]
                worst = self.all_reduce(local, "max")
                best = min(range(len(levels)), key=lambda i: (worst[i], i))
                self._lock(levels[best], "group (max over ranks of each level's median step time): "
                           + str({(lv or 768): round(v, 3) for lv, v in zip(levels, worst) if v < 1.0e8}))
        elif self.phase == "locked":
            self.pending.clear()
            self.since += 1
            if self.since >= self._RESCAN_STEPS:
                self.phase, self.why, self.t0, self.since = "probe", None, step, 0
