"""Host: the driver's one output loop (run_simulation.run_loop) and its schedule (run_simulation.Schedule) against a direct restatement of
the reference's loop -- step once, write a frame when the count before the step is a multiple of the interval, then count.  Fake solver,
engine and AVI writer: no GPU, no library."""
import types

import pytest

from sph_project_amd import run_simulation as R


class Recorder:
    """solver, engine and AVI writer in one"""

    def __init__(self):
        self.advances, self.syncs, self.closed = [], 0, 0

    def advance(self, n):
        self.advances.append(n)

    def synchronize(self):
        self.syncs += 1

    def close(self):
        self.closed += 1


def reference_frames(limit, interval, wants_frame):
    cnt, out = 0, []
    while cnt < limit:
        if cnt % interval == 0 and wants_frame:   # (the step itself comes first in the reference: no frame depends on it here)
            out.append(cnt)
        cnt += 1
    return out


def sched(limit, interval):
    return types.SimpleNamespace(limit=limit, output_interval=interval)


@pytest.mark.parametrize("wants_frame", [True, False])
def test_loop_writes_the_references_frames(wants_frame):
    for limit in range(1, 13):
        for interval in range(1, 6):
            rec, seen = Recorder(), []

            def write_frame(cnt):
                seen.append((cnt, sum(rec.advances)))
                return cnt % 2 == 0   # (frames are counted only when something was written)

            cnt, t_export, frames = R.run_loop(rec, rec, sched(limit, interval), wants_frame, write_frame, [rec])
            where = (limit, interval, wants_frame)
            assert cnt == limit, where
            assert [c for c, _ in seen] == reference_frames(limit, interval, wants_frame), where
            assert all(steps == c + 1 for c, steps in seen), where   # the frame of count c is written after step c + 1, as there
            assert sum(rec.advances) == limit and 0 not in rec.advances, (where, rec.advances)
            assert frames == sum(1 for c, _ in seen if c % 2 == 0) and t_export >= 0.0, where
            assert rec.closed == 1 and rec.syncs == len(seen) + 1, where
            if not wants_frame:
                assert rec.advances == [limit], where


def test_an_exception_in_the_callback_still_closes_the_avi_writer():
    rec = Recorder()

    def write_frame(cnt):
        raise RuntimeError("disk full")

    with pytest.raises(RuntimeError, match="disk full"):
        R.run_loop(rec, rec, sched(7, 2), True, write_frame, [rec])
    assert rec.closed == 1 and rec.advances == [1]


class Config:
    def __init__(self, **cfg):
        self.cfg = cfg

    def get_cfg(self, name):
        return self.cfg.get(name)


def _args(**kw):
    base = dict(scene_file="data/scenes/dam.json", output_dir=None, max_steps=None, render=False)
    return types.SimpleNamespace(**dict(base, **kw))


def test_schedule_steps_once_before_it_looks():
    cfg = Config(timeStepSize=4e-4, exportPly=True)
    assert R.Schedule(cfg, _args(max_steps=0)).limit == 1


def test_schedule_restates_the_interval_arithmetic():
    s = R.Schedule(Config(timeStepSize=4e-4, exportPly=True, exportFrame=True), _args(max_steps=50))
    assert (s.output_interval, s.limit) == (int((1.0 / 60) / 4e-4), 50)   # fps 60, totalTime 10 by default
    assert s.output_ply and not s.output_obj and not s.output_frames and s.out_dir == "dam_output"   # (frames need --render)
    s = R.Schedule(Config(timeStepSize=1e-3, fps=20, totalTime=0.5, outputInterval=7, exportFrame=True), _args(render=True, output_dir="o"))
    assert (s.output_interval, s.limit, s.out_dir) == (7, int(0.5 / 1e-3), "o") and s.output_frames
