"""Host: the driver's loop by scene time (run_simulation.run_loop_timed, adaptive time stepping) -- frames at the instants
j * output_interval * timeStepSize, one advance_to per frame interval, the end at totalTime, --max_steps.  Fake solver, engine and AVI
writer whose steps follow tests/cfl_model.py: no GPU, no library."""
import types

import pytest

from sph_project_amd import run_simulation as R
from tests import cfl_model as M

DT, D = 4e-4, 0.02
PARAMS = (0.15, 1e-5, 6e-4)


class FakeSolver:
    """solver, engine and AVI writer in one: advance_to steps with the model's rule at a speed that changes from step to step"""

    def __init__(self):
        self.time, self.steps, self.calls, self.syncs, self.closed = 0.0, 0, [], 0, 0
        self.container = types.SimpleNamespace(total_time=0.0)

    def _v2(self, k):
        return (2.5 + (self.steps + k) % 7) ** 2   # 2.5 .. 8.5 m/s: strictly inside the clamps

    def advance_to(self, t, max_steps=None):
        cap = (1 << 30) if max_steps is None else max_steps
        dts, self.time = M.advance(*PARAMS, D, self._v2, self.time, t, cap)
        self.steps += len(dts)
        self.container.total_time = self.time
        self.calls.append((t, max_steps, len(dts)))
        return len(dts)

    def synchronize(self):
        self.syncs += 1

    def close(self):
        self.closed += 1


def sched(interval, total_time):
    return types.SimpleNamespace(output_interval=interval, time_step=DT, total_time=total_time, limit=int(total_time / DT))


@pytest.mark.parametrize("interval, total", [(5, 15 * DT), (5, 17.5 * DT), (3, 3 * DT), (41, 0.05), (4, 2 * DT)])
def test_frames_fall_at_the_fixed_runs_instants(interval, total):
    s, seen = FakeSolver(), []
    cnt, t_export, frames = R.run_loop_timed(s, s, sched(interval, total), True, lambda c: seen.append((c, s.time)) or c % 2 == 0, [s])
    want = [j * interval for j in range(1000) if j * interval * DT < total]
    assert [c for c, _ in seen] == want
    for c, t in seen:   # each frame at its instant, within the landing tolerance
        assert abs(t - c * DT) <= 2.0 ** -20 * PARAMS[2], (c, t)
    assert abs(s.time - total) <= 2.0 ** -20 * PARAMS[2] and cnt == s.steps and cnt >= total / PARAMS[2] - 1
    assert [t for t, _, _ in s.calls] == pytest.approx([c * DT for c in want[1:]] + [total])   # one advance_to per frame interval
    assert frames == sum(1 for c, _ in seen if c % 2 == 0) and t_export >= 0.0
    assert s.closed == 1 and s.syncs == len(seen) + 1


def test_without_frames_it_is_one_call():
    s = FakeSolver()
    cnt, _, frames = R.run_loop_timed(s, s, sched(5, 0.01), False, lambda c: pytest.fail("a frame was written"), [s])
    assert s.calls == [(0.01, None, cnt)] and frames == 0 and abs(s.time - 0.01) <= 2.0 ** -20 * PARAMS[2] and s.closed == 1


@pytest.mark.parametrize("max_steps", [1, 2, 7, 12, 13, 10 ** 6])
def test_max_steps_caps_the_steps(max_steps):
    free = FakeSolver()
    total, _, _ = R.run_loop_timed(free, free, sched(5, 15 * DT), True, lambda c: True, [])
    s, seen = FakeSolver(), []
    cnt, _, frames = R.run_loop_timed(s, s, sched(5, 15 * DT), True, lambda c: seen.append(c) or True, [s], max_steps=max_steps)
    assert cnt == min(max_steps, total) == s.steps and frames == len(seen)
    assert all(done <= cap for _, cap, done in s.calls) and sum(done for _, _, done in s.calls) == cnt
    if max_steps >= total:
        assert seen == [0, 5, 10] and abs(s.time - 15 * DT) <= 2.0 ** -20 * PARAMS[2]
    else:
        assert s.time < 15 * DT and seen[0] == 0 and seen == sorted(set(seen)) and set(seen) <= {0, 5, 10}


def test_an_exception_in_the_callback_still_closes_the_avi_writer():
    s = FakeSolver()

    def boom(c):
        raise RuntimeError("disk full")

    with pytest.raises(RuntimeError, match="disk full"):
        R.run_loop_timed(s, s, sched(5, 15 * DT), True, boom, [s])
    assert s.closed == 1


def test_foam_stepper_gets_the_elapsed_scene_time():
    s, steps = FakeSolver(), []
    diffuse = types.SimpleNamespace(step=lambda container, dt: steps.append((s.steps, dt)))
    f = R.FoamStepper(s, s.container, diffuse, 4, DT)
    done = f.advance_to(15 * DT)
    assert done == s.steps and [k for k, _ in steps] == list(range(4, done + 1, 4))
    fresh = FakeSolver()
    dts, _ = M.advance(*PARAMS, D, fresh._v2, 0.0, 15 * DT)
    for q, (_, dt) in enumerate(steps):   # every diffuse step: the sum of the four step sizes behind it, not 4 * timeStepSize
        assert dt == pytest.approx(sum(dts[4 * q:4 * q + 4]), rel=1e-12) and dt != pytest.approx(4 * DT, rel=1e-3)
    assert f.advance_to(15 * DT, max_steps=3) == 0
