"""Early ray termination's planner with the march (loner_amd.step.ert_plan / ert_cost_us / ert_march_start, host
only): a plan's trailing run of two or more 64-sample phases is executed, and priced, as one march launch
(lnr_field_ert_march) when the march is on.  The constants are fitted to the traced C2 marches (DESIGN.md section
4.6): at 0.278 ns per ray-sample against the phases' 0.150 a march pays only for a short tail."""
import numpy as np

from loner_amd import step as S_

S, N = 512, 8192 * 512


def _hist(alive_at):
    """A histogram (bins of 64 samples + never) whose alive shares after samples 64 k are ``alive_at[k]``."""
    a = np.asarray(list(alive_at) + [0.0], dtype=np.float64)
    return np.round((a[:-1] - a[1:]) * 10000).astype(np.int64)


TRAINED_QUAD = [1, 1, 1, 0.9, 0.73, 0.34, 0.12, 0.05, 0.02]  # tests/test_ert_plan.py's trained C2 regime


def test_march_start():
    assert S_.ert_march_start([0, *range(128, S + 1, 64)]) == 1
    assert S_.ert_march_start([0, 256, 320, 384, 448, 512]) == 1
    assert S_.ert_march_start([0, 192, 320, 384, 448, 512]) == 2  # the run starts after the 128-wide phase
    assert S_.ert_march_start([0, *range(64, S + 1, 64)]) == 1  # the first phase, every ray, is never marched
    for b in ([0, 256, 512], [0, 256, 320, 384, 512], [0, 448, 512], [0, 192, 320, 384, 512], None):
        assert S_.ert_march_start(b) is None, b


def test_march_switch():
    """The march is on unless LONER_ERT_MARCH=0; switched off, no march plan is proposed and a trailing run of
    64-sample phases is priced phase by phase."""
    h = _hist(TRAINED_QUAD)
    alive = S_.ert_alive(h, S)
    assert S_.ert_plan(h, S, N) == S_.ert_plan(h, S, N, march=S_.ERT_MARCH)
    assert S_.ert_march_start(S_.ert_plan(h, S, N, march=False)) is None
    run = [0, 320, 384, 448, 512]
    assert S_.ert_cost_us(run, alive, S, N) == S_.ert_cost_us(run, alive, S, N, march=S_.ERT_MARCH)
    assert S_.ert_cost_us(run, alive, S, N, march=False) > S_.ert_cost_us(run, alive, S, N, march=True)
    phases = S_.ERT_FIXED_US + 3 * S_.ERT_PHASE_US + sum(
        S_.ERT_SAMPLE_NS * 1e-3 * N * alive[lo // 64] * (hi - lo) / S for lo, hi in zip(run[:-1], run[1:]))
    assert abs(S_.ert_cost_us(run, alive, S, N, march=False) - phases) < 1e-6


def test_trained_quad_plan_with_the_march():
    """With the march on, the fitted constants put the march from sample 320 just below the best phased plan
    (499.5 against 499.8 us modelled): the planner returns it, and its price agrees."""
    h = _hist(TRAINED_QUAD)
    alive = S_.ert_alive(h, S)
    phased = S_.ert_plan(h, S, N, march=False)
    t_phased = S_.ert_cost_us(phased, alive, S, N, march=False)
    b = S_.ert_plan(h, S, N, march=True)
    t = S_.ert_cost_us(b, alive, S, N, march=True)
    assert phased == [0, 320, 384, 512]
    assert b == [0, 320, 384, 448, 512] and S_.ert_march_start(b) == 1
    assert t < t_phased and t_phased - t < 0.01 * t_phased, (t, t_phased)
    # no plan, marched or not, is modelled cheaper than the one returned
    for c1 in range(64, S - 64, 64):
        assert S_.ert_cost_us([0, *range(c1, S + 1, 64)], alive, S, N, march=True) >= t
    # the model of the two traced marches (first phase + one compaction + march: 267 + 38 + 7 + 161 us from sample
    # 256, 207 + 31 + 8 + 274 us from 192, on the bench's alive shares)
    bench = S_.ert_alive(_hist([1, 1, .9939, .7759, .5598, .2806, .0794, .0023, 0]), S)
    assert abs(S_.ert_cost_us([0, *range(256, S + 1, 64)], bench, S, N, march=True) - 473) < 30
    assert abs(S_.ert_cost_us([0, *range(192, S + 1, 64)], bench, S, N, march=True) - 520) < 30


def test_no_termination_and_small_batches_plan_nothing():
    assert S_.ert_plan(_hist([1.0] * 8 + [0.97]), S, N, march=True) is None
    assert S_.ert_plan(_hist([1.0] * 8 + [0.97]), S, N, current=[0, 256, 320, 384, 448, 512], march=True) is None
    assert S_.ert_plan(_hist(TRAINED_QUAD), S, 64 * 512, march=True) is None
