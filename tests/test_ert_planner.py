"""Early ray termination's plan policy (loner_amd.ert.ErtPlanner, host only): when a new plan replaces the one in
use.  Counts are plain lists of running counter totals, one per 64-sample bin of S = 256 samples (+ the rays that
never terminate); the expected plans are ert_plan's own on the same histogram."""
import loner_amd.ert as E_

S, R = 256, 8192
N = R * S
EARLY = [0, 0, 6000, 1500, 692]  # most rays terminate between samples 128 and 192: cutting pays
LATE = [0, 0, 0, 500, 7692]  # hardly a ray terminates: termination does not pay
EARLIER = [0, 7000, 500, 500, 192]  # most rays terminate before sample 128: another cut


def _add(total, hist):
    return [t + h for t, h in zip(total, hist)]


def test_histograms_give_distinct_plans():
    a, b = E_.ert_plan(EARLY, S, N), E_.ert_plan(EARLIER, S, N, current=E_.ert_plan(EARLY, S, N), margin=0.0)
    assert a is not None and b is not None and a != b
    assert E_.ert_plan(LATE, S, N) is None


def test_no_counts_no_bounds_and_first_plan_at_once():
    p = E_.ErtPlanner(S, True)
    assert p.mode == "auto" and p.bounds() is None and p.key() is None
    p.observe([0] * 5, N, defer=True)  # no ray counted yet: nothing to plan from
    assert p.bounds() is None and p.shares is None
    p.observe(EARLY, N, defer=True)  # the first plan does not wait for a window boundary
    assert p.bounds() == E_.ert_plan(EARLY, S, N) and p.next is None
    assert p.shares == [float(v) for v in E_.ert_alive(EARLY, S)]
    assert p.key() == (tuple(p.bounds()), bool(p.march))


def test_deferred_plan_waits_for_adopt():
    p = E_.ErtPlanner(S, True)
    p.observe(EARLY, N, defer=True)
    first = p.bounds()
    tot = _add(EARLY, EARLIER)
    p.observe(tot, N, defer=True)
    want = E_.ert_plan(EARLIER, S, N, current=first, margin=0.0)
    assert want != first
    assert p.bounds() == first and p.next[0] == want  # unchanged until the window boundary
    assert p.next[1] == [float(v) for v in E_.ert_alive(EARLIER, S)]
    p.adopt()
    assert p.bounds() == want and p.next is None and p.shares == [float(v) for v in E_.ert_alive(EARLIER, S)]
    p.adopt()  # nothing deferred: a no-op
    assert p.bounds() == want


def test_confirming_counts_drop_the_deferred_plan():
    p = E_.ErtPlanner(S, True)
    p.observe(EARLY, N, defer=True)
    first = p.bounds()
    tot = _add(EARLY, EARLIER)
    p.observe(tot, N, defer=True)
    assert p.next is not None
    p.observe(_add(tot, EARLY), N, defer=True)  # the latest counts confirm the plan in use
    assert E_.ert_plan(EARLY, S, N, current=first, margin=0.0) == first
    assert p.next is None and p.bounds() == first
    p.adopt()
    assert p.bounds() == first


def test_eager_steps_change_plan_at_once():
    p = E_.ErtPlanner(S, True)
    p.observe(EARLY, N)
    first = p.bounds()
    p.observe(_add(EARLY, EARLIER), N)
    want = E_.ert_plan(EARLIER, S, N, current=first)  # (with ERT_MARGIN)
    assert want != first and p.bounds() == want and p.next is None


def test_counter_wrap_gives_the_same_deltas():
    base = [(1 << 32) - 100] * 5  # totals about to wrap
    p, q = E_.ErtPlanner(S, True), E_.ErtPlanner(S, True)
    p.prev = list(base)  # (as after an observation of these totals)
    p.observe([(b + h) & 0xFFFFFFFF for b, h in zip(base, EARLY)], N)  # wrapped past 2^32
    q.observe(EARLY, N)
    assert p.bounds() == q.bounds() == E_.ert_plan(EARLY, S, N) and p.shares == q.shares
    p.observe([b + h for b, h in zip(_add(base, EARLY), EARLIER)], N)  # (unmasked totals wrap the same way)
    q.observe(_add(EARLY, EARLIER), N)
    assert p.bounds() == q.bounds() and p.shares == q.shares


def test_fixed_mode_and_off():
    p = E_.ErtPlanner(S, True, mode=True, cuts=[0.5, 0.75], march=True)
    assert p.bounds() == [0, 128, 192, 256]
    assert p.begin_step() == ([0, 128, 192, 256], 1) and p.last == [0, 128, 192, 256] and p.marched == 1
    p.march = False
    assert p.begin_step() == ([0, 128, 192, 256], None) and p.key() == ((0, 128, 192, 256), False)
    p.observe(EARLIER, N)  # fixed cuts ignore the counts
    assert p.bounds() == [0, 128, 192, 256]
    off = E_.ErtPlanner(S, True, mode=False, cuts=[0.5, 0.75])
    assert off.bounds() is None and off.key() is None and off.begin_step() == (None, None)
    assert E_.ErtPlanner(S, False, mode=True, cuts=[0.5, 0.75]).bounds() is None  # the kernels cannot run phases
    assert E_.ErtPlanner(96, True, mode=True, cuts=[0.5]).bounds() is None  # not whole 64-sample waves
