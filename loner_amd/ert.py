"""Early ray termination's host side: the fitted cost model, the planner that picks a step's phases from the
termination counts, and the policy of when a new plan replaces the one in use (``ErtPlanner``).  No torch, no
HIP library: the step driver (loner_amd.step) feeds it counts and asks it for the coming step's phases."""
import itertools
import os

import numpy as np

# The cost model (us; csrc/field.hip, lnr_hashgrid_fwd_rays_phase + lnr_field_sigma_phase),
# fitted to round 6's kernel traces of the trained C2 step: the encode + sigma of one
# ray-sample ERT_SAMPLE_NS, phased or not; going phased ERT_FIXED_US; every phase after the first ERT_PHASE_US (its
# encode, sigma and list launches, latency-bound when few rays are left)
ERT_SAMPLE_NS, ERT_FIXED_US, ERT_PHASE_US = 0.150, 5.0, 28.0
# The march (lnr_field_ert_march): a plan's trailing run of two or more 64-sample phases runs as one launch, a
# workgroup per ray still alive marching 64 samples at a time.  Its cost: ERT_MARCH_FIXED_US for the launch plus
# ERT_MARCH_SAMPLE_NS per ray-sample marched, each unit over the rays alive at its start; fitted to the traced C2
# marches from samples 256 (0.48 M ray-samples, 161 us) and 192 (0.89 M, 274 us).  At
# nearly twice the phases' rate per sample (all 16 levels' gathers share an XCD's L2) a march pays for a short
# tail only: on the trained C2 field the planner takes [0, 320, 384, 448, 512], and the bench step went from
# 0.913 to 0.892 ms (medians of four interleaved runs each, every run faster).  LONER_ERT_MARCH=0 turns it off: a
# trailing run of 64-sample phases then goes phase by phase, and ert_plan proposes no march plan.
ERT_MARCH_SAMPLE_NS, ERT_MARCH_FIXED_US = 0.278, 27.0
ERT_MARCH = os.environ.get("LONER_ERT_MARCH", "1") != "0"
ERT_MAX_CUTS = 4
ERT_MARGIN = 0.02  # eager steps: a plan replaces the current one only when modelled this much faster (of the full
# encode); under graph replay a new plan waits for the window's captures and takes no margin (ErtPlanner.observe)


def ert_alive(hist, S):
    """From a termination histogram (lnr_loss_params.dev_term_hist: bin c // 64 per ray, c its samples before the
    transmittance product drops below LNR_ERT_T_MIN): the share of rays still alive after sample 64 k, k = 0..S/64."""
    h = np.asarray(hist, dtype=np.float64)
    tot = h.sum()
    if tot <= 0:
        return np.ones(S // 64 + 1)
    tail = np.cumsum(h[::-1])[::-1]  # rays with bin >= k
    return tail / tot


def ert_march_start(bounds):
    """The index i >= 1 into ``bounds`` ([0, c1, .., S] or None) at which the plan's trailing run of 64-sample
    phases starts, when that run has two or more phases (the march takes bounds[i:]; the first phase, every ray,
    stays on the dense encode), or None."""
    if bounds is None:
        return None
    i = len(bounds) - 1
    while i > 1 and bounds[i] - bounds[i - 1] == 64:
        i -= 1
    return i if len(bounds) - 1 - i >= 2 else None


def ert_cost_us(bounds, alive, S, n_samples, march=None):
    """Modelled encode + sigma time of one step (n_samples ray-samples) with the phases ``bounds``
    ([0, c1, .., S]) or, for None, without early ray termination.  ``march`` (default: ERT_MARCH): a trailing run
    of 64-sample phases (ert_march_start) is priced as the one march launch that executes it."""
    full = ERT_SAMPLE_NS * 1e-3 * n_samples
    if bounds is None:
        return full
    i0 = ert_march_start(bounds) if (ERT_MARCH if march is None else march) else None
    n_ph = len(bounds) - 1 if i0 is None else i0  # the phases run as launches of their own
    t = ERT_FIXED_US + ERT_PHASE_US * (n_ph - 1)
    for lo, hi in zip(bounds[:n_ph], bounds[1:n_ph + 1]):
        t += full * float(alive[lo // 64]) * (hi - lo) / S
    if i0 is not None:
        t += ERT_MARCH_FIXED_US
        for lo in bounds[i0:-1]:
            t += ERT_MARCH_SAMPLE_NS * 1e-3 * n_samples * float(alive[lo // 64]) * 64 / S
    return t


def ert_plan(hist, S, n_samples, current=None, max_cuts=ERT_MAX_CUTS, margin=ERT_MARGIN, march=None):
    """The early-ray-termination phases for the coming steps from the last steps' termination histogram: the
    cheapest under ert_cost_us among no termination, every set of at most ``max_cuts`` cuts at multiples of
    64 samples and (``march``, default ERT_MARCH) every march plan [0, c1, c1 + 64, .., S], kept only if it beats
    ``current`` (the plan in use: bounds or None) by ``margin`` of the full encode (so the graphs, captured per
    plan, are not re-captured for noise).  Returns bounds or None."""
    if S % 64 or S < 128:
        return None
    march = ERT_MARCH if march is None else march
    alive = ert_alive(hist, S)
    full = ert_cost_us(None, alive, S, n_samples, march)
    pos = list(range(64, S, 64))
    best, best_t = None, full
    cands = [[0, *cuts, S] for k in range(1, min(max_cuts, len(pos)) + 1) for cuts in itertools.combinations(pos, k)]
    if march:
        cands += [[0, *range(c1, S + 1, 64)] for c1 in pos[:-1]]
    for b in cands:
        t = ert_cost_us(b, alive, S, n_samples, march)
        if t < best_t:
            best, best_t = b, t
    cur_t = ert_cost_us(current, alive, S, n_samples, march)
    return best if best_t < cur_t - margin * full else current


class ErtPlanner:
    """Which phases the coming step runs, and when that changes.  ``mode``: False (never), True (always, at the
    fixed ``cuts``: fractions of the ``S`` samples per ray, rounded to whole 64-sample waves) or "auto" (``observe``
    plans from the termination counts).  ``march``: whether a plan's trailing run of 64-sample phases runs as one
    march launch.  ``supported``: whether the step's kernels can run phases at this S at all."""

    def __init__(self, S, supported, mode="auto", cuts=(0.5, 0.625, 0.75), march=ERT_MARCH):
        self.S, self.supported = S, bool(supported) and S % 64 == 0
        self.mode, self.cuts, self.march = mode, list(cuts), march
        self.plan = None  # auto: the phases in use, [0, c1, .., S], or None
        self.shares = None  # auto: the plan's alive shares after each 64-sample boundary (the encode's grid hints)
        self.next = None  # auto: (plan, alive shares) waiting for the next window (graph replay)
        self.prev = [0] * (S // 64 + 1)  # the counter totals of the last observation
        self.last = None  # the phases of the last step (tests, tools)
        self.marched = None  # where the last step's march started (an index into its phases), or None

    def bounds(self):
        """The phases [0, b1, ..., S] (whole 64-sample waves) of the coming step, or None: termination off (mode
        False, or auto with no plan that pays), or not applicable (n_samples not a multiple of 64 in {64 .. 512},
        or fewer than two phases)."""
        S = self.S
        if not self.supported or self.mode is False:
            return None
        if self.mode == "auto":
            return None if self.plan is None else list(self.plan)
        b = sorted({int(round(f * S / 64)) * 64 for f in self.cuts if 0.0 < f < 1.0} - {0, S})
        return [0] + b + [S] if b else None

    def key(self):
        """What a captured graph of the step depends on: the phases and how their tail runs."""
        b = self.bounds()
        return None if b is None else (tuple(b), bool(self.march))

    def begin_step(self):
        """The phases of the step being enqueued and where its march starts; kept as ``last`` and ``marched``."""
        self.last = self.bounds()
        self.marched = ert_march_start(self.last) if self.march else None
        return self.last, self.marched

    def observe(self, counts, n_samples, defer=False):
        """Re-plan (auto) from the termination counters' running totals ``counts`` (one per 64-sample bin, the
        slots summed; they wrap at 2^32), i.e. from what the steps since the last observation added, for steps of
        ``n_samples`` ray-samples.  ``defer``: graphs of this window are replaying.  Such a window keeps its plan:
        a new one would cost an eager step and a capture mid-window (~2 ms), so it waits for ``adopt()`` at the next
        window's captures, which are made anyway (no margin for those: the cheapest plan of the latest counts).
        The first plan is taken at once."""
        cur = [int(v) & 0xFFFFFFFF for v in counts]
        d = [(c - p) & 0xFFFFFFFF for c, p in zip(cur, self.prev)]
        self.prev = cur
        if self.mode != "auto" or sum(d) <= 0:
            return
        defer = defer and self.shares is not None
        plan = ert_plan(d, self.S, n_samples, self.plan, margin=0.0 if defer else ERT_MARGIN, march=self.march)
        if plan == self.plan and self.shares is not None:
            self.next = None  # the latest counts confirm the plan in use
            return
        # the alive shares are refreshed with the plan only (the graphs, captured per plan, hold the hints of
        # their capture)
        nxt = (plan, [float(v) for v in ert_alive(d, self.S)])
        if defer:
            self.next = nxt
        else:
            (self.plan, self.shares), self.next = nxt, None

    def adopt(self):
        """A window boundary: the plan ``observe`` deferred while graphs replayed takes effect."""
        if self.next is not None:
            (self.plan, self.shares), self.next = self.next, None
