"""The host side of registration on the cell grid (CPU only, no kernel launches): lnr_icp_grid_rings against its rule in
Python, the Python cell rule, and the argument checks of the ``search`` / ``align_search`` options."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from loner_amd import _lib
    _lib.lib()
    return _lib


def _rule(threshold, cell, max_rings=4):
    """lnr_icp_grid_rings' rule (include/loner_amd.h), written out here on its own: the smallest R >= 1 with
    (R cell)^2 (1 - 2^-20) >= thr2, thr2 the float32 square of the float32 threshold; 0 above ``max_rings``."""
    t = float(np.float32(threshold))
    thr2 = float(np.float32(t * t))
    for r in range(1, max_rings + 1):
        if (r * cell) * (r * cell) * (1.0 - 2.0 ** -20) >= thr2:
            return r
    return 0


@pytest.mark.parametrize("threshold", (1.5, 0.125))
def test_rings_follow_the_rule(L, threshold):
    from loner_amd import tracking as TR
    assert L.NN_MAX_RINGS == 4
    rings = L.lib().lnr_icp_grid_rings
    cells = sorted(set(np.geomspace(threshold / 4, 50.0, 400).tolist() +
                       [threshold / r * f for r in (1, 2, 3, 4) for f in (1 - 1e-6, 1.0, 1 + 1e-6, 1 + 2.0 ** -10)]))
    seen = set()
    for cell in cells:
        want = _rule(threshold, cell)
        assert rings(threshold, cell) == want == TR.icp_grid_rings_ref(threshold, cell), cell
        seen.add(want)
    assert seen == {0, 1, 2, 3, 4}  # threshold / 4 itself needs a fifth ring: (1 - 2^-20) thr2 < thr2
    assert rings(threshold, threshold / 4) == 0 and rings(threshold, 50.0) == 1


@pytest.mark.parametrize("threshold", (1.5, 0.125))
def test_rings_at_the_edge_of_the_smallest_cell(L, threshold):
    """The cell of the Python rule, threshold (1 + 2^-10) / 4, walks four rings, and so does the cell one ulp below it:
    (4 cell)^2 is then still thr2 (1 + 2^-9), far above thr2 / (1 - 2^-20): the 2^-10 of the Python rule is a margin,
    not the edge, so that cell needs four rings and not five, and the rule is what the function follows.  The edge
    where a fifth ring is needed, and the function returns 0, lies near threshold (1 + 2^-21) / 4: found here by
    bisection on the rule, and checked one ulp to either side."""
    rings = L.lib().lnr_icp_grid_rings
    floor = threshold * (1 + 2.0 ** -10) / 4
    below = float(np.nextafter(floor, 0.0))
    assert rings(threshold, floor) == _rule(threshold, floor) == 4
    assert rings(threshold, below) == _rule(threshold, below) == 4
    lo, hi = threshold / 4, floor  # rule(lo) == 0, rule(hi) == 4
    assert _rule(threshold, lo) == 0
    while float(np.nextafter(lo, np.inf)) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if _rule(threshold, mid) else (mid, hi)
    assert rings(threshold, hi) == 4 and rings(threshold, lo) == 0
    assert abs(hi / (threshold / 4) - 1) < 2.0 ** -20


def test_rings_refuse_bad_arguments(L):
    from loner_amd import tracking as TR
    rings = L.lib().lnr_icp_grid_rings
    inf, nan = float("inf"), float("nan")
    for threshold, cell in ((0.0, 1.0), (-1.5, 1.0), (nan, 1.0), (inf, 1.0), (1.5, 0.0), (1.5, -1.0), (1.5, nan),
                            (1.5, inf), (1.5, 1e-13), (3e38, 1e300)):  # the last: thr2 overflows to inf
        assert rings(threshold, cell) == 0, (threshold, cell)
        assert TR.icp_grid_rings_ref(threshold, cell) == 0, (threshold, cell)
    assert L.lib().lnr_icp_grid_workspace_bytes(0) == 0
    assert L.lib().lnr_icp_grid_workspace_bytes(L.ICP_MAX_POINTS + 1) == 0
    for n in (1, 16, 17, 100000):
        assert L.lib().lnr_icp_grid_workspace_bytes(n) == L.lib().lnr_icp_workspace_bytes(n) == -(-n // 16) * 256


def test_python_cell_rule_never_needs_too_many_rings(L):
    from loner_amd import tracking as TR
    rng = np.random.default_rng(3)
    for threshold in (1.5, 0.125, 1e-3, 0.3333333, 17.0, 1e4):
        for n in (1, 30, 1517, 1 << 17, 10 ** 6):
            for extent in (0.0, 1e-3, 1.0, 80.0, 5e3):
                lo = rng.normal(size=3) * 10
                hi = lo + extent * rng.uniform(0.2, 1.0, size=3)
                for factor in TR.ICP_CELL_FACTORS + (None, 1e-9):
                    cell = TR.icp_grid_cell(threshold, lo, hi, n, factor)
                    r = L.lib().lnr_icp_grid_rings(threshold, cell)
                    assert 1 <= r <= L.NN_MAX_RINGS, (threshold, n, extent, factor, cell)
    # the floor is what a tiny factor leaves
    assert TR.icp_grid_cell(1.5, (0, 0, 0), (1, 1, 1), 10 ** 6, 1e-9) == 1.5 * (1 + 2.0 ** -10) / 4
    assert TR.ICP_CELL_FACTOR in TR.ICP_CELL_FACTORS


def test_search_arguments_are_checked():
    from loner_amd import map_eval as ME
    from loner_amd import tracking as TR
    assert TR.TrackerSettings().search == "brute"
    assert TR.TrackerSettings(search="grid", downsample_type=None).search == "grid"
    with pytest.raises(ValueError, match="kdtree"):
        TR.TrackerSettings(search="kdtree")
    with pytest.raises(ValueError, match="kdtree"):
        TR.check_search("kdtree")
    with pytest.raises(NotImplementedError):
        TR.TrackerSettings(downsample_type="VOXEL", search="grid")
    assert ME.ALIGN_MAX_POINTS == 1 << 17 and ME.ALIGN_MAX_POINTS_GRID == 1_000_000
    rng = np.random.default_rng(1)
    est = rng.uniform(0, 1, size=(200, 3)).astype(np.float32)
    for fn in (ME.compare_point_clouds_ref, ME.compare_point_clouds, ME.align_clouds):
        kw = "search" if fn is ME.align_clouds else "align_search"
        with pytest.raises(ValueError, match="kdtree"):
            fn(est, est, **{kw: "kdtree"})
        with pytest.raises(ValueError, match="1000001"):
            fn(est, est, align_max_points=1_000_001, **{kw: "grid"})
        with pytest.raises(ValueError, match="2\\^17"):
            fn(est, est, align_max_points=(1 << 17) + 1, **{kw: "brute"})
        with pytest.raises(ValueError, match="2\\^17"):
            fn(est, est, align_max_points=(1 << 17) + 1)
        with pytest.raises(ValueError):
            fn(est, est, align_max_points=0, **{kw: "grid"})
    ME._check_align_cap((1 << 17) + 1, "grid")
    ME._check_align_cap(1_000_000, "grid")
    # past the cap check with "grid": the float64 comparison runs (no alignment, so no k-d tree of normals)
    stats = ME.compare_point_clouds_ref(est, est, align=False, align_max_points=(1 << 17) + 1, align_search="grid")
    assert stats["accuracy"] == 0.0 and stats["num_points"] > 0
