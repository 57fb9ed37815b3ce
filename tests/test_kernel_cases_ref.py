"""CPU checks of the references that the direct kernel tests compare against (tests/kernel_cases.py): the
conditions that make a comparison at rounding level meaningful are asserted here on the reference alone, so
they hold whatever the kernels compute."""
import numpy as np
import pytest
import torch

import kernel_cases as C
from loner_amd import pose as P

POSE_BIG = dict(S=5, n_lidar=[3276, 3275, 3275, 3275, 3275], n_sky=9)  # 16384 + 37 rays


# ----------------------------------------------------------------------------- pose chain
@pytest.mark.parametrize("far_m", C.POSE_FAR_M)
@pytest.mark.parametrize("big", [False, True])
def test_pose_case_branches_are_decided(far_m, big):
    """The kernel decides `clip < far_range` and the winning axis on fp32 values, the reference on fp64 ones: no
    pose-following ray of the random cases has its clip within 1e-5 (relative) of the range, nor its two best
    axes within 1e-5 of each other (fp32 evaluates a clip to a few 2^-24).  At both far ranges the clip
    wins on some rays and the range on others."""
    c = C.pose_case(far_m, **POSE_BIG) if big else C.pose_case(far_m, 5)
    m_range, m_axis, clipped = C.pose_branch_margins(c)
    assert m_range.min() > 1e-5 and m_axis.min() > 1e-5, (m_range.min(), m_axis.min())
    assert 0.05 < clipped.mean() < 0.95, clipped.mean()
    assert c["rays"].shape[0] == (16384 + 37 if big else 5 * 46)


def test_pose_case_reference_is_the_autograd_chain():
    """The reference of the kernel tests (ray_gradients + keyframe_gradients, float64, on fp32-rounded inputs) has
    exact zeros for the anchored keyframe, non-zero gradients elsewhere, and its magnitude chain dominates it."""
    for S in C.POSE_S:
        c = C.pose_case(14.0, S)
        ref, mag = C.pose_reference(c), C.pose_magnitude(c)
        assert np.all(ref[0] == 0) and np.all(mag[0] == 0)
        assert np.all(np.abs(ref[1:]) > 0) and np.all(np.abs(ref) <= mag * (1 + 1e-12))
    # the small-angle keyframes: autograd's derivative at |w| = 0 and 1e-8 is the first-order form to 1e-7
    aa = c["p6"][1:3, 3:].double().requires_grad_()
    Rm = P.axis_angle_to_matrix(aa)
    for i, (a, b) in enumerate([(2, 1), (0, 2), (1, 0)]):  # the +1 entry of [e_i]x
        g, = torch.autograd.grad(Rm[:, a, b].sum(), aa, retain_graph=True)
        np.testing.assert_allclose(g[:, i].numpy(), 1.0, atol=1e-7)


def test_pose_rounding_counts():
    assert C.pose_rounding_counts(1) == (9, 17) and C.pose_rounding_counts(64) == (9, 17)
    assert C.pose_rounding_counts(100) == (10, 18) and C.pose_rounding_counts(128) == (10, 18)


def test_far_branch_reference():
    """The far-term branch rays: what torch's autograd does at each tie, in float32 on the CPU (the reference of
    test_gpu_pose_kernels.test_far_term_branches).  d far / d o_axis = -1 / d_axis, d far / d d_axis = -t / d_axis
    on the axis and plane that win; everything is dyadic, so the values are exact."""
    c = C.far_branch_case()
    names = [r[0] for r in C.FAR_BRANCH_RAYS]
    zero = dict(c, d_pos=torch.zeros_like(c["d_pos"]), d_ray=torch.tensor([[0.0, -1.25]]).repeat(len(names), 1))

    def far_part(fr):
        g_o, g_d = P.ray_gradients(zero["rays"], zero["z"], zero["d_pos"], zero["d_ray"], fr)
        return dict(zip(names, torch.cat([g_o, g_d], 1).tolist()))

    g = far_part(8.0)
    assert g["plus_plane"] == [1.25 / 0.5, 0, 0, 1.25 * 1.5 / 0.5, 0, 0]
    assert g["minus_plane"] == [1.25 / -0.5, 0, 0, 1.25 * 2.5 / -0.5, 0, 0]
    assert g["unit_clip"] == [1.25, 0, 0, 1.25, 0, 0]
    assert g["zero_component"] == [1.25 / 0.5, 0, 0, 1.25 * 2.0 / 0.5, 0, 0]
    assert g["axis_tie"] == [1.25 / 0.5, 0, 0, 1.25 * 2.0 / 0.5, 0, 0]  # the first of the tying axes
    assert g["on_face_outward"] == [0.0] * 6 and g["outside_outward"] == [0.0] * 6
    assert g["outside_inward"] == [0, 1.25 / 0.25, 0, 0, 1.25 * 4.0 / 0.25, 0]
    # range 1 ties with unit_clip's clip (torch.minimum splits evenly); range 0.5 lies below it
    assert far_part(1.0)["unit_clip"] == [0.625, 0, 0, 0.625, 0, 0]
    assert far_part(0.5)["unit_clip"] == [0.0] * 6
    assert far_part(1.0)["plus_plane"] == [0.0] * 6  # clip 1.5 above the range
    # in float64 the axis tie is no tie (d + 1e-15 differs): why the branch test's reference is float32
    r64 = C.far_branch_rows(c, 8.0, torch.float64)
    r32 = C.far_branch_rows(c, 8.0, torch.float32)
    assert np.allclose(r64.numpy(), r32.numpy(), rtol=1e-6, atol=1e-6)
    assert torch.isfinite(r32).all()


# ----------------------------------------------------------------------------- sampler
def test_sampler_cases_cover_every_launch_shape():
    """lnr_sample_ogm's choice of kernel (csrc/sampler.hip), restated: every kernel form is among the shapes."""
    for S, want in C.SAMPLER_KERNEL.items():
        H, p2 = S // 2, 1 << (S - 1).bit_length()
        if H % 64 == 0 and 128 <= p2 <= 2048:
            kind = "rank" if (p2 // 64 >= 4 and 2 * H == p2) else ("wave" if 2 * H == p2 else "wave_padded")
        else:
            kind = "block"
        assert kind == want, (S, kind)
    assert set(C.SAMPLER_KERNEL) == set(C.SAMPLER_S)


@pytest.mark.parametrize("name", C.SAMPLER_CASES)
def test_sampler_reference_is_stable(name):
    """The bar of tests/test_gpu_sampler_shapes.py excludes no sample, so the reference itself must not sit on an
    edge: with every cdf entry moved one fp32 ulp at random (twice, two seeds) no depth of the oracle moves by
    4e-6 or more (measured: at most 2.2e-6, the in-kernel draws at S = 192; 8.2e-7 with injected draws, which
    kernel_cases.stable_draws keeps off the edges) -- no draw lands where a bin's denom crosses eps or where the
    searched bin changes to a far one.  Without the move the restatement is the oracle bit for bit."""
    c = C.sampler_case(name)
    ref = C.sampler_reference(c)
    np.testing.assert_array_equal(C.sampler_reference(c, cdf_ulps=False), ref)
    assert np.all(np.isfinite(ref)) and np.all(np.diff(ref, axis=1) >= 0)
    worst = 0.0
    for seed in (1, 2):
        moved = C.sampler_reference(c, cdf_ulps=np.random.default_rng(seed))
        worst = max(worst, float(np.abs(moved.astype(np.float64) - ref).max()))
    print(f"{name}: cdf moved by an ulp moves a depth by at most {worst:.2e}")
    assert worst < C.SAMPLER_REF_STABILITY, worst


# ----------------------------------------------------------------------------- preprocessing
@pytest.mark.parametrize("case", ["full", "partial"])
def test_sky_scan_reference(case):
    """The sky-ray scans of tests/test_gpu_preprocess.py, on the oracle alone: fp32 bin-centre directions bin where
    they were put; no candidate direction lies within 1e-3 degrees of the horizon threshold (the filter is decided
    the same way in fp32); the closing fills the small holes and keeps the 3 x 3 ones; holes at every border, the
    forced top rows and (full case) the theta = 180 wrap all show in the result."""
    from oracle import preprocess as opre
    dirs, holes = C.sky_scan(case)
    x, y, z = dirs.astype(np.float64)
    th = np.rad2deg(np.arctan2(y, x))
    ph = np.rad2deg(np.arctan2(np.sqrt(x ** 2 + y ** 2), z))
    assert np.abs(th - np.rint(th)).max() < 1e-4 and np.abs(ph - np.rint(ph)).max() < 1e-4
    tmin, pmin = int(np.rint(th).min()), int(np.rint(ph).min())
    assert pmin > 0 and (tmin == -180 and np.rint(th).max() == 180 if case == "full" else tmin > -180)
    rot = C.SKY_POSE[:3, :3]
    # every candidate (the empty bins after the closing, before the elevation filter): none near the threshold
    dw = opre.sky_rays(dirs, rot, horizon_deg=-1e9)
    elev = 90 - np.rad2deg(np.arctan2(np.sqrt(dw[0] ** 2 + dw[1] ** 2), dw[2]))
    assert np.abs(elev - 10.0).min() > 1e-3 and (elev < 10).any() and (elev > 10).any()
    ref = opre.sky_rays(dirs, rot)
    # the result's bins, recovered by rotating back
    back = rot.T @ ref
    col = np.rint(np.rad2deg(np.arctan2(back[1], back[0]))).astype(int) - tmin
    row = np.rint(np.rad2deg(np.arctan2(np.sqrt(back[0] ** 2 + back[1] ** 2), back[2]))).astype(int) - pmin
    got = set(zip(row.tolist(), col.tolist()))

    def inside(name):
        r0, r1, c0, c1 = holes[name]
        return {(r, c) for r in range(r0, r1 + 1) for c in range(c0, c1 + 1)} & got

    assert not inside("single_a") and not inside("single_b") and not inside("pair")
    assert len(inside("three")) == 9 and len(inside("three_by_four")) == 12
    assert len(inside("right")) == 9 and {r for r, _ in inside("top")} == {3, 4}
    assert any(inside(k) for k in holes if k.startswith("bottom"))       # part of the lowest rows is above 10 deg
    assert not all(len(inside(k)) == 9 for k in holes if k.startswith("bottom"))  # and part is filtered
    # the left hole: with the wrap, theta = 180 occupies (24, 0) and the closing keeps that corner filled; without,
    # 25 bins
    assert len(inside("left")) == (24 if case == "full" else 25), len(inside("left"))
    assert ref.shape[1] > 60


def test_motion_compensate_vec_is_the_oracle():
    """The vectorised float64 restatement equals oracle.preprocess.motion_compensate (the per-point loop) on every
    13th point of each case; the cases reach s < 0 and s > 1, the identity flag and a rotation near pi."""
    from oracle import preprocess as opre
    from scipy.spatial.transform import Rotation
    for name in C.MOTION_CASES:
        c = C.motion_case(name)
        idx = np.arange(0, 1000, 13)
        args = (c["start"], c["end"], c["t"][0], c["t"][1], c["target"])
        d0, r0 = opre.motion_compensate(c["dirs"][:, idx], c["dists"][idx], c["ts"][idx], *args)
        d1, r1 = C.motion_compensate_vec(c["dirs"], c["dists"], c["ts"], *args)
        np.testing.assert_allclose(d1[:, idx], d0, atol=1e-12)
        np.testing.assert_allclose(r1[idx], r0, rtol=1e-12)
        s = (c["ts"] - c["t"][0]) / (c["t"][1] - c["t"][0])
        assert s.min() < -0.1 and s.max() > 1.1
        ang = np.linalg.norm(Rotation.from_matrix(c["start"][:3, :3].T @ c["end"][:3, :3]).as_rotvec())
        want = {"general": 0.01 < ang < 1, "identity_rotation": ang < 1e-9, "near_pi": abs(ang - (np.pi - 1e-3)) < 1e-9}
        assert want[name], (name, ang)


def test_sampler_tie_case_reference():
    """kernel_cases.sampler_tie_case on the oracle alone: the first bin's mass is below eps, the first draw equals
    cdf[1] exactly and maps to the second bin's start, the draw one ulp lower to the first bin's; the two differ by
    a bin width, so the side of the search shows in the depths."""
    from oracle import render as orender
    c, bins, cdf = C.sampler_tie_case()
    assert np.all(cdf[:, 0] == 0) and np.all(cdf[:, 1] > 0) and np.all(cdf[:, 1] < 1e-5) and np.all(cdf[:, 2] > 0.99)
    assert np.all(c["u_pdf"][:, 0] == cdf[:, 1]) and np.all(c["u_pdf"][:, 1] < cdf[:, 1])
    zi = orender.sample_pdf(bins, np.tile(np.float32([0.0, 1.0]), (8, 1)), 4, c["u_pdf"])
    np.testing.assert_array_equal(zi[:, 0], bins[:, 1])
    np.testing.assert_allclose(zi[:, 1], bins[:, 0], atol=1e-5)
    assert np.all(bins[:, 1] - bins[:, 0] > 0.25)
    ref = C.sampler_reference(c)
    assert np.all(np.diff(ref, axis=1) >= 0) and np.all((ref == bins[:, 1:2]).sum(1) == 1)
