"""Inputs and float64 references shared by the direct kernel tests (tests/test_gpu_pose_kernels.py,
tests/test_gpu_sampler_shapes.py, tests/test_gpu_preprocess.py) and by the CPU tests that pin the conditions those references must meet
(tests/test_kernel_cases_ref.py).  Nothing here touches the GPU."""
import os

import numpy as np
import torch

from loner_amd import pose as P
from loner_amd.rays import WorldCube, build_lidar_rays

U32 = 2.0 ** -24  # fp32 unit roundoff

# ----------------------------------------------------------------------------- pose chain (csrc/pose.hip)
POSE_SEED = 9  # chosen so that test_pose_case_branches_are_decided holds (tests/test_kernel_cases_ref.py)
POSE_SCALE = 20.0
POSE_SHIFT = (0.5, -0.3, 0.2)
POSE_FAR_M = (30.0, 14.0)
POSE_S = (1, 5, 64, 100, 128)


def pose_tensors(K=5):
    """(K, 6) fp32 pose tensors: keyframe 0 anchored, then the axis-angles of the issue's list: exactly 0,
    (1e-8, 0, -1e-8) (below axis_angle_to_matrix's 1e-6 switch), norm 2e-6 (just above), norm pi - 1e-3;
    further keyframes random."""
    rng = np.random.default_rng(POSE_SEED)
    p6 = np.zeros((K, 6))
    p6[:, :3] = rng.uniform(-12, 12, (K, 3))
    p6[:, 3:] = rng.normal(0, 0.8, (K, 3))
    if K >= 5:
        p6[1, 3:] = 0.0
        p6[2, 3:] = [1e-8, 0.0, -1e-8]
        a = np.array([2.0, -1.0, 2.0]) / 3.0
        p6[3, 3:] = 2e-6 * a
        b = np.array([0.6, 0.0, -0.8])
        p6[4, 3:] = (np.pi - 1e-3) * b
    return torch.from_numpy(p6.astype(np.float32))


def pose_case(far_m, S, n_lidar=37, n_sky=9, K=5, optimise=None):
    """One input of ``lnr_pose_grad`` as tests/test_pose_chain.py builds it: build_lidar_rays in float64 from the
    fp32 pose tensors, cast to fp32 (R, 13); sorted z; normal d_pos / d_ray; LiDAR rays of optimised keyframes
    flagged 1, sky rays and the anchored keyframe's 0.  ``n_lidar``: one count or one per keyframe.  Every
    array is what the kernel gets (fp32 / int); ``far_range`` is the fp32-rounded far range in cube units."""
    dt = torch.float64
    rng = np.random.default_rng(POSE_SEED + 100)
    p6 = pose_tensors(K)
    optimise = [False] + [True] * (K - 1) if optimise is None else optimise
    wc = WorldCube(torch.tensor(POSE_SCALE, dtype=dt), torch.tensor(POSE_SHIFT, dtype=dt))
    ray_range = (1.0, float(far_m))
    counts = [n_lidar] * K if np.isscalar(n_lidar) else list(n_lidar)
    rays, kf, flag = [], [], []
    for k in range(K):
        Rk = P.axis_angle_to_matrix(p6[k, 3:].double())
        M = torch.cat([torch.cat([Rk, p6[k, :3, None].double()], 1), torch.tensor([[0, 0, 0, 1]], dtype=dt)], 0)
        for cnt, f in ((counts[k], 1.0 if optimise[k] else 0.0), (n_sky, 0.0)):
            dirs = torch.from_numpy(rng.normal(0, 1, (3, cnt)))
            dirs = dirs / dirs.norm(dim=0, keepdim=True)
            r, _ = build_lidar_rays(dirs, torch.ones(cnt, dtype=dt), M, ray_range, wc, ignore_world_cube=True)
            rays.append(r)
            kf += [k] * cnt
            flag += [f] * cnt
    rays = torch.cat(rays).float().contiguous()
    n = rays.shape[0]
    rs = np.random.default_rng(POSE_SEED + 1000 + S)
    z = torch.sort(torch.from_numpy(rs.uniform(0.01, 1.2, (n, S)).astype(np.float32)), 1)[0].contiguous()
    d_pos = torch.from_numpy(rs.normal(0, 1, (n * S, 3)).astype(np.float32))
    d_ray = torch.from_numpy(rs.normal(0, 1, (n, 2)).astype(np.float32))
    return dict(rays=rays, z=z, d_pos=d_pos, d_ray=d_ray, kf=torch.tensor(kf, dtype=torch.int32),
                flag=torch.tensor(flag, dtype=torch.float32), p6=p6, K=K, S=S, scale=POSE_SCALE,
                far_range=float(np.float32(far_m / POSE_SCALE)))


def pose_reference(c):
    """dL/d(pose tensors) (K, 6) of a ``pose_case`` by loner_amd.pose's torch chain in float64 on the fp32 inputs."""
    d = lambda t: t.double()  # noqa: E731
    g_o, g_d = P.ray_gradients(d(c["rays"]), d(c["z"]), d(c["d_pos"]), d(c["d_ray"]), c["far_range"])
    return P.keyframe_gradients(d(c["rays"]), g_o, g_d, c["kf"], d(c["flag"]), d(c["p6"]), c["scale"], c["K"]).numpy()


def pose_far_terms(c):
    """Per ray, in float64: the far term's dL/do and dL/dd alone (d_pos = 0, dL/d|d| = 0)."""
    rays = c["rays"].double()
    n = rays.shape[0]
    zero = torch.zeros(n, 1, dtype=torch.float64)
    g_o, g_d = P.ray_gradients(rays, zero, torch.zeros(n, 3, dtype=torch.float64),
                               torch.cat([zero, c["d_ray"][:, 1:2].double()], 1), c["far_range"])
    return g_o, g_d


def pose_magnitude(c):
    """The chain of ``pose_reference`` on absolute values, (K, 6): what a relative rounding of each intermediate
    can at most move the result by, per unit of relative error.  Per ray |g_o| <= sum|dpos| / 2 + |far term|,
    |g_d| <= sum z |dpos| / 2 + |dL/d|d|| |d| / |d| + |far term|; the projection's two terms add:
    |g_d| + |d| (|d| . |g_d|); the per-keyframe sums of |g_perp| |d|^T, times |R|, contracted with |dR/dw|."""
    rays, z, S = c["rays"].double(), c["z"].double(), c["S"]
    n = rays.shape[0]
    dp = c["d_pos"].double().abs().view(n, S, 3)
    d = rays[:, 3:6]
    fo, fd = pose_far_terms(c)
    a_o = 0.5 * dp.sum(1) + fo.abs()
    g_dn = c["d_ray"][:, 0:1].double().abs()
    a_d = 0.5 * (z[:, :, None] * dp).sum(1) + g_dn * d.abs() / d.norm(dim=1, keepdim=True) + fd.abs()
    a_p = a_d + d.abs() * (d.abs() * a_d).sum(1, keepdim=True)
    m = c["flag"].double()[:, None]
    K = c["K"]
    kf = c["kf"].long()
    at = torch.zeros(K, 3, dtype=torch.float64).index_add_(0, kf, a_o * m) / c["scale"]
    outer = ((a_p * m)[:, :, None] * d.abs()[:, None, :]).reshape(n, 9)
    am = torch.zeros(K, 9, dtype=torch.float64).index_add_(0, kf, outer)
    am = am.view(K, 3, 3)
    aa = c["p6"][:, 3:6].double().requires_grad_()
    Rm = P.axis_angle_to_matrix(aa)
    J = torch.zeros(K, 3, 3, 3, dtype=torch.float64)  # dR_ab / dw_i
    for a in range(3):
        for b in range(3):
            J[:, a, b, :], = torch.autograd.grad(Rm[:, a, b].sum(), aa, retain_graph=True)
    G = am @ Rm.detach().abs()
    ar = (G[:, :, :, None] * J.abs()).sum((1, 2))
    return torch.cat([at, ar], 1).numpy()


def pose_rounding_counts(S):
    """The longest chains of fp32 roundings in k_pose_rays up to the store into ray_ws, plus the final cast of the
    fp64 per-keyframe result to fp32 (k_pose_reduce works in double): (translation, rotation) counts.  A product's
    count is the sum of its factors' plus one, a sum's the largest of its terms' plus one (terms bounded in
    magnitude by ``pose_magnitude``).  With n = ceil(S / 64) per-lane additions:
      so: n + 6 (shuffle steps);                     sz: 1 (z p) + n + 6
      far term: dd = d + 1e-15f 1, t = (s - o) / dd 3, gd = -g t / dd 6, go = -g / dd 2
      |d| (3 products, 2 sums, sqrt) 3, d / |d| 4, times dL/d|d| 5
      g_o = so / 2 + go: n + 7;   stored, summed in double, / scale, cast: n + 8           (translation)
      g_d = (sz / 2 + ...) + gd: n + 9;   d . g_d: n + 12;   d (d . g_d): n + 13;   g_perp: n + 14;
      g_perp d^T: n + 15;   summed and contracted in double, cast: n + 16                  (rotation)"""
    n = (S + 63) // 64
    return n + 8, n + 16


def pose_branch_margins(c):
    """Per pose-following ray, on the float64 reference alone: the relative distance of the cube clip from the far
    range, and of the best axis' clip from the second best's.  The kernel takes both decisions on fp32 values."""
    rays = c["rays"].double()
    o, d = rays[:, 0:3], rays[:, 3:6]
    dd = d + 1e-15
    t = torch.stack([(-1.0 - o) / dd, (1.0 - o) / dd]).clamp(min=0).max(dim=0)[0]
    ts = torch.sort(t, dim=1)[0]
    clip = ts[:, 0]
    use = c["flag"] > 0
    m_range = ((clip - c["far_range"]).abs() / c["far_range"])[use]
    m_axis = ((ts[:, 1] - ts[:, 0]) / ts[:, 1])[use]
    return m_range.numpy(), m_axis.numpy(), (clip < c["far_range"])[use].numpy()


# far-term branches, one ray each: dyadic origins and directions, so that every t is exact in fp32
FAR_BRANCH_RAYS = [
    # name, origin, direction
    ("plus_plane", (0.25, 0.0, 0.0), (0.5, 0.25, 0.125)),       # t_x = 0.75 / 0.5 = 1.5 through +1
    ("minus_plane", (0.25, 0.0, 0.0), (-0.5, 0.25, 0.125)),     # t_x = -1.25 / -0.5 = 2.5 through -1
    ("unit_clip", (0.0, 0.0, 0.0), (1.0, 0.5, 0.25)),           # clip 1: below / equal to / above the ranges tried
    ("zero_component", (0.0, 0.5, 0.0), (0.5, 0.0, 0.25)),      # d_y = 0: t_y = 0.5 / 1e-15, never the minimum
    ("axis_tie", (0.0, 0.0, 0.0), (0.5, 0.5, 0.25)),            # t_x = t_y = 2: the first axis takes the gradient
    ("on_face_outward", (1.0, 0.0, 0.0), (0.5, 0.25, 0.125)),   # t_x: max(clamp(-4), clamp(0)) = 0, tie at the clamp
    ("outside_inward", (1.5, 0.0, 0.0), (-0.5, 0.25, 0.125)),   # t_x = 5 (far side), t_y = 4 wins
    ("outside_outward", (1.5, 0.0, 0.0), (0.5, 0.25, 0.125)),   # both x planes behind: clip 0, no gradient
]
FAR_BRANCH_RANGES = (0.5, 1.0, 8.0)


def far_branch_case():
    """The rays above as a ``lnr_pose_grad`` input with S = 2 and dyadic z, d_pos, d_ray (every sum exact)."""
    n = len(FAR_BRANCH_RAYS)
    rays = torch.zeros(n, 13)
    for i, (_, o, d) in enumerate(FAR_BRANCH_RAYS):
        rays[i, 0:3] = torch.tensor(o)
        rays[i, 3:6] = torch.tensor(d)
        rays[i, 6:9] = -rays[i, 3:6]
    rays[:, 11] = 0.0625
    rays[:, 12] = 8.0
    z = torch.tensor([[0.25, 0.75]]).repeat(n, 1).contiguous()
    d_pos = torch.tensor([[0.5, -0.25, 1.0], [-1.5, 0.75, 0.25]]).repeat(n, 1).contiguous()
    d_ray = torch.tensor([[0.75, -1.25]]).repeat(n, 1).contiguous()
    return dict(rays=rays, z=z, d_pos=d_pos, d_ray=d_ray, S=2)


def far_branch_rows(c, far_range, dtype=torch.float32):
    """The (R, 12) rows k_pose_rays stores for pose-following rays ([dL/do, g_perp d^T]) by the torch chain in
    ``dtype`` on the CPU.  float32: ties exist only there (1 + 1e-15 is 1 in fp32 and not in fp64)."""
    t = lambda a: a.to(dtype)  # noqa: E731
    rays = t(c["rays"])
    g_o, g_d = P.ray_gradients(rays, t(c["z"]), t(c["d_pos"]), t(c["d_ray"]), far_range)
    d = rays[:, 3:6]
    g_perp = g_d - d * (d * g_d).sum(1, keepdim=True)
    return torch.cat([g_o, (g_perp[:, :, None] * d[:, None, :]).reshape(-1, 9)], 1)


# ----------------------------------------------------------------------------- sampler (csrc/sampler.hip)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# launch shapes of lnr_sample_ogm: the block kernel (S / 2 no multiple of 64, or more than 2048 sort slots), the wave
# kernel at two depths per lane, the rank merge (4 and 16 per lane), the wave kernel with +inf padding
SAMPLER_S = (8, 64, 192, 320, 4096, 128, 256, 1024, 384, 640, 1536)
SAMPLER_KERNEL = {8: "block", 64: "block", 192: "block", 320: "block", 4096: "block", 128: "wave", 256: "rank",
                  1024: "rank", 384: "wave_padded", 640: "wave_padded", 1536: "wave_padded"}
SAMPLER_RTOL, SAMPLER_ATOL = 1e-5, 5e-6  # the project's sampler bar (tests/test_gpu_parity.py), no sample excluded
SAMPLER_REF_STABILITY = 4e-6  # the reference alone, its cdf moved by an ulp (tests/test_kernel_cases_ref.py)

_cache = {}


def _golden_samplers():
    if "g" not in _cache:
        g = np.load(os.path.join(GOLDEN, "samplers.npz"))
        _cache["g"] = (g["rays"].copy(), g["occ"].copy())
    return _cache["g"]


def _ogm_cdf(rays, occ, n, uj):
    """oracle.render.ogm_samples up to the inverse CDF: strata z (R, n / 2), bins (R, n / 2 - 1), cdf (R, n / 2 - 1)
    with its leading 0, in the oracle's arithmetic."""
    from oracle import render as orender
    F32 = np.float32
    o, d = rays[:, 0:3], rays[:, 3:6]
    z = orender.stratified(rays[:, -2:-1], rays[:, -1:], n // 2, uj)
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).astype(F32)
    probs = (F32(1) / (F32(1) + np.exp(-orender.grid_sample_3d(occ, pts)))).astype(F32)
    probs = (F32(2) * (np.clip(probs, F32(0.5), F32(1.0)) - F32(0.5))).astype(F32)
    bins = (F32(0.5) * (z[:, :-1] + z[:, 1:])).astype(F32)
    w = (probs[:, 1:-1] + F32(1e-5)).astype(F32)
    pdf = (w / w.astype(np.float64).sum(-1, keepdims=True).astype(F32)).astype(F32)
    cdf = np.cumsum(pdf.astype(np.float64), -1).astype(F32)
    return z, bins, np.concatenate([np.zeros((rays.shape[0], 1), F32), cdf], -1)


def _inverse_cdf(cdf, bins, u):
    """sample_pdf's lookup (oracle/render.py): the depths, and per draw (denom before the eps rule, c0, c1, bin
    width)."""
    F32 = np.float32
    R, M = cdf.shape[0], cdf.shape[1] - 1
    u = u.astype(F32)
    inds = np.stack([np.searchsorted(cdf[r], u[r], side="right") for r in range(R)])
    below, above = np.maximum(inds - 1, 0), np.minimum(inds, M)
    c0, c1 = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    b0, b1 = np.take_along_axis(bins, below, 1), np.take_along_axis(bins, above, 1)
    raw = (c1 - c0).astype(F32)
    denom = np.where(raw < F32(1e-5), F32(1), raw)
    return (b0 + (u - c0) / denom * (b1 - b0)).astype(F32), raw, c0, c1, np.abs(b1 - b0)


def stable_draws(rays, occ, S, rng):
    """u_jitter, u_pdf (R, S / 2) fp32 from ``rng``, the importance draws kept off the reference's own edges.  The
    inverse CDF is continuous in the cdf except where a bin's mass falls below sample_pdf's eps (denom < 1e-5
    becomes 1: the depth snaps to the bin's start, a jump of one bin width at its far end).  There a cdf entry
    that differs by an ulp (another summation order) moves the depth by whole bins, in the oracle as much as in
    a kernel.  So a draw is drawn again while, on the oracle's cdf, its bin's mass is below 2e-5 (inside such a
    bin, or near the eps rule), or it lies within 1e-6 (16 ulps) of either end of its bin (it could cross into
    one), or the bin is so steep that two ulps of cdf move the depth by 1e-6 (width 2^-23 / mass: wide bins of
    little mass at small S).  A condition on the reference alone; tests/test_kernel_cases_ref.py then moves the cdf
    and measures."""
    R, H = rays.shape[0], S // 2
    uj = rng.random((R, H), dtype=np.float32)
    up = rng.random((R, H), dtype=np.float32)
    _, bins, cdf = _ogm_cdf(rays, occ, S, uj)
    if np.all(bins[:, 1:] == bins[:, :-1]):  # far == near: every depth is the same, nothing to keep apart
        return uj, up
    for _ in range(64):
        _, raw, c0, c1, width = _inverse_cdf(cdf, bins, up)
        bad = (raw < 2e-5) | (up - c0 < 1e-6) | (c1 - up < 1e-6) | (width * 2.0 ** -23 > 1e-6 * raw)
        if not bad.any():
            return uj, up
        up[bad] = rng.random(int(bad.sum()), dtype=np.float32)
    raise RuntimeError("stable_draws: no stable draws")


def _draws():
    """u_jitter, u_pdf (32, S / 2) fp32 per S of SAMPLER_S, drawn from default_rng(0) in that order."""
    if "u" not in _cache:
        rays, occ = _golden_samplers()
        rng = np.random.default_rng(0)
        _cache["u"] = {S: stable_draws(rays, occ, S, rng) for S in SAMPLER_S}
    return _cache["u"]


def tiled_rays(n, seed):
    """n rays: the golden 32 repeated, each copy after the first with its own near / far (far shortened)."""
    rays, _ = _golden_samplers()
    rng = np.random.default_rng(seed)
    out = np.concatenate([rays] * ((n + 31) // 32))[:n].copy()
    scale = rng.uniform(0.5, 1.0, n).astype(np.float32)
    near = rng.uniform(0.0, 0.05, n).astype(np.float32)
    out[32:, 12] *= scale[32:]
    out[32:, 11] = near[32:]
    return out


def sampler_case(name):
    """A named input of lnr_sample_ogm: dict(rays, occ, S, u_jitter, u_pdf) with injected draws, or
    dict(rays, occ, S, key, ray_offset) for the kernel's own counter-based draws (oracle.rng restates them)."""
    from oracle import rng as orng
    rays, occ = _golden_samplers()
    kind, _, arg = name.partition(":")
    if kind == "shape":  # (a) the golden rays at every launch shape
        S = int(arg)
        uj, up = _draws()[S]
        return dict(rays=rays, occ=occ, S=S, u_jitter=uj, u_pdf=up)
    if kind == "rng":  # (b) in-kernel draws at a non-zero ray offset
        S = int(arg)
        return dict(rays=rays, occ=occ, S=S, key=orng.step_key(11, 5), ray_offset=70001)
    if kind == "stride":  # (c) more rays than one pass of the launch's blocks
        S = int(arg)
        r = tiled_rays({8: 4096 + 5, 128: 32768 + 5}[S], 200 + S)
        uj, up = stable_draws(r, occ, S, np.random.default_rng(100 + S))
        return dict(rays=r, occ=occ, S=S, u_jitter=uj, u_pdf=up)
    if kind == "edge":  # (d) occupancy and ray-bound edges
        what, _, s = arg.partition(":")
        S = int(s)
        r, o = rays.copy(), occ
        if what == "free":
            o = np.full_like(occ, -10.0)
        elif what == "occupied":
            o = np.full_like(occ, 10.0)
        elif what == "leaving":  # the second half of every ray lies outside the cube (zero padding: logit 0)
            r[:, 12] = 2.0 * r[:, 12]
        elif what == "degenerate":  # far == near, far < near
            r[:16, 12] = r[:16, 11]
            r[16:, 12] = r[16:, 11] - np.float32(0.01)
        else:
            raise KeyError(name)
        uj, up = stable_draws(r, o, S, np.random.default_rng(300 + S))
        return dict(rays=r, occ=o, S=S, u_jitter=uj, u_pdf=up)
    raise KeyError(name)


SAMPLER_CASES = ([f"shape:{S}" for S in SAMPLER_S] + ["rng:192", "rng:256", "stride:8", "stride:128"]
                 + [f"edge:{w}:{S}" for w in ("free", "occupied", "leaving", "degenerate") for S in (64, 256)])


def sampler_draws(c):
    """The case's (u_jitter, u_pdf), injected or restated from the kernel's counters."""
    from oracle import rng as orng
    if "u_jitter" in c:
        return c["u_jitter"], c["u_pdf"]
    R = c["rays"].shape[0]
    a, b = orng.ray_sample_grid(np.arange(c["ray_offset"], c["ray_offset"] + R), c["S"] // 2)
    return orng.uniform(c["key"], orng.STREAM_JITTER, a, b), orng.uniform(c["key"], orng.STREAM_PDF, a, b)


def sampler_reference(c, cdf_ulps=None):
    """oracle.render.ogm_samples on the case.  ``cdf_ulps`` (a Generator): the same with every computed cdf entry
    moved by one fp32 ulp up or down at random before the inverse-CDF lookup (what a different summation order in
    a kernel may do); False: the restatement unmoved, bit for bit the oracle (asserted in
    tests/test_kernel_cases_ref.py)."""
    from oracle import render as orender
    F32 = np.float32
    uj, up = sampler_draws(c)
    if cdf_ulps is None:
        return orender.ogm_samples(c["rays"], c["S"], c["occ"], uj, up)
    z, bins, cdf = _ogm_cdf(c["rays"], c["occ"], c["S"], uj)
    if cdf_ulps is not False:
        up_ = cdf_ulps.integers(0, 2, cdf[:, 1:].shape).astype(bool)
        cdf[:, 1:] = np.where(up_, np.nextafter(cdf[:, 1:], F32(2)), np.nextafter(cdf[:, 1:], F32(-1)))
    zi = _inverse_cdf(cdf, bins, up)[0]
    return np.sort(np.concatenate([z, zi], -1), -1).astype(F32)


UNIFORM_S = (2, 3, 65, 2048)


def uniform_case(S, jitter):
    rays, _ = _golden_samplers()
    u = np.random.default_rng(400 + S).random((32, S), dtype=np.float32) if jitter else None
    return dict(rays=rays, S=S, u_jitter=u)


# ----------------------------------------------------------------------------- preprocessing (csrc/preprocess.hip)
def pose_matrix(yaw, pitch, t, roll=0.0):
    from scipy.spatial.transform import Rotation
    m = np.eye(4)
    m[:3, :3] = Rotation.from_euler("zyx", [yaw, pitch, roll]).as_matrix()
    m[:3, 3] = t
    return m


SKY_POSE = pose_matrix(0.37, 0.2, [1.0, 2.0, 0.5], roll=-0.1)  # a tilt that lifts part of the lowest rows above 10 deg


def bin_directions(theta, phi):
    """(3, P) fp32 directions of the 1-degree bins (theta, phi) (integer degrees), formed in float64: each sits at
    its bin's centre, half a degree from where fp32 atan2 could round to the next bin."""
    th, ph = np.deg2rad(np.asarray(theta, np.float64)), np.deg2rad(np.asarray(phi, np.float64))
    return np.vstack([np.sin(ph) * np.cos(th), np.sin(ph) * np.sin(th), np.cos(ph)]).astype(np.float32)


def sky_scan(case):
    """A scan built from chosen occupied bins; returns dirs (3, P) fp32 and the holes' names -> (rows, cols) of the
    image (row = phi - phi.min(), col = theta - theta.min()).
    "full": theta -180 .. 180 (both ends: theta_img == 360 wraps to 0), phi 20 .. 85 (phi.min() > 0);
    "partial": theta -120 .. 100 (theta.min() > -180: the wrap never applies), phi 30 .. 80."""
    t0, t1, p0, p1 = (-180, 179, 20, 85) if case == "full" else (-120, 100, 30, 80)
    H, W = p1 - p0 + 1, t1 - t0 + 1
    occ = np.ones((H, W), bool)
    holes = {}

    def hole(name, r0, r1, c0, c1):
        occ[r0:r1 + 1, c0:c1 + 1] = False
        holes[name] = (r0, r1, c0, c1)

    hole("single_a", 10, 10, 50, 50)            # closed
    hole("single_b", 25, 25, 200, 200)          # closed
    hole("pair", 12, 12, 120, 121)              # 1 x 2: closed
    hole("three", 15, 17, 100, 102)             # 3 x 3: survives
    hole("three_by_four", 28, 30, 30, 33)       # survives
    hole("left", 20, 24, 0, 4)                  # touches the left border
    hole("right", 32, 34, W - 3, W - 1)         # the right border (col 359 in the full case)
    hole("top", 0, 4, 150, 152)                 # the top border: rows 0 .. 2 are forced occupied, 3 .. 4 stay
    for i, c in enumerate(range(20, W - 3, 60)):
        hole(f"bottom_{i}", H - 3, H - 1, c, c + 2)   # the bottom border, around the azimuth
    rr, cc = np.nonzero(occ)
    theta, phi = cc + t0, rr + p0
    if case == "full":
        # theta = +180 (column 360 -> 0): every fourth row outside the left hole, and the hole's last row, where
        # column 0 is occupied through the wrap alone (landing a row lower it would leave the hole whole)
        rows = np.array([r for r in range(2, H, 4) if not 20 <= r <= 24] + [24])
        theta, phi = np.r_[theta, np.full(rows.size, 180)], np.r_[phi, rows + p0]
    perm = np.random.default_rng(5).permutation(theta.size)  # no order in the scan
    return bin_directions(theta[perm], phi[perm]), holes


def motion_compensate_vec(dirs, dists, ts, start, end, t0, t1, target):
    """oracle.preprocess.motion_compensate for every point at once, float64: dirs (3, P) -> (dirs (3, P), dists)."""
    from scipy.spatial.transform import Rotation
    start, end, target = (np.asarray(m, np.float64) for m in (start, end, target))
    s = (np.asarray(ts, np.float64) - t0) / (t1 - t0)
    trans = (end[:3, 3] - start[:3, 3])[None] * s[:, None] + start[:3, 3][None]
    rv = Rotation.from_matrix(start[:3, :3].T @ end[:3, :3]).as_rotvec()
    ang = np.linalg.norm(rv)
    pts = (np.asarray(dirs, np.float64) * np.asarray(dists, np.float64)[None]).T  # (P, 3)
    if ang >= 1e-9:
        k = rv / ang
        a = (ang * s)[:, None]
        pts = pts * np.cos(a) + np.cross(k[None], pts) * np.sin(a) + k[None] * (pts @ k)[:, None] * (1 - np.cos(a))
    w = pts @ start[:3, :3].T + trans
    tinv = np.linalg.inv(target)
    out = (w @ tinv[:3, :3].T + tinv[:3, 3][None]).T
    d = np.linalg.norm(out, axis=0)
    return out / d, d


def motion_case(name, n=1000):
    """dirs (3, n), dists, ts (float64, fp32-representable), start, end, (t0, t1), target of a named case."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(21)
    dirs = rng.normal(0, 1, (3, n))
    dirs = (dirs / np.linalg.norm(dirs, axis=0)).astype(np.float32).astype(np.float64)
    dists = rng.uniform(1.0, 40.0, n).astype(np.float32).astype(np.float64)
    ts = np.linspace(-0.02, 0.12, n).astype(np.float32).astype(np.float64)  # below t0 and above t1: extrapolation
    start = pose_matrix(0.3, 0.02, [1.0, 2.0, 0.5])
    end = pose_matrix(0.45, -0.01, [1.8, 2.3, 0.6], roll=0.03)
    target = pose_matrix(0.36, 0.01, [1.3, 2.2, 0.52], roll=-0.02)  # neither end
    if name == "identity_rotation":  # equal rotations and a translation: the identity flag
        end = start.copy()
        end[:3, 3] = [1.8, 2.3, 0.6]
    elif name == "near_pi":  # a relative rotation of pi - 1e-3
        axis = np.array([0.6, -0.48, 0.64])
        end = end.copy()
        end[:3, :3] = start[:3, :3] @ Rotation.from_rotvec((np.pi - 1e-3) * axis).as_matrix()
    elif name != "general":
        raise KeyError(name)
    return dict(dirs=dirs, dists=dists, ts=ts, start=start, end=end, t=(0.0, 0.1), target=target)


MOTION_CASES = ("general", "identity_rotation", "near_pi")


def sampler_tie_case():
    """Draws that EQUAL a cdf entry, where searchsorted's side decides the bin (right=True: the bin above).  S = 8:
    four strata, two weights, cdf = [0, c1, c2].  Every ray runs along x from a free half-space (logit -20: prob
    exactly 0) into an occupied one (+20: exactly 1), jitter 1 / 2, so the weights are [1e-5f, 1 + 1e-5f] and the
    first bin's mass c1 = 1e-5f / wtot lies below sample_pdf's eps (denom becomes 1).  A draw u = c1 belongs to the
    second bin and maps to its start b1; taken for the first bin it maps to about b0, a bin width (0.29) lower.
    The tie is the reference's and the kernel's alike: with two weights every step to the cdf is one correctly
    rounded fp32 operation on identical operands (one sum, two quotients, one double sum rounded once), so the cdf
    is the same bit for bit -- unlike the random cases, this one is not stable under a moved cdf, on purpose."""
    R = 8
    occ = np.full((100, 100, 100), -20.0, np.float32)
    occ[:, :, 50:] = 20.0
    rays = np.zeros((R, 13), np.float32)
    rays[:, 0] = -0.5
    rays[:, 1] = np.linspace(-0.6, 0.6, R)
    rays[:, 2] = np.linspace(0.4, -0.4, R)
    rays[:, 3] = 1.0
    rays[:, 6] = -1.0
    rays[:, 11] = np.linspace(0.0, 0.03, R)  # near
    rays[:, 12] = np.linspace(1.0, 0.9, R)   # far
    uj = np.full((R, 4), 0.5, np.float32)
    _, bins, cdf = _ogm_cdf(rays, occ, 8, uj)
    c1 = cdf[:, 1]
    up = np.stack([c1, np.nextafter(c1, np.float32(0)), np.full(R, 0.5, np.float32), np.full(R, 0.9, np.float32)], 1)
    return dict(rays=rays, occ=occ, S=8, u_jitter=uj, u_pdf=up.astype(np.float32)), bins, cdf
