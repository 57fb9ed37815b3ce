"""``lnr_pose_grad`` and ``lnr_pose_adam`` (csrc/pose.hip) called directly through the C ABI, against the torch
statement of the chain (loner_amd/pose.py, pinned on the CPU against autograd by tests/test_pose_chain.py) in
float64 on the fp32 inputs the kernels get, and against torch.optim.Adam.  GPU only.  The inputs, the references and
the bound's derivation are in tests/kernel_cases.py; tests/test_kernel_cases_ref.py asserts on the reference alone
that no branch of the random cases is decided within fp32 rounding."""
import numpy as np
import pytest
import torch

import kernel_cases as C
from loner_amd import pose as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import _lib
    _lib.lib()
    return _lib


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def pose_grad(L, c, slots=None, slot0=0, slot_kf=None, slot_pose=None, n_rays=None, n_kf=None, p6=None, prefill=None):
    """One ``lnr_pose_grad`` call on a kernel_cases.pose_case: (grad (K, 6), ray_ws (R, 12)) on the host."""
    g = lambda t: None if t is None else t.cuda().contiguous()  # noqa: E731
    n = c["rays"].shape[0] if n_rays is None else n_rays
    K = c["K"] if n_kf is None else n_kf
    grad = torch.full((K, 6), float("nan") if prefill is None else prefill, dtype=torch.float32, device="cuda")
    ws = torch.full((max(n, 1), 12), float("nan"), dtype=torch.float32, device="cuda")
    p6 = c["p6"] if p6 is None else p6
    L.call("lnr_pose_grad", g(c["rays"]) if n else None, g(c["z"]) if n else None, g(c["d_pos"]) if n else None,
           g(c["d_ray"]) if n else None, n, c["S"], g(slots), slot0, g(c["kf"] if slot_kf is None else slot_kf),
           g(c["flag"] if slot_pose is None else slot_pose), g(p6), K, c["scale"], c["far_range"],
           ws if n else None, grad, L.stream())
    return host(grad), host(ws)


def check_bound(got, c):
    """|got - ref| <= c 2^-24 A per component (kernel_cases.pose_rounding_counts / pose_magnitude); returns the
    worst err / bound."""
    ref, mag = C.pose_reference(c), C.pose_magnitude(c)
    ct, cr = C.pose_rounding_counts(c["S"])
    bound = np.concatenate([ct * np.ones(3), cr * np.ones(3)])[None] * C.U32 * mag
    err = np.abs(got.astype(np.float64) - ref)
    opt = bound > 0
    ratio = float((err[opt] / bound[opt]).max())
    print(f"pose chain S={c['S']} far={c['far_range']:.3f} R={c['rays'].shape[0]}: worst err/bound {ratio:.3f}")
    assert np.all(err <= bound), (ratio, err / np.where(opt, bound, 1.0))
    assert np.all(got[~opt] == 0)
    return ratio


@pytest.mark.parametrize("far_m", C.POSE_FAR_M)
@pytest.mark.parametrize("S", C.POSE_S)
def test_pose_chain_against_fp64(L, S, far_m):
    """K = 5 keyframes of 37 LiDAR + 9 sky rays (keyframe 0 anchored; axis-angles 0, (1e-8, 0, -1e-8), norm 2e-6,
    norm pi - 1e-3), S in {1, 5, 64, 100, 128} (one partial lane pass, a full one, two, the second partial), far
    range 30 m and 14 m (the cube clip wins on some rays, the range on others).  Every component of the (K, 6)
    gradient: |got - ref| <= c 2^-24 A, with A the float64 chain on absolute values (kernel_cases.pose_magnitude)
    and c the longest chain of fp32 roundings in k_pose_rays plus the final cast, counted in
    kernel_cases.pose_rounding_counts: ceil(S / 64) + 8 for the translation, ceil(S / 64) + 16 for the rotation
    (per-lane additions, 6 shuffle steps, the products z p, the far term, d / |d|, the projection's dot product,
    its two terms, the outer product, the cast).  k_pose_reduce sums and contracts in double (relative 1e-16) and
    its first-order rotation derivative below |w| = 1e-6 is within |w| <= 1.5e-8 of autograd's, both far inside the
    bound.  The anchored keyframe and all sky rays give exact zeros.
    Measured on an MI355X: worst err / bound 0.036 over the ten cases (S = 1, 14 m), 0.003 at S = 128."""
    c = C.pose_case(far_m, S)
    got, ws = pose_grad(L, c)
    check_bound(got, c)
    assert np.all(got[0] == 0)
    assert np.all(ws[c["flag"].numpy() == 0] == 0)  # sky rays and the anchored keyframe's: zero rows
    assert np.all(np.isfinite(ws))


@pytest.mark.parametrize("far_range", C.FAR_BRANCH_RANGES)
def test_far_term_branches(L, far_range):
    """One ray per branch of far_grad (kernel_cases.FAR_BRANCH_RAYS: the +1 and the -1 plane, a zero direction
    component, two axes tying, the origin on a face and outside the cube), at far ranges below, equal to (the half
    share of torch.minimum) and above the unit clip.  Dyadic inputs: every t is exact in fp32, so the ties are
    ties.  Reference: the same torch chain in float32 on the CPU (tests/test_kernel_cases_ref.py pins what it does
    at each tie).  ray_ws rows agree to 4 fp32 ulps of the row's largest entry (the dot product d . g_d and
    1 / |d| may round differently in the two).  Measured: 0 ulps, every row equal."""
    c = C.far_branch_case()
    n = c["rays"].shape[0]
    cc = dict(c, kf=torch.zeros(n, dtype=torch.int32), flag=torch.ones(n), p6=torch.zeros(1, 6), K=1, scale=1.0,
              far_range=far_range)
    _, ws = pose_grad(L, cc)
    ref = C.far_branch_rows(c, far_range).numpy()
    tol = 4 * 2.0 ** -23 * np.abs(ref).max(1, keepdims=True)
    worst = float((np.abs(ws - ref) / tol).max())
    print(f"far branches at range {far_range}: worst err / (4 ulp) {worst:.3f}")
    assert np.all(np.abs(ws - ref) <= tol), (worst, ws, ref)
    # the far term alone (d_pos = 0, dL/d|d| = 0): exact, all values dyadic
    z0 = dict(cc, d_pos=torch.zeros_like(c["d_pos"]), d_ray=torch.tensor([[0.0, -1.25]]).repeat(n, 1).contiguous())
    _, ws0 = pose_grad(L, z0)
    g_o, _ = P.ray_gradients(z0["rays"], z0["z"], z0["d_pos"], z0["d_ray"], far_range)
    np.testing.assert_array_equal(ws0[:, :3], g_o.numpy())


def test_slots_list_equals_contiguous(L):
    """The same rays in the same order addressed through an int64 list slot = 3 r + 1 into a larger slot table
    (the other slots belong to another keyframe and follow the pose) and through slot0 + r into the contiguous
    table: the gradient is bit for bit the same."""
    c = C.pose_case(14.0, 100)
    n = c["rays"].shape[0]
    base, _ = pose_grad(L, c)
    off = 7
    kf_off = torch.cat([torch.full((off,), 3, dtype=torch.int32), c["kf"]])
    fl_off = torch.cat([torch.ones(off), c["flag"]])
    shifted, _ = pose_grad(L, c, slot0=off, slot_kf=kf_off, slot_pose=fl_off)
    np.testing.assert_array_equal(shifted, base)
    slots = 3 * torch.arange(n, dtype=torch.int64) + 1
    kf_big = torch.full((3 * n + 2,), 2, dtype=torch.int32)
    fl_big = torch.ones(3 * n + 2)
    kf_big[slots] = c["kf"]
    fl_big[slots] = c["flag"]
    listed, _ = pose_grad(L, c, slots=slots, slot0=12345, slot_kf=kf_big, slot_pose=fl_big)
    np.testing.assert_array_equal(listed, base)
    assert np.any(base[1:] != 0)


def test_grid_stride_counts_every_ray_once(L):
    """R = 16384 + 37 rays at S = 5, beyond the 4096 blocks of 4 waves k_pose_rays launches: the bound of
    test_pose_chain_against_fp64 holds (a ray skipped or counted twice moves a keyframe's gradient by about
    1 / 3000 of A, hundreds of times the bound).  Measured worst err / bound 0.002."""
    c = C.pose_case(14.0, 5, n_lidar=[3276, 3275, 3275, 3275, 3275], n_sky=9)
    assert c["rays"].shape[0] == 16384 + 37
    got, _ = pose_grad(L, c)
    check_bound(got, c)


def test_empty_batches(L):
    """n_rays = 0 with a NaN-prefilled gradient: every keyframe gets exact zeros; a keyframe that owns no ray
    gets exact zeros while the others keep their gradients."""
    c = C.pose_case(14.0, 5)
    got, _ = pose_grad(L, c, n_rays=0)
    assert got.shape == (5, 6) and np.all(got == 0)
    p6 = torch.cat([c["p6"], torch.tensor([[1.0, -2.0, 0.5, 0.3, -0.2, 0.9]])])
    base, _ = pose_grad(L, c)
    got, _ = pose_grad(L, c, n_kf=6, p6=p6)
    assert np.all(got[5] == 0)
    np.testing.assert_array_equal(got[:5], base)


def test_pose_adam_against_torch(L):
    """Six ``lnr_pose_adam`` steps against torch.optim.Adam (CPU, fp32) on the (K, 6) tensor: optimise mask
    [0, 1, 1, 0], a different lr each step, gradient magnitudes log-uniform over 1e-8 .. 1e3 (both sides of eps),
    at the project's Adam bar (rtol 1e-6, atol 1e-7) for p, m and v.  Masked keyframes keep p, m and v bit for
    bit (their gradients are non-zero).  After each step the rows' rotation is within one fp32 ulp (plus 1e-15 for
    the two float64 evaluations) of pose6_to_rows in float64 on the resulting fp32 tensor, the translation column
    is bitwise the tensor's.  With grad = NULL only the rows are written."""
    rng = np.random.default_rng(11)
    K = 4
    mask = np.array([0, 1, 1, 0], np.uint8)
    p0 = np.concatenate([rng.uniform(-10, 10, (K, 3)), rng.normal(0, 0.8, (K, 3))], 1).astype(np.float32)
    p0[2, 3:] = [1e-8, 0.0, -1e-8]
    m0 = np.zeros((K, 6), np.float32)
    v0 = np.zeros((K, 6), np.float32)
    m0[mask == 0] = rng.normal(0, 1, (2, 6))
    v0[mask == 0] = rng.uniform(0, 1, (2, 6))
    p, m, v = (torch.from_numpy(a.copy()).cuda() for a in (p0, m0, v0))
    rows = torch.full((K, 12), float("nan"), device="cuda")
    opt_u8 = torch.from_numpy(mask).cuda()
    q = torch.nn.Parameter(torch.from_numpy(p0[mask == 1].copy()))
    opt = torch.optim.Adam([q], lr=1e-3)

    def check_rows():
        got = host(rows).reshape(K, 3, 4)
        pn = host(p)
        ref = P.pose6_to_rows(torch.from_numpy(pn).double()).numpy().reshape(K, 3, 4)
        ulp = np.spacing(np.abs(ref[:, :, :3]).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got[:, :, :3] - ref[:, :, :3]) <= ulp + 1e-15)
        np.testing.assert_array_equal(got[:, :, 3], pn[:, :3])

    for step in range(1, 7):
        lr = float(np.float32(1e-3 * (0.5 + step / 4)))
        g = (10.0 ** rng.uniform(-8, 3, (K, 6)) * rng.choice([-1.0, 1.0], (K, 6))).astype(np.float32)
        for pg in opt.param_groups:
            pg["lr"] = lr
        q.grad = torch.from_numpy(g[mask == 1].copy())
        opt.step()
        L.call("lnr_pose_adam", p, m, v, torch.from_numpy(g).cuda(), opt_u8, K, step, lr, 0.9, 0.999, 1e-8, rows,
               L.stream())
        st = opt.state[q]
        np.testing.assert_allclose(host(p)[mask == 1], q.detach().numpy(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(host(m)[mask == 1], st["exp_avg"].numpy(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(host(v)[mask == 1], st["exp_avg_sq"].numpy(), rtol=1e-6, atol=1e-7)
        for got, ref in ((p, p0), (m, m0), (v, v0)):
            np.testing.assert_array_equal(host(got)[mask == 0], ref[mask == 0])
        check_rows()
    assert np.abs(host(p)[mask == 1] - p0[mask == 1]).min() > 0
    # grad = NULL: the rows only (m, v may be NULL too), pose6 unchanged
    p_before = host(p).copy()
    with torch.no_grad():
        p[1, 3:] = torch.tensor([0.0, 0.0, 0.0], device="cuda")
        p_before[1, 3:] = 0.0
    rows.fill_(float("nan"))
    L.call("lnr_pose_adam", p, None, None, None, None, K, 0, 0.0, 0.9, 0.999, 1e-8, rows, L.stream())
    np.testing.assert_array_equal(host(p), p_before)
    check_rows()
