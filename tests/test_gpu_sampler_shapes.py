"""``lnr_sample_ogm`` at every launch shape (csrc/sampler.hip: the block kernel, the wave kernel with and without +inf
padding, the rank merge) and ``lnr_sample_uniform``, against the numpy oracle (oracle/render.py), GPU only.  The
bar is the project's sampler bar (rtol 1e-5, atol 5e-6, tests/test_gpu_parity.py) with no sample excluded, and
depths non-decreasing.  The cases are built in tests/kernel_cases.py; tests/test_kernel_cases_ref.py asserts on the
oracle alone that none of the random ones sits on an edge of the inverse CDF (its cdf moved by an ulp moves no depth
by 4e-6); the one case that sits on an edge on purpose (a draw equal to a cdf entry) has a cdf that is exact."""
import numpy as np
import pytest
import torch

import kernel_cases as C
from oracle import render as orender

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import _lib
    _lib.lib()
    return _lib


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def run_ogm(L, c, perturb=1.0):
    R, S = c["rays"].shape[0], c["S"]
    z = torch.full((R, S), float("nan"), dtype=torch.float32, device="cuda")
    L.call("lnr_sample_ogm", cu(c["rays"]), R, S, cu(c["occ"]), c["occ"].shape[0], perturb, cu(c.get("u_jitter")),
           cu(c.get("u_pdf")), c.get("key", 0), c.get("ray_offset", 0), z, None, L.stream())
    return host(z)


def check_ogm(L, name, monkeypatch):
    monkeypatch.setenv("LONER_SAMPLER_RANK_MIN_RAYS", "0")  # the rank kernel wherever its shape allows it
    c = C.sampler_case(name)
    got, ref = run_ogm(L, c), C.sampler_reference(c)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{name}: {got.shape[0]} rays x {got.shape[1]}, worst |dz| {err.max():.2e} "
          f"(worst / (atol + rtol |z|) {(err / (C.SAMPLER_ATOL + C.SAMPLER_RTOL * np.abs(ref))).max():.3f})")
    assert np.all(np.isfinite(got)) and np.all(np.diff(got, axis=1) >= 0)
    np.testing.assert_allclose(got, ref, rtol=C.SAMPLER_RTOL, atol=C.SAMPLER_ATOL)


@pytest.mark.parametrize("S", C.SAMPLER_S)
def test_ogm_injected_draws_every_launch_shape(L, S, monkeypatch):
    """perturb = 1 with injected draws, the golden rays and occupancy grid, S over the block kernel's shapes (8, 64,
    192, 320, 4096), k_sampler_wave<2> (128), k_sampler_rank<4> and <16> (256, 1024) and the padded wave shapes
    (384, 640, 1536: strata + draws + inf padding through the full sort).  Measured on an MI355X: worst |dz|
    9.7e-7 over the eleven shapes (S = 4096: 0.14 of the bar; the others below 4.2e-7)."""
    check_ogm(L, f"shape:{S}", monkeypatch)


def test_ogm_draw_on_a_cdf_entry(L):
    """searchsorted(cdf, u, right=True) at u == cdf[k], in the block kernel (S = 8): a draw that equals the cdf entry
    above a bin of mass below eps belongs to the next bin and maps to its start; taken for the bin below it would
    map a bin width (0.29) lower.  kernel_cases.sampler_tie_case: the cdf has two entries, each formed by single
    correctly rounded fp32 operations, so the tie holds in the kernel as in the oracle."""
    c, bins, _ = C.sampler_tie_case()
    got, ref = run_ogm(L, c), C.sampler_reference(c)
    assert np.all(np.diff(got, axis=1) >= 0)
    np.testing.assert_allclose(got, ref, rtol=C.SAMPLER_RTOL, atol=C.SAMPLER_ATOL)
    assert np.all(np.isclose(got, bins[:, 1:2], rtol=0, atol=1e-6).sum(1) == 1)  # the tied draw: the second bin's start


@pytest.mark.parametrize("S", [192, 256])
def test_ogm_inkernel_draws_at_ray_offset(L, S, monkeypatch):
    """The kernels' own counter-based draws at ray_offset = 70001 (block kernel at 192, rank kernel at 256)
    against oracle.rng's restatement of them.  Measured worst |dz| 2.2e-6 (S = 192: 0.29 of the bar; the oracle
    alone moves by as much when its cdf moves by an ulp, tests/test_kernel_cases_ref.py)."""
    check_ogm(L, f"rng:{S}", monkeypatch)


@pytest.mark.parametrize("S", [8, 128])
def test_ogm_grid_stride(L, S, monkeypatch):
    """More rays than one pass of the launch: 4096 + 5 rays at S = 8 (block kernel, 4096 blocks) and 32768 + 5 at
    S = 128 (wave kernel, 8192 blocks of 4 waves); each ray (near / far varied per copy of the golden 32) equals
    the oracle's."""
    check_ogm(L, f"stride:{S}", monkeypatch)


@pytest.mark.parametrize("S", [64, 256])
@pytest.mark.parametrize("what", ["free", "occupied", "leaving", "degenerate"])
def test_ogm_occupancy_edges(L, what, S, monkeypatch):
    """An all-free grid (logits -10: uniform importance mass), an all-occupied one (+10), rays that leave the cube
    for half their length (zero padding: logit 0), and rays with far == near and far < near, on the block kernel
    (S = 64) and the rank kernel (S = 256)."""
    check_ogm(L, f"edge:{what}:{S}", monkeypatch)


@pytest.mark.parametrize("jitter", [True, False])
@pytest.mark.parametrize("S", C.UNIFORM_S)
def test_uniform_sampler_shapes(L, S, jitter):
    """lnr_sample_uniform at S in {2, 3, 65, 2048} (the smallest, an odd one, one past a wave, the largest: eight
    strata per thread), with injected jitter and without, at the existing bar (rtol 1e-6, atol 1e-7)."""
    c = C.uniform_case(S, jitter)
    R = c["rays"].shape[0]
    z = torch.full((R, S), float("nan"), dtype=torch.float32, device="cuda")
    L.call("lnr_sample_uniform", cu(c["rays"]), R, S, 1.0 if jitter else 0.0, cu(c["u_jitter"]), 0, 0, z, None,
           L.stream())
    ref = orender.uniform_samples(c["rays"], S, c["u_jitter"])
    np.testing.assert_allclose(host(z), ref, rtol=1e-6, atol=1e-7)
