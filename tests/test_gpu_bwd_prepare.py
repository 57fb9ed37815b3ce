"""The live backward's preparation (k_bwd_live_masks, k_bwd_live_list, k_bwd_count_live's chunk sums) against the
full backward, bitwise (GPU only).

Reference: lnr_hashgrid_bwd_rays_jac without LNR_BWD_LIVE (the full backward: its own count, k_bwd_chunk_sums,
no live list).  Under test: the same call with LNR_BWD_LIVE, in one call and as PREPARE_ONLY + PREPARED.  Inputs:
random fp16 J and a d_sigma whose zeros follow a crafted pattern of live 64-sample waves.  The live list works in
slabs of SLAB waves (one 64-bit mask each), the scans in chunks of 64 histogram rows of 8 live waves; the shapes:
256 rays x 512 samples (the default row minimum of the level-looped scatter the live backward needs, 32 slabs), and
with LONER_SCATTER_ROWS_MIN=1 8 x 512 (one slab, one scan chunk: no chunk sums) and 65 x 512 (a part-filled ninth
slab; with every wave live a second scan chunk of one row).  The runs of SLAB - 1, SLAB, SLAB + 1 live waves start
10 waves before a slab boundary; the 8-ray shape holds SLAB waves in all, so there the three runs are cut to its
SLAB - 1 waves from wave 1 on (a run of SLAB is its every-wave-live case).
The chunk sums are zeroed by the live call itself: the back-to-back and graph-replay tests run different patterns
on one workspace."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, SLAB = 512, 64
SHAPES = {"r256": (256, None), "r8": (8, "1"), "r65": (65, "1")}
PATTERNS = ("none", "first", "last", "scattered9", "all", "run_m1", "run", "run_p1")


def _live_waves(pattern, n_waves):
    if pattern == "none" or pattern == "first" or pattern == "last":
        return []
    if pattern == "scattered9":
        return sorted(np.random.default_rng(1).choice(n_waves, 9, replace=False).tolist())
    if pattern == "all":
        return list(range(n_waves))
    length = {"run_m1": SLAB - 1, "run": SLAB, "run_p1": SLAB + 1}[pattern]
    if n_waves <= SLAB:
        return list(range(1, SLAB))
    return list(range(SLAB - 10, SLAB - 10 + length))


def _d_sigma(pattern, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.zeros(n, dtype=torch.float32)
    if pattern == "first":
        d[5] = 0.25
    elif pattern == "last":
        d[n - 1] = -0.5
    else:
        for w in _live_waves(pattern, n // 64):
            v = torch.randn(64, generator=g) * (torch.rand(64, generator=g) < 0.3)
            v[int(torch.randint(64, (1,), generator=g))] = 1.5  # at least one live sample
            d[64 * w:64 * w + 64] = v
    return d


class Case:
    def __init__(self, L, R):
        from loner_amd import synthetic as syn
        self.L, self.R, self.N = L, R, R * S
        self.desc = L.grid_desc()
        rays, _ = syn.build_batch(syn.make_window("quad", 1, seed=5), "quad", 256, 0, "RANDOM", seed=3)
        self.rays = rays[:R].contiguous().cuda()
        g = torch.Generator().manual_seed(R)
        u = torch.rand(R, S, generator=g).sort(dim=1).values.cuda()
        self.z = (self.rays[:, 11:12] + (self.rays[:, 12:13] - self.rays[:, 11:12]) * u).contiguous()
        nl = int(self.desc.n_levels)
        self.jac = (0.1 * torch.randn(nl, self.N, 2, generator=g)).half().view(torch.int32).reshape(nl, self.N).cuda()
        self.n_out = 2 * sum(int(self.desc.size[l]) for l in range(nl))
        self.nb = sum((int(self.desc.size[l]) + 4095) // 4096 for l in range(nl))
        self.ws_bytes = int(L.lib().lnr_hashgrid_bwd_workspace_bytes(L.ctypes.byref(self.desc), self.N))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")
        self.refs = {}

    def run(self, d_sigma, flags, ws=None, out=None):
        L = self.L
        g = torch.full((self.n_out,), float("nan"), dtype=torch.float32, device="cuda") if out is None else out
        L.call("lnr_hashgrid_bwd_rays_jac", L.ctypes.byref(self.desc), self.rays, self.z, self.R, S, self.jac, d_sigma,
               self.N, g, None, None, self.ws if ws is None else ws, self.ws_bytes, flags, L.stream())
        return g

    def reference(self, pattern):
        """The full backward's gradient for a pattern (computed once, on a workspace of its own) and its d_sigma."""
        if pattern not in self.refs:
            d = _d_sigma(pattern, self.N).cuda()
            ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")
            self.refs[pattern] = (d, self.run(d, 0, ws=ws))
        return self.refs[pattern]

    def records(self, ws=None):
        ws = self.ws if ws is None else ws
        p = self.L.lib().lnr_hashgrid_bwd_seg_start(self.L.ctypes.byref(self.desc), self.N, self.L.ptr(ws))
        off = p - ws.data_ptr()
        return int(ws[off:off + 8 * (self.nb + 1)].view(torch.int64)[self.nb].item())


_cases = {}


@pytest.fixture
def case(request, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import _lib as L
    R, rows_min = SHAPES[request.param]
    if rows_min is None:
        monkeypatch.delenv("LONER_SCATTER_ROWS_MIN", raising=False)
    else:
        monkeypatch.setenv("LONER_SCATTER_ROWS_MIN", rows_min)  # (read at every launch)
    if request.param not in _cases:
        _cases[request.param] = Case(L, R)
    return _cases[request.param]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", list(SHAPES), indirect=True)
def test_live_equals_full(case, pattern):
    L = case.L
    d, ref = case.reference(pattern)
    assert bool(torch.isfinite(ref).all())
    if pattern == "none":
        assert not bool(ref.any())
    else:
        assert bool(ref.any())
    one = case.run(d, L.BWD_LIVE)
    rec_one = case.records()
    assert torch.equal(one, ref), f"live backward, one call: {float((one - ref).abs().max())}"
    two = torch.full_like(ref, float("nan"))
    case.run(d, L.BWD_LIVE | L.BWD_PREPARE_ONLY, out=two)
    assert bool(torch.isnan(two).all())  # (the prepare half writes no gradient)
    case.run(d, L.BWD_LIVE | L.BWD_PREPARED, out=two)
    assert torch.equal(two, ref), f"live backward, prepare + prepared: {float((two - ref).abs().max())}"
    assert case.records() == rec_one
    # the live path ran: it places records for live samples only (the full backward's coherent levels: every sample)
    if pattern == "none":
        assert rec_one == 0
    elif pattern != "all":
        case.run(d, 0)
        assert rec_one < case.records()


@pytest.mark.parametrize("case", ["r256", "r65"], indirect=True)
def test_back_to_back_patterns_on_one_workspace(case):
    """Different patterns enqueued back to back on one workspace, nothing in between: every call starts from the
    sums and lists the call before it left."""
    L = case.L
    seq = ("all", "scattered9", "run_p1", "none", "first", "all")
    refs = [case.reference(p) for p in seq]
    outs = [case.run(d, L.BWD_LIVE) for d, _ in refs]
    torch.cuda.synchronize()
    for p, o, (_, ref) in zip(seq, outs, refs):
        assert torch.equal(o, ref), p


@pytest.mark.parametrize("case", ["r256"], indirect=True)
def test_graph_replay_with_changed_d_sigma(case):
    """PREPARE_ONLY + PREPARED captured once, replayed with d_sigma changed in between (and once more unchanged)."""
    L = case.L
    d = torch.empty(case.N, dtype=torch.float32, device="cuda")
    out = torch.empty(case.n_out, dtype=torch.float32, device="cuda")
    d.copy_(case.reference("all")[0])
    case.run(d, L.BWD_LIVE, out=out)  # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        case.run(d, L.BWD_LIVE | L.BWD_PREPARE_ONLY, out=out)
        case.run(d, L.BWD_LIVE | L.BWD_PREPARED, out=out)
    for p in ("all", "scattered9", "scattered9", "run_m1", "none", "last"):
        ds, ref = case.reference(p)
        d.copy_(ds)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref), p
