"""Early ray termination's march (lnr_field_ert_march, csrc/field.hip k_ert_march; GPU only).

The march runs a plan's trailing 64-sample phases in one launch: a workgroup per ray still alive encodes 64
samples at all 16 levels, evaluates their sigma, multiplies the ray's transmittance by the unit's product and stops
or goes on.  Its contract is BITWISE equality with the phased sequence lnr_hashgrid_fwd_rays_phase ->
lnr_field_sigma_phase at the bounds lo, lo + 64, .., S: the encodings written (and nothing outside the units a ray
visited), the sigma workspace with its zeros, the status word.

test_march_equals_phases steers where every ray terminates through the injected noise (noise_std = 1): a sample
with noise -1e4 has relu(sigma + n) = 0, alpha = 0 and s = fl(1 + 1e-10) = 1; one with noise 1e30 has alpha = 1 and
s = 1e-10f = 1.00000001335e-10, so a ray's product falls below LNR_ERT_T_MIN = 1e-50 exactly at its sixth such sample
(five leave 1.0000000667e-50, 6.7e-8 relative above the threshold, far more than the 1e-13 by which differently
associated double products differ).  The placement is checked on the CPU with the oracle's compositing arithmetic
(oracle.render._deltas / _transmittance) before the GPU reference is asked the same.

test_march_step_bitwise_on_trained_field runs the engine on a trained field with the plan [0, 128, 192, .., 512]:
marched (eager and graph-replayed), phase by phase, and without termination, three steps with an OGM update, the
live backward and the fused Adam on: bitwise equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R = 70  # rays: no multiple of a wave, a workgroup or a list chunk
T_MIN = 1e-50  # LNR_ERT_T_MIN
SENTINEL = -1  # 0xFFFFFFFF: a pair of fp16 NaNs, which no encoding of a finite table is
N_NEVER = 6  # rays 0 .. 5 never terminate


def _kill_samples(S, lo):
    """Per ray the sample at which its product crosses the threshold (its sixth opaque sample), or -1: never."""
    k = np.full(R, -1, dtype=np.int64)
    k[N_NEVER] = 10            # dead at lo, early in the first phase
    k[N_NEVER + 1] = lo - 1    # dead at lo, on the first phase's last sample
    k[N_NEVER + 2] = lo + 63   # crosses on the last sample of the first marched unit
    k[N_NEVER + 3] = lo + 64   # five opaque samples end that unit: crosses on the first sample of the next
    k[N_NEVER + 4] = S - 30    # crosses in the final unit (which updates nothing)
    span = S - lo
    for r in range(N_NEVER + 5, R):
        k[r] = lo + ((r - N_NEVER - 5) * 37 + 5) % span  # spread over every unit after lo
    return k


def _steering_noise(S, lo):
    k = _kill_samples(S, lo)
    noise = np.full((R, S), -1e4, dtype=np.float32)
    for r in range(R):
        if k[r] >= 0:
            noise[r, k[r] - 5:k[r] + 1] = 1e30
    return noise, k


def _predict_dead_from(noise, z, rays_d, S, lo):
    """CPU: per ray the phase boundary from which it is dead under the phases' rule (the product of s over the
    phases [0, lo), [lo, lo + 64), .. so far below T_MIN; the last phase decides nothing), S for a ray that stays
    alive.  sigma does not enter:
    |sigma| << 1e4 on a random field, so relu(sigma + noise) is 0 or ~1e30 either way."""
    from oracle import render as orender
    dl = orender._deltas(z, rays_d)
    with np.errstate(over="ignore"):
        alphas = (np.float32(1) - np.exp(-dl * np.maximum(noise, np.float32(0)))).astype(np.float32)
    _, s = orender._transmittance(alphas)
    dead_from = np.full(R, S, dtype=np.int64)
    for r in range(R):
        t = 1.0
        bounds = [0, *range(lo, S, 64)]
        for p_lo, p_hi in zip(bounds[:-1], bounds[1:]):
            t *= float(np.prod(s[r, p_lo:p_hi].astype(np.float64)))
            if not t >= T_MIN:
                dead_from[r] = p_hi
                break
    return dead_from


@pytest.fixture(scope="module")
def field():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import step as S_
    from loner_amd import synthetic as syn
    dev = torch.device("cuda", 0)
    out = {}
    win = syn.make_window("quad", 2, seed=77)
    rays, _ = syn.build_batch(win, "quad", rays_per_kf=35, seed=3)
    assert rays.shape == (R, 13)
    for S in (256, 512):
        cfg = S_.StepConfig(n_samples=S)
        state = S_.FieldState(cfg, device=dev, seed=4242, table_init=0.1)  # a random table with full fp16 mantissas
        out[S] = (cfg, state)
    return dev, rays.to(dev), out


def _run(field, S, lo, steer):
    """The first phase [0, lo) with the existing entry points, then from identical copies the phases at 64-sample
    bounds (A) and the march (B).  Returns both copies' buffers and the inputs the CPU check needs."""
    from loner_amd import _lib as L
    dev, rays, states = field
    cfg, state = states[S]
    s = L.stream(dev)
    N = R * S
    key = L.step_key(11, 5)
    z = torch.empty(R, S, dtype=torch.float32, device=dev)
    L.call("lnr_sample_uniform", rays, R, S, 0.0, None, key, 0, z, None, s)
    if steer:
        noise_h, kills = _steering_noise(S, lo)
        noise, noise_std = torch.from_numpy(noise_h).to(dev), 1.0
    else:
        noise_h, kills, noise, noise_std = None, None, None, 0.0
    words = L.lib().lnr_field_train_workspace_words(R, S)
    buf = dict(enc=torch.full((cfg.n_levels, N), SENTINEL, dtype=torch.int32, device=dev),
               ws=torch.full((words,), 7.0, dtype=torch.float32, device=dev),
               T=torch.ones(R, dtype=torch.float64, device=dev),
               lists=torch.zeros(2, R, dtype=torch.int32, device=dev),
               counts=torch.zeros(2, dtype=torch.int32, device=dev),
               keep=torch.zeros(R, dtype=torch.int32, device=dev),
               status=torch.zeros(1, dtype=torch.int32, device=dev))

    def phase(b, q, p_lo, p_hi):
        lp = L.LossParams()
        lp.dev_status = b["status"].data_ptr()
        lin = None if q == 0 else b["lists"][(q - 1) % 2]
        cin = None if q == 0 else b["counts"][(q - 1) % 2:(q - 1) % 2 + 1]
        L.call("lnr_hashgrid_fwd_rays_phase", L.ctypes.byref(state.desc), rays, z, R, S, state.table_f16, b["enc"], N,
               None, 0, lin, cin, 0, p_lo, p_hi, s)
        L.call("lnr_field_sigma_phase", state.mlp_f16, b["enc"], N, rays, z, R, S, p_lo, p_hi, noise_std, noise, key, 0,
               L.ctypes.byref(lp), b["ws"], lin, cin, b["lists"][q % 2], b["counts"][q % 2:q % 2 + 1], b["T"],
               b["keep"], s)

    phase(buf, 0, 0, lo)
    torch.cuda.synchronize()
    A = {k: v.clone() for k, v in buf.items()}
    B = {k: v.clone() for k, v in buf.items()}
    for q, u in enumerate(range(lo, S, 64)):
        phase(A, q + 1, u, u + 64)
    lp = L.LossParams()
    lp.dev_status = B["status"].data_ptr()
    L.call("lnr_field_ert_march", L.ctypes.byref(state.desc), state.table_f16, B["enc"], N, state.mlp_f16, rays, z, R,
           S, lo, noise_std, noise, key, 0, L.ctypes.byref(lp), B["ws"], B["lists"][0], B["counts"][0:1], B["T"], s)
    torch.cuda.synchronize()
    sig_off = L.lib().lnr_dw_workspace_words(R)
    return A, B, dict(z=z.cpu().numpy(), d=rays[:, 3:6].cpu().numpy(), noise=noise_h, kills=kills, sig_off=sig_off)


def _check_equal(A, B, S, lo, dead_from, sig_off):
    """The march's buffers (B) against the phases' (A); dead_from[r]: the boundary from which ray r is dead (S: it
    stays alive), so the units it visited are those below max(dead_from, lo) (the first phase covers every ray)."""
    assert torch.equal(A["ws"], B["ws"]), "the sigma workspace differs"
    assert torch.equal(A["status"], B["status"]), "the status word differs"
    assert torch.equal(A["T"], B["T"]), "the transmittance products differ"
    visited = torch.zeros(R, S, dtype=torch.bool)
    for r in range(R):
        visited[r, :max(int(dead_from[r]), lo)] = True
    visited = visited.reshape(-1).to(A["enc"].device)
    encA, encB = A["enc"], B["enc"]
    assert torch.equal(encA[:, visited], encB[:, visited]), "an encoding of a visited unit differs"
    assert bool((encB[:, visited] != SENTINEL).all()), "the march left a visited unit's encoding unwritten"
    assert bool((encA[:, ~visited] == SENTINEL).all()), "the phases wrote outside the visited units"
    assert bool((encB[:, ~visited] == SENTINEL).all()), "the march wrote outside the visited units"
    sig = B["ws"][sig_off:sig_off + R * S].view(R, S)
    for r in range(R):
        if dead_from[r] < S:
            assert bool((sig[r, int(dead_from[r]):] == 0).all()), f"ray {r}: sigma not 0 from sample {dead_from[r]}"


@pytest.mark.parametrize("S,lo", [(256, 64), (512, 64), (256, 128), (512, 128)])
def test_march_equals_phases(field, S, lo):
    A, B, info = _run(field, S, lo, steer=True)
    kills = info["kills"]
    # the placement, on the CPU with the oracle's compositing arithmetic: every ray dies where it was steered to
    dead_from = _predict_dead_from(info["noise"], info["z"], info["d"], S, lo)
    want = np.where((kills >= 0) & (kills < S - 64), np.maximum((np.maximum(kills, 0) // 64 + 1) * 64, lo), S)
    assert np.array_equal(dead_from, want), (dead_from, want)
    # ... and the reference run itself shows that spread: its sigma zeros and its transmittance products
    sig_off = info["sig_off"]
    sigA = A["ws"][sig_off:sig_off + R * S].view(R, S).cpu().numpy()
    TA = A["T"].cpu().numpy()
    ref_dead = np.full(R, S, dtype=np.int64)
    for r in range(R):
        for u in range(S - 64, -1, -64):  # the first boundary from which every sigma is 0
            if np.any(sigA[r, u:] != 0):
                break
            ref_dead[r] = u
    assert np.array_equal(ref_dead, dead_from), (ref_dead, dead_from)
    assert np.array_equal(TA < T_MIN, dead_from < S), TA
    units = list(range(lo, S - 64, 64))  # the units after lo whose product decides something
    for u in units:
        assert np.any(dead_from == u + 64), f"no ray dies in unit [{u}, {u + 64})"
    assert dead_from[N_NEVER + 2] == lo + 64 and kills[N_NEVER + 2] % 64 == 63  # crosses on a unit's last sample
    # ... and on the next unit's first sample: alive at lo + 64 with five opaque samples behind it
    assert kills[N_NEVER + 3] == lo + 64 and dead_from[N_NEVER + 3] == (lo + 128 if lo + 64 < S - 64 else S)
    assert S - 64 <= kills[N_NEVER + 4] < S and dead_from[N_NEVER + 4] == S and TA[N_NEVER + 4] >= T_MIN  # final unit
    assert int(np.sum(kills < 0)) >= 5 and np.all(dead_from[:N_NEVER] == S) and np.all(TA[:N_NEVER] >= T_MIN)
    assert np.any(dead_from <= lo), "no ray already dead at lo"
    _check_equal(A, B, S, lo, dead_from, sig_off)


@pytest.mark.parametrize("S", [256, 512])
def test_march_without_noise_encodes_everything(field, S):
    """noise = None, noise_std = 0 on a random field: nothing terminates, the march visits every unit."""
    lo = 64
    A, B, info = _run(field, S, lo, steer=False)
    assert bool((A["T"] >= T_MIN).all()), "a ray terminated in the reference"
    assert int(A["counts"][((S - lo) // 64 - 1) % 2].item()) == R  # the last list the phases wrote holds every ray
    _check_equal(A, B, S, lo, np.full(R, S, dtype=np.int64), info["sig_off"])
    assert bool((B["enc"] != SENTINEL).all())


# ---------------------------------------------------------------------------------------------- the engine
N_KF, PER_KF, S_ENG = 4, 512, 512


@pytest.fixture(scope="module")
def trained():
    """A field trained as tests/test_gpu_live.py trains its own: 4 x 512 rays x 512 samples, 8 shuffled windows of 32
    steps, a new Adam per window, the OGM on."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import step as S_
    from loner_amd import synthetic as syn
    from loner_amd.rays import RayWindow
    dev = torch.device("cuda", 0)
    cfg = S_.StepConfig(n_samples=S_ENG)
    state = S_.FieldState(cfg, device=dev)
    pool = syn.make_window("quad", 12, seed=2000)
    rng = np.random.default_rng(3)
    eng = S_.StepEngine(state, N_KF * PER_KF, seed=5)
    eng.live_bwd, eng._live = False, False
    g = 1
    for _ in range(8):
        idx = rng.choice(len(pool), N_KF, replace=False)
        win = RayWindow([pool[i] for i in idx], syn.world_cube("quad"), syn.SENSORS["quad"]["ray_range"],
                        n_lidar=PER_KF, device=dev)
        state.reset_optimizer()
        for it in range(32):
            eng.step_window(win, global_step=g, iteration_idx=it)
            g += 1
        eng.release()
    window = RayWindow(syn.make_window("quad", N_KF, seed=1000), syn.world_cube("quad"),
                       syn.SENSORS["quad"]["ray_range"], n_lidar=PER_KF, device=dev)
    torch.cuda.synchronize()
    g = (g // 10 + 1) * 10 - 1  # the second of the three compared steps updates the OGM
    return cfg, state.state_dict(), window, g


def test_march_step_bitwise_on_trained_field(trained):
    from loner_amd import step as S_
    cfg, sd, window, g = trained
    plan = [0, *range(128, S_ENG + 1, 64)]
    assert S_.ert_march_start(plan) == 1
    out = {}
    for ert, march, graph in ((True, True, False), (True, True, True), (True, False, False), (False, False, False)):
        st = S_.FieldState(cfg, device="cuda")
        st.load_state_dict(sd)
        st.reset_optimizer()
        eng = S_.StepEngine(st, window.n_slots, seed=9)
        eng.live_bwd, eng._live = True, True
        eng.fused_adam = True
        eng.ert, eng.ert_march = ert, march
        eng.ert_cuts = [c / S_ENG for c in plan[1:-1]]
        eng.pipeline, eng.use_graph = False, graph
        alive = []
        for k in range(3):
            eng.step_window(window, global_step=g + k, iteration_idx=k)
            torch.cuda.synchronize()
            if ert:
                assert eng.ert_bounds() == plan
                assert eng.planner.marched == (1 if march else None)
            alive.append(eng.ert_alive_last())
        eng.finish()
        torch.cuda.synchronize()
        o = {k: getattr(st, k).clone() for k in ("params", "m", "v", "shadow", "occ")}
        o["grad_mlp"] = st.grad_mlp.clone()
        o["loss_out"] = eng.loss_out.clone()
        o["depth"] = eng.depth[:window.n_slots].clone()
        out[(ert, march, graph)] = (o, alive)
    ref, _ = out[(False, False, False)]
    phased, alive_phased = out[(True, False, False)]
    for key, (o, alive) in out.items():
        for k in o:
            assert torch.equal(phased[k], o[k]), f"{k} differs between the phased plan and {key} (ert, march, graph)"
            assert torch.equal(ref[k], o[k]), f"{k} differs between the step without termination and {key}"
        if key[0]:
            assert max(alive) < 1.0, (key, alive)  # some rays terminated
            assert alive == alive_phased, (key, alive, alive_phased)  # the march reports the phases' share
