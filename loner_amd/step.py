"""Fused optimiser step on the HIP C-ABI: the MI355X-native body of
``Optimizer._do_iterate_optimizer``'s step loop (src/mapping/optimizer.py:354-475).

One step = OGM sampling -> hash-grid encode -> fused [sigma MLP, compositing, LiDAR loss,
compositing backward, MLP backward] -> hash-grid backward -> (all-reduce) -> Adam
[-> OGM update every ``N_iters_acc`` global steps, checked before the increment as at
optimizer.py:466-469].  All buffers are allocated once; a step only enqueues kernels on the
current stream (no host synchronisation) and can be captured in a HIP graph.

Parameter layout (tcnn ``NetworkWithInputEncoding``: network first, then encoding):
    params[0:3072]            sigma MLP, W0 (64,32) then W1 (16,64), row-major [out][in]
    params[3072:]             hash table, (n_entries, 2), level-major
fp32 master + Adam moments; an fp16 shadow of the whole buffer feeds the forward kernels.
"""
import math
import os
import warnings
from dataclasses import dataclass, field

import torch

from . import _lib as L
from .ert import (ERT_FIXED_US, ERT_MARCH, ERT_MARCH_FIXED_US, ERT_MARCH_SAMPLE_NS, ERT_MARGIN,  # noqa: F401
                  ERT_MAX_CUTS, ERT_PHASE_US, ERT_SAMPLE_NS, ErtPlanner, ert_alive, ert_cost_us, ert_march_start,
                  ert_plan)


@dataclass
class LossConfig:
    """``model_config.loss`` (cfg/model_config/default_model_config.yaml:40-60)."""
    loss_selection: str = "L1_JS"
    min_js_score: float = 1.0
    max_js_score: float = 10.0
    js_alpha: float = 1.0
    decay_los_lambda: bool = False
    los_lambda: float = 1000.0
    min_los_lambda: float = 10.0
    los_lambda_decay_rate: float = 0.001
    los_lambda_decay_steps: float = 15000
    decay_depth_eps: bool = True
    depth_eps: float = 3.0
    min_depth_eps: float = 0.5
    depth_eps_decay_rate: float = 0.95
    depth_eps_decay_steps: float = 1
    depthloss_lambda: float = 0.005

    @staticmethod
    def from_dict(d):
        js = d.get("JS_loss", {})
        keys = {k: d[k] for k in LossConfig.__dataclass_fields__ if k in d}
        return LossConfig(**keys, min_js_score=js.get("min_js_score", 1.0), max_js_score=js.get("max_js_score", 10.0),
                          js_alpha=js.get("alpha", 1.0))

    def los_lambda_at(self, global_step):
        # optimizer.py:712-716 (and :846-848): decay evaluated on global_step + 1
        if self.decay_los_lambda:
            return max(self.los_lambda * (self.los_lambda_decay_rate ** ((global_step + 1) / self.los_lambda_decay_steps)),
                       self.min_los_lambda)
        return self.los_lambda

    def los_eps_at(self, iteration_idx):
        # optimizer.py:781-785
        if self.decay_depth_eps:
            return max(self.depth_eps * (self.depth_eps_decay_rate ** (iteration_idx / self.depth_eps_decay_steps)),
                       self.min_depth_eps)
        return self.depth_eps


@dataclass
class StepConfig:
    n_samples: int = 512              # render.N_samples_train
    perturb: float = 1.0              # render.perturb
    raw_noise_std: float = 1.0        # render.raw_noise_std
    lr: float = 0.01                  # train.lrate_sigma_mlp
    occ_res: int = 100                # occ_model.voxel_size
    occ_lr: float = 1e-4              # occ_model.lr
    n_iters_acc: int = 10             # occ_model.N_iters_acc
    sampler: str = "OGM"              # samples_selection.strategy
    n_levels: int = 16
    log2_hashmap_size: int = 18
    base_resolution: int = 16
    per_level_scale: float = 2.0
    loss: LossConfig = field(default_factory=LossConfig)


class FieldState:
    """Parameters, Adam moments, fp16 shadow and the occupancy grid, resident on one GPU.

    With a data-parallel or sharded ``StepEngine`` on this state, the last step's OGM update and shadow
    all-gathers may still be pending on the device: call the engine's ``finish()`` (or ``drop_prefetch()`` /
    ``release()``, which call it) before reading ``occ``, ``shadow`` or ``state_dict()`` directly."""

    def __init__(self, cfg: StepConfig, device="cuda", seed=1337, table_init=1e-4):
        self.cfg = cfg
        self.device = torch.device(device)
        self.desc = L.grid_desc(cfg.n_levels, 2, cfg.log2_hashmap_size, cfg.base_resolution, cfg.per_level_scale)
        self.n_entries = int(self.desc.n_entries)
        self.n_mlp = L.SIGMA_MLP_PARAMS
        self.n_params = self.n_mlp + 2 * self.n_entries
        self.n_padded = (self.n_params + 3) // 4 * 4
        dev = self.device
        self.params = torch.zeros(self.n_padded, dtype=torch.float32, device=dev)
        self.grad = torch.zeros_like(self.params)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.shadow = torch.zeros(self.n_padded, dtype=torch.float16, device=dev)
        self.occ = torch.zeros(cfg.occ_res ** 3, dtype=torch.float32, device=dev)
        self.occ_ws = torch.zeros(int(L.lib().lnr_ogm_workspace_words(cfg.occ_res)), dtype=torch.float32, device=dev)
        self.adam_step = 0
        # whether grad_table holds the last step's table gradient: a step with the table's Adam fused into
        # the backward (StepEngine.fused_adam) applies it where it is accumulated and never stores it
        self.grad_table_current = True
        self.init_params(seed, table_init)

    # tcnn init: FullyFusedMLP xavier-uniform per matrix, HashGrid U(-1e-4, 1e-4) (restated with a
    # counter-based generator: tcnn's PCG stream is not reproducible here)
    def init_params(self, seed=1337, table_init=1e-4):
        s = L.stream(self.device)
        a0 = math.sqrt(6.0 / (32 + 64))
        a1 = math.sqrt(6.0 / (64 + 16))
        p = self.params
        L.call("lnr_fill_uniform", (p), 64 * 32, seed, -a0, a0, 0, s)
        L.call("lnr_fill_uniform", L.ctypes.c_void_p(p.data_ptr() + 4 * 64 * 32), 16 * 64, seed + 1, -a1, a1, 0, s)
        L.call("lnr_fill_uniform", L.ctypes.c_void_p(p.data_ptr() + 4 * self.n_mlp), 2 * self.n_entries, seed + 2,
               -table_init, table_init, 0, s)
        self.refresh_shadow()

    def refresh_shadow(self):
        L.call("lnr_f32_to_f16", (self.params), (self.shadow), self.n_padded, L.stream(self.device))

    def reset_optimizer(self):
        """A new torch.optim.Adam per window / iteration config (optimizer.py:255-265)."""
        self.m.zero_()
        self.v.zero_()
        self.adam_step = 0

    # views
    @property
    def mlp_f16(self):
        return self.shadow[:self.n_mlp]

    @property
    def table_f16(self):
        return self.shadow[self.n_mlp:self.n_mlp + 2 * self.n_entries]

    @property
    def grad_table(self):
        """The table's slice of the flat gradient (the backward's output buffer).  NOT written by a step whose
        table Adam is fused into the backward (``grad_table_current`` is then False and the slice keeps an
        older gradient); use ``table_gradient()`` to read it safely."""
        return self.grad[self.n_mlp:self.n_mlp + 2 * self.n_entries]

    def table_gradient(self):
        """The last step's table gradient; raises when that step fused the table's Adam into the backward
        (the gradient never went to memory: run with StepEngine.fused_adam = False to keep it)."""
        if not self.grad_table_current:
            raise RuntimeError("the last step fused the table's Adam into the backward: its table gradient was "
                               "never stored (StepEngine.fused_adam = False keeps it)")
        return self.grad_table

    @property
    def grad_mlp(self):
        return self.grad[:self.n_mlp]

    def state_dict(self):
        return {"params": self.params[:self.n_params].clone(), "occupancy_grid": self.occ.clone(),
                "adam_step": self.adam_step, "m": self.m[:self.n_params].clone(), "v": self.v[:self.n_params].clone()}

    def load_state_dict(self, sd):
        self.params[:self.n_params].copy_(sd["params"])
        self.occ.copy_(sd["occupancy_grid"].reshape(-1))
        if "m" in sd:
            self.m[:self.n_params].copy_(sd["m"])
            self.v[:self.n_params].copy_(sd["v"])
            self.adam_step = int(sd.get("adam_step", 0))
        self.refresh_shadow()


FUSED_ADAM_MAX_N = 1 << 17  # samples up to which the step fuses the table's Adam into the backward ("auto")
ADAM = (0.9, 0.999, 1e-8)  # beta1, beta2, eps of every Adam launch here (torch.optim.Adam's defaults)
# the level at which the two gradient-exchange ranges split: [cut, L) first, then [0, cut) + MLP.  Modelled per
# cut from the measured per-range accumulate at C4 shard 1/8 (tools/zero_tail_model.py): the
# exchange's critical path is 3 us shorter at 6 than at 4 and 13-20 us shorter than at 8 (round 4's cut) for
# ring bandwidths of 100-400 GB/s
AR_CUT_DEFAULT = 6
# with the sharded optimiser's all-gathers on a communicator of their own (bench.py LONER_EXCHANGE_GROUPS=2), the
# gather of range 1 overlaps range 2's reduce-scatter, and the model puts the best cut at 8 (levels 8-15 first):
# 168 us exposed at 200 GB/s if the two share the link bandwidth, 148 us if not, against 191 / 156 at cut 6
# (tools/zero_tail_model.py, profiles/r06_zero_tail_model_C4s8.txt)
AR_CUT_TWO_GROUPS = 8


def _env_on(name):
    """An on/off switch of the environment: on unless set to 0."""
    return os.environ.get(name, "1") != "0"


def _env_tri(name):
    """A three-way switch of the environment: 1 -> True, 0 -> False, otherwise (the default) "auto"."""
    return {"0": False, "1": True}.get(os.environ.get(name, "auto"), "auto")


class _Readback:
    """A device value read on the host without a synchronisation: ``tick`` copies it to pinned memory behind an
    event, ``poll`` (at later steps) returns the host copy once the event has completed.  Inert without a GPU."""

    def __init__(self, shape, dtype, every):
        self.host = torch.zeros(shape, dtype=dtype).pin_memory() if torch.cuda.is_available() else None
        self.ev, self.ctr = None, every  # (due at the first step)

    def poll(self):
        if self.ev is None or not self.ev.query():
            return None
        self.ev = None
        return self.host

    def tick(self, every, src):
        """Count a step and, every ``every`` steps with no read in flight, arm one of the device tensor ``src()``."""
        self.ctr += 1
        if self.ev is None and self.ctr >= every and self.host is not None:
            self.ctr = 0
            self.host.copy_(src(), non_blocking=True)
            self.ev = torch.cuda.Event()
            self.ev.record()


class _RayBufs:
    """One set of the buffers step_window builds a step's rays into: rays, depths, validity, global ray 0's far
    bound, and either the samples ``z`` (all-valid windows) or the compacted rays and depths (``compacted``)."""

    def __init__(self, n_rays, S, dev, compacted=False):
        f32 = dict(dtype=torch.float32, device=dev)
        self.rays, self.dgt = torch.empty(n_rays, 13, **f32), torch.empty(n_rays, **f32)
        self.valid, self.far = torch.empty(n_rays, dtype=torch.uint8, device=dev), torch.empty(1, **f32)
        self.z = None if compacted else torch.empty(n_rays, S, **f32)
        self.rays_c = torch.empty(n_rays, 13, **f32) if compacted else None
        self.dgt_c = torch.empty(n_rays, **f32) if compacted else None

    def build(self, window, key, offset, n, **kw):
        window.build(key, offset, n, self.rays[:n], self.dgt[:n], self.valid[:n], None, self.far, **kw)

    def make_current(self, eng):
        """The buffers of the step in flight: rays, depth_gt, ray_valid, far_ref and z as step() uses them."""
        eng.z, eng.rays, eng.depth_gt, eng.ray_valid, eng.far_ref = self.z, self.rays, self.dgt, self.valid, self.far


class _Step:
    """What the stages of one step() share: the batch (rays, depth_gt, R, noise), prof, the stream (s, main), the
    per-step scalars (key, dsp, lp) and what a stage leaves for a later one (forked, count_work, fwd_hist, flags,
    mlp_adam_done)."""


def _planner_attr(name):
    return property(lambda self: getattr(self.planner, name), lambda self, v: setattr(self.planner, name, v))


class StepEngine:
    """Preallocated workspaces for a fixed ray-batch size; ``step`` runs one optimiser step."""

    def __init__(self, state: FieldState, n_rays: int, seed: int = 0, allreduce=None, ray_offset: int = 0,
                 zero=None, reduce_scatter=None, all_gather=None, ar_cut=None):
        self.state = state
        self.cfg = state.cfg
        self.n_rays = n_rays
        self.S = self.cfg.n_samples
        self.N = n_rays * self.S
        self.seed = seed
        self.ray_offset = ray_offset
        self.lr_factor = 1.0  # ExponentialLR: the caller sets gamma^k (optimizer.py:262, stepped per iteration)
        dev = state.device
        nl = self.cfg.n_levels
        # the encoding gradient: compact (d sigma / d enc as fp16 pairs + dL/dsigma, 4 + 4/L B per sample and
        # level) where the field kernel's per-ray path supports it, else d_enc itself (float2)
        self.compact_denc = self.S in (64, 128, 256, 512)
        # ---- the environment's switches, each with what it decides
        # level ranges of the bucketed gradient all-reduce, finest first: the first range's exchange
        # overlaps the later range's accumulation.  Every range is its own accumulate + finalize
        # launch pair, and at world size 1 over RCCL (no peer traffic; tools/dp_overhead.py, round 3) the step
        # cost 2.18-2.25 ms with one range, 2.23-2.30 with two (levels 8-15, then 0-7 + the MLP)
        # and 2.41-2.44 with four, against 2.12 without the hook; two ranges hide about half of the
        # 29.7 MB exchange for a fraction of the four ranges' cost.  LONER_AR_BUCKETS = 1, 2 or 4.
        # With two ranges the cut level is LONER_AR_CUT (default AR_CUT_DEFAULT; the modelled exposure of
        # the sharded optimiser's tail per cut: DESIGN.md section 7, tools/zero_tail_model.py).
        nbk = int(os.environ.get("LONER_AR_BUCKETS", "2"))
        if nbk <= 1:
            cuts = [nl, 0]
        elif nbk == 2:
            cut = int(os.environ.get("LONER_AR_CUT", str(AR_CUT_DEFAULT if ar_cut is None else ar_cut)))
            cuts = sorted({nl, min(max(cut, 1), max(nl - 1, 1)), 0}, reverse=True)
        else:
            cuts = sorted({nl, max(nl - 5, 1), max(nl - 10, 1), min(3, nl), 0}, reverse=True)
        self.ar_groups = [(cuts[i + 1], cuts[i]) for i in range(len(cuts) - 1)]
        # The live backward's histogram, scans and lists need dL/dsigma only, not the MLP backward's J: with
        # split_bwd (LONER_SPLIT_BWD, default 1) they run on a side stream beside the MLP backward
        # (lnr_field_train's LNR_LP_FORWARD_ONLY / BACKWARD_ONLY halves, the backward's LNR_BWD_PREPARE_ONLY /
        # PREPARED halves), captured as two branches of the step's graph; bitwise the one-stream step
        self.split_bwd = _env_on("LONER_SPLIT_BWD")
        # step_window on windows whose rays can fail the 1 m filter: two ray buffers, the next step's
        # build + compaction prefetched on a side stream (``prefetch``)
        self.prefetch = _env_on("LONER_PREFETCH")
        # step_window on windows whose rays all pass the filter: step k + 1's ray build and sampling
        # enqueued on a side stream right after step k (two ray / depth buffers), so they run in the
        # holes step k leaves (the scatter's last round, the accumulate's tail) instead of at the head
        # of step k + 1 (``pipeline``; not when step k updates the OGM, which the sampler reads)
        self.pipeline = _env_on("LONER_PIPELINE")
        # the single-GPU step's table Adam fused into the backward (lnr_hashgrid_bwd_rays_jac_adam, bitwise
        # the separate lnr_adam_step).  "auto" (default): for batches of at most 2^17 samples, whose
        # whole-bucket accumulation spreads the Adam work over a workgroup per bucket (C1 0.161 -> 0.152
        # ms); at C2 the record-balanced accumulation's bucket ends carry it less well (1.950 -> 1.958-
        # 1.989 ms), so there it stays a separate pass.  LONER_FUSED_ADAM=1 / 0 forces it on / off; the
        # data-parallel paths always exchange the gradient first.
        self.fused_adam = _env_tri("LONER_FUSED_ADAM")
        # step_window on all-valid windows, single process: the whole step (ray build, sampling, encode,
        # field, backward, Adam, and the OGM update on its steps) captured once per (window, OGM or not)
        # in a HIP graph and replayed, its per-step scalars (key, loss scalars, Adam coefficients) set in
        # device memory by one small launch before each replay (``lnr_step_scalars``): one graph launch
        # in place of ~18 kernel launches (LONER_GRAPH=0 turns it off; the pipelined path then runs)
        # LONER_GRAPH: auto (default: batches of at most 2^18 samples, where the host's launch cost is a
        # visible share of the step; measured C1 0.161 against 0.163 ms eager on a fast host, 0.188 against
        # 0.236 on a slow one; and from 2^22 samples, where every kernel fills the chip, so the eager path's
        # next-step prefetch (the sampler: texture-addresser work) slows the encode beside it about as much
        # as it hides: C2 1.910-1.916 against 1.918-1.923 ms eager since round 5's lighter sampler, 2.040
        # against 2.016 before it.  In between, the prefetch fills what the smaller kernels leave idle: C4
        # shard 1/8 0.374-0.381 eager against 0.380-0.381), 1 always, 0 never
        g = _env_tri("LONER_GRAPH")
        self.use_graph = g is True or (g == "auto" and (self.N <= (1 << 18) or self.N >= (1 << 22)))
        # The live backward (LNR_BWD_LIVE): a sample with dL/dsigma = 0 (relu(sigma + noise) = 0,
        # rendering_tcnn.py:260) adds exactly 0 to the table gradient, and on a trained field most samples are such
        # (~80 % at C2 after the driver's windows, bench.py --field trained; ~0 % in the first steps from init).
        # The live backward places records only for the others, after a histogram pass over them: bitwise the
        # full backward's gradient, so the choice is a matter of speed only.  Its work skips by 64-sample wave
        # (a wave without a live sample does nothing), and its histogram pass costs ~0.16 ms at C2 when every
        # wave is live (C2 backward 1.15 against 0.99 ms from init, 0.49 against 0.95 ms trained with 69 % of the
        # waves dead: break-even near 20 % dead waves).  LONER_LIVE_BWD: 1 always, 0 never, auto (default):
        # every live_probe_every steps the share of dead waves (no sample with dL/dsigma != 0) of the last step
        # is read back asynchronously (no host sync: an event polled at the next steps), and the live backward
        # runs while the share exceeds live_on (back to the full one below live_off).
        self.live_bwd = _env_tri("LONER_LIVE_BWD")
        self.live_on, self.live_off, self.live_probe_every = 0.25, 0.15, 16
        self._live = self.live_bwd is True
        # Early ray termination: a sample behind enough opaque ones has float transmittance exactly 0 in the
        # compositing, so its weight is 0 and neither its sigma nor its encoding can change any output
        # (csrc/field.hip, LNR_ERT_T_MIN; 45 % of a trained C2 batch lies behind T = 0, tools/dead_bound.py).  The
        # forward then runs in phases of samples per ray (ert_bounds): each phase encodes and evaluates the rays still
        # alive and updates their transmittance, and a ray below 1e-50 skips the later phases.  Empirically bitwise
        # the step without it (tests/test_gpu_live.py; not a theorem: the compositing's double products associate
        # differently, csrc/field.hip gives the bound that keeps the skipped samples out of every float result).
        # With ert_march (on unless LONER_ERT_MARCH=0, see ert.ERT_MARCH) a plan's trailing run of 64-sample phases
        # runs as one launch, the march (lnr_field_ert_march), bitwise the phases.
        # LONER_ERT: auto (default): the compositing counts where every ray terminates (term_hist,
        # lnr_loss_params.dev_term_hist), read back like the live backward's probe (no host sync), and ert_plan
        # picks the phases, or none, from the last steps' counts under a fitted cost model
        # (on the trained C2 field three cuts, on C4's forest, where few rays terminate,
        # none); 1: always, at the fixed cuts LONER_ERT_CUTS (fractions of n_samples, default 0.5,0.625,0.75); 0: never.
        # ``ert``, ``ert_cuts`` and ``ert_march`` are the planner's mode, cuts and march (loner_amd.ert.ErtPlanner).
        ert_cuts = [float(v) for v in os.environ.get("LONER_ERT_CUTS", "0.5,0.625,0.75").split(",") if v.strip()]
        self.planner = ErtPlanner(self.S, self.compact_denc, _env_tri("LONER_ERT"), ert_cuts, ERT_MARCH)
        # ---- the step's workspaces
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)  # LNR_STATUS_* bits
        self._warned_clip = False
        self.enc = torch.empty(nl, self.N, dtype=torch.int32, device=dev)
        self.ws = torch.empty(L.lib().lnr_field_train_workspace_words(n_rays, self.S), dtype=torch.float32, device=dev)
        if self.compact_denc:
            self.d_jac = torch.empty(nl, self.N, dtype=torch.int32, device=dev)
            self.d_enc = None
        else:
            self.d_enc = torch.empty(nl, self.N, 2, dtype=torch.float32, device=dev)
        self._r_last = n_rays  # the last step's ray count (d_sigma's place in the workspace follows it)
        self.bwd_ws_bytes = int(L.lib().lnr_hashgrid_bwd_workspace_bytes(L.ctypes.byref(state.desc), self.N))
        self.bwd_ws = torch.empty(self.bwd_ws_bytes, dtype=torch.uint8, device=dev)
        # the backward's per-level max |d_enc| (record scales), written by the field kernel's MLP backward
        self.level_max_ptr = L.ctypes.c_void_p(L.lib().lnr_hashgrid_bwd_level_max(L.ctypes.byref(state.desc), self.N,
                                                                                   L.ptr(self.bwd_ws)))
        self.stats = torch.zeros(n_rays, L.RAY_STATS, dtype=torch.float32, device=dev)
        self.depth = torch.empty(n_rays, dtype=torch.float32, device=dev)
        self.opacity = torch.empty(n_rays, dtype=torch.float32, device=dev)
        self.loss_out = torch.zeros(8, dtype=torch.float32, device=dev)
        self.n_opaque = torch.zeros(1, dtype=torch.float32, device=dev)
        # the opaque count (and its all-reduce) runs on a side stream, off the critical path: only the
        # field kernel needs it (forked after the rays exist, joined before the field kernel)
        self._side = torch.cuda.Stream(device=dev)
        self._fork, self._join = torch.cuda.Event(), torch.cuda.Event()
        # the split backward's side stream (split_bwd)
        self._bside = torch.cuda.Stream(device=dev)
        self._bfork, self._bjoin = torch.cuda.Event(), torch.cuda.Event()
        # the live backward's probe (live_probe): the last step's count of live waves, of _probe_n
        self._live_read, self._probe_n = _Readback(1, torch.int64, self.live_probe_every), 1
        # ---- the exchange.  allreduce: callable(tensor[, async_op]) summing in place across ranks
        # (torch.distributed.all_reduce semantics), or None
        self.allreduce = allreduce
        # Sharded optimiser (ZeRO-1): zero = (rank, world).  Each level range's gradient slice is
        # reduce-scattered instead of all-reduced (reduce_scatter(out, inp, async_op), the semantics of
        # torch.distributed.reduce_scatter_tensor), the rank runs Adam on its 1/world chunk of every range,
        # and the updated fp16 shadow chunks are all-gathered (all_gather(out, inp, async_op), as
        # all_gather_into_tensor).  The fp32 master and the moments stay current only on each chunk's
        # owner: sync_master() all-gathers the master (checkpoints).  With zero but no collectives (one
        # process), the step does one rank's share of Adam and nothing else: the per-rank work of an
        # N-GPU run, for measuring it on one GPU (bench.py --shard-of).
        self.zero = None
        if zero is not None:
            zr, zw = int(zero[0]), int(zero[1])
            if not 0 <= zr < zw:
                raise ValueError(f"zero=(rank, world) out of range: {zero}")
            self.zero = (zr, zw)
            self.reduce_scatter, self.all_gather = reduce_scatter, all_gather
            if zw > 1 and allreduce is not None and (reduce_scatter is None or all_gather is None):
                raise ValueError("a sharded optimiser over ranks needs reduce_scatter and all_gather hooks")
            self.zero_chunks = []  # per level range: (a0, a1, chunk), this rank owning [a0 + r c, a0 + (r+1) c)
            for l0, l1 in self.ar_groups:
                a0, a1 = self._ar_range(l0, l1)
                if (a1 - a0) % (4 * zw):
                    raise ValueError(f"levels [{l0}, {l1}) hold {a1 - a0} parameters, not a multiple of 4 x {zw} ranks "
                                     "(the sharded optimiser needs equal, 16-B aligned chunks)")
                self.zero_chunks.append((a0, a1, (a1 - a0) // zw))
            if len(self.zero_chunks) > L.ADAM_MAX_RANGES:
                raise ValueError(f"{len(self.zero_chunks)} level ranges: at most {L.ADAM_MAX_RANGES} (one Adam launch)")
            self.zero_grad = [torch.empty(c, dtype=torch.float32, device=dev) for _, _, c in self.zero_chunks]
        self._pending_shadow = []  # async all-gather works of the last sharded step (finish())
        # data-parallel OGM step: the grid gradient's all-reduce runs asynchronously and the SGD step that
        # consumes it is enqueued before the grid's next reader (the next step's sampler, or finish())
        self._pending_ogm = None
        # ---- on-device ray building (step_window): two buffer sets per path, the next step's built beside this one
        self._pf, self._pf_parity = None, 0  # windows with invalid rays (prefetch)
        self._pf_stream = torch.cuda.Stream(device=dev)
        self._pf_fork = torch.cuda.Event()
        self._pf_bufs = [_RayBufs(n_rays, self.S, dev, compacted=True) for i in range(2)]
        self._pp, self._pp_parity = None, 0  # all-valid windows (pipeline, and the graph step)
        self._pp_stream = torch.cuda.Stream(device=dev)
        self._pp_fork = torch.cuda.Event()
        self._pp_bufs = [_RayBufs(n_rays, self.S, dev) for i in range(2)]
        self._pp_bufs[0].make_current(self)  # z, rays, depth_gt, ray_valid, far_ref
        self.dev_step = torch.zeros(8, dtype=torch.int32, device=dev)  # the graph step's lnr_step_scalars (32 B)
        self._graphs, self._graph_window = {}, None
        self._capture_stream = torch.cuda.Stream(device=dev)
        # ---- joint pose + map (loner_amd.pose): with pose_grad on, the step also writes per ray [dL/d|d|, dL/dfar]
        # (d_ray, from the field kernel) and per sample dL/dpos01 (d_pos, the hash grid's input gradient,
        # before the table's Adam); ``poses`` (a pose.PoseWindow) then takes its Adam step after every
        # step_window step and rewrites the window's pose rows, which the next step's ray build reads
        self.pose_grad = False
        self.map_frozen = False
        self.poses = None
        self.d_ray = self.d_pos = None
        self._last_batch = None
        # ---- early ray termination's device state: the lists of rays still alive (two buffers, alternating),
        # their counts, the transmittance products and a scratch word per ray; the termination counts and their
        # read-back (ert_probe)
        self.ert_lists = torch.zeros(2, max(n_rays, 1), dtype=torch.int32, device=dev)
        self.ert_counts = torch.zeros(2, dtype=torch.int32, device=dev)
        self.ert_T = torch.ones(n_rays, dtype=torch.float64, device=dev)
        self.ert_keep = torch.zeros(max(n_rays, 1), dtype=torch.int32, device=dev)
        nb = self.S // 64 + 1
        self.term_hist = (torch.zeros(L.TERM_HIST_SLOTS, nb, dtype=torch.int32, device=dev) if self.S % 64 == 0
                          else None)  # (slots spread the compositing's atomics; ert_probe sums them)
        self._term_read = (_Readback((L.TERM_HIST_SLOTS, nb), torch.int32, self.live_probe_every)
                           if self.term_hist is not None else None)

    ert, ert_cuts, ert_march = _planner_attr("mode"), _planner_attr("cuts"), _planner_attr("march")

    def ert_bounds(self):
        """The early-ray-termination phases [0, b1, ..., S] of the coming step, or None (ErtPlanner.bounds)."""
        return self.planner.bounds()

    def _adam(self, c, a, b, grad=None):
        """Adam on parameters [a, b) at st.adam_step (``grad``: their gradient where it is not st.grad's slice)."""
        st = self.state
        L.call("lnr_adam_step", st.params[a:b], st.shadow[a:b], st.grad[a:b] if grad is None else grad, st.m[a:b],
               st.v[a:b], b - a, st.adam_step, self.map_lr(), *ADAM, c.dsp, c.s)

    def _mlp_adam(self, c):
        """Adam on the parameters outside the table (the MLP, and the padding tail), at st.adam_step."""
        st = self.state
        nm, nt = st.n_mlp, 2 * st.n_entries
        self._adam(c, 0, nm)
        if st.n_padded > nm + nt:
            self._adam(c, nm + nt, st.n_padded)

    def fuses_adam(self, N=None):
        """Whether the step runs the table's Adam inside the backward's accumulation (LONER_FUSED_ADAM: 1, 0, auto):
        one GPU (no exchange), the compact encoding gradient, and (auto) a batch of at most FUSED_ADAM_MAX_N samples
        or the live backward, whose unit accumulation takes the epilogue without spilling (the record-balanced one
        of a large full backward does not: k_bwd_accum<*, true>); C2 trained 0.949 -> 0.934 ms, C4 1.199 -> 1.182
        (the separate Adam's 237 MB of table traffic moves under the LDS-bound accumulation)."""
        N = self.N if N is None else N
        return self.allreduce is None and self.zero is None and self.compact_denc and (
            self.fused_adam is True or (self.fused_adam == "auto" and (N <= FUSED_ADAM_MAX_N or self._live)))

    def ert_alive_last(self):
        """The share of the last step's rays still alive after its last cut (early ray termination), or 1.0
        without phases (a host sync: tests and tools).  A marched plan writes no lists: the share is counted from
        the transmittance products the march left, the rays with T >= LNR_ERT_T_MIN after the last cut -- the
        same rays the last list would hold."""
        b = self.planner.last
        if b is None or len(b) < 3:
            return 1.0
        if self.planner.marched is not None:
            return int((self.ert_T[:self._r_last] >= L.ERT_T_MIN).sum().item()) / max(self._r_last, 1)
        return int(self.ert_counts[(len(b) - 3) % 2].item()) / max(self._r_last, 1)

    def ert_probe(self):
        """LONER_ERT=auto: re-plan the phases from the termination counts the steps since the last probe added to
        term_hist (read back behind an event, no host sync; the first probe after the first step, then every
        live_probe_every steps).  While a window's graphs replay the planner defers a new plan to the next window."""
        rb = self._term_read
        if self.ert != "auto" or rb is None:
            return
        got = rb.poll()
        if got is not None:
            self.planner.observe(got.long().sum(0).tolist(), self._r_last * self.S,
                                 defer=self._graph_window is not None)
        rb.tick(self.live_probe_every, lambda: self.term_hist)

    def map_lr(self):
        """The map's Adam learning rate this step: lrate_sigma_mlp x the ExponentialLR factor, or 0 while the
        map is frozen (``map_frozen``: pose tracking, optimizer.py:232,255-257; Adam with a zero step size
        leaves every parameter bit for bit as it is)."""
        return 0.0 if self.map_frozen else self.cfg.lr * self.lr_factor

    def set_poses(self, poses):
        """Optimise the window's poses with the map (``poses``: a loner_amd.pose.PoseWindow), or stop (None).
        The pose gradient's buffers are allocated on first use."""
        self.poses = poses
        self.pose_grad = poses is not None
        if self.pose_grad and self.d_ray is None:
            dev = self.state.device
            self.d_ray = torch.zeros(self.n_rays, 2, dtype=torch.float32, device=dev)
            self.d_pos = torch.zeros(self.N, 3, dtype=torch.float32, device=dev)
        self.drop_prefetch()  # a prefetched build read the poses before this step's update

    def loss_params(self, global_step, iteration_idx, scale, far_ref, n_rays_global, dev_far_ref=None):
        # (flags: lnr_field_train stores the MLP gradient, no zeroing launch, and finalizes the loss scalars into
        # loss_out in its last launch, no lnr_loss_finalize launch)
        lc = self.cfg.loss
        return L.LossParams(
            kind=L.LOSS_KINDS[lc.loss_selection], scale=float(scale), los_lambda=float(lc.los_lambda_at(global_step)),
            depthloss_lambda=lc.depthloss_lambda, min_depth_eps=lc.min_depth_eps, min_js=lc.min_js_score,
            max_js=lc.max_js_score, js_alpha=lc.js_alpha, los_eps=float(lc.los_eps_at(iteration_idx)),
            far_ref=0.0 if far_ref is None else float(far_ref), inv_n_opaque=0.0,
            inv_rs=1.0 / float(n_rays_global * self.S), dev_n_opaque=self.n_opaque.data_ptr(),
            dev_far_ref=None if dev_far_ref is None else dev_far_ref.data_ptr(), dev_status=self.status.data_ptr(),
            dev_loss_out=self.loss_out.data_ptr(), flags=L.LP_DW_OVERWRITE)

    def check_status(self, clear=True):
        """Read the device status word (one host sync; call it as often as the caller wants, e.g. once
        per window).  Raises like the reference's per-step ``assert not torch.isnan(loss), "NaN Loss
        Encountered"`` (optimizer.py:854) and warns once, like DecoupledNeRF (nerf_tcnn.py:74-78),
        when a non-finite sigma was clipped.  Returns the bits."""
        bits = int(self.status.item())
        if clear:
            self.status.zero_()
        if bits & L.STATUS_SIGMA_CLIPPED and not self._warned_clip:
            self._warned_clip = True
            warnings.warn("Clipping infinite outputs. Will not warn about this again (but it will happen again)")
        if bits & L.STATUS_NAN_LOSS:
            raise RuntimeError("NaN Loss Encountered")
        return bits

    def _ar_range(self, l0, l1):
        """[a0, a1) of level range [l0, l1) in the flat parameter buffer (range 0 also holds the MLP)."""
        st = self.state
        a0 = 0 if l0 == 0 else st.n_mlp + 2 * int(st.desc.offset[l0])
        return a0, st.n_mlp + 2 * int(st.desc.offset[l1])

    def sync_master(self):
        """Sharded optimiser: all-gather the fp32 master (and the Adam moments) chunks so every rank holds
        the whole current state (e.g. before a checkpoint).  A no-op otherwise."""
        self.finish()
        if self.zero is None or self.zero[1] == 1 or self.all_gather is None:
            return
        st, (zr, zw) = self.state, self.zero
        for a0, a1, c in self.zero_chunks:
            for buf in (st.params, st.m, st.v):
                self.all_gather(buf[a0:a1], buf[a0 + zr * c:a0 + (zr + 1) * c])

    def _allreduce_async(self, t):
        """``allreduce(t, async_op=True)`` when the hook supports it (torch.distributed's
        all_reduce does: the returned work's wait() makes the current stream wait), else a
        blocking call."""
        try:
            return self.allreduce(t, async_op=True)
        except TypeError:
            self.allreduce(t)
            return None

    @staticmethod
    def _mark(prof, stage):
        """Record a HIP event on the current stream (the stream every kernel here is launched on)."""
        if prof is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            prof.setdefault(stage, []).append(ev)

    def _ogm_due(self, global_step, update_ogm=None):
        """Whether this step updates the OGM: every N_iters_acc global steps (optimizer.py:466-469) by default."""
        return global_step % self.cfg.n_iters_acc == 0 if update_ogm is None else update_ogm

    def step(self, rays, depth_gt, global_step, iteration_idx=0, scale=1.0, far_ref=None, n_rays_global=None,
             u_jitter=None, u_pdf=None, noise=None, update_ogm=None, prof=None, presampled=False, dev_step=None,
             fork_count=True):
        """rays (R,13) fp32, depth_gt (R,) fp32 normalised, both on this GPU, R <= the engine's
        capacity.  Returns the device loss buffer [loss, mean_eps, depth_term, los_term, opacity_term,
        n_opaque] (no host sync).  ``far_ref``: the far bound of global ray 0, a float or a 1-element
        device tensor.  ``prof``: optional dict collecting (begin, end) HIP event pairs per stage.
        ``dev_step``: a device ``lnr_step_scalars`` holding this step's key, loss scalars and Adam
        coefficients, read by the kernels instead of their host arguments (the graph-captured step)."""
        st, m = self.state, self._mark
        R = rays.shape[0]
        assert rays.shape == (R, 13) and depth_gt.shape == (R,) and R <= self.n_rays, (rays.shape, self.n_rays)
        if far_ref is None:
            raise ValueError("far_ref (far bound of global ray 0) is required; optimizer.py:724")
        dev_far = far_ref if isinstance(far_ref, torch.Tensor) else None
        far_h = None if dev_far is not None else float(far_ref)
        c = _Step()
        c.rays, c.depth_gt, c.R, c.noise, c.prof = rays, depth_gt, R, noise, prof
        c.s, c.main = L.stream(st.device), torch.cuda.current_stream(st.device)
        c.key = L.step_key(self.seed, global_step)
        c.dsp = None if dev_step is None else dev_step.data_ptr()
        lp = c.lp = self.loss_params(global_step, iteration_idx, scale, far_h, R if n_rays_global is None else
                                     n_rays_global, dev_far)
        lp.dev_step = c.dsp
        lp.dev_d_ray = self.d_ray.data_ptr() if self.pose_grad else None
        # (counted under fixed phases too, for the tools' alive shares: no measurable cost, C2 0.903 ms either way)
        lp.dev_term_hist = self.term_hist.data_ptr() if self.ert is not False and self.term_hist is not None else None
        # 1. opaque count (global)
        self._count_opaque(c, far_h, dev_far, fork_count or self.allreduce is not None)
        # 2. sampling (``presampled``: step_window's pipeline already drew self.z for these rays); the previous
        # step's data-parallel OGM update lands first (the sampler reads the grid)
        self._apply_pending_ogm()
        m(prof, "sample")
        if not presampled:
            self._sample(rays, R, self.z, c.key, c.s, u_jitter, u_pdf, c.dsp)
        m(prof, "sample")
        # 3. encode (+ backward record histogram); it reads the fp16 shadow, which the previous step's
        # sharded-optimiser all-gathers may still be writing
        self.finish()
        self._encode(c)
        # 4. fused field + loss + backward through compositing and MLP, then the poses' share of the gradient
        self._field(c)
        if self.pose_grad:
            self._pose_grad(c)
        # 5-7. hash-grid backward, gradient exchange, Adam (+ fp16 shadow)
        if self.zero is not None:
            self._bwd_adam_sharded(c)
        elif self.fuses_adam():
            self._bwd_adam_fused(c)
        else:
            self._bwd_adam_replicated(c)
        # 8. OGM every N_iters_acc global steps
        if self._ogm_due(global_step, update_ogm):
            m(prof, "ogm")
            self.ogm_update(rays, depth_gt, scale)
            m(prof, "ogm")
        return self.loss_out

    def _count_opaque(self, c, far_h, dev_far, fork):
        """Stage 1: the local count of opaque rays + its all-reduce.  ``fork``: on the side stream, so both overlap
        sampling + encode (the field kernel first needs the count: _field joins); else (a captured single-stream
        step) inline, one stream in the graph."""
        dev = self.state.device
        c.forked, c.count_work = fork, None

        def count(s):
            L.call("lnr_count_opaque", c.depth_gt, c.R, 0.0 if far_h is None else far_h, dev_far, self.n_opaque, s)

        if not fork:
            return count(c.s)
        self._fork.record(c.main)
        with torch.cuda.stream(self._side):
            self._side.wait_event(self._fork)
            count(L.stream(dev))
            if self.allreduce is not None:
                c.count_work = self._allreduce_async(self.n_opaque)
            self._join.record(self._side)

    def _sample(self, rays, R, z, key, s, u_jitter=None, u_pdf=None, dsp=None):
        """Stage 2's launch: S depths per ray into ``z``, OGM-guided or uniform (samples_selection.strategy)."""
        cfg = self.cfg
        if cfg.sampler == "OGM":
            L.call("lnr_sample_ogm", rays, R, self.S, self.state.occ, cfg.occ_res, cfg.perturb, u_jitter, u_pdf, key,
                   self.ray_offset, z, dsp, s)
        else:
            L.call("lnr_sample_uniform", rays, R, self.S, cfg.perturb, u_jitter, key, self.ray_offset, z, dsp, s)

    def _encode(self, c):
        """Stage 3: the hash-grid encode of every sample, or, with early ray termination (see __init__), phase by
        phase the encode and sigma of the rays still alive (the list phase q - 1 left; every ray in phase 0; a ray
        that terminates gets sigma 0 at its later samples), then the march over the plan's trailing 64-sample
        phases, from the list the last phase before it left."""
        st, cfg, m = self.state, self.cfg, self._mark
        rays, R, S, N, lp, s = c.rays, c.R, self.S, self.N, c.lp, c.s
        desc = L.ctypes.byref(st.desc)
        m(c.prof, "encode")
        # the backward's record histogram, counted from the forward's corners, for the full backward (the live one
        # counts its live records itself)
        c.fwd_hist = not self._live
        hist = (self.bwd_ws, self.bwd_ws_bytes) if c.fwd_hist else (None, 0)
        ert, i0 = self.planner.begin_step()
        if ert is None:
            L.call("lnr_hashgrid_fwd_rays", desc, rays, self.z, R, S, st.table_f16, self.enc, N, *hist, s)
        else:
            # (a profiled march step keeps every launch inside the "encode" pair: bench.py scales the
            # "sigma_phase" pairs by the plan's phases, which the march does not launch)
            lp.flags |= L.LP_SIGMA_READY
            mp = c.prof if i0 is None else None
            est = self.planner.shares
            for q in range(len(ert) - 1 if i0 is None else i0):
                lo, hi = ert[q], ert[q + 1]
                lin = None if q == 0 else self.ert_lists[(q - 1) % 2]
                cin = None if q == 0 else self.ert_counts[(q - 1) % 2:(q - 1) % 2 + 1]
                expect = 0 if (q == 0 or est is None) else int(est[lo // 64] * R) + 64
                L.call("lnr_hashgrid_fwd_rays_phase", desc, rays, self.z, R, S, st.table_f16, self.enc, N,
                       *(hist if q == 0 else (None, 0)), lin, cin, expect, lo, hi, s)
                m(mp, "sigma_phase")
                L.call("lnr_field_sigma_phase", st.mlp_f16, self.enc, N, rays, self.z, R, S, lo, hi,
                       cfg.raw_noise_std, c.noise, c.key, self.ray_offset, L.ctypes.byref(lp), self.ws, lin, cin,
                       self.ert_lists[q % 2], self.ert_counts[q % 2:q % 2 + 1], self.ert_T, self.ert_keep, s)
                m(mp, "sigma_phase")
            if i0 is not None:
                q = i0 - 1
                L.call("lnr_field_ert_march", desc, st.table_f16, self.enc, N, st.mlp_f16, rays, self.z, R, S,
                       ert[i0], cfg.raw_noise_std, c.noise, c.key, self.ray_offset, L.ctypes.byref(lp), self.ws,
                       self.ert_lists[q % 2], self.ert_counts[q % 2:q % 2 + 1], self.ert_T, s)
        m(c.prof, "encode")

    def _field_train(self, c, extra):
        st, lp = self.state, c.lp
        lp.flags |= extra
        L.call("lnr_field_train", st.mlp_f16, self.enc, self.N, c.rays, self.z, c.depth_gt, c.R, self.S,
               self.cfg.raw_noise_std, c.noise, c.key, self.ray_offset, L.ctypes.byref(lp), self.d_enc, st.grad_mlp,
               self.ws, self.stats, self.depth, self.opacity, None, self.level_max_ptr,
               self.d_jac if self.compact_denc else None, c.s)
        lp.flags &= ~extra

    def _field(self, c):
        """Stage 4: fused field + loss + backward through compositing and MLP (stores the MLP gradient, and the
        loss scalars into loss_out), after joining the opaque count.  Leaves the table backward's flags in c.flags."""
        st, m, main = self.state, self._mark, c.main
        if c.forked:
            main.wait_event(self._join)
        if c.count_work is not None:
            c.count_work.wait()  # orders the current stream after the collective (no host sync)
        c.flags = (L.BWD_COUNTS_READY if c.fwd_hist else 0) | L.BWD_LEVEL_MAX_READY | (L.BWD_LIVE if self._live else 0)
        c.mlp_adam_done = False
        split = (self.split_bwd and self._live and self.compact_denc and c.prof is None and self.allreduce is None
                 and self.zero is None)
        m(c.prof, "field")
        if split:
            # compositing (dL/dsigma), then the backward's preparation on the side stream beside the MLP backward
            self._field_train(c, L.LP_FORWARD_ONLY)
            self._bfork.record(main)
            with torch.cuda.stream(self._bside):
                self._bside.wait_event(self._bfork)
                self._grid_bwd(c.rays, c.R, c.flags | L.BWD_PREPARE_ONLY, L.stream(st.device))
                self._bjoin.record(self._bside)
            self._field_train(c, L.LP_BACKWARD_ONLY)
            if self.fuses_adam():
                # the MLP's Adam (its gradient is complete) while the side stream still prepares the backward
                st.adam_step += 1
                self._mlp_adam(c)
                c.mlp_adam_done = True
            main.wait_event(self._bjoin)
            c.flags |= L.BWD_PREPARED
        else:
            self._field_train(c, 0)
        m(c.prof, "field")
        self._r_last = c.R

    def _pose_grad(self, c):
        """Stage 4b, the poses' share: dL/dpos01 per sample (tcnn's input gradient) from the table the forward
        read, before the table's Adam changes it."""
        self._mark(c.prof, "pose_grad")
        self._grid_bwd(c.rays, c.R, 0, c.s, d_pos=True)
        self._mark(c.prof, "pose_grad")

    def _grid_bwd(self, rays, R, flags, s, d_pos=False):
        """The hash-grid backward launch on the last step's encoding gradient (compact or not): the table
        gradient into st.grad_table under ``flags`` (LNR_BWD_*: also its prepare half and its record placement
        without accumulation), or (``d_pos``) the input gradient into self.d_pos instead."""
        st = self.state
        if d_pos:
            out = (None, st.table_f16, self.d_pos, None, 0, 0)
        else:
            st.grad_table_current = True
            out = (st.grad_table, None, None, self.bwd_ws, self.bwd_ws_bytes, flags)
        if self.compact_denc:
            L.call("lnr_hashgrid_bwd_rays_jac", L.ctypes.byref(st.desc), rays, self.z, R, self.S, self.d_jac,
                   self.d_sigma(R), self.N, *out, s)
        else:
            L.call("lnr_hashgrid_bwd_rays", L.ctypes.byref(st.desc), rays, self.z, R, self.S, self.d_enc, self.N,
                   *out, s)

    def _accum_range(self, c, l0, l1):
        """Accumulate levels [l0, l1) of the records _grid_bwd placed (LNR_BWD_NO_ACCUM) into the table gradient."""
        st = self.state
        L.call("lnr_hashgrid_bwd_accum_flags", L.ctypes.byref(st.desc), c.R * self.S, self.bwd_ws, self.bwd_ws_bytes,
               l0, l1, st.grad_table, c.flags & L.BWD_LIVE, c.s)

    def _bwd_adam_fused(self, c):
        """Stages 5 + 7 on one GPU: the table's Adam inside the backward (lnr_hashgrid_bwd_rays_jac_adam: each
        entry's gradient updates its parameter where the accumulation finishes it, bitwise lnr_adam_step's
        result), then Adam on the MLP's parameters alone (unless the split field stage already ran it)."""
        st, m = self.state, self._mark
        m(c.prof, "grid_bwd")
        if not c.mlp_adam_done:
            st.adam_step += 1
        st.grad_table_current = False
        nm, nt = st.n_mlp, 2 * st.n_entries
        epi = L.AdamEpilogue(L.ptr(st.params[nm:nm + nt]), L.ptr(st.shadow[nm:nm + nt]), L.ptr(st.m[nm:nm + nt]),
                             L.ptr(st.v[nm:nm + nt]), st.adam_step, self.map_lr(), *ADAM, c.dsp)
        L.call("lnr_hashgrid_bwd_rays_jac_adam", L.ctypes.byref(st.desc), c.rays, self.z, c.R, self.S, self.d_jac,
               self.d_sigma(c.R), self.N, L.ctypes.byref(epi), self.bwd_ws, self.bwd_ws_bytes, c.flags, c.s)
        m(c.prof, "grid_bwd")
        m(c.prof, "adam")
        if not c.mlp_adam_done:
            self._mlp_adam(c)
        m(c.prof, "adam")

    def _bwd_adam_replicated(self, c):
        """Stages 5-7, every replica holding the whole optimiser: backward, gradient all-reduce (if any), Adam."""
        st, m = self.state, self._mark
        m(c.prof, "grid_bwd")
        if self.allreduce is None:
            self._grid_bwd(c.rays, c.R, c.flags, c.s)
            m(c.prof, "grid_bwd")
        else:
            # 6. bucketed by level range: each range's slice of the gradient is all-reduced (async) while the
            # next range accumulates; the MLP gradient travels with the last range
            self._grid_bwd(c.rays, c.R, c.flags | L.BWD_NO_ACCUM, c.s)
            pending = []
            for l0, l1 in self.ar_groups:
                self._accum_range(c, l0, l1)
                a0, a1 = self._ar_range(l0, l1)
                pending.append(self._allreduce_async(st.grad[a0:a1]))
            m(c.prof, "grid_bwd")
            m(c.prof, "allreduce")
            for w in pending:
                if w is not None:
                    w.wait()
            m(c.prof, "allreduce")
        st.adam_step += 1
        m(c.prof, "adam")
        L.call("lnr_adam_step", st.params, st.shadow, st.grad, st.m, st.v, st.n_padded, st.adam_step,
               self.map_lr(), *ADAM, c.dsp, c.s)
        m(c.prof, "adam")

    def _bwd_adam_sharded(self, c):
        """Stages 5-7 with the sharded optimiser (see __init__), pipelined per level range: each range
        is accumulated and its gradient slice reduce-scattered (asynchronous: the next range accumulates
        meanwhile); then, range by range as its reduce-scatter lands, Adam on this rank's chunk of it and
        the all-gather of that chunk's fp16 shadow (asynchronous).  Nothing waits for the all-gathers here:
        the next reader of the shadow (the next step's encode, after its ray build and sampling, or
        finish()) does, so the gather overlaps the next step's head.  Exposed per step: the last range's
        reduce-scatter and its Adam (the cut: AR_CUT_DEFAULT)."""
        st, m = self.state, self._mark
        zr, zw = self.zero
        comm = self.allreduce is not None and zw > 1
        rs = [None] * len(self.zero_chunks)
        m(c.prof, "grid_bwd")
        if comm:
            self._grid_bwd(c.rays, c.R, c.flags | L.BWD_NO_ACCUM, c.s)
            for i, ((l0, l1), (a0, a1, _), out) in enumerate(zip(self.ar_groups, self.zero_chunks, self.zero_grad)):
                self._accum_range(c, l0, l1)
                rs[i] = self.reduce_scatter(out, st.grad[a0:a1], async_op=True)
        else:  # one process: this rank's share of the work only (no exchange)
            self._grid_bwd(c.rays, c.R, c.flags, c.s)
        m(c.prof, "grid_bwd")
        st.adam_step += 1
        m(c.prof, "adam")
        if not comm:
            # this rank's chunk of every level range, one launch (lnr_adam_step_ranges)
            rng = (L.AdamRange * len(self.zero_chunks))()
            for i, (a0, a1, n) in enumerate(self.zero_chunks):
                o = a0 + zr * n
                rng[i] = L.AdamRange(L.ptr(st.params[o:o + n]), L.ptr(st.shadow[o:o + n]), L.ptr(st.grad[o:o + n]),
                                     L.ptr(st.m[o:o + n]), L.ptr(st.v[o:o + n]), n)
            L.call("lnr_adam_step_ranges", rng, len(self.zero_chunks), st.adam_step, self.map_lr(), *ADAM, c.dsp, c.s)
        else:
            pend = []
            for i, ((a0, a1, n), g) in enumerate(zip(self.zero_chunks, self.zero_grad)):
                if rs[i] is not None:
                    rs[i].wait()  # orders the current stream after this range's reduce-scatter
                o = a0 + zr * n
                self._adam(c, o, o + n, g)
                pend.append(self.all_gather(st.shadow[a0:a1], st.shadow[o:o + n], async_op=True))
            self._pending_shadow = [w for w in pend if w is not None]
            if c.prof is not None:
                self.finish()  # a profiled step keeps its stages apart
        m(c.prof, "adam")

    def live_probe(self, n_rays=None):
        """LONER_LIVE_BWD=auto: pick the backward for the coming steps from the share of dead 64-sample waves
        (see __init__).  Called after every step by step_window; a probe is a count of the last step's waves
        holding a non-zero dL/dsigma, read back without a host sync (_Readback).  Also runs the
        early-ray-termination probe (ert_probe)."""
        self.ert_probe()
        if self.live_bwd != "auto":
            return
        rb = self._live_read
        got = rb.poll()
        if got is not None:
            dead = 1.0 - float(got[0]) / self._probe_n
            self._live = dead > (self.live_off if self._live else self.live_on)

        def live_waves():
            r = self._r_last if n_rays is None else n_rays
            nw = r * self.S // 64
            self._probe_n = max(nw, 1)
            return torch.count_nonzero(self.d_sigma(r)[:64 * nw].view(nw, 64).ne(0).any(1)).view(1)

        rb.tick(self.live_probe_every, live_waves)

    def finish(self):
        """Order the current stream after the sharded optimiser's pending shadow all-gathers (the shadow is
        then whole again).  step() calls it before its encode; call it before reading the fp16 parameters
        elsewhere (checkpoints, evaluation on the same FieldState).  A no-op without pending gathers."""
        self._apply_pending_ogm()
        pend, self._pending_shadow = self._pending_shadow, []
        for w in pend:
            w.wait()

    def d_sigma(self, n_rays=None):
        """dL/dsigma (n_rays * S) of the last step: lnr_field_train leaves it in its workspace after the dW
        slabs, whose count follows the call's ray count."""
        r = self._r_last if n_rays is None else n_rays
        off = int(L.lib().lnr_dw_workspace_words(r))
        return self.ws[off:off + r * self.S]

    def denc_f32(self):
        """The last step's encoding gradient as (L, N, 2) fp32 (tests and tools; the step itself keeps
        the compact form: d_sigma * J, computed exactly so in the backward)."""
        if not self.compact_denc:
            return self.d_enc
        nl, n = self.cfg.n_levels, self._r_last * self.S
        ds = self.d_sigma().view(1, n, 1)
        # (J is not written where a 32-sample pair's dL/dsigma are all 0: d_enc is 0 there, include/loner_amd.h)
        return torch.where(ds == 0, 0.0, self.d_jac.view(torch.float16).view(nl, self.N, 2)[:, :n].float() * ds)

    def ogm_update(self, rays, depth_gt, scale):
        """Optimizer._step_occupancy_grid (optimizer.py:897-908).  Data-parallel: the grid gradient
        is all-reduced before the SGD step so every replica applies the global-batch update; the all-reduce
        is asynchronous and the SGD step waits for it at the grid's next reader (``_apply_pending_ogm``)."""
        st = self.state
        s = L.stream(st.device)
        if self.allreduce is None:
            L.call("lnr_ogm_update", (rays), (self.z), (depth_gt), rays.shape[0], self.S, float(scale),
                   self.cfg.occ_lr, (st.occ), (st.occ_ws), st.occ_ws.numel(), self.cfg.occ_res, s)
            return
        L.call("lnr_ogm_grad", (rays), (self.z), (depth_gt), rays.shape[0], self.S, float(scale),
               (st.occ_ws), st.occ_ws.numel(), self.cfg.occ_res, s)
        g = st.occ_ws[:st.occ.numel()]
        # asynchronous: nothing on this step's stream waits for it; the SGD step is enqueued (after a wait on
        # the collective) right before the grid's next reader (_apply_pending_ogm)
        self._pending_ogm = (self._allreduce_async(g), g)

    def _apply_pending_ogm(self):
        """Enqueue the data-parallel OGM step's SGD update once its gradient all-reduce is waited for (a
        no-op without one pending)."""
        p, self._pending_ogm = self._pending_ogm, None
        if p is None:
            return
        w, g = p
        if w is not None:
            w.wait()  # orders the current stream after the collective (no host sync)
        L.call("lnr_sgd_step", self.state.occ, g, self.state.occ.numel(), self.cfg.occ_lr, L.stream(self.state.device))

    def step_window(self, window, global_step, iteration_idx=0, n_rays_global=None, prof=None, n_slots=None, **kw):
        """One optimiser step whose rays are selected and built on the device from a resident
        ``loner_amd.rays.RayWindow`` (optimizer.py:363-424 + the step above).  This rank builds the
        window's slots [ray_offset, ray_offset + n_slots) (n_slots <= capacity, default the
        capacity).  When the window can produce invalid rays (``window.all_valid`` False) they are
        dropped as the reference drops them, which needs the batch size on the host: one
        synchronisation, only on such windows."""
        n = self.n_rays if n_slots is None else int(n_slots)
        if not 0 <= n <= self.n_rays or self.ray_offset + n > window.n_slots:
            raise ValueError(f"slots [{self.ray_offset}, {self.ray_offset + n}) outside the window "
                             f"({window.n_slots}) or the engine capacity ({self.n_rays})")
        if self.poses is not None and self.poses.window is not window:
            raise ValueError("step_window: the engine's PoseWindow belongs to another window (set_poses)")
        out = self._step_window_any(window, global_step, iteration_idx, n, n_rays_global, prof, kw)
        if self.poses is not None:
            # joint pose + map: the poses' Adam step on this step's gradient; the next build reads the new poses
            m = self._mark
            m(prof, "pose_adam")
            rays, slots = self._last_batch
            self.poses.step(self, rays, slots, self.lr_factor)  # (slots None: the engine's [ray_offset, + n))
            m(prof, "pose_adam")
        return out

    def _step_window_any(self, window, global_step, iteration_idx, n, n_rays_global, prof, kw):
        m = self._mark
        if window.all_valid and (self.poses is None or self.poses.stay_valid):
            out = self._step_window_pipelined(window, global_step, iteration_idx, n, n_rays_global, prof, kw)
            if self.poses is not None:
                self._last_batch = (self.rays[:n], None)
            return out
        # Windows with rays the 1 m filter drops: the batch size must reach the host (one sync per step).
        # The build and compaction of step k + 1 run on a side stream while step k runs, so that sync
        # never waits for the main stream: the host stays a step ahead of the GPU (double-buffered).
        main = torch.cuda.current_stream(self.state.device)
        want = (global_step, n, self.ray_offset, n_rays_global)
        pf, self._pf = self._pf, None
        if pf is not None:
            # a prefetch is consumed or discarded only after the main stream waits for it, so the
            # window it read (kept alive by pf["window"] until now) is free for reuse afterwards
            main.wait_event(pf["done"])
        if pf is None or pf["window"] is not window or pf["want"] != want:
            m(prof, "rays")
            pf = self._build_compact(window, global_step, n, n_rays_global, self._pf_parity, main)
            m(prof, "rays")
        self._pf_parity = pf["parity"]
        self._pf_fork.record(main)  # the other buffer is free once everything enqueued so far is done
        out = self.step(pf["rays"], pf["dgt"], global_step, iteration_idx, scale=window.scale, far_ref=pf["far"],
                        n_rays_global=pf["n_glob"], prof=prof, **kw)
        self.live_probe(pf["rays"].shape[0])
        if self.poses is not None:
            self._last_batch = (pf["rays"], pf["slots"])
            return out  # (no prefetch: the next build must read the poses this step's pose update writes)
        if self.prefetch:
            with torch.cuda.stream(self._pf_stream):
                self._pf_stream.wait_event(self._pf_fork)
                self._pf = self._build_compact(window, global_step + 1, n, n_rays_global, 1 - self._pf_parity,
                                               self._pf_stream)
        return out

    def _step_window_pipelined(self, window, global_step, iteration_idx, n, n_rays_global, prof, kw):
        """step_window for windows with no invalid rays (fixed batch size, no host sync), with step
        k + 1's build + sampling prefetched (``pipeline``)."""
        if (self.use_graph and prof is None and self.allreduce is None and not
                any(k in kw for k in ("u_jitter", "u_pdf", "noise", "presampled"))):
            return self._step_window_graph(window, global_step, iteration_idx, n, n_rays_global, kw)
        m = self._mark
        main = torch.cuda.current_stream(self.state.device)
        want = (global_step, n, self.ray_offset)
        pp, self._pp = self._pp, None
        if pp is not None:
            # consumed or discarded, the prefetch is waited for first: the main stream's later work
            # (and the caching allocator's reuse of the window it read, which pp["window"] kept alive
            # until here) is ordered after its side-stream reads
            main.wait_event(pp["done"])
        if pp is not None and pp["window"] is window and pp["want"] == want:
            parity, presampled = pp["parity"], pp["sampled"]
            b = self._pp_bufs[parity]
        else:
            parity, presampled = self._pp_parity, False
            b = self._pp_bufs[parity]
            m(prof, "rays")
            b.build(window, L.step_key(self.seed, global_step), self.ray_offset, n)
            m(prof, "rays")
        self._pp_parity = parity
        b.make_current(self)
        # the previous step's data-parallel OGM update (its SGD step, pending until the grid's next reader) lands
        # before the fork: the prefetch below samples the grid on the side stream after waiting on this fork only
        self._apply_pending_ogm()
        self._pp_fork.record(main)  # the other buffers are free once everything enqueued so far is done
        out = self.step(b.rays[:n], b.dgt[:n], global_step, iteration_idx, scale=window.scale, far_ref=b.far,
                        n_rays_global=window.n_slots if n_rays_global is None else n_rays_global, prof=prof,
                        presampled=presampled, **kw)
        self.live_probe(n)
        if not self.pipeline or prof is not None or "u_jitter" in kw or "u_pdf" in kw or self.poses is not None:
            return out  # (a profiled step keeps its stages apart; a pose step's update precedes the next build)
        bq = self._pp_bufs[1 - parity]
        key = L.step_key(self.seed, global_step + 1)
        # (the OGM sampler reads the grid step k may update)
        sample = self.cfg.sampler != "OGM" or not self._ogm_due(global_step, kw.get("update_ogm"))
        with torch.cuda.stream(self._pp_stream):
            self._pp_stream.wait_event(self._pp_fork)
            bq.build(window, key, self.ray_offset, n)
            if sample:
                self._sample(bq.rays[:n], n, bq.z, key, L.stream(self.state.device))
            done = torch.cuda.Event()
            done.record(self._pp_stream)
        self._pp = dict(window=window, want=(global_step + 1, n, self.ray_offset), parity=1 - parity, sampled=sample,
                        done=done)
        return out

    def drop_prefetch(self):
        """Discard a pending prefetch (the main stream waits for its side-stream work, then the window it
        read is released).  step_window does this itself when the next call does not match."""
        main = torch.cuda.current_stream(self.state.device)
        for pend in (self._pp, self._pf):
            if pend is not None:
                main.wait_event(pend["done"])
        self._pp = self._pf = None
        self.finish()

    def release(self):
        """End of a window: drop_prefetch(), and the HIP graphs captured for this window with the window
        itself (their captured pointers keep its device tensors alive), so two windows' resident data never
        coexist; a deferred early-ray-termination plan takes effect.  Optimizer calls it when a window's
        iterations are done."""
        self.drop_prefetch()
        self._graphs.clear()
        self._graph_window = None
        self.planner.adopt()

    def step_scalars(self, global_step, iteration_idx=0, adam_step=None):
        """The host ``lnr_step_scalars`` of a step: the values the eager step passes as kernel arguments
        (the same host arithmetic), for a captured step to read from device memory."""
        st, cfg = self.state, self.cfg
        sc = L.StepScalars()
        sc.key = L.step_key(self.seed, global_step)
        sc.los_lambda = float(cfg.loss.los_lambda_at(global_step))
        sc.los_eps = float(cfg.loss.los_eps_at(iteration_idx))
        t = st.adam_step + 1 if adam_step is None else adam_step
        a, b = L.ctypes.c_float(), L.ctypes.c_float()
        L.check(L.lib().lnr_adam_coefficients(t, self.map_lr(), *ADAM[:2], L.ctypes.byref(a), L.ctypes.byref(b)),
                "lnr_adam_coefficients")
        sc.adam_step_size, sc.adam_bc2_sqrt = a.value, b.value
        return sc

    def _step_window_graph(self, window, global_step, iteration_idx, n, n_rays_global, kw):
        """step_window as a replayed HIP graph (see __init__): the whole step, ray build included, on one stream.
        Graphs are captured per (OGM step or not, batch, backward) and per window: the first step of each runs
        eagerly with the device scalars (every kernel loaded; the step's own result) and is then captured without
        executing; later steps set their scalars (one small launch) and replay.  Bitwise the eager path
        (tests/test_gpu_rays.py::test_graph_replay_equals_eager).  (The next step's build + sampling as a forked
        branch of the graph measured slower than the single-stream graph at every fork point, round 5: DESIGN.md
        section 4d; removed in round 6, commit history before e32a0b7.)"""
        st = self.state
        if self._pp is not None or self._pf is not None:
            self.drop_prefetch()
        self.finish()
        ogm = bool(self._ogm_due(global_step, kw.get("update_ogm")))
        n_glob = window.n_slots if n_rays_global is None else n_rays_global
        if self._graph_window is not window:  # a new window: its tensors back the captured pointers
            self._graphs.clear()
            self._graph_window = window
            self.planner.adopt()
        p = self._pp_parity
        gkey = (p, ogm, n, self.ray_offset, n_glob, self.zero, self._live, self.pose_grad, self.planner.key())
        s = L.stream(st.device)
        sc = (L.StepScalars * 1)()
        sc[0] = self.step_scalars(global_step, iteration_idx)
        L.call("lnr_step_scalars_set", sc, 1, self.dev_step, s)
        b = self._pp_bufs[p]
        b.make_current(self)

        def body():
            b.build(window, sc[0].key, self.ray_offset, n, dev_step=self.dev_step)
            return self.step(b.rays[:n], b.dgt[:n], global_step, iteration_idx, scale=window.scale,
                             far_ref=b.far, n_rays_global=n_glob, update_ogm=ogm, dev_step=self.dev_step,
                             fork_count=False)

        g = self._graphs.get(gkey)
        if g is not None:
            g.replay()
            st.adam_step += 1
            self._r_last = n
            self.live_probe(n)
            return self.loss_out
        out = body()  # this step, eagerly
        saved = st.adam_step
        g = torch.cuda.CUDAGraph()
        cs = self._capture_stream
        cs.wait_stream(torch.cuda.current_stream(st.device))
        with torch.cuda.stream(cs):  # capture_begin / _end directly: no device sync, gc or cache flush
            g.capture_begin()  # (its own memory pool, which stays empty: the captured step allocates nothing)
            try:
                body()  # recorded, not executed
            finally:
                g.capture_end()
        torch.cuda.current_stream(st.device).wait_stream(cs)
        st.adam_step = saved
        self._graphs[gkey] = g
        self.live_probe(n)
        return out

    def _build_compact(self, window, global_step, n, n_rays_global, parity, stream):
        """Build slots [ray_offset, ray_offset + n) of ``window`` for ``global_step`` into ray buffer
        ``parity`` on ``stream`` and drop the invalid rays (order kept; one host sync on that stream);
        the global count is all-reduced when data-parallel."""
        b = self._pf_bufs[parity]
        with torch.cuda.stream(stream):
            b.build(window, L.step_key(self.seed, global_step), self.ray_offset, n)
            idx = torch.nonzero(b.valid[:n]).squeeze(1)
            k = int(idx.numel())  # (the sync)
            slots = idx + self.ray_offset  # (the window slots of the kept rays: the pose gradient's keyframes)
            torch.index_select(b.rays[:n], 0, idx, out=b.rays_c[:k])
            torch.index_select(b.dgt[:n], 0, idx, out=b.dgt_c[:k])
            cnt = torch.tensor([float(k)], device=self.state.device)
            if self.allreduce is not None:
                self.allreduce(cnt)
            n_glob = int(cnt.item())
            done = torch.cuda.Event()
            done.record(stream)
        return dict(window=window, want=(global_step, n, self.ray_offset, n_rays_global), rays=b.rays_c[:k],
                    dgt=b.dgt_c[:k], far=b.far, n_glob=n_glob, done=done, parity=parity, slots=slots)
