"""Mesh extraction from the trained map (the reference's analysis/mesher.py, without skimage or open3d).

    build_lidar_directions   the synthetic full-sweep direction grid (mesher.py:29-50)
    Mesher                   renders every skip_step-th pose's sweep through the sigma field with the training
                             sampler, max-accumulates the compositing weights into a voxel volume
                             (``lnr_volume_splat_max``, mesher.py:139-180) and extracts the level set with indexed
                             marching cubes (``lnr_marching_cubes_count`` / ``_emit``)
    marching_cubes           the two kernels with the scan between them (torch.cumsum), on a GPU volume
    splat_max_ref, marching_cubes_ref
                             numpy restatements of the kernels' semantics with the same table and ordering: the
                             tests' CPU oracle, and what a host without a GPU can run
    write_ply, read_ply      binary little-endian PLY, with vertex normals on request (``mesh_cloud.vertex_normals``);
                             the reader also takes Open3D's default output

Volume layout: the accumulated volume is the reference's flat ``results``: cell = x_buck * nz + y_buck * nx * nz +
z_buck, kept literally: the C-order index of an (ny, nx, nz) array; ``Mesher.volume()`` applies the reference's
reshape(ny, nx, nz).transpose(1, 0, 2).

Deviation: the reference's ``results[idx] = max(results[idx], w)`` keeps the LAST of the duplicate indices of a chunk;
the kernel keeps the true maximum (an integer atomic max on the bits of the non-negative weight), which is what the
line means and makes the volume independent of sample order and chunking.
"""
import numpy as np
import torch

from . import mc_table as T


# ---------------------------------------------------------------------------------------------- numpy restatements
def bucketize_ref(v, b):
    """torch.bucketize(v, b, right=False) of float32 values against float64 boundaries: the first i with b[i] >= v."""
    return np.searchsorted(np.asarray(b, np.float64), np.asarray(v, np.float32).astype(np.float64), side="left")


def splat_max_ref(rays, z, weights, depth, variance, bx, by, bz, depth_max, var_max=0.0, volume=None):
    """``lnr_volume_splat_max`` in numpy; returns the flat float32 volume (nx * ny * nz), accumulated into
    ``volume`` when given."""
    rays, z, w = np.asarray(rays, np.float32), np.asarray(z, np.float32), np.asarray(weights, np.float32)
    bx, by, bz = (np.asarray(b, np.float64) for b in (bx, by, bz))
    nx, ny, nz = len(bx), len(by), len(bz)
    vol = np.zeros(nx * ny * nz, np.float32) if volume is None else volume
    ok_ray = np.asarray(depth, np.float32) < np.float32(depth_max)
    if var_max > 0:
        ok_ray &= np.asarray(variance, np.float32) < np.float32(var_max)
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).astype(np.float32)  # o + d z, rounded per op
    ok = np.broadcast_to(ok_ray[:, None], z.shape) & (w > 0)
    idx = np.zeros(z.shape, np.int64)
    for a, (b, stride) in enumerate(((bx, nz), (by, nx * nz), (bz, 1))):
        p = pts[..., a].astype(np.float64)
        ok = ok & (p >= b[0]) & (p <= b[-1])
        idx += bucketize_ref(pts[..., a], b) * stride
    ok &= idx < vol.size
    np.maximum.at(vol, idx[ok], w[ok])
    return vol


def marching_cubes_ref(volume, level, spacing=(1.0, 1.0, 1.0)):
    """``lnr_marching_cubes_count`` + scan + ``_emit`` in numpy: volume (nx, ny, nz) -> verts (V, 3) float32 in grid
    units (index x spacing), faces (F, 3) int32.  Inside = value > level; the vertex of a crossed edge belongs to the
    voxel at the edge's lower end; vertex ids follow voxel order (ix ny + iy) nz + iz, then the axis; triangles
    follow the cell order, then the table's."""
    vol = np.ascontiguousarray(volume, np.float32)
    nx, ny, nz = vol.shape
    level = np.float32(level)
    sp = np.asarray(spacing, np.float32)
    inside = vol > level
    crossed = np.zeros((nx, ny, nz, 3), bool)
    crossed[:-1, :, :, 0] = inside[:-1] != inside[1:]
    crossed[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    crossed[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    own = np.argwhere(crossed)  # rows in (ix, iy, iz, axis) order: the vertex order
    n_verts = len(own)
    a = own[:, :3]
    b = a.copy()
    b[np.arange(n_verts), own[:, 3]] += 1
    fa, fb = vol[a[:, 0], a[:, 1], a[:, 2]], vol[b[:, 0], b[:, 1], b[:, 2]]
    with np.errstate(all="ignore"):
        t = (level - fa) / (fb - fa)
    verts = a.astype(np.float32) * sp
    verts[np.arange(n_verts), own[:, 3]] += t * sp[own[:, 3]]
    vid = np.full((nx, ny, nz, 3), -1, np.int64)
    vid[crossed] = np.arange(n_verts)
    if min(nx, ny, nz) < 2:
        return verts, np.zeros((0, 3), np.int32)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(T.CORNER):
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    cells = np.argwhere(T.TRI_COUNT[case] > 0)  # in cell order
    cfg = case[cells[:, 0], cells[:, 1], cells[:, 2]]
    n_tri = T.TRI_COUNT[cfg].astype(np.int64)
    start = np.cumsum(n_tri) - n_tri
    faces = np.zeros((int(n_tri.sum()), 3), np.int32)
    for k in range(T.MAX_TRIS):
        sel = n_tri > k
        for m in range(3):
            e = T.TRI_TABLE[cfg[sel], 3 * k + m].astype(np.int64)
            o = cells[sel] + T.EDGE_OFFSET[e]
            faces[start[sel] + k, m] = vid[o[:, 0], o[:, 1], o[:, 2], T.EDGE_AXIS[e]]
    assert (faces >= 0).all()
    return verts, faces


def sphere_volume(n=24, r=8.0):
    """The signed distance r - |p - c| of a sphere centred in an n^3 grid (the tests' analytic volume)."""
    g = np.arange(n, dtype=np.float32)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    c = np.float32((n - 1) / 2.0)
    return (np.float32(r) - np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)).astype(np.float32)


def case_histogram(volume, level):
    """How often each of the 256 corner configurations occurs among the volume's cells."""
    inside = np.asarray(volume) > level
    nx, ny, nz = inside.shape
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(T.CORNER):
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    return np.bincount(case.reshape(-1), minlength=256)


# ---------------------------------------------------------------------------------------------- PLY
def write_ply(path, vertices, faces, normals=None):
    """Binary little-endian PLY: float x, y, z (and nx, ny, nz when ``normals`` (V, 3) is given) per vertex; uchar 3 +
    int vertex_indices per face."""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), "<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), "<i4").reshape(-1, 3)
    names = "xyz"
    if normals is not None:
        n = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), "<f4").reshape(-1, 3)
        if len(n) != len(v):
            raise ValueError(f"write_ply: {len(n)} normals for {len(v)} vertices")
        v, names = np.ascontiguousarray(np.concatenate((v, n), axis=1)), ("x", "y", "z", "nx", "ny", "nz")
    rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"], rec["i"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\n" + "".join(f"property float {a}\n" for a in names) +
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4",
              "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """(vertices (V, 3) float32, faces (F, 3) int32, normals (V, 3) float32 or None) of a triangle-mesh PLY: what
    ``write_ply`` writes and Open3D's default output.  Format binary_little_endian or ascii; element vertex with
    float or double x y z, optional nx ny nz of either type and any further scalar properties (colours), which are
    skipped; element face with one ``list uchar int|uint vertex_indices`` of 3 per face.  Anything else raises
    ValueError naming the header line."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header")
    stop = raw.find(b"\n", end) if end >= 0 else -1
    if not raw.startswith(b"ply") or stop < 0:
        raise ValueError(f"read_ply: {path}: no PLY header")
    fmt, elements = None, []
    for line in raw[:stop].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info", "end_header"):
            continue
        bad = ValueError(f"read_ply: unsupported header line {line.strip()!r}")
        if w[0] == "format" and len(w) == 3 and w[1] in ("binary_little_endian", "ascii") and w[2] == "1.0":
            fmt = w[1]
        elif w[0] == "element" and len(w) == 3 and w[1] in ("vertex", "face") and w[2].isdigit() and \
                w[1] not in [e[0] for e in elements]:
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements and elements[-1][0] == "vertex" and len(w) == 3 and w[1] in _PLY_TYPES:
            if w[2] in ("x", "y", "z", "nx", "ny", "nz") and w[1] not in ("float", "float32", "double", "float64"):
                raise bad
            elements[-1][2].append((w[2], "<" + _PLY_TYPES[w[1]]))
        elif w[0] == "property" and elements and elements[-1][0] == "face" and len(w) == 5 and w[1] == "list" and \
                w[2] in ("uchar", "uint8") and w[3] in ("int", "int32", "uint", "uint32") and \
                w[4] in ("vertex_indices", "vertex_index") and not elements[-1][2]:
            elements[-1][2].append(("i", "<" + _PLY_TYPES[w[3]]))
        else:
            raise bad
    if fmt is None or [e[0] for e in elements] != ["vertex", "face"] or not elements[1][2]:
        raise ValueError(f"read_ply: {path}: the header needs a format line, then element vertex, then element face "
                         "with its vertex_indices")
    (_, nv, vprops), (_, nf, fprops) = elements
    names = [p[0] for p in vprops]
    if len(set(names)) != len(names) or not all(a in names for a in "xyz"):
        raise ValueError(f"read_ply: {path}: element vertex needs x, y, z once each, got {names}")
    has_normals = all(a in names for a in ("nx", "ny", "nz"))
    body = raw[stop + 1:]
    if fmt == "ascii":
        tok = body.split()
        if len(tok) < nv * len(names) + nf * 4:
            raise ValueError(f"read_ply: {path}: the data ends early")
        vt = np.array(tok[:nv * len(names)], dtype=np.float64).reshape(nv, len(names))
        col = {a: vt[:, k] for k, a in enumerate(names)}
        ft = np.array(tok[nv * len(names):nv * len(names) + nf * 4], dtype=np.int64).reshape(nf, 4)
        counts, idx = ft[:, 0], ft[:, 1:]
    else:
        vdt, fdt = np.dtype(vprops), np.dtype([("n", "u1"), ("i", fprops[0][1], (3,))])
        if len(body) < nv * vdt.itemsize + nf * fdt.itemsize:
            raise ValueError(f"read_ply: {path}: the data ends early")
        col = np.frombuffer(body, vdt, nv)
        frec = np.frombuffer(body, fdt, nf, nv * vdt.itemsize)
        counts, idx = frec["n"], frec["i"]
    if (counts != 3).any():
        raise ValueError(f"read_ply: {path}: a face is not a triangle")
    vertices = np.stack([col[a] for a in "xyz"], axis=1).astype(np.float32)
    normals = np.stack([col[a] for a in ("nx", "ny", "nz")], axis=1).astype(np.float32) if has_normals else None
    return vertices, np.ascontiguousarray(idx).astype(np.int32), normals


# ---------------------------------------------------------------------------------------------- directions
def build_lidar_directions(vertical_fov, vertical_resolution=0.25, horizontal_resolution=0.25):
    """The sweep of mesher.py:29-50 as sensor-frame unit directions (3, P) float32: elevations
    arange(fov[0], fov[1], vertical_resolution) degrees (outer), azimuths arange(0, 360, horizontal_resolution)."""
    elev = torch.arange(vertical_fov[0], vertical_fov[1], vertical_resolution).deg2rad()
    azim = torch.arange(0, 360, horizontal_resolution).deg2rad()
    polar = (torch.pi / 2 - elev).reshape(-1, 1).expand(-1, azim.numel()).reshape(-1)
    azim = azim.reshape(1, -1).expand(elev.numel(), -1).reshape(-1)
    return torch.stack((torch.cos(azim) * torch.sin(polar), torch.sin(azim) * torch.sin(polar),
                        torch.cos(polar))).to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------- GPU path
def marching_cubes(volume, level, spacing=(1.0, 1.0, 1.0), timer=None):
    """Indexed marching cubes of a contiguous float32 GPU volume (nx, ny, nz): verts (V, 3) float32 in grid
    units, faces (F, 3) int32, both on the device.  One host read (V, F) sizes the outputs."""
    from . import _lib as L
    if volume.dtype != torch.float32 or volume.dim() != 3:
        raise ValueError("marching_cubes: expected a float32 (nx, ny, nz) volume")
    timer = timer or _NoTimer()
    dev = volume.device
    nx, ny, nz = volume.shape
    s = L.stream(dev)
    counts = torch.empty(2, nx * ny * nz, dtype=torch.int32, device=dev)
    with timer("count"):
        L.call("lnr_marching_cubes_count", volume, nx, ny, nz, float(level), counts[0], counts[1], s)
    with timer("scan"):
        incl = torch.stack((torch.cumsum(counts[0], 0), torch.cumsum(counts[1], 0)))  # int64; 1-D scans
        offsets = incl - counts
        n_verts, n_faces = (int(v) for v in incl[:, -1].tolist())
    if n_verts >= 2 ** 31:
        raise RuntimeError(f"marching_cubes: {n_verts} vertices do not fit int32 face indices")
    verts = torch.empty(n_verts, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
    if n_verts and n_faces:
        with timer("emit"):
            L.call("lnr_marching_cubes_emit", volume, nx, ny, nz, float(level), float(spacing[0]), float(spacing[1]),
                   float(spacing[2]), offsets[0], offsets[1], n_verts, n_faces, verts, faces, s)
    return verts, faces


class _NoTimer:
    def __call__(self, name):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class StageTimer:
    """Device-event timing of named stages; ``times_ms()`` synchronises once and sums each stage's intervals."""

    def __init__(self):
        self.events = []

    def __call__(self, name):
        self._name = name
        return self

    def __enter__(self):
        self._start = torch.cuda.Event(enable_timing=True)
        self._start.record()
        return self

    def __exit__(self, *a):
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        self.events.append((self._name, self._start, end))
        return False

    def times_ms(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.events:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return out


class Mesher:
    """analysis/mesher.py's Mesher on a ``loner_amd.step.FieldState``.  ``poses``: the keyframes' lidar poses (4, 4),
    in order (the checkpoint's ``poses``); every ``skip_step``-th one is rendered.  The sweep is rendered as
    Model.forward(testing=False, return_variance=True) renders it: ``n_samples`` = the training sample count, the
    state's sampler with jitter (render.perturb), sigma noise on, 'default' compositing."""

    def __init__(self, state, poses, world_cube, ray_range, resolution=0.2,
                 marching_cubes_bound=((-40, 20), (0, 20), (-3, 15)), level_set=0, lidar_vertical_fov=(-22.5, 22.5),
                 n_samples=None, chunk=8192, vertical_resolution=0.25, horizontal_resolution=0.25, timer=None):
        self.state = state
        self.poses = [torch.as_tensor(p).detach().to("cpu", torch.float32) for p in poses]
        self.world_cube = world_cube
        self.ray_range = (float(ray_range[0]), float(ray_range[1]))
        self.resolution = float(resolution)
        self.marching_cubes_bound = np.array(marching_cubes_bound, np.float64)
        self.level_set = float(level_set)
        self.S = int(state.cfg.n_samples if n_samples is None else n_samples)
        if self.S % 64:
            raise ValueError(f"n_samples={self.S} must be a multiple of 64")
        self.chunk = int(chunk)
        self.timer = timer or _NoTimer()
        # float32 cube constants widened to float64, as numpy widens the reference's
        self.scale = float(np.float32(world_cube.scale_factor.reshape(-1)[0].item()))
        self.shift = world_cube.shift.reshape(-1).to(torch.float32).numpy().astype(np.float64)
        self.directions = build_lidar_directions(lidar_vertical_fov, vertical_resolution, horizontal_resolution)
        dev = state.device
        self.xyz = self.get_grid_uniform()
        if min(len(b) for b in self.xyz) < 3:
            raise ValueError("marching_cubes_bound / resolution gives fewer than 3 grid points on an axis")
        self.boundaries = [torch.from_numpy(b).to(dev) for b in self.xyz]
        nx, ny, nz = (len(b) for b in self.xyz)
        self.results = torch.zeros(nx * ny * nz, dtype=torch.float32, device=dev)
        self.z = torch.empty(self.chunk, self.S, dtype=torch.float32, device=dev)
        self.weights = torch.empty(self.chunk, self.S, dtype=torch.float32, device=dev)
        self.enc = torch.empty(state.cfg.n_levels, self.chunk * self.S, dtype=torch.int32, device=dev)
        self.n_rays = 0

    def get_grid_uniform(self):
        """The reference's grid (mesher.py:70-97): per axis linspace(bound_lo, bound_hi, int(length / resolution))
        in normalised units, float64."""
        bound = (self.marching_cubes_bound + self.shift[:, None]) / self.scale
        length = self.marching_cubes_bound[:, 1] - self.marching_cubes_bound[:, 0]
        num = (length / self.resolution).astype(int)
        return [np.linspace(bound[a, 0], bound[a, 1], num[a]) for a in range(3)]

    def accumulate(self, skip_step=15, var_threshold=None, key=0):
        """Render every skip_step-th pose's sweep and max-accumulate its weights into the volume."""
        from . import _lib as L
        from .evaluate import scan_window
        st = self.state
        cfg, dev = st.cfg, st.device
        s = L.stream(dev)
        S, stride = self.S, self.chunk * self.S
        depth_max = (self.ray_range[1] - 0.25) / self.scale
        var_max = 0.0 if var_threshold is None else float(var_threshold)
        if var_threshold is not None and var_max <= 0:
            raise ValueError("var_threshold must be positive (None: no variance test)")
        bx, by, bz = self.boundaries
        scan = dict(directions=self.directions, distances=torch.ones(self.directions.shape[1]))
        for k, pose in enumerate(self.poses[::skip_step]):
            with self.timer("rays"):
                win = scan_window(scan, pose, self.world_cube, self.ray_range, dev)
                rays, _, valid = win.build_all()
                if not win.all_valid:  # the reference drops rays that fail the 1 m filter (ray_utils.py:319-322)
                    rays = rays[valid.bool()].contiguous()
            R = rays.shape[0]
            self.n_rays += R
            pose_key = L.step_key(key, k)
            depth = torch.empty(R, dtype=torch.float32, device=dev)
            opacity = torch.empty(R, dtype=torch.float32, device=dev)
            variance = torch.empty(R, dtype=torch.float32, device=dev)
            for r0 in range(0, R, self.chunk):
                n = min(self.chunk, R - r0)
                rc = rays[r0:r0 + n]
                with self.timer("render"):
                    if cfg.sampler == "OGM":
                        L.call("lnr_sample_ogm", rc, n, S, st.occ, cfg.occ_res, cfg.perturb, None, None, pose_key, r0,
                               self.z, None, s)
                    else:
                        L.call("lnr_sample_uniform", rc, n, S, cfg.perturb, None, pose_key, r0, self.z, None, s)
                    L.call("lnr_hashgrid_fwd_rays", L.ctypes.byref(st.desc), rc, self.z, n, S, st.table_f16, self.enc,
                           stride, None, 0, s)
                    L.call("lnr_field_render", st.mlp_f16, self.enc, stride, rc, self.z, n, S, 0, cfg.raw_noise_std,
                           None, pose_key, r0, depth[r0:r0 + n], opacity[r0:r0 + n], variance[r0:r0 + n],
                           self.weights, s)
                with self.timer("splat"):
                    L.call("lnr_volume_splat_max", rc, self.z, self.weights, depth[r0:r0 + n], variance[r0:r0 + n], n,
                           S, bx, len(self.xyz[0]), by, len(self.xyz[1]), bz, len(self.xyz[2]), depth_max, var_max,
                           self.results, s)
        return self.results

    def reset(self):
        self.results.zero_()
        self.n_rays = 0

    def volume(self):
        """The (nx, ny, nz) volume: the reference's reshape(ny, nx, nz).transpose(1, 0, 2), contiguous."""
        nx, ny, nz = (len(b) for b in self.xyz)
        return self.results.reshape(ny, nx, nz).permute(1, 0, 2).contiguous()

    def spacing(self):
        return tuple(float(b[2] - b[1]) for b in self.xyz)  # mesher.py:197-199

    def to_world(self, verts):
        """Grid-unit vertices -> world metres (mesher.py:216-221), float64 arithmetic, float32 result."""
        origin = [float(b[0]) for b in self.xyz]
        if isinstance(verts, np.ndarray):
            return ((verts.astype(np.float64) + np.array(origin)) * self.scale - self.shift).astype(np.float32)
        o = torch.tensor(origin, dtype=torch.float64, device=verts.device)
        sh = torch.from_numpy(self.shift).to(verts.device)
        return ((verts.double() + o) * self.scale - sh).float()

    def extract(self):
        """Marching cubes of the accumulated volume -> (vertices (V, 3) float32 world metres, faces (F, 3) int32)."""
        with self.timer("transpose"):
            vol = self.volume()
        verts, faces = marching_cubes(vol, self.level_set, self.spacing(), self.timer)
        with self.timer("to_world"):
            verts = self.to_world(verts)
        return verts, faces

    def get_mesh(self, skip_step=15, var_threshold=None, key=0):
        """The reference's get_mesh: a fresh volume from every skip_step-th pose, then the level set."""
        self.reset()
        self.accumulate(skip_step, var_threshold, key)
        return self.extract()
