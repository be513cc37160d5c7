"""Mesh export of a trained field: what the reference's extract_mesh.py does with skimage.measure.marching_cubes and
plyfile, on the GPU (libngp_hip.so: ngp_mc_count / ngp_mc_emit, include/ngp_hip.h M1) and with a PLY writer of our
own.

  marching_cubes(volume, level, spacing, origin) -> verts (V,3) f32, faces (F,3) i32 on the volume's device
  extract_mesh(model, ...)                        -> the same for NGP.density sampled on a dense lattice
  write_ply(path, verts, faces, normals) / read_ply(path)

Triangles are wound so that (v1-v0) x (v2-v0) points toward lower density (out of the object).  Ambiguous cell faces
are resolved by one face-local rule (inside corners are separated), so closed surfaces come out as closed 2-manifolds;
the triangle order and the ambiguity choices are not skimage's (Lewiner) ones.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import call, call_host, check_input

_f32 = torch.float32


def _vec3(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().reshape(-1).tolist()
    v = [float(a) for a in v]
    if len(v) != 3:
        raise ValueError(f"expected 3 values, got {len(v)}")
    return v


def marching_cubes(volume, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """volume (nx, ny, nz) f32 CUDA tensor, C order (meshgrid indexing='ij') -> verts (V,3) f32, faces (F,3) int32,
    both on the volume's device.  Inside iff v > level (NaN and v == level are outside); a vertex on the lattice edge
    from idx along axis a lies at origin + (idx + t*e_a) * spacing, t = (level-v0)/(v1-v0) clamped to [0,1].
    Runs count -> emit on the current stream and reads the two totals back once (to size the outputs)."""
    check_input(volume, "volume")
    if volume.dtype != _f32 or volume.dim() != 3:
        raise ValueError(f"volume must be a 3-D float32 tensor, got {tuple(volume.shape)} {volume.dtype}")
    nx, ny, nz = volume.shape
    dev = volume.device
    spacing, origin = _vec3(spacing), _vec3(origin)
    if min(nx, ny, nz) < 2:
        return torch.empty(0, 3, dtype=_f32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev)
    n_ws = call_host("mc_workspace", nx, ny, nz)
    if n_ws < 0:
        raise ValueError(f"lattice {tuple(volume.shape)} has 2^31 points or more")
    ws = torch.empty(n_ws, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    call("mc_count", volume, nx, ny, nz, float(level), ws, totals)
    n_v, n_f = totals.tolist()
    if n_v < 0 or n_f < 0:
        raise RuntimeError(f"marching cubes on {tuple(volume.shape)}: more than 2^31-1 vertices or triangles")
    verts = torch.empty(n_v, 3, dtype=_f32, device=dev)
    faces = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    if n_v:
        call("mc_emit", volume, nx, ny, nz, float(level), (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), ws,
             verts, faces)
    return verts, faces


def lattice_axes(lo, hi, resolution, device):
    """the sample coordinates of each axis: torch.linspace(lo, hi, n), as the reference's extract_mesh.py"""
    n = (resolution,) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
    if len(n) != 3 or min(n) < 2:
        raise ValueError(f"resolution must be an int or 3 ints, each >= 2: {resolution}")
    return n, [torch.linspace(lo[a], hi[a], n[a], device=device) for a in range(3)]


def lattice_spacing(lo, hi, n, reference_spacing=False):
    """extent/(n-1) per axis (where linspace put the samples), or extent/n (the reference's extract_mesh.py)"""
    return [(hi[a] - lo[a]) / (n[a] if reference_spacing else n[a] - 1) for a in range(3)]


@torch.no_grad()
def density_volume(model, lo, hi, resolution=512, chunk=128 ** 3):
    """NGP.density(x, grad=False) (grid_fwd + mlp2_fwd) on the lattice linspace(lo, hi, n) per axis -> (nx, ny, nz)
    f32 on the model's device.  The points are made chunk by chunk on the device (never the whole lattice at once)."""
    dev = model.xyz_min.device
    n, axes = lattice_axes(lo, hi, resolution, dev)
    vol = torch.empty(n, dtype=_f32, device=dev)
    flat = vol.view(-1)
    nyz = n[1] * n[2]
    for s in range(0, flat.numel(), chunk):
        idx = torch.arange(s, min(s + chunk, flat.numel()), device=dev)
        i = idx // nyz
        r = idx - i * nyz
        j = r // n[2]
        pts = torch.stack((axes[0][i], axes[1][j], axes[2][r - j * n[2]]), -1)
        flat[s:s + pts.shape[0]] = model.density(pts, grad=False)
    return vol


@torch.no_grad()
def vertex_normals(model, verts, chunk=128 ** 3):
    """-grad(sigma)/|grad(sigma)| at each vertex through NGP.grad (the analytic gradient of the field), chunked;
    (0,0,0) where the gradient vanishes"""
    out = torch.empty_like(verts)
    for s in range(0, verts.shape[0], chunk):
        _, _, g = model.grad(verts[s:s + chunk].contiguous())
        out[s:s + chunk] = -torch.nn.functional.normalize(g, dim=-1)
    return out


def extract_mesh(model, xyz_min=None, xyz_max=None, resolution=512, level=10.0, chunk=128 ** 3, normals=False,
                 reference_spacing=False):
    """Mesh of the level set {sigma = level} of `model` (an NGP) -> verts (V,3), faces (F,3) [, normals (V,3)].

    The lattice spans [xyz_min, xyz_max] (default: the model's own box) with `resolution` (an int or (nx, ny, nz))
    points per axis at torch.linspace positions, i.e. a spacing of extent/(n-1); the density is evaluated in chunks of
    `chunk` points.  By default vertices lie where the density was sampled (origin xyz_min, spacing extent/(n-1)).

    reference_spacing=True reproduces the placement of the reference's extract_mesh.py: it samples at extent/(n-1) but
    hands skimage a spacing of extent/n, so its meshes are shrunk by (n-1)/n toward xyz_min (v_ref - lo =
    (v - lo) * (n-1)/n).  Its own call is xyz_min=(-1,-0.3,-1), xyz_max=(1,0.15,1), resolution=(512,128,512),
    level=10.

    normals=True adds per-vertex unit normals -grad(sigma)/|grad(sigma)| (pointing out of the object)."""
    lo = _vec3(model.xyz_min if xyz_min is None else xyz_min)
    hi = _vec3(model.xyz_max if xyz_max is None else xyz_max)
    vol = density_volume(model, lo, hi, resolution, chunk)
    verts, faces = marching_cubes(vol, level, lattice_spacing(lo, hi, vol.shape, reference_spacing), lo)
    if normals:
        return verts, faces, vertex_normals(model, verts, chunk)
    return verts, faces


# ---------------------------------------------------------------------------------------------------------------- PLY
def _ply_header(n_v, n_f, normals):
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else [])
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n_v}"]
    lines += [f"property float {p}" for p in props]
    lines += [f"element face {n_f}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


_FACE = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])   # 13 bytes per face, unaligned as in the file


def write_ply(path, verts, faces, normals=None):
    """binary little-endian PLY with the element / property names the reference writes through plyfile:
    vertex (float x y z [nx ny nz]), face (list uchar int vertex_indices)"""
    v = verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    v = v.astype("<f4").reshape(-1, 3)
    if normals is not None:
        nm = normals.detach().cpu().numpy() if isinstance(normals, torch.Tensor) else np.asarray(normals)
        v = np.concatenate([v, nm.astype("<f4").reshape(-1, 3)], 1)
    rec = np.empty(f.shape[0], _FACE)
    rec["n"] = 3
    rec["idx"] = f.reshape(-1, 3)
    with open(path, "wb") as fh:
        fh.write(_ply_header(v.shape[0], rec.shape[0], normals is not None))
        fh.write(np.ascontiguousarray(v).tobytes())
        fh.write(rec.tobytes())


def read_ply(path):
    """-> (verts (V,3) f32, faces (F,3) int32, normals (V,3) f32 or None) of a file write_ply wrote"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    if header[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    counts, props, elem = {}, [], None
    for line in header[2:-1]:
        w = line.split()
        if w[0] == "element":
            elem = w[1]
            counts[elem] = int(w[2])
        elif w[0] == "property" and elem == "vertex":
            if w[1] != "float":
                raise ValueError(f"{path}: vertex property {line!r} is not supported")
            props.append(w[2])
        elif w[0] == "property" and line != "property list uchar int vertex_indices":
            raise ValueError(f"{path}: face property {line!r} is not supported")
    n_v, n_f, k = counts["vertex"], counts["face"], len(props)
    v = np.frombuffer(data, "<f4", n_v * k, end).reshape(n_v, k)
    rec = np.frombuffer(data, _FACE, n_f, end + 4 * n_v * k)
    if n_f and (rec["n"] != 3).any():
        raise ValueError(f"{path}: only triangles are supported")
    nrm = v[:, 3:6].astype(np.float32) if props[3:6] == ["nx", "ny", "nz"] else None
    return v[:, :3].astype(np.float32), rec["idx"].astype(np.int32), nrm
