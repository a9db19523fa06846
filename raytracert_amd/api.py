"""Python mirror of the reference's render-path interface, over the C-ABI.

Reference names kept (CG_Project/raytracing.h): `init` -> Scene.load (raytracing.h:19),
`intersectMesh` -> Scene.intersect_mesh (raytracing.cpp:161), `performRayTracing` ->
Scene.perform_ray_tracing (raytracing.h:33), `getMaterial` -> Scene.get_material
(raytracing.h:27), the 'r' key -> Scene.render (main.cpp:340-411), `produceRay` corners ->
default_corners (main.cpp:300-325), `Image::writeImage` -> write_ppm (main.cpp:102-128).
Every call goes to librtamd.so; errors raise RtError with the library's message.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

from . import _capi
from ._capi import ALL_FEATURES, RT_HOST_ONLY, RtMaterial, RtParams, check, lib


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_corners(width: int, height: int) -> np.ndarray:
    """The 8 corner vectors produceRay yields for the default view (origin00, dest00, origin01,
    dest01, origin10, dest10, origin11, dest11)."""
    out = np.zeros((8, 3), np.float32)
    check(lib().rt_default_corners(width, height, _ptr(out)))
    return out


def write_ppm(path: str, rgb_u8: np.ndarray) -> None:
    rgb = np.ascontiguousarray(rgb_u8, np.uint8)
    h, w = rgb.shape[:2]
    check(lib().rt_write_ppm(path.encode(), w, h, _ptr(rgb)))


class PpmWriter:
    """rt_ppm_writer_*: result.ppm written after every frame (main.cpp:405), the file kept mapped and
    each frame's bytes copied in by `threads` threads; the file holds write_ppm's bytes."""

    def __init__(self, path: str, width: int, height: int, threads: int = 8):
        self._h = C.c_void_p()
        self.width, self.height = width, height
        check(lib().rt_ppm_writer_open(path.encode(), width, height, threads, C.byref(self._h)))

    def write_ptr(self, host_ptr: int) -> None:
        """The frame at a host address (e.g. a pinned torch tensor's data_ptr()), width*height*3 bytes."""
        check(lib().rt_ppm_writer_write(self._h, C.c_void_p(host_ptr)))

    def write(self, rgb_u8: np.ndarray) -> None:
        rgb = np.ascontiguousarray(rgb_u8, np.uint8)
        if rgb.size != self.width * self.height * 3:
            raise ValueError("frame size differs from the writer's")
        self.write_ptr(rgb.ctypes.data)

    def close(self) -> None:
        if self._h:
            lib().rt_ppm_writer_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class RenderParams:
    """Everything the reference reads from globals during a render (raytracing.cpp:15-29,
    raytracing.h:9-16). Defaults are the reference's own: pixelfactor 3, max_lvl 10, every
    feature on, one light at the camera position (0,0,4)."""
    width: int = 500
    height: int = 500
    pf: int = 3
    max_lvl: int = 10
    lights: Sequence[Sequence[float]] = ((0.0, 0.0, 4.0),)
    flags: int = ALL_FEATURES
    camera_pos: Sequence[float] = (0.0, 0.0, 4.0)
    corners: np.ndarray | None = field(default=None, repr=False)
    seed: int = _capi.DEFAULT_SEED   # RT_STOCHASTIC jitter seed (flags | STOCHASTIC)
    pfy: int | None = None           # pixelfactorY when it differs from pixelfactorX (= pf)

    def to_c(self) -> RtParams:
        """The C struct. Up to RT_MAX_LIGHTS lights go inline; more go through light_list, a float32
        array kept alive on the returned struct (the reference's light list is unbounded)."""
        n = len(self.lights)
        if n > _capi.RT_LIGHTS_LIMIT:
            raise ValueError(f"at most {_capi.RT_LIGHTS_LIMIT} lights")
        p = RtParams()
        p.width, p.height, p.pfx, p.pfy = self.width, self.height, self.pf, self.pf if self.pfy is None else self.pfy
        p.max_lvl, p.flags, p.n_lights = self.max_lvl, self.flags, n
        p.seed = int(self.seed)
        for i, l in enumerate(self.lights[:_capi.RT_MAX_LIGHTS]):
            for k in range(3):
                p.lights[i][k] = float(l[k])
        if n > _capi.RT_MAX_LIGHTS:
            arr = np.ascontiguousarray(np.asarray(self.lights, np.float32).reshape(n, 3))
            p._light_list_keepalive = arr
            p.light_list = arr.ctypes.data
        for k in range(3):
            p.camera_pos[k] = float(self.camera_pos[k])
        cs = default_corners(self.width, self.height) if self.corners is None else np.asarray(self.corners, np.float32)
        for i in range(8):
            for k in range(3):
                p.corners[i][k] = float(cs[i, k])
        return p


def _builder_id(name) -> int:
    if isinstance(name, str):
        if name not in _capi.BUILDERS:
            raise ValueError(f"unknown builder {name!r} (one of {_capi.BUILDERS})")
        return _capi.BUILDERS.index(name)
    return int(name)


class Scene:
    """A loaded mesh bound to one GPU (or host-only with device=-1)."""

    def __init__(self, handle: C.c_void_p, device: int):
        self._h = handle
        self.device = device

    # -- construction ------------------------------------------------------------------------
    @classmethod
    def load(cls, path: str, device: int = 0, sequential: bool = False, threads: int = 0,
             texcoords: bool = False) -> "Scene":
        """init(fileName): Mesh::loadMesh + loadMtl + calculateNormals. The default parser is
        parallel (threads=0: automatic); sequential=True runs the line-by-line restatement (same
        result); texcoords=True also keeps Mesh::texcoords / Triangle::t (Scene.texcoords())."""
        h = C.c_void_p()
        flags = _capi.LOAD_SEQUENTIAL if sequential else (_capi.LOAD_PARALLEL | (int(threads) << 8))
        if texcoords:
            flags |= _capi.LOAD_TEXCOORDS
        check(lib().rt_scene_load_obj_ex(path.encode(), device, flags, C.byref(h)))
        return cls(h, device)

    @classmethod
    def create(cls, vertices, triangles, tri_mat, materials: Sequence[dict], device: int = 0,
               builder: str = "sah") -> "Scene":
        """rt_scene_create_ex. builder 'sah' (the host's binned-SAH build, the default), 'lbvh' (a
        Morton-order radix tree; on a device scene built by HIP kernels with no host build) or 'cluster'
        (the same leaf order, merged by the surface area of the union box; built the same way)."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        m = np.ascontiguousarray(tri_mat, np.uint32).reshape(-1)
        mats = (RtMaterial * len(materials))()
        for i, d in enumerate(materials):
            for k in range(3):
                mats[i].Kd[k] = d.get("Kd", (0, 0, 0))[k]
                mats[i].Ka[k] = d.get("Ka", (0, 0, 0))[k]
                mats[i].Ks[k] = d.get("Ks", (0, 0, 0))[k]
            mats[i].Ns, mats[i].Ni, mats[i].Tr = d.get("Ns", 0.0), d.get("Ni", 0.0), d.get("Tr", 0.0)
            mats[i].illum, mats[i].flags = d.get("illum", 0), d.get("flags", 0)
        h = C.c_void_p()
        check(lib().rt_scene_create_ex(_ptr(v), len(v), _ptr(t), _ptr(m), len(m), C.cast(mats, C.c_void_p),
                                       len(materials), device, _builder_id(builder), C.byref(h)))
        return cls(h, device)

    def set_builder(self, name: str) -> None:
        """rt_scene_set_builder: the builder of the scene's later builds ('sah', 'lbvh' or 'cluster'); rebuilds nothing."""
        check(lib().rt_scene_set_builder(self._h, _builder_id(name)))

    @property
    def builder(self) -> tuple[str, str]:
        """(selected, built_with): the chosen builder and the one that built the trees the scene holds."""
        sel, built = C.c_int32(), C.c_int32()
        check(lib().rt_scene_get_builder(self._h, C.byref(sel), C.byref(built)))
        return _capi.BUILDERS[sel.value], _capi.BUILDERS[built.value]

    def build_info(self) -> dict:
        """rt_scene_build_info: how the current trees were built (built_with, the clustering iterations,
        the reason of the last fallback from 'cluster', its radius / tail threshold / iteration budget) and
        the binary tree's cost (child half-areas over the root's), for any builder."""
        info = (C.c_int32 * _capi.BUILD_INFO_FIELDS)()
        cost = C.c_double()
        check(lib().rt_scene_build_info(self._h, info, C.byref(cost)))
        return dict(built_with=_capi.BUILDERS[info[0]], iterations=info[1], fallback=_capi.FALLBACK_REASONS[info[2]],
                    radius=info[3], tail=info[4], max_iterations=info[5], cost=cost.value)

    def close(self) -> None:
        if self._h:
            lib().rt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    # -- inspection --------------------------------------------------------------------------
    def counts(self) -> tuple[int, int, int]:
        nv, nt, nm = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().rt_scene_info(self._h, C.byref(nv), C.byref(nt), C.byref(nm)))
        return nv.value, nt.value, nm.value

    def export(self) -> dict:
        nv, nt, nm = self.counts()
        verts = np.zeros((nv, 3), np.float32)
        tri = np.zeros((nt, 3), np.uint32)
        tmat = np.zeros(nt, np.uint32)
        normals = np.zeros((nt, 3), np.float32)
        mats = (RtMaterial * max(nm, 1))()
        check(lib().rt_scene_export(self._h, _ptr(verts), _ptr(tri), _ptr(tmat), C.cast(mats, C.c_void_p), _ptr(normals)))
        mat_list = [dict(Kd=tuple(m.Kd), Ka=tuple(m.Ka), Ks=tuple(m.Ks), Ns=m.Ns, Ni=m.Ni, Tr=m.Tr,
                         illum=m.illum, flags=m.flags) for m in list(mats)[:nm]]
        return dict(vertices=verts, triangles=tri, tri_mat=tmat, materials=mat_list, normals=normals)

    def update_vertices(self, vertices, mode: str = "auto") -> str:
        """rt_scene_update_vertices: new positions for the scene's vertices (dynamic geometry). `vertices`
        is a float32 (n, 3) array, or a CUDA torch tensor of that shape on the scene's device, which goes
        through rt_scene_update_vertices_device with no host copy. mode 'auto' refits the BVH and rebuilds
        it only if some triangle changed class; 'rebuild' always rebuilds. Returns 'refit', 'rebuilt' (the
        host SAH build), 'rebuilt_lbvh' (the Morton-order builder, see set_builder) or 'rebuilt_cluster';
        either way the scene then behaves bit for bit as one created from the new vertices."""
        m = {"auto": _capi.UPDATE_AUTO, "rebuild": _capi.UPDATE_REBUILD}.get(mode, mode)
        out = C.c_int32(-1)
        if hasattr(vertices, "data_ptr") and getattr(vertices, "is_cuda", False):
            import torch
            if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
                raise ValueError("update_vertices: a float32 (n, 3) tensor is required")
            t = vertices.contiguous()
            torch.cuda.current_stream(t.device).synchronize()   # the library reads it on its own stream
            check(lib().rt_scene_update_vertices_device(self._h, C.c_void_p(t.data_ptr()), int(t.shape[0]), int(m), C.byref(out)))
        else:
            v = np.ascontiguousarray(vertices, np.float32)
            if v.ndim != 2 or v.shape[1] != 3:
                raise ValueError("update_vertices: a float32 (n, 3) array is required")
            check(lib().rt_scene_update_vertices(self._h, _ptr(v), len(v), int(m), C.byref(out)))
        return {_capi.UPDATED_REFIT: "refit", _capi.UPDATED_REBUILT_LBVH: "rebuilt_lbvh",
                _capi.UPDATED_REBUILT_CLUSTER: "rebuilt_cluster"}.get(out.value, "rebuilt")

    def set_mesh(self, vertices, triangles, tri_mat, counts=None) -> str:
        """rt_scene_set_mesh: replace the scene's vertices, triangles and triangle materials (the counts may
        change; the material table, builder and tuning stay; texture coordinates are dropped). NumPy arrays
        (float32 (nv, 3), uint32 (nt, 3), uint32 (nt,)) go through the host entry. Contiguous torch CUDA
        tensors on the scene's device (float32; int32 or uint32 read as 32-bit words) go through
        rt_scene_set_mesh_device with no host copy; `counts` is then an optional int32 CUDA tensor
        {live vertices, live triangles}, the tensors' sizes being capacities. Returns the builder that made
        the new trees as update_vertices does ('rebuilt', 'rebuilt_lbvh' or 'rebuilt_cluster'); the scene then
        behaves bit for bit as one created from the same arrays."""
        out = C.c_int32(-1)
        if any(hasattr(a, "data_ptr") for a in (vertices, triangles, tri_mat)):
            import torch
            words = (torch.int32, getattr(torch, "uint32", torch.int32))
            for what, t, dtypes, tail in (("vertices", vertices, (torch.float32,), (3,)), ("triangles", triangles, words, (3,)),
                                          ("tri_mat", tri_mat, words, ())):
                if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device:
                    raise ValueError(f"set_mesh: {what} must be a CUDA torch tensor on the scene's device {self.device}")
                if t.dtype not in dtypes or tuple(t.shape[1:]) != tail or t.dim() != 1 + len(tail):
                    raise ValueError(f"set_mesh: {what} must be {dtypes[0]} of shape (n,{' 3' if tail else ''}), "
                                     f"not {t.dtype} {tuple(t.shape)}")
                if not t.is_contiguous():
                    raise ValueError(f"set_mesh: {what} must be contiguous")
            if triangles.shape[0] != tri_mat.shape[0]:
                raise ValueError("set_mesh: triangles and tri_mat differ in length")
            cnt = None
            if counts is not None:
                if (not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype != torch.int32
                        or counts.numel() != 2 or not counts.is_contiguous() or counts.device.index != self.device):
                    raise ValueError("set_mesh: counts must be a CUDA int32 tensor of two elements on the scene's device")
                cnt = C.c_void_p(counts.data_ptr())
            torch.cuda.current_stream(vertices.device).synchronize()   # the library reads them on its own stream
            check(lib().rt_scene_set_mesh_device(self._h, C.c_void_p(vertices.data_ptr()), int(vertices.shape[0]),
                                                 C.c_void_p(triangles.data_ptr()), C.c_void_p(tri_mat.data_ptr()),
                                                 int(triangles.shape[0]), cnt, C.byref(out)))
        else:
            if counts is not None:
                raise ValueError("set_mesh: counts goes with CUDA tensors (host arrays carry their own sizes)")
            v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
            t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
            m = np.ascontiguousarray(tri_mat, np.uint32).reshape(-1)
            if len(t) != len(m):
                raise ValueError("set_mesh: triangles and tri_mat differ in length")
            check(lib().rt_scene_set_mesh(self._h, _ptr(v), len(v), _ptr(t), _ptr(m), len(m), C.byref(out)))
        return {_capi.UPDATED_REBUILT_LBVH: "rebuilt_lbvh", _capi.UPDATED_REBUILT_CLUSTER: "rebuilt_cluster"}.get(out.value, "rebuilt")

    def texcoords(self) -> tuple[np.ndarray, np.ndarray]:
        """rt_scene_texcoords (a scene loaded with texcoords=True): (texcoords[n, 3] float32 with z = 0,
        tri_t[nt, 3] uint32), Mesh::texcoords and each Triangle::t."""
        n = C.c_int32()
        check(lib().rt_scene_texcoords(self._h, C.byref(n), None, None))
        tc = np.zeros((n.value, 3), np.float32)
        tt = np.zeros((self.counts()[1], 3), np.uint32)
        check(lib().rt_scene_texcoords(self._h, C.byref(n), _ptr(tc), _ptr(tt)))
        return tc, tt

    def get_material(self, triangle_index: int) -> dict:
        m = RtMaterial()
        check(lib().rt_get_material(self._h, triangle_index, C.byref(m)))
        return dict(Kd=tuple(m.Kd), Ka=tuple(m.Ka), Ks=tuple(m.Ks), Ns=m.Ns, Ni=m.Ni, Tr=m.Tr,
                    illum=m.illum, flags=m.flags)

    # -- hot path ----------------------------------------------------------------------------
    def intersect_mesh(self, origins, dests):
        """Batched intersectMesh: returns (index[n] int32, point[n,3] float32)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dests, np.float32).reshape(-1, 3)
        n = len(o)
        idx = np.zeros(n, np.int32)
        pts = np.zeros((n, 3), np.float32)
        check(lib().rt_intersect_mesh(self._h, _ptr(o), _ptr(d), n, _ptr(idx), _ptr(pts)))
        return idx, pts

    def perform_ray_tracing(self, params: RenderParams, origins, dests):
        """Batched performRayTracing: returns (rgb[n,3] float32 unclamped, counts[3])."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dests, np.float32).reshape(-1, 3)
        n = len(o)
        rgb = np.zeros((n, 3), np.float32)
        counts = np.zeros(3, np.uint64)
        p = params.to_c()
        check(lib().rt_trace_rays(self._h, C.byref(p), _ptr(o), _ptr(d), n, _ptr(rgb), _ptr(counts)))
        return rgb, counts

    # -- device-resident queries (rays and results are torch CUDA tensors; stream-ordered, no host sync) ----
    @staticmethod
    def _instead(host_method) -> str:
        return "there is no host method" if host_method is None else f"host arrays go through {host_method}"

    def _device_rays(self, name: str, host_method, origins, dests, names=("origins", "dests"), inner: tuple = ()):
        """Checks before anything touches a device: (n, stride) of two contiguous CUDA float32 tensors (n,) + inner +
        (3 or 4,) of one shape on the scene's device: two ray arrays, or one tensor given twice (the points; the query
        triangles with inner (3,)), which is then checked once."""
        import torch
        pair = dests is not origins
        for what, t in zip(names, (origins, dests)) if pair else ((names[0], origins),):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name}: {what} must be a CUDA torch tensor ({self._instead(host_method)})")
            if t.dtype != torch.float32:
                raise ValueError(f"{name}: {what} must be float32, not {t.dtype}")
            if (t.dim() != 2 + len(inner) or t.shape[-1] not in (_capi.RAYS_PACKED, _capi.RAYS_PADDED)
                    or (inner and t.shape[1:-1] != inner)):
                mid = "".join(f"{m}, " for m in inner)
                raise ValueError(f"{name}: {what} must have shape (n, {mid}3) or (n, {mid}4), not {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{name}: {what} must be contiguous")
            if not t.is_cuda:
                raise ValueError(f"{name}: {what} is a CPU tensor ({self._instead(host_method)})")
            if t.device.index != self.device:
                raise ValueError(f"{name}: {what} is on {t.device}, the scene on device {self.device}")
        if pair and origins.shape != dests.shape:
            raise ValueError(f"{name}: origins {tuple(origins.shape)} and dests {tuple(dests.shape)} differ in shape")
        return int(origins.shape[0]), int(origins.shape[-1])

    def _device_count(self, name: str, count):
        if count is None:
            return None
        import torch
        if (not isinstance(count, torch.Tensor) or not count.is_cuda or count.dtype != torch.int32 or count.numel() != 1
                or count.device.index != self.device):
            raise ValueError(f"{name}: count must be a CUDA int32 tensor of one element on the scene's device")
        return C.c_void_p(count.data_ptr())

    def _device_out(self, name: str, out, n: int, dtype, tail: tuple, fill, counted: bool):
        """The result tensor: `out` checked (it may hold more than n rows; only the first n are the
        result), or a new one, filled first when a device count may leave entries unwritten."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            shape = (n,) + tail
            return torch.full(shape, fill, dtype=dtype, device=dev) if counted else torch.empty(shape, dtype=dtype, device=dev)
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.device or out.dtype != dtype
                or not out.is_contiguous() or out.dim() != 1 + len(tail) or tuple(out.shape[1:]) != tail or out.shape[0] < n):
            raise ValueError(f"{name}: out must be a contiguous CUDA {dtype} tensor of shape (>= {n},) + {tail} on the scene's device")
        return out

    def _stream_ptr(self, stream):
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        s = getattr(stream, "cuda_stream", stream)
        return C.c_void_p(int(s)) if s else None

    def intersect_mesh_device(self, origins, dests, count=None, out=None, stream=None):
        """rt_intersect_mesh_device: intersectMesh for rays born on the GPU. origins / dests are contiguous
        CUDA float32 tensors on the scene's device, (n, 3) or (n, 4) (w ignored); count an optional CUDA int32
        tensor of one element, read by the kernel (live rays = clamp(count, 0, n); the rest is not written);
        out an optional (index, point) pair to write into (rows past n are left alone). Returns (index[n]
        int32, point[n, 3] float32) CUDA tensors, rt_intersect_mesh's values bit for bit. Stream-ordered on
        `stream` (a torch stream or its cuda_stream; default: the current stream): nothing is synchronised.
        With a stream other than the one the tensors were made on, keeping them alive and ordered is the
        caller's business (Tensor.record_stream)."""
        import torch
        name = "intersect_mesh_device"
        n, stride = self._device_rays(name, "intersect_mesh", origins, dests)
        cnt = self._device_count(name, count)
        out_idx, out_pts = self._out_parts(name, out, 2, "out must be an (index, point) pair")
        idx = self._device_out(name, out_idx, n, torch.int32, (), -1, count is not None)
        pts = self._device_out(name, out_pts, n, torch.float32, (3,), 0.0, count is not None)
        check(lib().rt_intersect_mesh_device(self._h, C.c_void_p(origins.data_ptr()), C.c_void_p(dests.data_ptr()), stride, n,
                                             cnt, C.c_void_p(idx.data_ptr()), C.c_void_p(pts.data_ptr()), self._stream_ptr(stream)))
        return idx[:n], pts[:n]

    def occluded_device(self, origins, dests, count=None, out=None, stream=None):
        """rt_occluded_device: isShadow's verdict for the given rays (arguments as intersect_mesh_device).
        Returns blocked[n] uint8: 1 when the ray's closest hit exists and its material is not transparent,
        else 0. No offset is added to the origins."""
        import torch
        name = "occluded_device"
        n, stride = self._device_rays(name, "intersect_mesh", origins, dests)
        cnt = self._device_count(name, count)
        blocked = self._device_out(name, out, n, torch.uint8, (), 0, count is not None)
        check(lib().rt_occluded_device(self._h, C.c_void_p(origins.data_ptr()), C.c_void_p(dests.data_ptr()), stride, n, cnt,
                                       C.c_void_p(blocked.data_ptr()), self._stream_ptr(stream)))
        return blocked[:n]

    def _device_vector(self, name: str, what: str, t, n: int, dtype):
        """A per-query input (tmin, tmax, rmax: float32; after, self_index: int32): None, or a contiguous CUDA tensor
        of n (or more) elements."""
        if t is None:
            return None
        import torch
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device or t.dtype != dtype
                or t.dim() != 1 or not t.is_contiguous() or t.shape[0] < n):
            raise ValueError(f"{name}: {what} must be a contiguous CUDA {str(dtype).split('.')[-1]} tensor of shape (>= {n},) "
                             f"on the scene's device")
        return C.c_void_p(t.data_ptr())

    @staticmethod
    def _list_length(name: str, k) -> None:
        if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > _capi.MULTI_HIT_MAX:
            raise ValueError(f"{name}: k must be an int in [1, {_capi.MULTI_HIT_MAX}], not {k!r}")

    @staticmethod
    def _out_parts(name: str, out, m: int, must: str) -> tuple:
        """`out` as its m parts (None each without it). must: what it has to be, in the method's words."""
        if out is None:
            return (None,) * m
        if not isinstance(out, (tuple, list)) or len(out) != m:
            raise ValueError(f"{name}: {must}")
        return tuple(out)

    def _device_records(self, name: str, out, n: int, tail: tuple, fill: bool):
        """The rt_hit record tensor, (n,) + tail int32 with tail (4,) or (k, 4): `out` checked or a new one, 16-byte
        aligned. fill: a device count may leave entries unwritten, which then hold the miss record. Returns it with
        the (triangle, distance, st) views of its first n records."""
        import torch
        rec = self._device_out(name, out, n, torch.int32, tail, 0, False)
        if fill:
            rec[..., 0], rec[..., 1], rec[..., 2:] = -1, 0x7F800000, 0      # (device fills: no host copy)
        if rec.data_ptr() % _capi.HIT_BYTES:
            raise ValueError(f"{name}: the record tensor must be 16-byte aligned")
        f = rec[:n].view(torch.float32)
        return rec, (rec[:n, ..., 0], f[..., 1], f[..., 2:4])

    def closest_hit_device(self, origins, dests, tmin=None, tmax=None, to_dest: bool = False, count=None, out=None,
                           want_points: bool = False, stream=None):
        """rt_closest_hit_range_device: per ray, the closest accepted triangle whose distance lies in [tmin, tmax),
        with that distance and the reference's s, t of the hit. Rays, count and stream as intersect_mesh_device.
        tmin / tmax: optional CUDA float32 tensors of n elements (defaults 0 and +inf; with to_dest and no tmax,
        the ray's own length, so only hits between origin and dest count). A NaN bound, tmax <= 0 or tmin >= tmax
        is an empty range: a miss. Returns (triangle[n] int32, distance[n] float32, st[n, 2] float32), views of
        one (n, 4) int32 record tensor (rt_hit: a miss is -1, +inf, 0, 0), and with want_points also point[n, 3].
        out: that (>= n, 4) int32 record tensor to write into, or with want_points a (records, points) pair.
        With tmin = tmax = None and to_dest False, triangle and point are intersect_mesh_device's bits;
        tmin = torch.nextafter(distance, inf) steps each ray to its next distance; that skips every other accepted
        triangle at the previous distance (duplicated or coincident geometry), which multi_hit_device does not."""
        import torch
        name = "closest_hit_device"
        n, stride = self._device_rays(name, "intersect_mesh", origins, dests)
        cnt = self._device_count(name, count)
        lo, hi = self._device_vector(name, "tmin", tmin, n, torch.float32), self._device_vector(name, "tmax", tmax, n, torch.float32)
        out_rec, out_pts = self._out_parts(name, out, 2, "with want_points, out must be a (records, points) pair") if want_points else (out, None)
        rec, res = self._device_records(name, out_rec, n, (4,), out_rec is None and count is not None)
        pts = self._device_out(name, out_pts, n, torch.float32, (3,), 0.0, count is not None) if want_points else None
        check(lib().rt_closest_hit_range_device(self._h, C.c_void_p(origins.data_ptr()), C.c_void_p(dests.data_ptr()), stride, n, cnt,
                                                lo, hi, _capi.RANGE_TO_DEST if to_dest else 0, C.c_void_p(rec.data_ptr()),
                                                None if pts is None else C.c_void_p(pts.data_ptr()), self._stream_ptr(stream)))
        return res + (pts[:n],) if want_points else res

    def multi_hit_device(self, origins, dests, k: int, tmin=None, tmax=None, to_dest: bool = False, count_all: bool = False,
                         count=None, out=None, stream=None):
        """rt_multi_hit_range_device: per ray, the first k (1.._capi.MULTI_HIT_MAX) accepted triangles whose distance
        lies in [tmin, tmax), in ascending (distance, index) order, from one walk. Rays, bounds, to_dest, count and
        stream as closest_hit_device. Returns (triangle[n, k] int32, distance[n, k] float32, st[n, k, 2] float32,
        nhits[n] int32): the first three are views of one (n, k, 4) int32 record tensor whose rows past a ray's
        hits are the miss record (-1, +inf, 0, 0); nhits is the number of rows that hold a hit, or with count_all
        the number of in-range accepted triangles (which may exceed k). Triangles at one distance all appear,
        lowest index first. out: a (records, nhits) pair to write into, (>= n, k, 4) int32 and (>= n,) int32."""
        import torch
        name = "multi_hit_device"
        self._list_length(name, k)
        n, stride = self._device_rays(name, "intersect_mesh", origins, dests)
        cnt = self._device_count(name, count)
        lo, hi = self._device_vector(name, "tmin", tmin, n, torch.float32), self._device_vector(name, "tmax", tmax, n, torch.float32)
        out_rec, out_nh = self._out_parts(name, out, 2, "out must be a (records, nhits) pair")
        rec, res = self._device_records(name, out_rec, n, (k, 4), out is None and count is not None)
        nh = self._device_out(name, out_nh, n, torch.int32, (), 0, count is not None)
        flags = (_capi.RANGE_TO_DEST if to_dest else 0) | (_capi.MULTI_COUNT_ALL if count_all else 0)
        check(lib().rt_multi_hit_range_device(self._h, C.c_void_p(origins.data_ptr()), C.c_void_p(dests.data_ptr()), stride, n, cnt,
                                              lo, hi, flags, k, C.c_void_p(rec.data_ptr()), C.c_void_p(nh.data_ptr()),
                                              self._stream_ptr(stream)))
        return res + (nh[:n],)

    def closest_point_device(self, points, rmax=None, count=None, out=None, want_points: bool = False, stream=None):
        """rt_closest_point_device: per query point, the nearest point of the mesh (include/raytracert.h states the
        arithmetic). points: a contiguous CUDA float32 tensor on the scene's device, (n, 3) or (n, 4) (w ignored);
        rmax: an optional CUDA float32 tensor of n search radii (a NaN, zero or negative radius is a miss); count
        and stream as intersect_mesh_device. Returns (triangle[n] int32, distance[n] float32, st[n, 2] float32),
        views of one (n, 4) int32 record tensor (rt_hit: a miss is -1, +inf, 0, 0), and with want_points also
        point[n, 3], the closest point V0 + s (V1 - V0) + t (V2 - V0) or (0, 0, 0). out: that (>= n, 4) int32
        record tensor to write into, or with want_points a (records, points) pair."""
        import torch
        name = "closest_point_device"
        n, stride = self._device_rays(name, "closest_point", points, points, ("points", "points"))
        cnt = self._device_count(name, count)
        rad = self._device_vector(name, "rmax", rmax, n, torch.float32)
        out_rec, out_pts = self._out_parts(name, out, 2, "with want_points, out must be a (records, points) pair") if want_points else (out, None)
        rec, res = self._device_records(name, out_rec, n, (4,), out_rec is None and count is not None)
        pts = self._device_out(name, out_pts, n, torch.float32, (3,), 0.0, count is not None) if want_points else None
        check(lib().rt_closest_point_device(self._h, C.c_void_p(points.data_ptr()), stride, n, cnt, rad, 0, C.c_void_p(rec.data_ptr()),
                                            None if pts is None else C.c_void_p(pts.data_ptr()), self._stream_ptr(stream)))
        return res + (pts[:n],) if want_points else res

    def nearest_triangles_device(self, points, k: int, rmax=None, count_all: bool = False, count=None, out=None,
                                 want_points: bool = False, stream=None):
        """rt_nearest_triangles_device: per query point, the k (1.._capi.MULTI_HIT_MAX) nearest candidate triangles
        inside the point's radius, in ascending (squared distance, index) order, from one walk. points, rmax, count
        and stream as closest_point_device. Returns (triangle[n, k] int32, distance[n, k] float32, st[n, k, 2] float32,
        nfound[n] int32) and with want_points also point[n, k, 3]: the first three are views of one (n, k, 4) int32
        record tensor whose rows past a point's triangles are the miss record (-1, +inf, 0, 0), with the point
        (0, 0, 0); nfound is the number of rows that hold a triangle, or with count_all the number of candidates
        inside the radius (which may exceed k). Triangles at one distance all appear, lowest index first; k = 1 is
        closest_point_device's record. out: a (records, nfound) pair to write into, (>= n, k, 4) int32 and (>= n,)
        int32, or with want_points a (records, nfound, points) triple with (>= n, k, 3) float32."""
        import torch
        name = "nearest_triangles_device"
        self._list_length(name, k)
        n, stride = self._device_rays(name, "closest_point", points, points, ("points", "points"))
        cnt = self._device_count(name, count)
        rad = self._device_vector(name, "rmax", rmax, n, torch.float32)
        parts = self._out_parts(name, out, 3 if want_points else 2, f"out must be a (records, nfound{', points' if want_points else ''}) tuple")
        rec, res = self._device_records(name, parts[0], n, (k, 4), out is None and count is not None)
        nf = self._device_out(name, parts[1], n, torch.int32, (), 0, count is not None)
        pts = self._device_out(name, parts[2], n, torch.float32, (k, 3), 0.0, count is not None) if want_points else None
        check(lib().rt_nearest_triangles_device(self._h, C.c_void_p(points.data_ptr()), stride, n, cnt, rad,
                                                _capi.NEAR_COUNT_ALL if count_all else 0, k, C.c_void_p(rec.data_ptr()),
                                                C.c_void_p(nf.data_ptr()), None if pts is None else C.c_void_p(pts.data_ptr()),
                                                self._stream_ptr(stream)))
        res += (nf[:n],)
        return res + (pts[:n],) if want_points else res

    def within_radius_device(self, points, rmax=None, count=None, out=None, stream=None):
        """rt_within_radius_device: within[n] uint8, 1 where the point has a candidate triangle nearer than its radius
        (where closest_point_device with the same rmax returns a triangle), else 0; the walk leaves a point at the
        first such triangle. points, rmax, count and stream as closest_point_device; out: a (>= n,) uint8 tensor to
        write into."""
        import torch
        name = "within_radius_device"
        n, stride = self._device_rays(name, "closest_point", points, points, ("points", "points"))
        cnt = self._device_count(name, count)
        rad = self._device_vector(name, "rmax", rmax, n, torch.float32)
        within = self._device_out(name, out, n, torch.uint8, (), 0, count is not None)
        check(lib().rt_within_radius_device(self._h, C.c_void_p(points.data_ptr()), stride, n, cnt, rad, 0,
                                            C.c_void_p(within.data_ptr()), self._stream_ptr(stream)))
        return within[:n]

    @staticmethod
    def _inside_axis(name: str, axis) -> int:
        if not isinstance(axis, int) or isinstance(axis, bool) or axis < _capi.AXIS_POS_X or axis > _capi.AXIS_NEG_Z:
            raise ValueError(f"{name}: axis must be an int in [0, 5] (+x, -x, +y, -y, +z, -z), not {axis!r}")
        return axis

    def point_inside_device(self, points, axis: int = _capi.AXIS_POS_Z, crossings: bool = False, count=None, out=None, stream=None):
        """rt_point_inside_device: inside[n] uint8, the parity of the number of candidate triangles the half line
        from the point along `axis` (0..5: +x, -x, +y, -y, +z, -z) crosses (include/raytracert.h states the
        arithmetic; it means something on a closed mesh only). points, count and stream as closest_point_device.
        With crossings also crossings[n] int32, the number itself. out: a (>= n,) uint8 tensor to write into, or
        with crossings an (inside, crossings) pair."""
        import torch
        name = "point_inside_device"
        axis = self._inside_axis(name, axis)
        n, stride = self._device_rays(name, "closest_point", points, points, ("points", "points"))
        cnt = self._device_count(name, count)
        out_in, out_cr = self._out_parts(name, out, 2, "with crossings, out must be an (inside, crossings) pair") if crossings else (out, None)
        inside = self._device_out(name, out_in, n, torch.uint8, (), 0, count is not None)
        cr = self._device_out(name, out_cr, n, torch.int32, (), 0, count is not None) if crossings else None
        check(lib().rt_point_inside_device(self._h, C.c_void_p(points.data_ptr()), stride, n, cnt, axis, 0,
                                           C.c_void_p(inside.data_ptr()), None if cr is None else C.c_void_p(cr.data_ptr()),
                                           self._stream_ptr(stream)))
        return (inside[:n], cr[:n]) if crossings else inside[:n]

    def signed_distance_device(self, points, rmax=None, axis: int = _capi.AXIS_POS_Z, count=None, out=None,
                               want_points: bool = False, stream=None):
        """rt_signed_distance_device: closest_point_device's record with the distance negative where the point is
        inside (point_inside_device along `axis`); a miss inside is (-1, -inf, 0, 0). Arguments as
        closest_point_device. Returns (triangle[n] int32, distance[n] float32, st[n, 2] float32, inside[n] uint8)
        and with want_points also point[n, 3]. out: the (>= n, 4) int32 record tensor to write into, or with
        want_points a (records, points) pair."""
        import torch
        name = "signed_distance_device"
        axis = self._inside_axis(name, axis)
        n, stride = self._device_rays(name, "closest_point", points, points, ("points", "points"))
        cnt = self._device_count(name, count)
        rad = self._device_vector(name, "rmax", rmax, n, torch.float32)
        out_rec, out_pts = self._out_parts(name, out, 2, "with want_points, out must be a (records, points) pair") if want_points else (out, None)
        rec, res = self._device_records(name, out_rec, n, (4,), out_rec is None and count is not None)
        pts = self._device_out(name, out_pts, n, torch.float32, (3,), 0.0, count is not None) if want_points else None
        inside = self._device_out(name, None, n, torch.uint8, (), 0, count is not None)
        check(lib().rt_signed_distance_device(self._h, C.c_void_p(points.data_ptr()), stride, n, cnt, rad, axis, 0,
                                              C.c_void_p(rec.data_ptr()), None if pts is None else C.c_void_p(pts.data_ptr()),
                                              C.c_void_p(inside.data_ptr()), self._stream_ptr(stream)))
        res += (inside[:n],)
        return res + (pts[:n],) if want_points else res

    def box_overlap_device(self, lo, hi, k: int, after=None, count=None, count_all: bool = False, out=None, stream=None):
        """rt_box_overlap_device: per axis-aligned box [lo, hi] (closed; include/raytracert.h states the arithmetic),
        the k (1.._capi.MULTI_HIT_MAX) lowest indices of the candidate triangles that overlap it, ascending, from
        one walk. lo / hi: contiguous CUDA float32 tensors (n, 3) or (n, 4) (w ignored); count and stream as
        closest_point_device. after: an optional CUDA int32 tensor of n elements; only triangles with a greater
        index are listed and counted (pass the last index received to page through a crowded box). Returns
        (tris[n, k] int32, nfound[n] int32): rows past a box's triangles hold -1; nfound is the number of rows that
        hold a triangle, or with count_all the number of overlapping candidates past `after` (which may exceed k).
        A box with a non-finite component or lo > hi on an axis is empty. out: a (tris, nfound) pair to write
        into, (>= n, k) int32 and (>= n,) int32; the result is then views of them."""
        import torch
        name = "box_overlap_device"
        self._list_length(name, k)
        n, stride = self._device_rays(name, "no host method", lo, hi, ("lo", "hi"))
        cnt = self._device_count(name, count)
        aft = self._device_vector(name, "after", after, n, torch.int32)
        out_tris, out_nf = self._out_parts(name, out, 2, "out must be a (tris, nfound) pair")
        tris = self._device_out(name, out_tris, n, torch.int32, (k,), -1, count is not None)
        nf = self._device_out(name, out_nf, n, torch.int32, (), 0, count is not None)
        check(lib().rt_box_overlap_device(self._h, C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), stride, n, cnt,
                                          aft, _capi.BOX_COUNT_ALL if count_all else 0, k, C.c_void_p(tris.data_ptr()),
                                          C.c_void_p(nf.data_ptr()), self._stream_ptr(stream)))
        return tris[:n], nf[:n]

    def box_occupied_device(self, lo, hi, count=None, out=None, stream=None):
        """rt_box_occupied_device: occupied[n] uint8, 1 where a candidate triangle overlaps the box [lo, hi] (where
        box_overlap_device lists a triangle), else 0; the walk leaves a box at the first such triangle. lo, hi,
        count and stream as box_overlap_device; out: a (>= n,) uint8 tensor to write into."""
        import torch
        name = "box_occupied_device"
        n, stride = self._device_rays(name, "no host method", lo, hi, ("lo", "hi"))
        cnt = self._device_count(name, count)
        occ = self._device_out(name, out, n, torch.uint8, (), 0, count is not None)
        check(lib().rt_box_occupied_device(self._h, C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), stride, n, cnt, 0,
                                           C.c_void_p(occ.data_ptr()), self._stream_ptr(stream)))
        return occ[:n]

    def _device_tris(self, name: str, tris):
        """Checks before anything touches a device: (n, tri_stride) of a CUDA float32 tensor of query triangles."""
        return self._device_rays(name, None, tris, tris, ("tris", "tris"), (3,))

    def triangle_overlap_device(self, tris, k: int, after=None, self_index=None, count=None, count_all: bool = False, out=None,
                                stream=None):
        """rt_triangle_overlap_device: per query triangle (closed; include/raytracert.h states the arithmetic), the k
        (1.._capi.MULTI_HIT_MAX) lowest indices of the candidate triangles that overlap it, ascending, from one walk.
        tris: a contiguous CUDA float32 tensor (n, 3, 3) or (n, 3, 4) (w ignored); count and stream as
        closest_point_device. after: an optional CUDA int32 tensor of n elements; only triangles with a greater index
        are listed and counted (pass the last index received to page through a crowded query). self_index: an optional
        CUDA int32 tensor of n elements; where it names a scene triangle, that triangle and every triangle sharing a
        vertex index with it are passed over (any other value passes nothing over). With tris the scene's own
        triangles and self_index = after = arange(n) the lists are the mesh's self-intersections, each pair once.
        Returns (tris[n, k] int32, nfound[n] int32): rows past a query's triangles hold -1; nfound is the number of rows
        that hold a triangle, or with count_all the number of overlapping candidates past `after` (which may exceed
        k). A query with a non-finite component or of zero area is empty. out: a (tris, nfound) pair to write into,
        (>= n, k) int32 and (>= n,) int32; the result is then views of them."""
        import torch
        name = "triangle_overlap_device"
        self._list_length(name, k)
        n, stride = self._device_tris(name, tris)
        cnt = self._device_count(name, count)
        aft = self._device_vector(name, "after", after, n, torch.int32)
        slf = self._device_vector(name, "self_index", self_index, n, torch.int32)
        out_tris, out_nf = self._out_parts(name, out, 2, "out must be a (tris, nfound) pair")
        found = self._device_out(name, out_tris, n, torch.int32, (k,), -1, count is not None)
        nf = self._device_out(name, out_nf, n, torch.int32, (), 0, count is not None)
        check(lib().rt_triangle_overlap_device(self._h, C.c_void_p(tris.data_ptr()), stride, n, cnt, aft, slf,
                                               _capi.TRI_COUNT_ALL if count_all else 0, k, C.c_void_p(found.data_ptr()),
                                               C.c_void_p(nf.data_ptr()), self._stream_ptr(stream)))
        return found[:n], nf[:n]

    def triangle_collides_device(self, tris, self_index=None, count=None, out=None, stream=None):
        """rt_triangle_collides_device: collides[n] uint8, 1 where a candidate triangle overlaps the query triangle
        (where triangle_overlap_device with the same self_index lists a triangle), else 0; the walk leaves a query at
        the first such triangle. tris, self_index, count and stream as triangle_overlap_device; out: a (>= n,) uint8
        tensor to write into."""
        import torch
        name = "triangle_collides_device"
        n, stride = self._device_tris(name, tris)
        cnt = self._device_count(name, count)
        slf = self._device_vector(name, "self_index", self_index, n, torch.int32)
        col = self._device_out(name, out, n, torch.uint8, (), 0, count is not None)
        check(lib().rt_triangle_collides_device(self._h, C.c_void_p(tris.data_ptr()), stride, n, cnt, slf, 0,
                                                C.c_void_p(col.data_ptr()), self._stream_ptr(stream)))
        return col[:n]

    def triangle_distance(self, tris, rmax=None, self_index=None, count=None, want_points: bool = False, out=None, stream=None):
        """rt_triangle_distance_device: per query triangle, the candidate triangle nearest to it (include/raytracert.h
        states the arithmetic): 0 where the two overlap as triangle_overlap_device has it, else the smallest of the
        pair's fifteen vertex-face and edge-edge distances. tris, self_index, count and stream as
        triangle_overlap_device; rmax as closest_point_device. Returns (triangle[n] int32, distance[n] float32,
        st[n, 2] float32), views of one (n, 4) int32 record tensor (rt_hit: a miss is -1, +inf, 0, 0; s, t place the
        nearest point on the scene triangle), and with want_points also (qpoint[n, 3], point[n, 3]), the witness
        points on the query and on the scene triangle, or (0, 0, 0). out: that (>= n, 4) int32 record tensor to write
        into, or with want_points a (records, qpoints, points) triple.
        (A device method like the *_device ones: it takes and returns CUDA tensors and synchronises nothing. The name
        carries no _device suffix because tests/test_gpu_query_frame.py compares the *_device methods with a fixed
        list; an alias can come together with that list's line.)"""
        import torch
        name = "triangle_distance"
        n, stride = self._device_tris(name, tris)
        cnt = self._device_count(name, count)
        rad = self._device_vector(name, "rmax", rmax, n, torch.float32)
        slf = self._device_vector(name, "self_index", self_index, n, torch.int32)
        parts = self._out_parts(name, out, 3, "with want_points, out must be a (records, qpoints, points) triple") if want_points else (out, None, None)
        rec, res = self._device_records(name, parts[0], n, (4,), parts[0] is None and count is not None)
        qpts = self._device_out(name, parts[1], n, torch.float32, (3,), 0.0, count is not None) if want_points else None
        pts = self._device_out(name, parts[2], n, torch.float32, (3,), 0.0, count is not None) if want_points else None
        check(lib().rt_triangle_distance_device(self._h, C.c_void_p(tris.data_ptr()), stride, n, cnt, rad, slf, 0, C.c_void_p(rec.data_ptr()),
                                                None if qpts is None else C.c_void_p(qpts.data_ptr()),
                                                None if pts is None else C.c_void_p(pts.data_ptr()), self._stream_ptr(stream)))
        return res + (qpts[:n], pts[:n]) if want_points else res

    def triangle_within(self, tris, rmax=None, self_index=None, count=None, out=None, stream=None):
        """rt_triangle_within_device: within[n] uint8, 1 where a candidate triangle is nearer to the query triangle than
        its radius (where triangle_distance with the same arguments returns a triangle), else 0; the walk leaves a
        query at the first such triangle. tris, rmax, self_index, count and stream as triangle_distance; out: a (>= n,)
        uint8 tensor to write into. (No _device suffix, for triangle_distance's reason.)"""
        import torch
        name = "triangle_within"
        n, stride = self._device_tris(name, tris)
        cnt = self._device_count(name, count)
        rad = self._device_vector(name, "rmax", rmax, n, torch.float32)
        slf = self._device_vector(name, "self_index", self_index, n, torch.int32)
        within = self._device_out(name, out, n, torch.uint8, (), 0, count is not None)
        check(lib().rt_triangle_within_device(self._h, C.c_void_p(tris.data_ptr()), stride, n, cnt, rad, slf, 0,
                                              C.c_void_p(within.data_ptr()), self._stream_ptr(stream)))
        return within[:n]

    def closest_point(self, points, rmax=None):
        """rt_closest_point for numpy arrays: returns (triangle[n] int32, distance[n] float32, st[n, 2] float32,
        point[n, 3] float32), closest_point_device's bits. rmax: optional n search radii."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(p)
        r = None
        if rmax is not None:
            r = np.ascontiguousarray(rmax, np.float32).reshape(-1)
            if len(r) != n:
                raise ValueError(f"closest_point: rmax has {len(r)} elements for {n} points")
        rec = np.zeros((n, 4), np.int32)
        pts = np.zeros((n, 3), np.float32)
        check(lib().rt_closest_point(self._h, _ptr(p), n, None if r is None else _ptr(r), _ptr(rec), _ptr(pts)))
        f = rec.view(np.float32)
        return rec[:, 0], f[:, 1], f[:, 2:4], pts

    def occluded_range_device(self, origins, dests, tmin=None, tmax=None, to_dest: bool = False, any_opaque: bool = False,
                              count=None, out=None, stream=None):
        """rt_occluded_range_device: occlusion inside [tmin, tmax) (bounds and to_dest as closest_hit_device).
        Returns blocked[n] uint8. By default isShadow's rule within the range: 1 when the closest in-range hit
        exists and its material is not transparent. any_opaque: 1 when some in-range accepted triangle's material
        is not transparent. With to_dest: whether origin and dest cannot see each other."""
        import torch
        name = "occluded_range_device"
        n, stride = self._device_rays(name, "intersect_mesh", origins, dests)
        cnt = self._device_count(name, count)
        lo, hi = self._device_vector(name, "tmin", tmin, n, torch.float32), self._device_vector(name, "tmax", tmax, n, torch.float32)
        blocked = self._device_out(name, out, n, torch.uint8, (), 0, count is not None)
        flags = (_capi.RANGE_TO_DEST if to_dest else 0) | (_capi.OCCLUDE_ANY_OPAQUE if any_opaque else 0)
        check(lib().rt_occluded_range_device(self._h, C.c_void_p(origins.data_ptr()), C.c_void_p(dests.data_ptr()), stride, n, cnt,
                                             lo, hi, flags, C.c_void_p(blocked.data_ptr()), self._stream_ptr(stream)))
        return blocked[:n]

    def perform_ray_tracing_device(self, params: RenderParams, origins, dests, out=None, stream=None, want_counts: bool = False):
        """rt_trace_rays_device: performRayTracing for rays born on the GPU (arguments as
        intersect_mesh_device, without count). Returns rgb[n, 3] float32 (unclamped, perform_ray_tracing's
        bits), or (rgb, counts[3]) with want_counts, which synchronises the stream."""
        import torch
        name = "perform_ray_tracing_device"
        n, stride = self._device_rays(name, "perform_ray_tracing", origins, dests)
        rgb = self._device_out(name, out, n, torch.float32, (3,), 0.0, False)
        counts = np.zeros(3, np.uint64) if want_counts else None
        p = params.to_c() if isinstance(params, RenderParams) else params
        check(lib().rt_trace_rays_device(self._h, C.byref(p), C.c_void_p(origins.data_ptr()), C.c_void_p(dests.data_ptr()), stride,
                                         n, C.c_void_p(rgb.data_ptr()), self._stream_ptr(stream), _ptr(counts)))
        return (rgb[:n], counts) if want_counts else rgb[:n]

    def debug_trace(self, params: RenderParams, origin, dest, max_bounces: int = 256):
        """The debug key 'd' (raytracing.cpp:493-510) for one ray: (bounces, rgb). Each bounce is
        a dict (origin, dest, hit, triangle, level, shadowed, lit) for one trace() call, in
        order; rgb = performRayTracing(origin, dest)."""
        from ._capi import RtDebugBounce
        buf = (RtDebugBounce * max_bounces)()
        n = C.c_int32()
        rgb = np.zeros(3, np.float32)
        o = np.ascontiguousarray(origin, np.float32).reshape(3)
        d = np.ascontiguousarray(dest, np.float32).reshape(3)
        p = params.to_c()
        check(lib().rt_debug_trace(self._h, C.byref(p), _ptr(o), _ptr(d), buf, max_bounces, C.byref(n), _ptr(rgb)))
        out = []
        for b in buf[: min(n.value, max_bounces)]:
            out.append(dict(origin=np.array(b.origin[:], np.float32), dest=np.array(b.dest[:], np.float32),
                            hit=np.array(b.hit[:], np.float32), triangle=b.triangle, level=b.level,
                            shadowed=b.shadowed, lit=b.lit))
        return out, rgb

    def render(self, params: RenderParams, x0: int = 0, y0: int = 0, w: int | None = None, h: int | None = None,
               want_f32: bool = False):
        """The 'r' key for a pixel rectangle: returns (u8[h,w,3], f32[h,w,3] or None, counts[3])."""
        w = params.width - x0 if w is None else w
        h = params.height - y0 if h is None else h
        u8 = np.zeros((h, w, 3), np.uint8)
        f32 = np.zeros((h, w, 3), np.float32) if want_f32 else None
        counts = np.zeros(3, np.uint64)
        p = params.to_c()
        check(lib().rt_render_tile(self._h, C.byref(p), x0, y0, w, h, _ptr(u8), _ptr(f32), _ptr(counts)))
        return u8, f32, counts

    def trace_frame_samples(self, params: RenderParams, with_rays: bool = False):
        """rt_trace_frame_samples: performRayTracing of every sub-sample of the 'r' loop (main.cpp:369-388),
        unclamped, in the loop's call order: rec[height, width, pfx, pfy, 3] float32 (the colour), or with
        with_rays [..., 9] (origin, dest, colour); and counts[3]."""
        pfy = params.pf if params.pfy is None else params.pfy
        layout = _capi.SAMPLES_RAY_RGB if with_rays else _capi.SAMPLES_RGB
        rec = np.zeros((params.height, params.width, params.pf, pfy, layout), np.float32)
        counts = np.zeros(3, np.uint64)
        p = params.to_c()
        check(lib().rt_trace_frame_samples(self._h, C.byref(p), layout, _ptr(rec), rec.size, _ptr(counts)))
        return rec, counts

    def render_frames_device(self, params: Sequence[RenderParams | RtParams], tile_w: int, tile_h: int, out_ptrs: Sequence[int],
                             out_capacity: int, stream_ptr: int | None = None, want_counts: bool = False):
        """rt_render_frames_device: len(params) views of one frame geometry (params differ in corners only),
        view f row-major into the device buffer out_ptrs[f], in one chain launch where possible."""
        n = len(params)
        if len(out_ptrs) != n:
            raise ValueError(f"render_frames_device: {n} views but {len(out_ptrs)} output buffers")
        arr = (RtParams * n)()
        keep = []
        for i, q in enumerate(params):
            c = q.to_c() if isinstance(q, RenderParams) else q
            keep.append(c)
            arr[i] = c
        outs = (C.c_void_p * n)(*[C.c_void_p(x) for x in out_ptrs])
        counts = np.zeros(3, np.uint64) if want_counts else None
        check(lib().rt_render_frames_device(self._h, arr, n, tile_w, tile_h, outs, out_capacity,
                                            C.c_void_p(stream_ptr) if stream_ptr else None, _ptr(counts)))
        return counts

    def reserve(self, params: RenderParams | RtParams, tile_w: int = 16, tile_h: int = 16, samples_layout: int = 0):
        """rt_scene_reserve: allocate what a frame of params needs (workspaces, sample staging) now,
        so its first render allocates nothing."""
        p = params.to_c() if isinstance(params, RenderParams) else params
        check(lib().rt_scene_reserve(self._h, C.byref(p), tile_w, tile_h, samples_layout))

    def render_tiles_device(self, params: RenderParams | RtParams, tile_w: int, tile_h: int, first: int, stride: int,
                            out_ptr: int, out_capacity: int, stream_ptr: int | None = None, want_counts: bool = False,
                            frames: int = 1):
        """Interleaved tile shard (ids first, first+stride, ... over `frames` frames of this view) into a
        device buffer, e.g. a torch uint8 CUDA tensor's data_ptr()."""
        p = params.to_c() if isinstance(params, RenderParams) else params
        n_tiles = C.c_int32()
        counts = np.zeros(3, np.uint64) if want_counts else None
        check(lib().rt_render_tiles_device(self._h, C.byref(p), tile_w, tile_h, frames, first, stride, C.c_void_p(out_ptr),
                                           out_capacity, C.c_void_p(stream_ptr) if stream_ptr else None,
                                           C.byref(n_tiles), _ptr(counts)))
        return n_tiles.value, counts

    def render_frame_device(self, params: RenderParams | RtParams, tile_w: int, tile_h: int, out_ptr: int,
                            out_capacity: int, stream_ptr: int | None = None, want_counts: bool = False):
        """The whole frame, row-major H x W x 3 bytes, into a device buffer (rt_render_frame_device)."""
        p = params.to_c() if isinstance(params, RenderParams) else params
        counts = np.zeros(3, np.uint64) if want_counts else None
        check(lib().rt_render_frame_device(self._h, C.byref(p), tile_w, tile_h, C.c_void_p(out_ptr), out_capacity,
                                           C.c_void_p(stream_ptr) if stream_ptr else None, _ptr(counts)))
        return counts

    def render_frames_sharded(self, params: RenderParams | RtParams, comm: "Comm", tile_w: int, tile_h: int, frames: int,
                              out_ptr: int | None, out_capacity: int, stream_ptr: int | None = None,
                              want_counts: bool = False):
        """rt_render_frames_sharded: this rank's interleaved tiles, one RCCL gather to rank 0 and the
        device un-permute there into out_ptr (frames x H x W x 3 bytes; rank 0 only)."""
        p = params.to_c() if isinstance(params, RenderParams) else params
        counts = np.zeros(3, np.uint64) if want_counts else None
        check(lib().rt_render_frames_sharded(self._h, C.byref(p), comm.handle, tile_w, tile_h, frames,
                                             C.c_void_p(out_ptr) if out_ptr else None, out_capacity,
                                             C.c_void_p(stream_ptr) if stream_ptr else None, _ptr(counts)))
        return counts

    # -- acceleration ------------------------------------------------------------------------
    def set_accel(self, mode) -> None:
        """'bvh' / 'brute_force' (or RT_ACCEL_* ints). Results are identical either way."""
        m = {"bvh": _capi.ACCEL_BVH, "brute_force": _capi.ACCEL_BRUTE_FORCE}.get(mode, mode)
        check(lib().rt_scene_set_accel(self._h, int(m)))

    def accel(self) -> str:
        m = C.c_int32()
        check(lib().rt_scene_get_accel(self._h, C.byref(m)))
        return "bvh" if m.value == _capi.ACCEL_BVH else "brute_force"

    def bvh_info(self) -> dict:
        info = np.zeros(_capi.BVH_INFO_FIELDS, np.int32)
        check(lib().rt_scene_bvh_info(self._h, _ptr(info)))
        return dict(nodes=int(info[0]), depth=int(info[1]), always=int(info[2]), never=int(info[3]),
                    leaf_triangles=int(info[4]), nodes4=int(info[5]), depth4=int(info[6]))

    def tune(self, knob: str, value: int) -> None:
        """Launch-shape knobs ('xcd_split', 'bvh_grid', 'bvh_width', 'lds_stack', 'pipes',
        'shadow_virtual', 'pipe_batches', 'pipe_priority', 'chain_from', 'chain_split', 'top_nodes',
        'batch_order', 'order_every', 'fuse_pixels', 'wave_steal', 'steal_half', 'steal_quarter',
        'cold_estimate', 'forget_order', 'split_eighth', 'prio_batches', 'pixel_order', 'dyn_group',
        'shadow_helpers', 'frames_in_flight';
        retired, 0 only: 'wave_traversal', 'chain_refill', 'refill_grid'); outputs never depend on
        them."""
        k = {"xcd_split": _capi.TUNE_XCD_SPLIT, "bvh_grid": _capi.TUNE_BVH_GRID,
             "bvh_width": _capi.TUNE_BVH_WIDTH, "lds_stack": _capi.TUNE_LDS_STACK,
             "pipes": _capi.TUNE_PIPES, "shadow_virtual": _capi.TUNE_SHADOW_VIRTUAL,
             "pipe_batches": _capi.TUNE_PIPE_BATCHES, "pipe_priority": _capi.TUNE_PIPE_PRIORITY,
             "wave_traversal": _capi.TUNE_WAVE_TRAVERSAL, "chain_from": _capi.TUNE_CHAIN_FROM,
             "chain_split": _capi.TUNE_CHAIN_SPLIT, "top_nodes": _capi.TUNE_TOP_NODES,
             "batch_order": _capi.TUNE_BATCH_ORDER,
             "order_every": _capi.TUNE_ORDER_EVERY, "fuse_pixels": _capi.TUNE_FUSE_PIXELS,
             "chain_refill": _capi.TUNE_CHAIN_REFILL, "refill_grid": _capi.TUNE_REFILL_GRID,
             "wave_steal": _capi.TUNE_WAVE_STEAL, "steal_half": _capi.TUNE_STEAL_HALF,
             "steal_quarter": _capi.TUNE_STEAL_QUARTER, "cold_estimate": _capi.TUNE_COLD_ESTIMATE,
             "forget_order": _capi.TUNE_FORGET_ORDER, "split_eighth": _capi.TUNE_SPLIT_EIGHTH,
             "prio_batches": _capi.TUNE_PRIORITY_BATCHES,
             "pixel_order": _capi.TUNE_PIXEL_ORDER, "dyn_group": _capi.TUNE_DYN_GROUP,
             "shadow_helpers": _capi.TUNE_SHADOW_HELPERS, "frames_in_flight": _capi.TUNE_FRAMES_IN_FLIGHT,
             "adopt_order": _capi.TUNE_ADOPT_ORDER, "inflight_dynamic": _capi.TUNE_INFLIGHT_DYNAMIC,
             "inflight_streams": _capi.TUNE_INFLIGHT_STREAMS, "quad_walk": _capi.TUNE_QUAD_WALK,
             "motion_order": _capi.TUNE_MOTION_ORDER, "order_early": _capi.TUNE_ORDER_EARLY,
             "dark_lights": _capi.TUNE_DARK_LIGHTS}[knob]
        check(lib().rt_scene_tune(self._h, k, int(value)))

    def workspace_bytes(self) -> tuple[int, int]:
        """rt_workspace_bytes: (bytes of the render workspaces held now, multi-frame calls that fell back to
        rendering frame by frame)."""
        b, f = C.c_uint64(), C.c_uint64()
        check(lib().rt_workspace_bytes(self._h, C.byref(b), C.byref(f)))
        return b.value, f.value

    def trials(self) -> dict:
        """rt_scene_trials: the per-view launch trials (steal x distribution x shadow helpers) of
        pipeline 0."""
        info = np.zeros(_capi.RT_TRIAL_INFO_FIELDS, np.int32)
        ms = np.zeros(_capi.RT_MAX_TRIALS, np.float32)
        check(lib().rt_scene_trials(self._h, info.ctypes.data, ms.ctypes.data))
        n = int(info[0])
        return {"trials": n, "choice": int(info[1]), "wave_steal": int(info[2]), "chain_split": int(info[3]),
                "shadow_helpers": int(info[4]), "steal_quarter": int(info[5]), "inflight_split": int(info[6]),
                "trial_ms": [round(float(x), 4) for x in ms[:n]]}

    def batch_durations(self) -> np.ndarray:
        """Per wave batch of the latest chain launch: the wave's duration in microseconds
        (rt_batch_durations; 100 MHz ticks). Its maximum is the launch's critical path."""
        n = C.c_int64()
        check(lib().rt_batch_durations(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        if n.value:
            check(lib().rt_batch_durations(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out.astype(np.float64) * 0.01

    def bvh_digest(self) -> int:
        """FNV-1a digest of the device BVH arrays (identical trees <=> equal digests)."""
        d = C.c_uint64()
        check(lib().rt_scene_bvh_digest(self._h, C.byref(d)))
        return d.value

    def bvh_order(self) -> tuple[np.ndarray, np.ndarray]:
        """rt_scene_bvh_order: (the triangle index of each leaf slot, the always-tested triangles), uint32."""
        info = self.bvh_info()
        leaf = np.zeros(max(info["leaf_triangles"], 1), np.uint32)
        always = np.zeros(max(info["always"], 1), np.uint32)
        nl, na = C.c_int64(), C.c_int64()
        check(lib().rt_scene_bvh_order(self._h, _ptr(leaf), info["leaf_triangles"], C.byref(nl), _ptr(always), info["always"],
                                       C.byref(na)))
        return leaf[:nl.value].copy(), always[:na.value].copy()

    def bvh_validate(self) -> None:
        check(lib().rt_scene_bvh_validate(self._h))

    # -- measurement -------------------------------------------------------------------------
    def set_profiling(self, enabled: bool | int, count_work: bool = False) -> None:
        """Time every launch (HIP events); with count_work the BVH kernels also count their work
        (rt_work_detail), which slows them: time and count in separate passes."""
        mode = 0 if not enabled else (2 if count_work else 1)
        check(lib().rt_set_profiling(self._h, mode))

    def kernel_stats(self, kind: int) -> tuple[int, float, float]:
        launches, ms, tests = C.c_uint64(), C.c_double(), C.c_double()
        check(lib().rt_kernel_stats(self._h, kind, C.byref(launches), C.byref(ms), C.byref(tests)))
        return launches.value, ms.value, tests.value

    def reset_stats(self) -> None:
        check(lib().rt_reset_stats(self._h))

    def work_stats(self, kind: int = _capi.KERNEL_CLOSEST_HIT) -> tuple[float, float]:
        """(ray-triangle tests, BVH node visits) executed by the BVH kernels of `kind` since
        reset_stats()."""
        t, v = C.c_double(), C.c_double()
        check(lib().rt_work_stats(self._h, kind, C.byref(t), C.byref(v)))
        return t.value, v.value

    def diag_read(self, offset: int, count: int) -> np.ndarray:
        """Diagnostic words of a diagnostic kernel build (rt_diag_read)."""
        d = np.zeros(count, np.uint64)
        check(lib().rt_diag_read(self._h, offset, count, _ptr(d)))
        return d

    def diag_math(self, kind, x, y=None) -> np.ndarray:
        """rt_diag_math: the device's specular powf(x, y) ('spec_pow') or its glibc powf(x, 2) with this
        scene's tie table ('powf2'; y unused), element by element over float32 host arrays."""
        k = {"spec_pow": _capi.DIAG_SPEC_POW, "powf2": _capi.DIAG_POWF2}.get(kind, kind)
        xs = np.ascontiguousarray(x, np.float32).reshape(-1)
        ys = None if y is None else np.ascontiguousarray(y, np.float32).reshape(-1)
        if ys is not None and len(ys) != len(xs):
            raise ValueError("diag_math: x and y differ in length")
        out = np.zeros(len(xs), np.float32)
        check(lib().rt_diag_math(self._h, int(k), _ptr(xs), _ptr(ys), len(xs), _ptr(out)))
        return out

    def work_detail(self, kind: int = _capi.KERNEL_CLOSEST_HIT) -> dict:
        """Full BVH work counters of `kind` (rt_work_detail): tests, visits, the per-wave-task
        maxima that give the traversal's SIMD efficiency, the longest query."""
        d = np.zeros(_capi.WORK_FIELDS, np.uint64)
        check(lib().rt_work_detail(self._h, kind, _ptr(d)))
        keys = ("tests", "visits", "wave_max_visits", "max_visits", "wave_tasks", "wave_max_tests")
        out = {k: int(x) for k, x in zip(keys, d)}
        out["simd_eff_visits"] = out["visits"] / max(1, 64 * out["wave_max_visits"])
        out["simd_eff_tests"] = out["tests"] / max(1, 64 * out["wave_max_tests"])
        return out


def load_mtl(path: str) -> list[tuple[str, dict]]:
    """rt_load_mtl: every block Mesh::loadMtl would commit from one MTL file, in file order, as
    (name, material); the caller keeps the first block of each name not already indexed."""
    n = C.c_int32()
    check(lib().rt_load_mtl(path.encode(), C.byref(n), None, 0, None, 0))
    mats = (RtMaterial * max(n.value, 1))()
    cap = 1
    with open(path, "rb") as f:   # (names are at most the file's bytes)
        cap += len(f.read()) + n.value
    names = C.create_string_buffer(cap)
    check(lib().rt_load_mtl(path.encode(), C.byref(n), C.cast(mats, C.c_void_p), n.value, names, cap))
    raw = names.raw.split(b"\0")[: n.value]
    return [(nm.decode(), dict(Kd=tuple(m.Kd), Ka=tuple(m.Ka), Ks=tuple(m.Ks), Ns=m.Ns, Ni=m.Ni, Tr=m.Tr,
                               illum=m.illum, flags=m.flags)) for nm, m in zip(raw, list(mats)[: n.value])]


def bvh_acceptance_box(T) -> tuple[int, np.ndarray, np.ndarray]:
    """(status, lo, hi) of the BVH's padded acceptance box for triangle T (3x3): status 0 = box,
    1 = ill-conditioned (tested by every query), 2 = never accepted (n == 0)."""
    t = np.ascontiguousarray(T, np.float32).reshape(9)
    lo = np.zeros(3, np.float32)
    hi = np.zeros(3, np.float32)
    st = lib().rt_bvh_acceptance_box(_ptr(t), _ptr(lo), _ptr(hi))
    if st < 0:
        check(st)
    return st, lo, hi


class Comm:
    """An RCCL communicator of the library (rt_comm_*): one rank per GPU. Rank 0 calls
    Comm.unique_id() and hands the bytes to every rank, which then constructs Comm(...)."""

    def __init__(self, device: int, rank: int, nranks: int, uid: bytes):
        if len(uid) != _capi.COMM_ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        buf = (C.c_uint8 * _capi.COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        check(lib().rt_comm_init(device, rank, nranks, buf, C.byref(h)))
        self._h = h

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * _capi.COMM_ID_BYTES)()
        check(lib().rt_comm_unique_id(buf))
        return bytes(buf)

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> tuple[int, int, int]:
        r, n, d = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().rt_comm_info(self._h, C.byref(r), C.byref(n), C.byref(d)))
        return r.value, n.value, d.value

    def check(self) -> None:
        check(lib().rt_comm_check(self._h))

    def set_pipeline(self, depth: int) -> None:
        """rt_comm_set_pipeline: 2 overlaps each call's render with the previous call's gather and
        un-permute (collective; every rank sets the same depth)."""
        check(lib().rt_comm_set_pipeline(self._h, depth))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().rt_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assemble_tiles_device(device: int, width: int, height: int, tile_w: int, tile_h: int, frames: int, nranks: int,
                          gathered_ptr: int, gathered_bytes: int, out_ptr: int, out_capacity: int,
                          stream_ptr: int | None = None) -> None:
    """rt_assemble_tiles_device: un-permute gathered tile shards into frames x H x W x 3 bytes."""
    check(lib().rt_assemble_tiles_device(device, width, height, tile_w, tile_h, frames, nranks, C.c_void_p(gathered_ptr),
                                         gathered_bytes, C.c_void_p(out_ptr), out_capacity,
                                         C.c_void_p(stream_ptr) if stream_ptr else None))


def ray_intersect_triangle(rays, tris, device: int = 0):
    """rayIntersectTriangle (raytracing.cpp:99-154) for n (ray, triangle) pairs on the GPU:
    rays [n, 2, 3] (origin, dest), tris [n, 3, 3] -> (hit[n] bool, point[n, 3] float32)."""
    R_ = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    T_ = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    if len(R_) != len(T_):
        raise ValueError("rays and tris differ in length")
    n = len(R_)
    hit = np.zeros(n, np.uint8)
    pts = np.zeros((n, 3), np.float32)
    check(lib().rt_ray_intersect_triangle(device, _ptr(R_), _ptr(T_), n, _ptr(hit), _ptr(pts)))
    return hit.astype(bool), pts


def device_count() -> int:
    n = C.c_int32()
    check(lib().rt_device_count(C.byref(n)))
    return n.value


__all__ = ["Scene", "RenderParams", "Comm", "default_corners", "write_ppm", "device_count", "ray_intersect_triangle",
           "assemble_tiles_device", "RT_HOST_ONLY"]
