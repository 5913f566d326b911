"""glaze_amd -- MI355X-native render path behind glaze's Scene / parse / Renderer interface.

Python mirror of the slice of the reference's public Rust API that `glaze-cli` drives
(lib/src/lib.rs:10-24, cli/src/main.rs:76-121), implemented over the C ABI of libglaze_hip.so
(include/glaze_abi.h).  Names, argument meaning and error behaviour follow the reference:

    parsed   = glaze_amd.parse("scene.glaze")                       # glaze::parse            parser/mod.rs:93
    instance = glaze_amd.RayTraceInstance.new()                     # Option<RayTraceInstance> vulkan/instance.rs:376
    scene    = glaze_amd.RayTraceScene.new(instance, parsed)        # vulkan/scene.rs:1414
    renderer = glaze_amd.RayTraceRenderer.new(instance, scene, w, h)# vulkan/raytracer.rs:164
    renderer.set_integrator(glaze_amd.Integrator.PATH_TRACE)
    image    = renderer.draw(spp, callback)                         # HxWx4 uint8 sRGB, raytracer.rs:615

The render path has no CPU fallback: without libglaze_hip.so / a gfx950 device, RayTraceInstance.new()
returns None exactly like the reference does without a ray-tracing capable Vulkan device.
"""
import ctypes as C
import enum

import numpy as np

from . import abi
from .abi import GlazeError
from .scene_desc import MESH_DTYPE, VERTEX_DTYPE, SceneDesc, make_camera, make_light, make_material, make_meta  # noqa: F401

__all__ = ["parse", "converted_file", "ParsedScene", "RayTraceInstance", "RayTraceScene", "RayTraceRenderer", "Integrator",
           "GlazeError", "SceneDesc", "host_denoise", "host_despeckle", "host_reproject", "host_project_points", "host_skin", "host_bone_dual_quats", "host_clip_bones", "host_morph", "host_vertex_normals", "host_weld_groups",
           "host_project_constants"]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Integrator(enum.Enum):
    """lib/src/vulkan/raytracer.rs:30-86"""
    DIRECT = abi.DIRECT
    PATH_TRACE = abi.PATH_TRACE

    @staticmethod
    def values():
        return [Integrator.DIRECT, Integrator.PATH_TRACE]

    def name_str(self):
        return "Direct light only" if self is Integrator.DIRECT else "Path tracing"

    def steps_per_sample(self, pt_steps=6):
        return 1 if self is Integrator.DIRECT else pt_steps


class ParsedScene:
    """`Box<dyn ParsedScene>` (lib/src/parser/mod.rs:294-323): lazy, per-chunk getters."""

    def __init__(self, handle, path):
        self._h = handle
        self.path = path

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_h", None):
            abi.lib().glz_parsed_free(self._h)
            self._h = None

    def _take(self):
        h, self._h = self._h, None
        if not h:
            raise ValueError("parsed scene was already consumed by RayTraceScene.new")
        return h

    def _array(self, fn, ctype):
        L = abi.lib()
        n = abi.check(fn(self._h, None, 0))
        arr = (ctype * max(1, n))()
        abi.check(fn(self._h, C.cast(arr, C.c_void_p), n))
        return arr, n

    def vertices(self):
        arr, n = self._array(abi.lib().glz_parsed_vertices, abi.Vertex)
        return np.frombuffer(arr, dtype=np.float32, count=n * 8).reshape(n, 8).copy()

    def meshes(self):
        """[(id, material, indices uint32[])]"""
        arr, n = self._array(abi.lib().glz_parsed_meshes, abi.Mesh)
        idx_arr, ni = self._array(abi.lib().glz_parsed_indices, C.c_uint32)
        idx = np.frombuffer(idx_arr, dtype=np.uint32, count=ni)
        return [dict(id=arr[i].id, material=arr[i].material,
                     indices=idx[arr[i].index_offset:arr[i].index_offset + arr[i].index_count].copy()) for i in range(n)]

    def transforms(self):
        arr, n = self._array(abi.lib().glz_parsed_transforms, abi.Transform)
        return np.frombuffer(arr, dtype=np.float32, count=n * 16).reshape(n, 16).copy()

    def instances(self):
        arr, n = self._array(abi.lib().glz_parsed_instances, abi.MeshInstance)
        return np.frombuffer(arr, dtype=np.uint16, count=n * 2).reshape(n, 2).copy()

    def cameras(self):
        arr, n = self._array(abi.lib().glz_parsed_cameras, abi.Camera)
        return [arr[i] for i in range(n)]

    def materials(self):
        arr, n = self._array(abi.lib().glz_parsed_materials, abi.Material)
        return [arr[i] for i in range(n)]

    def lights(self):
        arr, n = self._array(abi.lib().glz_parsed_lights, abi.Light)
        return [arr[i] for i in range(n)]

    def textures(self):
        """[(format, pixels HxW or HxWx4 uint8, name, mip_levels)]"""
        arr, n = self._array(abi.lib().glz_parsed_textures, abi.Texture)
        out = []
        for i in range(n):
            t = arr[i]
            ch = 1 if t.format == abi.TEX_GRAY else 4
            buf = (C.c_uint8 * (t.width * t.height * ch)).from_address(t.pixels)
            px = np.frombuffer(buf, dtype=np.uint8).copy()
            px = px.reshape(t.height, t.width) if ch == 1 else px.reshape(t.height, t.width, 4)
            out.append((t.format, px, t.name.decode("utf8", "replace"), t.mip_levels))
        return out

    def meta(self):
        m = abi.Meta()
        abi.check(abi.lib().glz_parsed_meta(self._h, C.byref(m)))
        return m

    def update(self, cameras=None, materials=None, lights=None, textures=None, meta=None):
        """ParsedScene::update (lib/src/parser/v1.rs:364-422): None keeps the chunk as stored; the file is rewritten.

        cameras / materials / lights: lists of abi.Camera / abi.Material / abi.Light;
        textures: [(format, pixels, name)] or [(format, pixels, name, mip_levels)]; meta: abi.Meta."""
        keep = []

        def arr(items, ctype):
            if items is None:
                return None, -1
            a = (ctype * max(1, len(items)))(*items)
            keep.append(a)
            return C.cast(a, C.c_void_p), len(items)

        cam, ncam = arr(cameras, abi.Camera)
        mat, nmat = arr(materials, abi.Material)
        lig, nlig = arr(lights, abi.Light)
        tex, ntex = (None, -1) if textures is None else _texture_array(textures, keep)
        abi.check(abi.lib().glz_parsed_update(self._h, cam, ncam, mat, nmat, lig, nlig, tex, ntex,
                                              C.cast(C.pointer(meta), C.c_void_p) if meta is not None else None))


def _transform_array(transforms):
    t = np.ascontiguousarray(transforms, np.float32)
    if t.ndim != 2 or t.shape[1] != 16:
        raise ValueError("transforms must be an (n, 16) array of column-major 4x4 matrices, got shape %s" % (t.shape,))
    return t


def _vertex_array(vertices):
    """(n, 8) float32 of an (n, 8) array, a VERTEX_DTYPE array (SceneDesc.vertices as it is) or an abi.Vertex array"""
    if isinstance(vertices, C.Array) and vertices._type_ is abi.Vertex:
        v = np.frombuffer(vertices, np.float32).reshape(-1, 8)
    elif getattr(vertices, "dtype", None) == VERTEX_DTYPE:
        v = np.ascontiguousarray(vertices).view(np.float32).reshape(-1, 8)
    else:
        v = np.ascontiguousarray(vertices, np.float32)
    if v.ndim != 2 or v.shape[1] != 8:
        raise ValueError("vertices must be an (n, 8) array (position, normal, texture coordinate), got shape %s" % (v.shape,))
    return v


def host_instance_boxes(desc, budget=0):
    """The top level's instance boxes by the host rule on a SceneDesc, without a device ((n, 4) float32 lo, hi; one per instance that
    names an existing mesh).  A mesh's box is the min / max of its vertices here.  budget 0 = the library's exact-box budget."""
    c = desc.as_c()
    n = abi.check(abi.lib().glz_host_instance_boxes(C.byref(c), budget, None, None))
    lo, hi = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    abi.check(abi.lib().glz_host_instance_boxes(C.byref(c), budget, _ptr(lo), _ptr(hi)))
    return lo, hi


def _denoise_frames(result, aov0, aov1):
    r = np.ascontiguousarray(result, np.float32)
    if r.ndim != 3 or r.shape[2] != 4:
        raise ValueError("result must be H x W x 4")
    a0 = np.ascontiguousarray(aov0, np.float32)
    a1 = np.ascontiguousarray(aov1, np.float32)
    if a0.shape != r.shape or a1.shape != r.shape:
        raise ValueError("aov0 and aov1 must have result's shape")
    return r, a0, a1


def host_denoise(result, aov0, aov1, **params):
    """glz_host_denoise: the denoiser's filter on the host (no device), the reference of the device kernels.  result, aov0 = (normal, depth),
    aov1 = (albedo, instance bits): H x W x 4 float32; params: the fields of glz_denoise_params (defaults: the library's)."""
    r, a0, a1 = _denoise_frames(result, aov0, aov1)
    out = np.zeros_like(r)
    p = abi.DenoiseParams(**params)
    abi.check(abi.lib().glz_host_denoise(r.shape[1], r.shape[0], _ptr(r), _ptr(a0), _ptr(a1), C.cast(C.byref(p), C.c_void_p), _ptr(out)))
    return out


def host_despeckle(result, aov0, aov1, with_filter=False, denoise=None, **params):
    """glz_host_despeckle: the firefly rejection on the host (no device), the reference of k_despeckle.  Frames as host_denoise; params: the
    fields of glz_despeckle_params (defaults: the library's); denoise: a dict of glz_denoise_params fields (only eps_albedo matters without
    the filter).  with_filter: the filter's passes run on the rejection's output -- what read_denoised returns with the rejection enabled;
    otherwise the re-modulated rejection output -- what read_despeckled returns."""
    r, a0, a1 = _denoise_frames(result, aov0, aov1)
    out = np.zeros_like(r)
    d, p = abi.DespeckleParams(**params), abi.DenoiseParams(**(denoise or {}))
    abi.check(abi.lib().glz_host_despeckle(r.shape[1], r.shape[0], _ptr(r), _ptr(a0), _ptr(a1), C.cast(C.byref(d), C.c_void_p), C.cast(C.byref(p), C.c_void_p),
                                           1 if with_filter else 0, _ptr(out)))
    return out


def _reproject_frames(motion, prev_color, prev_aov0, prev_aov1):
    frames = [np.ascontiguousarray(f, np.float32) for f in (motion, prev_color, prev_aov0, prev_aov1)]
    if frames[0].ndim != 3 or frames[0].shape[2] != 4 or any(f.shape != frames[0].shape for f in frames):
        raise ValueError("motion, prev_color, prev_aov0 and prev_aov1 must all be H x W x 4")
    return frames


def host_project_constants(camera, width, height):
    """glz_host_project_constants: (world2camera, camera2screen with m[5] negated), each 16 float32, column-major -- the two matrices
    whose inverses glz_host_push_constants hands the kernels, formed in float64 and rounded once."""
    out = np.zeros(32, np.float32)
    abi.check(abi.lib().glz_host_project_constants(C.cast(C.byref(camera), C.c_void_p), width, height, _ptr(out)))
    return out[:16].copy(), out[16:].copy()


def host_project_points(camera, width, height, points):
    """glz_host_project_points: project_point of include/glaze_abi.h on an (n, 3) array of world points, on the host (no device):
    (n, 3) float32 (fx, fy, z), (0, 0, +inf) where the projection is invalid."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    out = np.zeros_like(pts)
    abi.check(abi.lib().glz_host_project_points(C.cast(C.byref(camera), C.c_void_p), width, height, _ptr(pts), pts.shape[0], _ptr(out)))
    return out


def host_reproject(motion, prev_color, prev_aov0, prev_aov1, **params):
    """glz_host_reproject: the reprojection rule on the host (no device), the reference of k_reproject.  motion: the plane read_motion
    returns; prev_color, prev_aov0 = (normal, depth), prev_aov1 = (albedo, instance bits): the previous frames; all H x W x 4 float32.
    params: the fields of glz_reproject_params (default: the library's).  Returns (reprojected rgb, confidence), H x W x 4."""
    m, c, a0, a1 = _reproject_frames(motion, prev_color, prev_aov0, prev_aov1)
    out = np.zeros_like(m)
    p = abi.ReprojectParams(**params)
    abi.check(abi.lib().glz_host_reproject(m.shape[1], m.shape[0], _ptr(m), _ptr(c), _ptr(a0), _ptr(a1), C.cast(C.byref(p), C.c_void_p), _ptr(out)))
    return out


def _skin_arrays(joints, weights):
    j = np.ascontiguousarray(joints)
    if j.ndim != 2 or j.shape[1] != 4 or j.dtype.kind not in "iu" or (j.size and (j.min() < 0 or j.max() > 0xFFFF)):
        raise ValueError("joints must be an (n, 4) integer array of bone indices below 65536")
    w = np.ascontiguousarray(weights, np.float32)
    if w.shape != j.shape:
        raise ValueError("weights must be (n, 4), one per joint")
    return np.ascontiguousarray(j, np.uint16), w


_SKIN_BLENDS = {"linear": abi.SKIN_LINEAR, "dual_quaternion": abi.SKIN_DUAL_QUATERNION}


def _skin_blend(blend):
    if blend not in _SKIN_BLENDS:
        raise ValueError("blend must be 'linear' or 'dual_quaternion'")
    return _SKIN_BLENDS[blend]


def host_skin(bind, joints, weights, bones, blend="linear"):
    """glz_host_skin: the skinning rule (include/glaze_abi.h holds the specification) on the host, no device, the reference of k_skin (the skin step of k_deform under the linear rule).
    bind: n vertices in any form update_vertices takes; joints: (n, 4) integers; weights: (n, 4) float32; bones: (n_bones, 16) float32,
    column-major.  blend="dual_quaternion": glz_host_skin_dq, the dual-quaternion rule, the reference of k_skin_dq (the same step under that rule).  Returns the posed
    vertices, (n, 8) float32."""
    fn = abi.lib().glz_host_skin_dq if _skin_blend(blend) == abi.SKIN_DUAL_QUATERNION else abi.lib().glz_host_skin
    v = _vertex_array(bind)
    j, w = _skin_arrays(joints, weights)
    b = _transform_array(bones)
    if j.shape[0] != v.shape[0]:
        raise ValueError("joints and weights must have one row per vertex")
    out = np.zeros_like(v)
    abi.check(fn(_ptr(v), _ptr(j), _ptr(w), v.shape[0], _ptr(b), b.shape[0], _ptr(out)))
    return out


def host_bone_dual_quats(bones):
    """glz_host_bone_dual_quats: the bone conversion of the dual-quaternion rule, (n_bones, 16) float32 matrices -> (n_bones, 8) float32,
    the unit quaternion (x, y, z, w) and the dual part (dx, dy, dz, dw) a bone, as the kernels of that mode read them."""
    b = _transform_array(bones)
    out = np.zeros((b.shape[0], 8), np.float32)
    abi.check(abi.lib().glz_host_bone_dual_quats(_ptr(b), b.shape[0], _ptr(out)))
    return out


_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def _skeleton_struct(skin, parents, inverse_bind, root):
    """(abi.Skeleton, the arrays it points into) of parents (n_bones integers, -1 a root), inverse_bind (n_bones, 16) and root (16, or None)"""
    raw = np.ascontiguousarray(parents)
    if raw.ndim != 1 or raw.dtype.kind not in "iu" or (raw.size and (raw.min() < -0x80000000 or raw.max() > 0x7FFFFFFF)):
        raise ValueError("parents must be a 1-d array of bone indices, -1 for a root")
    p = np.ascontiguousarray(raw, np.int32)
    ib = _transform_array(inverse_bind)
    if ib.shape[0] != p.shape[0]:
        raise ValueError("inverse_bind must have one matrix per bone")
    r = _IDENTITY if root is None else tuple(float(x) for x in np.asarray(root, np.float32).reshape(16))
    return abi.Skeleton(int(skin), p.shape[0], _ptr(p), _ptr(ib), (C.c_float * 16)(*r)), (p, ib)


def _clip_struct(skeleton, n_bones, times, translations, rotations, scales, morph_weights):
    """(abi.Clip, the arrays it points into) of times (n_keys,), translations (n_keys, n_bones, 3), rotations (n_keys, n_bones, 4) as
    (x, y, z, w), scales (n_keys, n_bones, 3) or None, morph_weights (n_keys, n_targets) or None"""
    t = np.ascontiguousarray(times, np.float32).reshape(-1)
    nk = t.shape[0]
    tr = np.ascontiguousarray(translations, np.float32)
    ro = np.ascontiguousarray(rotations, np.float32)
    sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
    if tr.shape != (nk, n_bones, 3) or ro.shape != (nk, n_bones, 4) or (sc is not None and sc.shape != (nk, n_bones, 3)):
        raise ValueError("translations and scales must be (n_keys, n_bones, 3), rotations (n_keys, n_bones, 4)")
    mw = None if morph_weights is None else np.ascontiguousarray(morph_weights, np.float32)
    if mw is not None and (mw.ndim != 2 or mw.shape[0] != nk):
        raise ValueError("morph_weights must be (n_keys, n_targets)")
    clip = abi.Clip(int(skeleton), nk, _ptr(t), _ptr(tr), _ptr(ro), None if sc is None else _ptr(sc), None if mw is None else _ptr(mw), 0 if mw is None else mw.shape[1])
    return clip, (t, tr, ro, sc, mw)


def host_clip_bones(parents, inverse_bind, times, translations, rotations, time, scales=None, morph_weights=None, root=None):
    """glz_host_clip_bones: the clip rule (include/glaze_abi.h holds the specification) on the host, no device, the reference of
    k_clip_bones.  parents, inverse_bind, root: as add_skeleton takes them; times, translations, rotations, scales, morph_weights: as
    add_clip takes them.  Returns the (n_bones, 16) float32 bone matrices pose() takes -- or, for a clip with a weight track, (bones,
    the (n_targets,) float32 lerped weights)."""
    sk, keep = _skeleton_struct(-1, parents, inverse_bind, root)
    clip, keep2 = _clip_struct(-1, sk.n_bones, times, translations, rotations, scales, morph_weights)
    bones = np.zeros((sk.n_bones, 16), np.float32)
    weights = np.zeros(clip.n_targets, np.float32) if clip.morph_weights else None
    abi.check(abi.lib().glz_host_clip_bones(C.cast(C.byref(sk), C.c_void_p), C.cast(C.byref(clip), C.c_void_p), float(time), _ptr(bones), None if weights is None else _ptr(weights)))
    return bones if weights is None else (bones, weights)


def _morph_targets(targets, n_vertices):
    """(abi.MorphTarget array, the arrays it points into) of a list of (indices | None, d_position, d_normal)"""
    keep, rows = [], []
    for t in targets:
        if len(t) != 3:
            raise ValueError("a target is (indices or None, d_position, d_normal)")
        dp, dn = (np.ascontiguousarray(d, np.float32).reshape(-1, 3) for d in t[1:])
        if t[0] is None:
            idx, n = None, int(n_vertices)
        else:
            raw = np.ascontiguousarray(t[0])
            if raw.ndim != 1 or (raw.size and (raw.dtype.kind not in "iu" or raw.min() < 0 or raw.max() > 0xFFFFFFFF)):
                raise ValueError("a target's indices must be a 1-d array of vertex indices")
            idx = np.ascontiguousarray(raw, np.uint32)
            n = idx.shape[0]
        if dp.shape != (n, 3) or dn.shape != (n, 3):
            raise ValueError("d_position and d_normal must be (n, 3), one row per entry (per vertex for a dense target)")
        keep += [idx, dp, dn]
        rows.append(abi.MorphTarget(None if idx is None else _ptr(idx), _ptr(dp), _ptr(dn), n))
    return (abi.MorphTarget * max(1, len(rows)))(*rows), keep


def host_morph(base, targets, weights):
    """glz_host_morph: the morph rule (include/glaze_abi.h holds the specification) on the host, no device, the reference of k_morph (the morph step of k_deform).
    base: n vertices in any form update_vertices takes; targets: a list of (indices | None, d_position, d_normal), indices relative to
    base, strictly ascending, None = dense; weights: one float32 a target.  Returns the morphed vertices, (n, 8) float32."""
    v = _vertex_array(base)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w.shape[0] != len(targets):
        raise ValueError("weights must have one entry per target")
    arr, keep = _morph_targets(targets, v.shape[0])
    out = v.copy()
    abi.check(abi.lib().glz_host_morph(_ptr(v), v.shape[0], C.cast(arr, C.c_void_p), len(targets), _ptr(w), _ptr(out)))
    return out


def _group_array(groups, n):
    """n uint32 labels, or None"""
    if groups is None:
        return None
    raw = np.ascontiguousarray(groups)
    if raw.shape != (int(n),) or raw.dtype.kind not in "iu" or (raw.size and (raw.min() < 0 or raw.max() > 0xFFFFFFFF)):
        raise ValueError("groups must be one label per vertex of the range")
    return np.ascontiguousarray(raw, np.uint32)


def host_vertex_normals(vertices, indices, meshes, first, n, groups=None):
    """glz_host_vertex_normals: the normal rule (include/glaze_abi.h holds the specification) on the host, no device, the reference of
    k_face_vectors and k_vertex_normals.  vertices: a scene's whole vertex array in any form update_vertices takes; indices: its uint32
    index array; meshes: its MESH_DTYPE array; [first, first + n): the set's range; groups: n labels below n, or None.  Returns the
    range's vertices with the rule's normals, (n, 8) float32."""
    v = _vertex_array(vertices)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    m = np.ascontiguousarray(meshes, MESH_DTYPE).reshape(-1)
    g = _group_array(groups, n)
    out = np.zeros((int(n), 8), np.float32)
    abi.check(abi.lib().glz_host_vertex_normals(_ptr(v), v.shape[0], _ptr(idx), idx.shape[0], _ptr(m), m.shape[0], int(first), int(n),
                                                None if g is None else _ptr(g), _ptr(out)))
    return out


def host_weld_groups(vertices):
    """glz_host_weld_groups: one uint32 label per vertex, the lowest index whose position and normal words are bit-equal to its own --
    what add_normals(groups=...) takes to keep a seam of duplicated vertices smooth."""
    v = _vertex_array(vertices)
    out = np.zeros(v.shape[0], np.uint32)
    abi.check(abi.lib().glz_host_weld_groups(_ptr(v), v.shape[0], _ptr(out)))
    return out


def _texture_array(textures, keep):
    texs = (abi.Texture * max(1, len(textures)))()
    for i, t in enumerate(textures):
        fmt, px, name = t[0], np.ascontiguousarray(t[1], np.uint8), t[2]
        keep.append(px)
        texs[i].format, texs[i].height, texs[i].width = fmt, px.shape[0], px.shape[1]
        texs[i].mip_levels = t[3] if len(t) > 3 else 1
        texs[i].pixels = px.ctypes.data
        texs[i].name = name.encode("utf8")[:abi.NAME_MAX - 1]
    keep.append(texs)
    return C.cast(texs, C.c_void_p), len(textures)


class Serializer:
    """glaze::Serializer (lib/src/parser/mod.rs:130-233): `Serializer(path).with_vertices(v)....serialize()`."""

    def __init__(self, path):
        self.path = str(path)
        self._v = np.zeros((0, 8), np.float32)
        self._meshes, self._transforms, self._instances = [], np.zeros((0, 16), np.float32), np.zeros((0, 2), np.uint16)
        self._cameras, self._textures, self._materials, self._lights, self._meta = [], [], [], [], None

    def with_vertices(self, v):
        v = np.ascontiguousarray(v)
        self._v = (v.view(np.float32) if v.dtype.names else v.astype(np.float32, copy=False)).reshape(-1, 8)
        return self

    def with_meshes(self, meshes):
        """[dict(id, material, indices)]"""
        self._meshes = list(meshes)
        return self

    def with_transforms(self, t):
        t = np.ascontiguousarray(t)
        self._transforms = (t.view(np.float32) if t.dtype.names else t.astype(np.float32, copy=False)).reshape(-1, 16)
        return self

    def with_instances(self, i):
        i = np.ascontiguousarray(i)
        self._instances = (i.view(np.uint16) if i.dtype.names else i.astype(np.uint16, copy=False)).reshape(-1, 2)
        return self

    def with_cameras(self, c):
        self._cameras = list(c)
        return self

    def with_textures(self, t):
        self._textures = list(t)
        return self

    def with_materials(self, m):
        self._materials = list(m)
        return self

    def with_lights(self, l):
        self._lights = list(l)
        return self

    def with_metadata(self, m):
        self._meta = m
        return self

    def serialize(self):
        keep = []
        d = abi.SerializeDescC()
        idx = np.concatenate([np.asarray(m["indices"], np.uint32).ravel() for m in self._meshes]) if self._meshes else np.zeros(0, np.uint32)
        meshes = (abi.Mesh * max(1, len(self._meshes)))()
        off = 0
        for i, m in enumerate(self._meshes):
            n = int(np.asarray(m["indices"]).size)
            meshes[i].id, meshes[i].material, meshes[i].index_offset, meshes[i].index_count = m["id"], m["material"], off, n
            off += n
        d.vertices, d.n_vertices = (self._v.ctypes.data if self._v.size else None), self._v.shape[0]
        d.indices, d.n_indices = (idx.ctypes.data if idx.size else None), idx.size
        d.meshes, d.n_meshes = C.cast(meshes, C.c_void_p), len(self._meshes)
        d.transforms, d.n_transforms = (self._transforms.ctypes.data if self._transforms.size else None), self._transforms.shape[0]
        d.instances, d.n_instances = (self._instances.ctypes.data if self._instances.size else None), self._instances.shape[0]
        for name, items, ctype in (("cameras", self._cameras, abi.Camera), ("materials", self._materials, abi.Material),
                                   ("lights", self._lights, abi.Light)):
            a = (ctype * max(1, len(items)))(*items)
            keep.append(a)
            setattr(d, name, C.cast(a, C.c_void_p))
            setattr(d, "n_" + name, len(items))
        d.textures, d.n_textures = _texture_array(self._textures, keep)
        if self._meta is not None:
            d.meta = C.cast(C.pointer(self._meta), C.c_void_p)
        keep += [idx, meshes]
        abi.check(abi.lib().glz_serialize(self.path.encode(), C.byref(d)))


def parse(path):
    """glaze::parse (lib/src/parser/mod.rs:93-116).  Raises GlazeError (io::Error) on a bad file."""
    h = abi.lib().glz_parse(str(path).encode())
    if not h:
        raise abi.last_error()
    return ParsedScene(h, str(path))


def save_image(path, rgba8):
    """image.save() of the CLI (cli/src/main.rs:121): HxWx4 uint8 -> .png or .jpg by extension."""
    a = np.ascontiguousarray(rgba8, np.uint8)
    abi.check(abi.lib().glz_save_image(str(path).encode(), a.ctypes.data, a.shape[1], a.shape[0]))


def convert_obj(obj_path, out_path, gen_mipmaps=False):
    """glaze-converter for OBJ input (converter/src/main.rs:116-637, assimp-free subset).  Returns the element counts."""
    counts = (C.c_uint64 * 6)()
    abi.check(abi.lib().glz_convert_obj(str(obj_path).encode(), str(out_path).encode(), int(gen_mipmaps), counts))
    return dict(zip(("vertices", "triangles", "meshes", "materials", "textures", "lights"), (int(c) for c in counts)))


def converted_file(path):
    """lib/src/parser/mod.rs:259-271"""
    return bool(abi.lib().glz_converted_file(str(path).encode()))


class RayTraceInstance:
    """lib/src/vulkan/instance.rs:376-427"""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def new(hip_device=-1):
        """Returns None when no gfx950 device (or no libglaze_hip.so code object) is usable."""
        h = abi.lib().glz_instance_create(hip_device)
        return RayTraceInstance(h) if h else None

    @property
    def device(self):
        return abi.lib().glz_instance_device(self._h)

    @property
    def stream(self):
        """hipStream_t (as int) all kernels of this instance run on."""
        return abi.lib().glz_instance_stream(self._h)

    def set_bvh_builder(self, name):
        """'auto' (default, = 'sah': binned SAH on the GPU), 'lbvh', 'ploc' or 'sah_host' (the SAH builder's host reference) for scenes created afterwards."""
        abi.check(abi.lib().glz_instance_set_bvh_builder(self._h, {"lbvh": 0, "ploc": 1, "sah": 2, "auto": 3, "sah_host": 4}[name]))

    def set_as_levels(self, mode):
        """'auto' (two levels when instancing multiplies the triangles more than four times), 'flat' or 'two_level' for scenes created afterwards."""
        abi.check(abi.lib().glz_instance_set_as_levels(self._h, {"auto": 0, "flat": 1, "two_level": 2}[mode]))

    def debug_detmath(self, fn, x, y=None):
        """include/glz_detmath.h run on the device: fn 'sin', 'cos', 'acos', 'atan2' (atan2(y, x)), 'log2' or 'floor'"""
        x = np.ascontiguousarray(x, np.float32).ravel()
        y = None if y is None else np.ascontiguousarray(y, np.float32).ravel()
        if fn == "atan2" and (y is None or y.size != x.size):
            raise ValueError("atan2 needs y of x's size")
        out = np.zeros_like(x)
        code = {"sin": 0, "cos": 1, "acos": 2, "atan2": 3, "log2": 4, "floor": 5}[fn]
        abi.check(abi.lib().glz_debug_detmath(self._h, code, _ptr(x), None if y is None else _ptr(y), _ptr(out), x.size))
        return out

    def debug_color_to_spec(self, rgb, illuminant=False):
        """the kernels' from_surface_color (or from_illuminant_color) of an (n, 3) array of colours: (n, 16) float32"""
        rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
        out = np.zeros((rgb.shape[0], 16), np.float32)
        abi.check(abi.lib().glz_debug_color_to_spec(self._h, int(bool(illuminant)), _ptr(rgb), rgb.shape[0], _ptr(out)))
        return out

    def debug_denoise(self, result, aov0, aov1, **params):
        """the device filter on host arrays (upload, kernels, read back): bit for bit glaze_amd.host_denoise"""
        r, a0, a1 = _denoise_frames(result, aov0, aov1)
        out = np.zeros_like(r)
        p = abi.DenoiseParams(**params)
        abi.check(abi.lib().glz_debug_denoise(self._h, r.shape[1], r.shape[0], _ptr(r), _ptr(a0), _ptr(a1), C.cast(C.byref(p), C.c_void_p), _ptr(out)))
        return out

    def debug_despeckle(self, result, aov0, aov1, with_filter=False, denoise=None, want_ms=False, **params):
        """the device side of glaze_amd.host_despeckle on host arrays (upload, kernels, read back), bit for bit alike; with want_ms also the
        device-event time of k_despeckle alone in milliseconds (a pair)"""
        r, a0, a1 = _denoise_frames(result, aov0, aov1)
        out = np.zeros_like(r)
        d, p = abi.DespeckleParams(**params), abi.DenoiseParams(**(denoise or {}))
        ms = C.c_float(0.0)
        abi.check(abi.lib().glz_debug_despeckle(self._h, r.shape[1], r.shape[0], _ptr(r), _ptr(a0), _ptr(a1), C.cast(C.byref(d), C.c_void_p),
                                                C.cast(C.byref(p), C.c_void_p), 1 if with_filter else 0, _ptr(out), C.cast(C.byref(ms), C.c_void_p)))
        return (out, ms.value) if want_ms else out

    def debug_project_points(self, camera, width, height, points):
        """the device side of glaze_amd.host_project_points on a host array (upload, kernel, read back), bit for bit alike"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out = np.zeros_like(pts)
        abi.check(abi.lib().glz_debug_project_points(self._h, C.cast(C.byref(camera), C.c_void_p), width, height, _ptr(pts), pts.shape[0], _ptr(out)))
        return out

    def debug_reproject(self, motion, prev_color, prev_aov0, prev_aov1, want_ms=False, **params):
        """the device side of glaze_amd.host_reproject on host arrays (upload, kernel, read back), bit for bit alike; with want_ms also the
        device-event time of k_reproject in milliseconds (a pair)"""
        m, c, a0, a1 = _reproject_frames(motion, prev_color, prev_aov0, prev_aov1)
        out = np.zeros_like(m)
        p = abi.ReprojectParams(**params)
        ms = C.c_float(0.0)
        abi.check(abi.lib().glz_debug_reproject(self._h, m.shape[1], m.shape[0], _ptr(m), _ptr(c), _ptr(a0), _ptr(a1), C.cast(C.byref(p), C.c_void_p), _ptr(out),
                                                C.cast(C.byref(ms), C.c_void_p)))
        return (out, ms.value) if want_ms else out

    def __del__(self):
        if getattr(self, "_h", None):
            abi.lib().glz_instance_destroy(self._h)
            self._h = None


class RayTraceScene:
    """lib/src/vulkan/scene.rs:1352-1556"""

    def __init__(self, handle, instance, keep=None):
        self._h = handle
        self.instance = instance
        self._keep = keep
        self._owned = True

    @staticmethod
    def new(instance, parsed):
        if isinstance(parsed, SceneDesc):
            return RayTraceScene.from_desc(instance, parsed)
        h = abi.lib().glz_scene_create(instance._h, parsed._take())
        if not h:
            raise abi.last_error()
        return RayTraceScene(h, instance)

    @staticmethod
    def from_desc(instance, desc):
        c = desc.as_c()
        h = abi.lib().glz_scene_create_from_desc(instance._h, C.byref(c))
        if not h:
            raise abi.last_error()
        return RayTraceScene(h, instance)

    def info(self):
        i = abi.SceneInfo()
        abi.check(abi.lib().glz_scene_get_info(self._h, C.byref(i)))
        return i

    def camera(self):
        c = abi.Camera()
        abi.check(abi.lib().glz_scene_camera(self._h, C.byref(c)))
        return c

    # ---- parity hooks (tests) ----
    def debug_trace_closest(self, origins, dirs, tmin=1e-4):
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = o.shape[0]
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        tri, inst = (np.zeros(n, np.uint32) for _ in range(2))
        abi.check(abi.lib().glz_debug_trace_closest(self._h, _ptr(o), _ptr(d), n, tmin, _ptr(t), _ptr(tri), _ptr(inst), _ptr(u), _ptr(v)))
        return t, tri, inst, u, v

    def debug_sample_texture(self, texture, uv, footprint=None):
        """the kernels' sampler on n coordinates uv (n x 2), RGBA (n x 4): level 0, or with footprint (n x 4: lod_base, du, dv, taps)
        texture2d_lod over the mip chain (built first)"""
        uv = np.ascontiguousarray(np.asarray(uv, np.float32).reshape(-1, 2))
        n = uv.shape[0]
        fp = None if footprint is None else np.ascontiguousarray(np.broadcast_to(np.asarray(footprint, np.float32), (n, 4)))
        out = np.zeros((n, 4), np.float32)
        abi.check(abi.lib().glz_debug_sample_texture(self._h, texture, _ptr(uv), None if fp is None else _ptr(fp), n, _ptr(out)))
        return out

    # the kernels' shading routines one call at a time; arguments and results as OracleScene.bsdf_value / bsdf_sample / light_sample
    def debug_bsdf_value(self, material_id, wo, wi, uv=(0.5, 0.5), rand=None, frame=None):
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        n = wo.shape[0]
        rnd = np.ascontiguousarray(rand if rand is not None else np.zeros(n), np.float32)
        uvv = np.ascontiguousarray(uv, np.float32).reshape(2)
        fr = None if frame is None else np.ascontiguousarray(frame, np.float32).reshape(9)
        if wi.shape[0] != n or rnd.size != n:
            raise ValueError("wo, wi and rand differ in length")
        value, pdf = np.zeros((n, 16), np.float32), np.zeros(n, np.float32)
        abi.check(abi.lib().glz_debug_bsdf_value(self._h, material_id, _ptr(wo), _ptr(wi), _ptr(uvv), _ptr(rnd), None if fr is None else _ptr(fr), n,
                                                 _ptr(value), _ptr(pdf)))
        return value, pdf

    def debug_set_spectra(self, material_id, ior, ior2abs2):
        """metal spectra of the caller's (16 bins each) for one material, for debug_bsdf_value / debug_bsdf_sample (glz_debug_scene_set_spectra)"""
        n, a = np.ascontiguousarray(ior, np.float32).reshape(16), np.ascontiguousarray(ior2abs2, np.float32).reshape(16)
        abi.check(abi.lib().glz_debug_scene_set_spectra(self._h, material_id, _ptr(n), _ptr(a)))

    def debug_bsdf_sample(self, material_id, wo, rand3, uv=(0.5, 0.5), frame=None):
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(rand3, np.float32).reshape(-1, 3)
        n = wo.shape[0]
        uvv = np.ascontiguousarray(uv, np.float32).reshape(2)
        fr = None if frame is None else np.ascontiguousarray(frame, np.float32).reshape(9)
        if r.shape[0] != n:
            raise ValueError("wo and rand3 differ in length")
        wi, value, pdf = np.zeros((n, 3), np.float32), np.zeros((n, 16), np.float32), np.zeros(n, np.float32)
        abi.check(abi.lib().glz_debug_bsdf_sample(self._h, material_id, _ptr(wo), _ptr(uvv), _ptr(r), None if fr is None else _ptr(fr), n, _ptr(wi),
                                                  _ptr(value), _ptr(pdf)))
        return wi, value, pdf

    def debug_light_sample(self, light_index, positions, rand3, scene_radius=1.0):
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(rand3, np.float32).reshape(-1, 3)
        n = p.shape[0]
        if r.shape[0] != n:
            raise ValueError("positions and rand3 differ in length")
        wi, dist, pdf, em = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 16), np.float32)
        abi.check(abi.lib().glz_debug_light_sample(self._h, light_index, _ptr(p), _ptr(r), n, scene_radius, _ptr(wi), _ptr(dist), _ptr(pdf), _ptr(em)))
        return wi, dist, pdf, em

    def debug_trace_any(self, origins, dirs, tmax, tmin=1e-3):
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        tm = np.ascontiguousarray(tmax, np.float32)
        out = np.zeros(o.shape[0], np.uint8)
        abi.check(abi.lib().glz_debug_trace_any(self._h, _ptr(o), _ptr(d), _ptr(tm), o.shape[0], tmin, _ptr(out)))
        return out

    def debug_derivatives(self):
        n = abi.check(abi.lib().glz_debug_read_derivatives(self._h, None, 0))
        out = np.zeros((n, 12), np.float32)
        abi.check(abi.lib().glz_debug_read_derivatives(self._h, _ptr(out), n))
        return out

    def debug_rt_materials(self):
        n = abi.check(abi.lib().glz_debug_read_rt_materials(self._h, None, 0))
        out = np.zeros(n, np.uint8)
        abi.check(abi.lib().glz_debug_read_rt_materials(self._h, _ptr(out), n))
        return out

    def debug_rt_lights(self):
        n = abi.check(abi.lib().glz_debug_read_rt_lights(self._h, None, 0))
        out = np.zeros(n, np.uint8)
        abi.check(abi.lib().glz_debug_read_rt_lights(self._h, _ptr(out), n))
        return out

    def debug_sky(self):
        n = abi.check(abi.lib().glz_debug_read_sky(self._h, None, 0))
        out = np.zeros(n, np.float32)
        abi.check(abi.lib().glz_debug_read_sky(self._h, _ptr(out), n))
        return out

    def debug_texture_level(self, texture, level):
        """HxW[x4] uint8 pixels of one mip level as the device holds it (level 0 = the texture), or None past the last level."""
        w, h = C.c_uint32(), C.c_uint32()
        n = abi.check(abi.lib().glz_debug_read_texture_level(self._h, texture, level, None, 0, C.byref(w), C.byref(h)))
        if n == 0:
            return None
        out = np.zeros(n, np.uint8)
        abi.check(abi.lib().glz_debug_read_texture_level(self._h, texture, level, _ptr(out), n, C.byref(w), C.byref(h)))
        return out.reshape(h.value, w.value) if n == w.value * h.value else out.reshape(h.value, w.value, 4)

    def debug_bvh(self):
        i = self.info()
        nodes = np.zeros((max(1, i.bvh_nodes), 16), np.uint32)
        tris = np.zeros((max(1, i.n_as_triangles), 12), np.float32)
        abi.check(abi.lib().glz_debug_read_bvh(self._h, _ptr(nodes), i.bvh_nodes, _ptr(tris), i.n_as_triangles))
        return nodes[:i.bvh_nodes], tris[:i.n_as_triangles]

    def debug_leaf_records(self):
        """The 64-byte per-leaf records the tracers read ((n, 16) uint32; a two-level scene's are its meshes' concatenated)."""
        n = abi.check(abi.lib().glz_debug_read_leaf_records(self._h, None, 0))
        out = np.zeros((max(1, n), 16), np.uint32)
        abi.check(abi.lib().glz_debug_read_leaf_records(self._h, _ptr(out), n))
        return out[:n]

    def debug_tlas_instances(self):
        """The 192-byte TlasInstance records of a two-level scene in the top level's leaf order (uint8; empty when flattened)."""
        n = abi.check(abi.lib().glz_debug_read_tlas_instances(self._h, None, 0))
        out = np.zeros(n, np.uint8)
        abi.check(abi.lib().glz_debug_read_tlas_instances(self._h, _ptr(out), n))
        return out

    def debug_instance_boxes(self, on_device, budget=0):
        """Instance boxes ((n, 4) float32 lo, hi) of a two-level scene under its current transforms: the host rule (on_device False)
        or the device kernel; budget 0 = the library's exact-box budget.  None for a flattened scene."""
        n = abi.check(abi.lib().glz_debug_instance_boxes(self._h, int(bool(on_device)), budget, None, None))
        if n == 0:
            return None
        lo, hi = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        abi.check(abi.lib().glz_debug_instance_boxes(self._h, int(bool(on_device)), budget, _ptr(lo), _ptr(hi)))
        return lo, hi

    def debug_box_kernel_ms(self):
        """device-event time (ms) of the instance-box kernels the last time they ran for this scene; -1 if never"""
        return float(abi.lib().glz_debug_box_kernel_ms(self._h))

    def debug_bvh8(self):
        """The 8-wide nodes of the same hierarchy ((n, 32) uint32; empty for two-level scenes and scenes of one leaf)."""
        n = self.info().bvh_nodes8
        nodes = np.zeros((max(1, n), 32), np.uint32)
        abi.check(abi.lib().glz_debug_read_bvh8(self._h, _ptr(nodes), n))
        return nodes[:n]

    def __del__(self):
        if getattr(self, "_h", None):
            abi.lib().glz_scene_destroy(self._h)
            self._h = None


class RayTraceRenderer:
    """lib/src/vulkan/raytracer.rs:109-687"""

    def __init__(self, handle, instance, scene, width, height):
        self._h = handle
        self.instance = instance
        self.scene = scene
        self.width, self.height = width, height

    @staticmethod
    def new(instance, scene, width, height):
        h = abi.lib().glz_renderer_create(instance._h, scene._h if scene is not None else None, width, height)
        if not h:
            raise abi.last_error()
        return RayTraceRenderer(h, instance, scene, width, height)

    def __del__(self):
        if getattr(self, "_h", None):
            abi.lib().glz_renderer_destroy(self._h)
            self._h = None

    # ---- reference API ----
    def set_integrator(self, integrator):
        abi.check(abi.lib().glz_renderer_set_integrator(self._h, integrator.value if isinstance(integrator, Integrator) else int(integrator)))

    def set_exposure(self, exposure):
        abi.check(abi.lib().glz_renderer_set_exposure(self._h, exposure))

    def update_camera(self, camera):
        abi.check(abi.lib().glz_renderer_update_camera(self._h, C.byref(camera)))

    def change_resolution(self, width, height):
        abi.check(abi.lib().glz_renderer_change_resolution(self._h, width, height))
        self.width, self.height = width, height

    def change_scene(self, scene):
        abi.check(abi.lib().glz_renderer_change_scene(self._h, scene._h))
        self.scene = scene

    def update_materials_and_lights(self, materials, lights, textures=None):
        """raytracer.rs:311-326.  textures: None (keep) or [(format, pixels, name)] replacing the scene's texture array."""
        m = (abi.Material * max(1, len(materials)))(*materials)
        l = (abi.Light * max(1, len(lights)))(*lights)
        keep = []
        t, nt = (None, 0) if textures is None else _texture_array(textures, keep)
        abi.check(abi.lib().glz_renderer_update_materials_and_lights(self._h, C.cast(m, C.c_void_p), len(materials), C.cast(l, C.c_void_p),
                                                                     len(lights), t, nt))

    def update_transforms(self, transforms):
        """Moves the instances: transforms is (n, 16) float32, column-major (as SceneDesc.transforms), n = the scene's transform count.
        The scene's structure is rebuilt for them (every renderer sharing the scene sees the move) and accumulation restarts."""
        t = _transform_array(transforms)
        abi.check(abi.lib().glz_renderer_update_transforms(self._h, _ptr(t), t.shape[0]))

    _GEOMETRY_MODES = {"refit": abi.GEOMETRY_REFIT, "rebuild": abi.GEOMETRY_REBUILD}

    def update_vertices(self, vertices, first=0, mode="refit"):
        """Deforms the meshes: vertices is an (n, 8) float32 array (position, normal, texture coordinate, as SceneDesc.vertices) or an
        abi.Vertex array, written over the scene's vertices [first, first + n).  mode 'refit' keeps the hierarchy's topology and refits
        it on the device, 'rebuild' runs the builder again; either way the scene then equals one created with the new vertices (every
        renderer sharing it sees the change) and accumulation restarts."""
        v = _vertex_array(vertices)
        abi.check(abi.lib().glz_renderer_update_vertices(self._h, _ptr(v), int(first), v.shape[0], self._GEOMETRY_MODES.get(mode, mode)))

    def add_skin(self, first, joints, weights, n_bones, blend="linear"):
        """A skin over the scene's vertices [first, first + n): joints (n, 4) integers below n_bones, weights (n, 4) float32.  The bind pose
        is what the scene's vertices hold there now.  blend: 'linear' or 'dual_quaternion', as set_skin_blend takes it.  Returns the
        skin's id; the skin is the scene's (every renderer sharing it sees it)."""
        mode = _skin_blend(blend)
        j, w = _skin_arrays(joints, weights)
        skin = abi.Skin(int(first), j.shape[0], _ptr(j), _ptr(w), int(n_bones))
        skin_id = abi.check(abi.lib().glz_renderer_add_skin(self._h, C.cast(C.byref(skin), C.c_void_p)))
        self.__dict__.setdefault("_skin_sizes", {})[skin_id] = j.shape[0]   # (add_morph(skin=...) takes its vertex count from here)
        if mode != abi.SKIN_LINEAR:
            abi.check(abi.lib().glz_renderer_set_skin_blend(self._h, skin_id, mode))
        return skin_id

    def set_skin_blend(self, skin, blend):
        """How a skin blends its bones from its next pose on: 'linear' (linear-blend skinning, the default) or 'dual_quaternion' (the
        blend is a rigid motion per vertex: joints keep their volume under twist and bend, normals stay exact).  Writes no vertex."""
        abi.check(abi.lib().glz_renderer_set_skin_blend(self._h, int(skin), _skin_blend(blend)))

    def skin_blend(self, skin):
        """'linear' or 'dual_quaternion'"""
        mode = abi.check(abi.lib().glz_renderer_skin_blend(self._h, int(skin)))
        return next(k for k, v in _SKIN_BLENDS.items() if v == mode)

    def remove_skin(self, skin):
        """Frees a skin; the vertices stay as they are."""
        abi.check(abi.lib().glz_renderer_remove_skin(self._h, int(skin)))

    @staticmethod
    def _pose_array(poses):
        """abi.Pose array of {skin id: (n_bones, 16) bones} and the arrays it points into"""
        keep = [_transform_array(b) for b in poses.values()]
        arr = (abi.Pose * max(1, len(poses)))(*[abi.Pose(int(k), _ptr(b), b.shape[0]) for k, b in zip(poses.keys(), keep)])
        return arr, keep

    def pose(self, poses, mode="refit"):
        """Poses skins on the device: poses is {skin id: (n_bones, 16) float32 bone matrices, column-major, joint_now x inverse_bind in the
        mesh's object space}.  Every named skin is written from its bind pose and the structure follows once, as update_vertices does in
        `mode`; accumulation restarts."""
        arr, keep = self._pose_array(poses)
        abi.check(abi.lib().glz_renderer_pose_skins(self._h, C.cast(arr, C.c_void_p), len(poses), self._GEOMETRY_MODES.get(mode, mode)))

    def debug_skin_timing(self, skin, bones, reps=20):
        """k_skin (k_deform with the skin step alone; k_skin_dq for a skin in that mode) alone on one skin, into a scratch buffer (the scene is untouched): milliseconds per launch, device events around reps launches"""
        arr, keep = self._pose_array({skin: bones})
        ms = C.c_float(0.0)
        abi.check(abi.lib().glz_debug_skin_timing(self._h, C.cast(arr, C.c_void_p), int(reps), C.cast(C.byref(ms), C.c_void_p)))
        return ms.value

    def add_morph(self, first, targets, skin=None, n_vertices=None):
        """Morph targets over the scene's vertices [first, first + n): targets is a list of (indices | None, d_position, d_normal), indices
        relative to `first`, strictly ascending, None = a dense target.  skin=None: free-standing, the base is what the scene's vertices
        hold there now, and n is n_vertices (or, with a dense target in the list, its length); skin=id: attached to that skin -- the base
        is the skin's bind pose, `first` must be the skin's and n is the skin's.  Returns the morph's id."""
        if n_vertices is None and skin is not None:
            n_vertices = self.__dict__.get("_skin_sizes", {}).get(int(skin))
        if n_vertices is None:
            dense = [np.asarray(t[1]).reshape(-1, 3).shape[0] for t in targets if t[0] is None]
            if not dense:
                raise ValueError("n_vertices is needed when no target is dense")
            n_vertices = dense[0]
        arr, keep = _morph_targets(targets, n_vertices)
        m = abi.Morph(int(first), int(n_vertices), C.cast(arr, C.c_void_p), len(targets), -1 if skin is None else int(skin))
        return abi.check(abi.lib().glz_renderer_add_morph(self._h, C.cast(C.byref(m), C.c_void_p)))

    def remove_morph(self, morph):
        """Frees a morph; the vertices stay as they are."""
        abi.check(abi.lib().glz_renderer_remove_morph(self._h, int(morph)))

    @classmethod
    def _animation(cls, morphs, poses):
        """abi.Animation of {morph id: weights} and {skin id: bones}, and what it points into"""
        morphs, poses = morphs or {}, poses or {}
        ws = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in morphs.values()]
        marr = (abi.MorphWeights * max(1, len(morphs)))(*[abi.MorphWeights(int(k), _ptr(w), w.shape[0]) for k, w in zip(morphs.keys(), ws)])
        parr, bones = cls._pose_array(poses)
        a = abi.Animation(C.cast(marr, C.c_void_p) if morphs else None, len(morphs), C.cast(parr, C.c_void_p) if poses else None, len(poses))
        return a, (ws, marr, parr, bones)

    def animate(self, morphs=None, poses=None, mode="refit"):
        """Morphs and poses in one update of the structure: morphs is {morph id: weights, one float32 a target}, poses {skin id: bones} as
        pose() takes them.  A free-standing morph is blended from its base; a skin whose morph is named too is morphed, then skinned, in
        one kernel; an attached morph must come with its skin's pose.  Nothing is kept between calls: every call starts from the bases."""
        a, keep = self._animation(morphs, poses)
        abi.check(abi.lib().glz_renderer_animate(self._h, C.cast(C.byref(a), C.c_void_p), self._GEOMETRY_MODES.get(mode, mode)))

    def debug_morph_timing(self, morphs, poses=None, reps=20):
        """k_morph (k_deform with the morph step alone) on one morph (morphs={id: weights}), or k_morph_skin (both steps) on an attached
        morph with its skin's pose, alone into a scratch buffer (the scene is untouched): (milliseconds per launch, the bytes one
        launch moves)"""
        a, keep = self._animation(morphs, poses)
        ms, nbytes = C.c_float(0.0), C.c_uint64(0)
        abi.check(abi.lib().glz_debug_morph_timing(self._h, C.cast(C.byref(a), C.c_void_p), int(reps), C.cast(C.byref(ms), C.c_void_p), C.cast(C.byref(nbytes), C.c_void_p)))
        return ms.value, nbytes.value

    def add_skeleton(self, skin, parents, inverse_bind, root=None):
        """A skeleton on a skin: parents (n_bones integers, -1 a root, else below the bone's own index), inverse_bind (n_bones, 16) float32,
        column-major, and root (16 floats; None: the identity), the matrix roots are multiplied under.  n_bones must be the skin's, and a
        skin has at most one skeleton.  Returns the skeleton's id; the skeleton is the scene's, as the skin is."""
        sk, keep = _skeleton_struct(skin, parents, inverse_bind, root)
        sid = abi.check(abi.lib().glz_renderer_add_skeleton(self._h, C.cast(C.byref(sk), C.c_void_p)))
        self.__dict__.setdefault("_skeleton_bones", {})[sid] = sk.n_bones   # (add_clip checks its arrays' shapes against it)
        return sid

    def remove_skeleton(self, skeleton):
        """Frees a skeleton and its clips; the vertices stay as they are."""
        abi.check(abi.lib().glz_renderer_remove_skeleton(self._h, int(skeleton)))

    def add_clip(self, skeleton, times, translations, rotations, scales=None, morph_weights=None):
        """A keyframed clip on a skeleton, uploaded once: times (n_keys,) strictly ascending, translations (n_keys, n_bones, 3), rotations
        (n_keys, n_bones, 4) as (x, y, z, w), scales (n_keys, n_bones, 3) or None (every scale 1), morph_weights (n_keys, n_targets) or
        None -- allowed when the skeleton's skin carries an attached morph with that many targets.  Returns the clip's id."""
        n_bones = self.__dict__.get("_skeleton_bones", {}).get(int(skeleton))
        if n_bones is None:
            n_bones = np.asarray(translations).shape[1] if np.asarray(translations).ndim == 3 else 0
        clip, keep = _clip_struct(skeleton, n_bones, times, translations, rotations, scales, morph_weights)
        return abi.check(abi.lib().glz_renderer_add_clip(self._h, C.cast(C.byref(clip), C.c_void_p)))

    def remove_clip(self, clip):
        """Frees a clip."""
        abi.check(abi.lib().glz_renderer_remove_clip(self._h, int(clip)))

    @staticmethod
    def _play_array(plays):
        """abi.Play array of a list of (clip id, time)"""
        plays = list(plays)
        return (abi.Play * max(1, len(plays)))(*[abi.Play(int(c), float(t)) for c, t in plays]), len(plays)

    def play(self, plays, mode="refit"):
        """Plays clips on the device: plays is a list of (clip id, time), at most one clip a skeleton.  One kernel makes every named
        skeleton's bone table (and morph weight table) from the clips' keys, each skin is then written from its bind pose, and the
        structure follows once, as pose() and animate() do in `mode`; accumulation restarts.  No bone crosses the bus."""
        arr, n = self._play_array(plays)
        abi.check(abi.lib().glz_renderer_play(self._h, C.cast(arr, C.c_void_p), n, self._GEOMETRY_MODES.get(mode, mode)))

    def debug_clip_bones(self, clip, time, n_bones, blend="linear", n_targets=0):
        """k_clip_bones alone for one play, no vertex written: the bone table as the device holds it, (n_bones, 12) float32 (three rows
        a bone) for a skin whose blend is 'linear', (n_bones, 8) for 'dual_quaternion' -- `blend` must be the skin's -- and, with
        n_targets > 0 (a clip with a weight track), (table, the (n_targets,) weight table)."""
        arr, _ = self._play_array([(clip, time)])
        rows = np.zeros((int(n_bones), 4 * (2 if _skin_blend(blend) == abi.SKIN_DUAL_QUATERNION else 3)), np.float32)
        weights = np.zeros(int(n_targets), np.float32) if n_targets else None
        abi.check(abi.lib().glz_debug_clip_bones(self._h, C.cast(arr, C.c_void_p), _ptr(rows), None if weights is None else _ptr(weights)))
        return rows if weights is None else (rows, weights)

    def debug_clip_timing(self, plays, reps=20):
        """k_clip_bones alone, one launch for all of plays (the scene is untouched): milliseconds per launch, device events around reps launches"""
        arr, n = self._play_array(plays)
        ms = C.c_float(0.0)
        abi.check(abi.lib().glz_debug_clip_timing(self._h, C.cast(arr, C.c_void_p), n, int(reps), C.cast(C.byref(ms), C.c_void_p)))
        return ms.value

    def add_normals(self, first, n_vertices, groups=None):
        """A normal set over the scene's vertices [first, first + n_vertices): from now on their normals are the normal rule
        (include/glaze_abi.h) of the positions the device holds, made again after every update_vertices, pose and animate that reaches
        them -- in place of the normals those calls write.  groups: n_vertices labels below n_vertices (equal labels share one normal),
        None = every vertex on its own, "weld" = host_weld_groups of what read_vertices gives for the range.  Returns the set's id."""
        if isinstance(groups, str):
            if groups != "weld":
                raise ValueError("groups must be labels, None or 'weld'")
            groups = host_weld_groups(self.read_vertices(first, n_vertices))
        g = _group_array(groups, n_vertices)
        s = abi.Normals(int(first), int(n_vertices), None if g is None else _ptr(g))
        return abi.check(abi.lib().glz_renderer_add_normals(self._h, C.cast(C.byref(s), C.c_void_p)))

    def remove_normals(self, normals):
        """Frees a normal set; the vertices stay as they are."""
        abi.check(abi.lib().glz_renderer_remove_normals(self._h, int(normals)))

    def debug_normals_timing(self, normals, reps=20):
        """k_face_vectors and k_vertex_normals of one set, each alone into scratch (the scene is untouched): ((milliseconds per launch of
        the face kernel, of the vertex kernel), (the bytes one launch of each moves))"""
        ms, nbytes = (C.c_float * 2)(), (C.c_uint64 * 2)()
        abi.check(abi.lib().glz_debug_normals_timing(self._h, int(normals), int(reps), C.cast(ms, C.c_void_p), C.cast(nbytes, C.c_void_p)))
        return (ms[0], ms[1]), (nbytes[0], nbytes[1])

    def read_vertices(self, first, n):
        """The scene's current vertices [first, first + n) as the device holds them: (n, 8) float32"""
        out = np.zeros((int(n), 8), np.float32)
        abi.check(abi.lib().glz_renderer_read_vertices(self._h, int(first), int(n), _ptr(out)))
        return out

    def geometry_update_info(self):
        """glz_geometry_update_info of the scene's last update_vertices: mode, meshes_touched, update_ms and the box-area figures whose
        ratio box_area / box_area_built says how far a refitted tree has degraded.  Raises GlazeError before any update."""
        i = abi.GeometryUpdateInfo()
        abi.check(abi.lib().glz_renderer_geometry_update_info(self._h, C.byref(i)))
        return i

    def refresh_binded_textures(self, textures):
        """raytracer.rs:328-356: new texture array under the same materials and lights; accumulation continues."""
        keep = []
        t, nt = _texture_array(textures, keep)
        abi.check(abi.lib().glz_renderer_refresh_binded_textures(self._h, t, nt))

    def set_texture_lod(self, mode):
        """0 = level 0 always (the reference's ray-tracing stages), 1 = ray-cone level of detail over the mip chain, 2 = ray cones
        with an anisotropic footprint (up to 16 probes along the footprint's long axis).  Restarts."""
        abi.check(abi.lib().glz_renderer_set_texture_lod(self._h, int(mode)))

    def set_devices(self, devices):
        """Render on several GPUs of this process (tiles t % n == i on devices[i], RCCL exchange onto devices[0] at every read-back);
        devices[0] must be the instance's device.  [d] returns to one device."""
        arr = (C.c_int * len(devices))(*devices)
        abi.check(abi.lib().glz_renderer_set_devices(self._h, arr, len(devices)))

    def set_launch_mode(self, mode):
        """'auto' (by the pixels this device owns), 'two_kernels' (k_trace + k_shade per launch) or 'path' (the per-wave launch loop, k_path);
        the image does not depend on it"""
        abi.check(abi.lib().glz_renderer_set_launch_mode(self._h, {"auto": 0, "two_kernels": 1, "path": 2}[mode]))

    def launch_mode(self):
        return {1: "two_kernels", 2: "path"}[int(abi.lib().glz_renderer_launch_mode(self._h))]

    def set_node_width(self, width):
        """0 (by the pixels this device owns), 4 (k_trace over the 4-wide nodes) or 8 (k_trace8 over the 8-wide nodes: small tile shares);
        the image does not depend on it"""
        abi.check(abi.lib().glz_renderer_set_node_width(self._h, int(width)))

    def node_width(self):
        return int(abi.lib().glz_renderer_node_width(self._h))

    def device_count(self):
        return int(abi.lib().glz_renderer_device_count(self._h))

    def device_scene_info(self, i):
        """scene info of the replica device i of set_devices renders (0 = this renderer's own scene)"""
        info = abi.SceneInfo()
        abi.check(abi.lib().glz_renderer_device_scene_info(self._h, i, C.byref(info)))
        return info

    def set_chains(self, n):
        """Concurrent launch chains over this rank's tiles (0 = automatic); the image does not depend on it."""
        abi.check(abi.lib().glz_renderer_set_chains(self._h, n))

    def wait_idle(self):
        abi.check(abi.lib().glz_renderer_wait_idle(self._h))

    def steps_per_sample(self):
        return abi.lib().glz_renderer_steps_per_sample(self._h)

    def draw(self, spp, callback=None, want_image=True):
        """draw(spp, callback) -> HxWx4 uint8 sRGB image (raytracer.rs:615-687)."""
        out = np.zeros((self.height, self.width, 4), np.uint8) if want_image else None
        cb = abi.DRAW_CALLBACK((lambda _u: callback()) if callback else (lambda _u: None))
        abi.check(abi.lib().glz_renderer_draw(self._h, spp, C.cast(cb, C.c_void_p) if callback else None, None, _ptr(out) if want_image else None))
        return out

    # ---- progressive API (draw_frame) ----
    def restart(self):
        abi.check(abi.lib().glz_renderer_restart(self._h))

    def step(self, n=1):
        abi.check(abi.lib().glz_renderer_step(self._h, n))

    def read_rgba8(self):
        out = np.zeros((self.height, self.width, 4), np.uint8)
        abi.check(abi.lib().glz_renderer_read_rgba8(self._h, _ptr(out)))
        return out

    # ---- build-defined extensions ----
    def set_seed(self, seed):
        abi.check(abi.lib().glz_renderer_set_seed(self._h, seed))

    def set_depth(self, pt_steps):
        abi.check(abi.lib().glz_renderer_set_depth(self._h, pt_steps))

    def read_hdr(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        abi.check(abi.lib().glz_renderer_read_hdr(self._h, _ptr(out)))
        return out

    def read_result(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        abi.check(abi.lib().glz_renderer_read_result(self._h, _ptr(out)))
        return out

    # ---- post: first-hit feature buffers and the denoiser ----
    def read_aov(self, name):
        """Runs the first-hit pass (one centre ray per pixel, the whole frame) and returns one of its planes, H x W x 4 float32:
        'normal_depth' (or 0) = (shading normal facing the camera, hit distance; +inf for a miss), 'albedo_instance' (or 1) = (albedo,
        the bits of the instance index; view the last channel as uint32, 0xFFFFFFFF for a miss)."""
        which = {"normal_depth": abi.AOV_NORMAL_DEPTH, "albedo_instance": abi.AOV_ALBEDO_INSTANCE}.get(name, name)
        out = np.zeros((self.height, self.width, 4), np.float32)
        abi.check(abi.lib().glz_renderer_read_aov(self._h, which, _ptr(out)))
        return out

    def set_denoise(self, **params):
        """the fields of glz_denoise_params; those left out take the library's defaults.  Accumulation goes on."""
        p = abi.DenoiseParams(**params)
        abi.check(abi.lib().glz_renderer_set_denoise(self._h, C.cast(C.byref(p), C.c_void_p)))

    def read_denoised(self, want_rgba8=False):
        """The result image through the denoiser: H x W x 4 float32, and with want_rgba8 also its 8-bit sRGB image (a pair)."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        img = np.zeros((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        abi.check(abi.lib().glz_renderer_read_denoised(self._h, _ptr(out), _ptr(img) if want_rgba8 else None))
        return (out, img) if want_rgba8 else out

    def set_despeckle(self, enabled=True, **params):
        """Firefly rejection (glz_despeckle_params: radius, trim, ratio; those left out take the library's defaults).  enabled: read_denoised
        runs it ahead of the filter; read_despeckled applies it whatever the flag says.  Accumulation goes on."""
        p = abi.DespeckleParams(**params)
        abi.check(abi.lib().glz_renderer_set_despeckle(self._h, 1 if enabled else 0, C.cast(C.byref(p), C.c_void_p)))

    def despeckle(self):
        """(enabled, dict of the parameters in force)"""
        p = abi.DespeckleParams()
        on = abi.check(abi.lib().glz_renderer_despeckle(self._h, C.cast(C.byref(p), C.c_void_p)))
        return bool(on), dict(radius=p.radius, trim=p.trim, ratio=p.ratio)

    def read_despeckled(self, want_rgba8=False):
        """The result image through the firefly rejection alone (no filter pass): H x W x 4 float32, and with want_rgba8 also its 8-bit
        sRGB image (a pair)."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        img = np.zeros((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        abi.check(abi.lib().glz_renderer_read_despeckled(self._h, _ptr(out), _ptr(img) if want_rgba8 else None))
        return (out, img) if want_rgba8 else out

    def _previous_state(self, prev_camera, prev_transforms, prev_vertices, first_vertex):
        """abi.PreviousState and the arrays it points into (keep them alive as long as the state is used)"""
        t = None if prev_transforms is None else _transform_array(prev_transforms)
        v = None if prev_vertices is None else _vertex_array(prev_vertices)
        state = abi.PreviousState(C.cast(C.byref(prev_camera), C.c_void_p), None if t is None else _ptr(t), 0 if t is None else t.shape[0],
                                  None if v is None else _ptr(v), int(first_vertex), 0 if v is None else v.shape[0])
        return state, (prev_camera, t, v)

    def read_motion(self, prev_camera, prev_transforms=None, prev_vertices=None, first_vertex=0, prev_poses=None, prev_morphs=None):
        """The motion plane (include/glaze_abi.h holds the specification): H x W x 4 float32, per pixel (where the first hit of the centre
        ray was on screen under prev_camera, prev_transforms and prev_vertices, minus the pixel's own centre; its distance from the previous
        eye; the hit's instance bits).  prev_transforms: (n, 16) float32 as update_transforms takes them, None = the instances did not move.
        prev_vertices: what the scene's vertices [first_vertex, first_vertex + n) held in the previous frame, in any form update_vertices
        takes, None = the meshes did not deform.  prev_poses: {skin id: bones} as pose() takes them, the PREVIOUS frame's -- the previous
        vertices are then made on the device (prev_vertices must be None).  prev_morphs: {morph id: weights} as animate() takes them, the
        PREVIOUS frame's, with prev_poses as animate() would need them.  Accumulation goes on."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        if prev_morphs is not None:
            state, keep = self._previous_state(prev_camera, prev_transforms, prev_vertices, first_vertex)
            a, keep_animation = self._animation(prev_morphs, prev_poses)
            abi.check(abi.lib().glz_renderer_read_motion_animated(self._h, C.cast(C.byref(state), C.c_void_p), C.cast(C.byref(a), C.c_void_p), _ptr(out)))
            return out
        if prev_poses is not None:
            state, keep = self._previous_state(prev_camera, prev_transforms, prev_vertices, first_vertex)
            arr, keep_bones = self._pose_array(prev_poses)
            abi.check(abi.lib().glz_renderer_read_motion_posed(self._h, C.cast(C.byref(state), C.c_void_p), C.cast(arr, C.c_void_p), len(prev_poses), _ptr(out)))
            return out
        if prev_vertices is not None:
            state, keep = self._previous_state(prev_camera, prev_transforms, prev_vertices, first_vertex)
            abi.check(abi.lib().glz_renderer_read_motion_from(self._h, C.cast(C.byref(state), C.c_void_p), _ptr(out)))
            return out
        t = None if prev_transforms is None else _transform_array(prev_transforms)
        abi.check(abi.lib().glz_renderer_read_motion(self._h, C.cast(C.byref(prev_camera), C.c_void_p), None if t is None else _ptr(t), 0 if t is None else t.shape[0],
                                                     _ptr(out)))
        return out

    def debug_motion_timing(self, prev_camera, prev_transforms=None, prev_vertices=None, first_vertex=0):
        """read_motion's pass without the read-back: the device-event time of k_motion alone (with prev_vertices: of k_motion_deform), in
        milliseconds"""
        ms = C.c_float(0.0)
        if prev_vertices is not None:
            state, keep = self._previous_state(prev_camera, prev_transforms, prev_vertices, first_vertex)
            abi.check(abi.lib().glz_debug_motion_timing_from(self._h, C.cast(C.byref(state), C.c_void_p), C.cast(C.byref(ms), C.c_void_p)))
            return ms.value
        t = None if prev_transforms is None else _transform_array(prev_transforms)
        abi.check(abi.lib().glz_debug_motion_timing(self._h, C.cast(C.byref(prev_camera), C.c_void_p), None if t is None else _ptr(t), 0 if t is None else t.shape[0],
                                                    C.cast(C.byref(ms), C.c_void_p)))
        return ms.value

    def reproject(self, prev_camera, prev_color, prev_aov0, prev_aov1, prev_transforms=None, prev_vertices=None, first_vertex=0, prev_poses=None, prev_morphs=None, **params):
        """The previous frame's colour carried to this frame's pixels with disocclusion rejection: H x W x 4 float32 (rgb, confidence
        0 .. 1).  prev_color: any H x W x 4 image of the previous frame; prev_aov0 / prev_aov1: read_aov(0) / read_aov(1) of the previous
        state in first-hit mode; prev_transforms, prev_vertices, first_vertex, prev_poses, prev_morphs: as read_motion takes them; params: glz_reproject_params
        (depth_tolerance).  Accumulation goes on."""
        shape = (self.height, self.width, 4)
        c, a0, a1 = (np.ascontiguousarray(f, np.float32) for f in (prev_color, prev_aov0, prev_aov1))
        if c.shape != shape or a0.shape != shape or a1.shape != shape:
            raise ValueError("prev_color, prev_aov0 and prev_aov1 must be H x W x 4 of the renderer's size")
        out = np.zeros(shape, np.float32)
        p = abi.ReprojectParams(**params)
        if prev_morphs is not None:
            state, keep = self._previous_state(prev_camera, prev_transforms, prev_vertices, first_vertex)
            a, keep_animation = self._animation(prev_morphs, prev_poses)
            abi.check(abi.lib().glz_renderer_reproject_animated(self._h, C.cast(C.byref(state), C.c_void_p), C.cast(C.byref(a), C.c_void_p), _ptr(c), _ptr(a0), _ptr(a1),
                                                                C.cast(C.byref(p), C.c_void_p), _ptr(out)))
            return out
        if prev_poses is not None:
            state, keep = self._previous_state(prev_camera, prev_transforms, prev_vertices, first_vertex)
            arr, keep_bones = self._pose_array(prev_poses)
            abi.check(abi.lib().glz_renderer_reproject_posed(self._h, C.cast(C.byref(state), C.c_void_p), C.cast(arr, C.c_void_p), len(prev_poses), _ptr(c), _ptr(a0),
                                                             _ptr(a1), C.cast(C.byref(p), C.c_void_p), _ptr(out)))
            return out
        if prev_vertices is not None:
            state, keep = self._previous_state(prev_camera, prev_transforms, prev_vertices, first_vertex)
            abi.check(abi.lib().glz_renderer_reproject_from(self._h, C.cast(C.byref(state), C.c_void_p), _ptr(c), _ptr(a0), _ptr(a1), C.cast(C.byref(p), C.c_void_p),
                                                            _ptr(out)))
            return out
        t = None if prev_transforms is None else _transform_array(prev_transforms)
        abi.check(abi.lib().glz_renderer_reproject(self._h, C.cast(C.byref(prev_camera), C.c_void_p), None if t is None else _ptr(t), 0 if t is None else t.shape[0],
                                                   _ptr(c), _ptr(a0), _ptr(a1), C.cast(C.byref(p), C.c_void_p), _ptr(out)))
        return out

    _GUIDE_MODES = {"first_hit": abi.GUIDE_FIRST_HIT, "through_specular": abi.GUIDE_THROUGH_SPECULAR}

    def set_guide_mode(self, mode, max_bounces=4):
        """Which surface read_aov and read_denoised take their planes from: 'first_hit' (the default) or 'through_specular', which follows
        the path's own ray through Mirror and Glass to the first vertex that is not specular, at most max_bounces (1 .. 8) bounces
        (include/glaze_abi.h holds the specification).  Accumulation goes on."""
        abi.check(abi.lib().glz_renderer_set_guide_mode(self._h, self._GUIDE_MODES.get(mode, mode), int(max_bounces)))

    def guide_mode(self):
        """(mode name, max_bounces) in force; max_bounces means nothing in 'first_hit'"""
        b = C.c_uint32()
        mode = abi.check(abi.lib().glz_renderer_guide_mode(self._h, C.byref(b)))
        return {v: k for k, v in self._GUIDE_MODES.items()}[mode], b.value

    def debug_guide_chain(self, segment):
        """the rays of segment `segment` of every pixel's guide chain under the mode in force (0 = the camera rays): origins, directions
        (H x W x 3 float32, zero where the chain has no such segment) and alive (H x W bool)"""
        o = np.zeros((self.height, self.width, 3), np.float32)
        d = np.zeros((self.height, self.width, 3), np.float32)
        alive = np.zeros((self.height, self.width), np.uint8)
        abi.check(abi.lib().glz_debug_guide_chain(self._h, int(segment), _ptr(o), _ptr(d), _ptr(alive)))
        return o, d, alive.astype(bool)

    def debug_camera_rays(self, offset=(0.5, 0.5)):
        """camera_ray() of every pixel at one sub-pixel offset, on the device: origins, directions (H x W x 3 float32 each)"""
        o = np.zeros((self.height, self.width, 3), np.float32)
        d = np.zeros((self.height, self.width, 3), np.float32)
        abi.check(abi.lib().glz_debug_camera_rays(self._h, float(offset[0]), float(offset[1]), _ptr(o), _ptr(d)))
        return o, d

    def debug_post_timing(self):
        """one run of the post stages between device events, ms: {'first_hit_trace', 'first_hit_attributes', 'demodulate', 'passes': [...]}"""
        ms = np.zeros(abi.POST_TIMING_SLOTS, np.float32)
        abi.check(abi.lib().glz_debug_post_timing(self._h, _ptr(ms)))
        return {"first_hit_trace": float(ms[0]), "first_hit_attributes": float(ms[1]), "demodulate": float(ms[2]), "passes": [float(x) for x in ms[3:]]}

    def launch_constants(self, launch):
        s = C.c_uint32()
        off = (C.c_float * 2)()
        abi.check(abi.lib().glz_renderer_launch_constants(self._h, launch, C.byref(s), off))
        return s.value, (off[0], off[1])

    def push_constants(self):
        out = np.zeros(32, np.float32)
        abi.check(abi.lib().glz_renderer_push_constants(self._h, _ptr(out)))
        return out

    def set_partition(self, rank, world):
        abi.check(abi.lib().glz_renderer_set_partition(self._h, rank, world))

    def export_device(self, which, device_ptr):
        abi.check(abi.lib().glz_renderer_export_device(self._h, which, C.c_void_p(device_ptr)))

    def packed_pixels(self, rank, world):
        """pixels (of 4 floats) in the packed tiles of partition (rank, world) of this renderer's frame"""
        return int(abi.lib().glz_renderer_packed_pixels(self._h, rank, world))

    def export_packed(self, which, device_ptr):
        """this rank's tiles only, tile-major, into a device buffer of packed_pixels(rank, world) x 4 floats"""
        abi.check(abi.lib().glz_renderer_export_packed(self._h, which, C.c_void_p(device_ptr)))

    def scatter_packed(self, rank, world, packed_ptr, frame_ptr):
        """rank 0: puts the packed tiles received from `rank` into their place of a full-frame device buffer"""
        abi.check(abi.lib().glz_renderer_scatter_packed(self._h, rank, world, C.c_void_p(packed_ptr), C.c_void_p(frame_ptr)))

    def scatter_packed_all(self, world, packed_ptr, stride_pixels, frame_ptr):
        """the receiving side of a gather in one call: the parts of ranks 0 .. world - 1 lie `stride_pixels` pixels apart in one device buffer"""
        abi.check(abi.lib().glz_renderer_scatter_packed_all(self._h, world, C.c_void_p(packed_ptr), stride_pixels, C.c_void_p(frame_ptr)))

    def tonemap_device(self, device_ptr):
        out = np.zeros((self.height, self.width, 4), np.uint8)
        abi.check(abi.lib().glz_renderer_tonemap_device(self._h, C.c_void_p(device_ptr), _ptr(out)))
        return out

    def enable_counters(self, counters=False, kernel_timing=True):
        abi.check(abi.lib().glz_renderer_enable_counters(self._h, (1 if counters else 0) | (2 if kernel_timing else 0)))

    def stats(self):
        s = abi.RenderStats()
        abi.check(abi.lib().glz_renderer_get_stats(self._h, C.byref(s)))
        return s
