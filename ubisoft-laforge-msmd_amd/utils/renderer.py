"""Mesh renderer on the MI355X (surface of reference utils/renderer.py:14-128, which draws through pyrender / EGL).

An Instinct card has no graphics pipe, so the image is made by two compute launches (csrc/render.hip):
vertex normals + camera + projection, then a z-buffered 64 x 64-tile rasteriser with Lambert shading; a texture adds a third,
deferred launch that shades the covered pixels from a mip pyramid.  Coverage and depth
follow the OpenGL conventions the reference's renderer works under (pixel centres at +0.5, top-left fill rule, row 0 at the
top, eye depth with 0 for the background as pyrender returns it); the shading model is this project's own (Lambert + ambient on
the reference's base colour, lights and ambient level), not pyrender's metallic-roughness shader, so colours are not pixel-equal.
There is NO CLIPPING: a face with a vertex nearer than `near` is dropped whole.

Texture (tex_img + tex_uv = {'vt', 'ft'}) follows the ordinary OpenGL / OBJ conventions: GL_REPEAT wrap, GL_LINEAR
magnification, GL_LINEAR_MIPMAP_LINEAR minification with an analytic per-pixel level of detail, v up, no sRGB conversion.  The
texel replaces the base colour of the shading model above.  `vt` is indexed per corner through `ft`, so a seam needs no
duplicated vertex (the reference writes an OBJ file and reloads it for that), and normals stay those of the topology `f`.

Per-vertex colours (vertex_colors, (V, 3 | 4) or per frame (B, V, 3 | 4) uint8) replace the base colour with the colour
interpolated from the face's corners with the perspective-correct weights: lit like a texel, or with ``lit=False`` stored as it
is, which is how a heat map of a scalar on the vertices is drawn (utils/metrics.render_comparison).

``samples=4`` draws anti-aliased: coverage, depth and shading at four sample points per pixel (the rotated grid (96, 32),
(224, 96), (32, 160), (160, 224) in 1/256 pixel units from the pixel's top-left corner), each exactly as the pixel centre is
treated at one sample, resolved by the rounded mean of the four samples' bytes, an uncovered sample counting as the
background.  ``samples=1``, the default, is the pixel-centre renderer and its bits.

``render_mesh`` keeps the reference's signature and returns numpy arrays; ``render_vertices`` takes the (B, V, 3) device
tensor FLAME produces and leaves colour and depth on the device.
"""
from __future__ import annotations

import hashlib

import numpy as np

import torch

from .. import ops


def vertex_face_csr(faces, n_vertices):
    """Vertex -> incident-face table of a triangle list: (offsets (V + 1) int32, face ids (3 F) int32).  The faces of vertex
    v are ids[offsets[v]:offsets[v + 1]], ascending, each face once (a face that repeats a vertex is still one face);
    the tail of `ids` beyond offsets[V] is padding (-1).  Raises ValueError on a vertex id outside [0, V)."""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    V, Fc = int(n_vertices), f.shape[0]
    if Fc == 0:
        raise ValueError("faces is empty")
    if f.min() < 0 or f.max() >= V:
        raise ValueError(f"faces refer to vertices outside [0, {V})")
    pairs = np.unique(f.reshape(-1) * Fc + np.repeat(np.arange(Fc, dtype=np.int64), 3))    # sorted by (vertex, face)
    vert, face = pairs // Fc, pairs % Fc
    offsets = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(vert, minlength=V), out=offsets[1:])
    ids = np.full(3 * Fc, -1, np.int32)
    ids[:face.shape[0]] = face
    return offsets.astype(np.int32), ids


def validate_texture(tex_img, tex_uv, n_faces):
    """tex_img (Ht, Wt, 3 | 4) uint8 with 1 <= Ht, Wt <= 4096 and tex_uv = {'vt': (Nt, 2) float, 'ft': (F, 3) integer} with F =
    n_faces -> (image, vt float32, ft int32), contiguous numpy arrays.  TypeError for a wrong container, shape or dtype (an
    image that is not uint8 included), ValueError for an image size outside the limits, `ft` rows != n_faces or an `ft` entry
    outside [0, Nt)."""
    img = np.asarray(tex_img)
    if img.dtype != np.uint8:
        raise TypeError(f"tex_img must be uint8, got {img.dtype}")
    if img.ndim != 3 or img.shape[2] not in (3, 4):
        raise TypeError(f"tex_img must have shape (Ht, Wt, 3) or (Ht, Wt, 4), got {img.shape}")
    if not (1 <= img.shape[0] <= ops.TEXTURE_MAX_SIDE and 1 <= img.shape[1] <= ops.TEXTURE_MAX_SIDE):
        raise ValueError(f"a {img.shape[0]} x {img.shape[1]} texture is outside [1, {ops.TEXTURE_MAX_SIDE}]")
    try:
        vt, ft = tex_uv["vt"], tex_uv["ft"]
    except (TypeError, KeyError, IndexError) as e:
        raise TypeError("tex_uv must be a mapping with 'vt' (Nt, 2) and 'ft' (F, 3)") from e
    vt, ft = np.asarray(vt), np.asarray(ft)
    if not np.issubdtype(vt.dtype, np.floating) or vt.ndim != 2 or vt.shape[1] != 2 or vt.shape[0] == 0:
        raise TypeError(f"tex_uv['vt'] must be a float (Nt, 2) array, got {vt.dtype} {vt.shape}")
    if not np.issubdtype(ft.dtype, np.integer) or ft.ndim != 2 or ft.shape[1] != 3:
        raise TypeError(f"tex_uv['ft'] must be an integer (F, 3) array, got {ft.dtype} {ft.shape}")
    if ft.shape[0] != int(n_faces):
        raise ValueError(f"tex_uv['ft'] has {ft.shape[0]} rows for {int(n_faces)} faces")
    ft = ft.astype(np.int64)
    if ft.min() < 0 or ft.max() >= vt.shape[0]:
        raise ValueError(f"tex_uv['ft'] refers to texture coordinates outside [0, {vt.shape[0]})")
    return np.ascontiguousarray(img), np.ascontiguousarray(vt, np.float32), np.ascontiguousarray(ft.astype(np.int32))


def vertex_color_table(vertex_colors, n_frames, n_vertices, device):
    """vertex_colors (V, 3 | 4) or (B, V, 3 | 4) uint8, a tensor or anything numpy reads -> the contiguous (V, 4) / (B, V, 4) uint8
    table on `device` (three channels padded once with alpha 255).  TypeError for a dtype other than uint8, ValueError for a shape
    that is neither; both name the expected shape."""
    B, V = int(n_frames), int(n_vertices)
    want = f"({V}, 3 | 4) or ({B}, {V}, 3 | 4) uint8"
    c = vertex_colors if torch.is_tensor(vertex_colors) else torch.from_numpy(np.ascontiguousarray(vertex_colors))
    if c.dtype != torch.uint8:
        raise TypeError(f"vertex_colors must be {want}, got dtype {c.dtype}")
    if c.dim() not in (2, 3) or c.shape[-1] not in (3, 4) or c.shape[-2] != V or (c.dim() == 3 and c.shape[0] != B):
        raise ValueError(f"vertex_colors must be {want}, got shape {tuple(c.shape)}")
    c = c.detach().to(device)
    if c.shape[-1] == 3:
        c = torch.cat([c, torch.full_like(c[..., :1], 255)], dim=-1)
    return c.contiguous()


def _content_key(x):
    """Cache key of a tensor (its storage and version) or of anything numpy reads (its contents)."""
    if torch.is_tensor(x):
        return ("t", x.data_ptr(), tuple(x.shape), x.dtype, str(x.device), x._version)
    x = np.ascontiguousarray(x)
    return ("n", hashlib.sha1(x.tobytes()).hexdigest(), x.shape, str(x.dtype))


def rodrigues(r):
    """3 x 3 rotation of the axis-angle vector r as cv2.Rodrigues defines it: angle = |r|, identity at 0 (float64)."""
    r = np.asarray(r, np.float64).reshape(3)
    th = float(np.sqrt(r @ r))
    if th == 0.0:
        return np.eye(3)
    k = r / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + (1.0 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


class MeshRenderer:
    def __init__(self, size, fov=16 / 180 * np.pi, camera_pose=None, light_pose=None, black_bg=False, samples=1):
        self.width, self.height = int(size[0]), int(size[1])       # the reference hands `size` on as (width, height)
        if not (0 < self.width <= 16384 and 0 < self.height <= 16384):
            raise ValueError(f"size {size} is outside (0, 16384]")
        if samples not in ops.RENDER_SAMPLES:
            raise ValueError(f"samples must be one of {ops.RENDER_SAMPLES}, got {samples!r}")
        self.samples = int(samples)
        self.fov = float(fov)
        self.frustum = {"near": 0.01, "far": 3.0}
        self.base_color = np.array([0.3, 0.3, 0.3])
        self.ambient = np.array([0.2, 0.2, 0.2])
        self.light_intensity = 2.0
        self.light_angle = np.pi / 6.0
        self.bg_color = (0, 0, 0) if black_bg else (255, 255, 255)
        if camera_pose is None:
            camera_pose = np.eye(4)
            camera_pose[:3, 3] = np.array([0, 0, 1])
        if light_pose is None:
            light_pose = np.eye(4)
            light_pose[:3, 3] = np.array([0, 0, 1])
        self._consts = {}          # device -> (view, shade, lights)
        self._csr = {}             # faces key -> (faces int32, offsets, ids) on the device
        self._tex = {}             # texture key -> (pyramid, vt, ft, Ht, Wt) on the device
        self.set_camera_pose(camera_pose)
        self.set_lighting_pose(light_pose)

    # ------------------------------------------------------------------ scene state
    def set_camera_pose(self, camera_pose):
        self.camera_pose = np.array(camera_pose, np.float64)
        self._consts.clear()

    def set_lighting_pose(self, light_pose):
        self.light_pose = np.array(light_pose, np.float64)
        self.light_poses = self._get_light_poses(self.light_angle, self.light_pose.copy())
        self._consts.clear()

    @staticmethod
    def _get_light_poses(light_angle, light_pose):
        """Five poses: the given one and four whose POSITION is turned by +-light_angle about x and y (reference
        utils/renderer.py:110-128).  The rotation part is left alone and a directional light has no position, so all five
        shine along the given pose's -z axis: kept as the reference has it."""
        origin = light_pose[:3, 3].copy()
        poses = [light_pose.copy()]
        for axis in ([light_angle, 0, 0], [-light_angle, 0, 0], [0, -light_angle, 0], [0, light_angle, 0]):
            p = light_pose.copy()
            p[:3, 3] = rodrigues(axis) @ origin
            poses.append(p)
        return poses

    def _device_consts(self, device):
        key = str(device)
        if key not in self._consts:
            world_to_eye = np.linalg.inv(self.camera_pose)
            lights = np.zeros((len(self.light_poses), 4), np.float32)
            for k, pose in enumerate(self.light_poses):
                d = world_to_eye[:3, :3] @ pose[:3, 2]                 # towards the light: the pose's +z axis, in eye space
                lights[k, :3] = d / np.linalg.norm(d)
                lights[k, 3] = self.light_intensity
            shade = np.concatenate([self.base_color, self.ambient]).astype(np.float32)
            view = np.ascontiguousarray(world_to_eye[:3, :], np.float32)
            self._consts[key] = tuple(torch.from_numpy(a).to(device) for a in (view, shade, lights))
        return self._consts[key]

    def _tables(self, faces, n_vertices, device):
        """faces (tensor or array) -> (faces int32 (F, 3), csr offsets, csr face ids) on `device`, cached per faces object
        (a tensor by its storage and version, an array by its contents)."""
        if torch.is_tensor(faces):
            key = ("t", faces.data_ptr(), tuple(faces.shape), faces.dtype, str(faces.device), faces._version, n_vertices, str(device))
        else:
            faces = np.ascontiguousarray(faces)
            key = ("n", hashlib.sha1(faces.tobytes()).hexdigest(), faces.shape, str(faces.dtype), n_vertices, str(device))
        hit = self._csr.get(key)
        if hit is None:
            host = faces.detach().cpu().numpy() if torch.is_tensor(faces) else faces
            host = host.astype(np.int64).reshape(-1, 3)
            off, ids = vertex_face_csr(host, n_vertices)
            if len(self._csr) >= 8:
                self._csr.pop(next(iter(self._csr)))
            # the tensor itself is kept with its tables, so its storage cannot be recycled under the key
            hit = (faces, torch.from_numpy(host.astype(np.int32)).to(device), torch.from_numpy(off).to(device),
                   torch.from_numpy(ids).to(device))
            self._csr[key] = hit
        return hit[1:]

    def _texture(self, tex_img, tex_uv, n_faces, device):
        """tex_img, tex_uv -> (pyramid (n_texels, 4) fp32, vt (Nt, 2) fp32, ft (F, 3) int32, Ht, Wt) on `device`, cached per
        texture (tensors by their storage and version, arrays by their contents); at most 4 textures are kept."""
        try:
            parts = (tex_img, tex_uv["vt"], tex_uv["ft"])
        except (TypeError, KeyError, IndexError) as e:
            raise TypeError("tex_uv must be a mapping with 'vt' (Nt, 2) and 'ft' (F, 3)") from e
        key = tuple(_content_key(x) for x in parts) + (int(n_faces), str(device))
        hit = self._tex.get(key)
        if hit is None:
            host = [x.detach().cpu().numpy() if torch.is_tensor(x) else x for x in parts]
            img, vt, ft = validate_texture(host[0], {"vt": host[1], "ft": host[2]}, n_faces)
            pyramid = ops.texture_pyramid(torch.from_numpy(img).to(device))
            if len(self._tex) >= 4:
                self._tex.pop(next(iter(self._tex)))
            # the objects themselves are kept with their tables, so a tensor's storage cannot be recycled under the key
            hit = (parts, pyramid, torch.from_numpy(vt).to(device), torch.from_numpy(ft).to(device), img.shape[0], img.shape[1])
            self._tex[key] = hit
        return hit[1:]

    # ------------------------------------------------------------------ rendering
    def render_vertices(self, vertices, faces, t_center=None, rot=None, return_face_id=False, return_screen=False, tex_img=None,
                        tex_uv=None, return_uv=False, vertex_colors=None, lit=True):
        """vertices (B, V, 3) CUDA tensor (fp32, or fp16 / bf16: cast) -> colour (B, H, W, 3) uint8 (a view of the RGBA
        buffer) and eye depth (B, H, W) fp32 (0 = background), both on the device.  rot: (3,) or (B, 3) axis-angle about
        t_center (3,) per frame.  return_face_id appends the winning face id per pixel (int32, -1 = background);
        return_screen appends the vertex stage's screen (B, V, 3) = (x_s, y_s, depth) and eye-space normals (B, V, 3).
        tex_img (Ht, Wt, 3 | 4) uint8 with tex_uv = {'vt': (Nt, 2), 'ft': (F, 3)} (validate_texture) draws the mesh textured;
        return_uv (textured only) appends (u, v, level of detail) per pixel, (B, H, W, 3) fp32 with zeros on the background.
        With samples=4 colour is the resolve of the four samples, depth the least depth over the pixel's covered samples, the
        face id is per sample, (B, H, W, 4), and return_uv is a ValueError.
        vertex_colors (V, 3 | 4) uint8 shared by the frames, or (B, V, 3 | 4) per frame, a device tensor or a numpy array (alpha
        ignored), draws the mesh in the colours interpolated from its vertices: under the lighting as a texel
        is, or with lit=False as they are, the same everywhere on the face.  Together with tex_img it is a TypeError."""
        if vertex_colors is not None and (tex_img is not None or tex_uv is not None):
            raise TypeError("vertex_colors and a texture are not drawn together: give one of them")
        if (tex_img is None) != (tex_uv is None):
            if tex_uv is None:
                raise NotImplementedError("a texture needs a uv table: tex_uv = {'vt', 'ft'} (there are no default per-vertex "
                                          "texture coordinates)")
            raise TypeError("tex_uv is given without tex_img")
        if return_uv and tex_img is None:
            raise TypeError("return_uv needs tex_img and tex_uv")
        if return_uv and self.samples != 1:
            raise ValueError("return_uv is per pixel: it is not offered at four samples per pixel")
        if not torch.is_tensor(vertices) or not vertices.is_cuda or vertices.dim() != 3 or vertices.shape[2] != 3:
            raise TypeError("vertices must be a (B, V, 3) CUDA tensor")
        device = vertices.device
        verts = vertices.detach().float().contiguous()
        B, V, _ = verts.shape
        vcol = None if vertex_colors is None else vertex_color_table(vertex_colors, B, V, device)      # refused before a launch
        faces_d, off, ids = self._tables(faces, V, device)
        view, shade, lights = self._device_consts(device)
        rot_d = tc_d = None
        if rot is not None:
            rot_d = torch.as_tensor(rot, dtype=torch.float32, device=device).reshape(-1, 3).expand(B, 3).contiguous()
            tc = np.zeros(3) if t_center is None else t_center
            tc_d = torch.as_tensor(tc, dtype=torch.float32, device=device).reshape(3).contiguous()
        focal = 1.0 / np.tan(self.fov / 2.0)
        screen, normals = ops.render_vertices(verts, faces_d, off, ids, view, focal, self.height, self.width, tc_d, rot_d)
        r, g, b = self.bg_color
        background = r | g << 8 | b << 16 | 255 << 24
        rgba, depth, face_id = ops.render_raster(screen, normals, faces_d, shade, lights, self.height, self.width,
                                                 self.frustum["near"], self.frustum["far"], background,
                                                 want_face_id=return_face_id or tex_img is not None or vcol is not None,
                                                 samples=self.samples)
        if vcol is not None:
            ops.render_shade_vertex_color(screen, normals, faces_d, vcol, shade, lights, face_id, rgba, self.frustum["near"],
                                          lit=lit, samples=self.samples, background=background)
        uvl = None
        if tex_img is not None:
            pyramid, vt, ft, tex_h, tex_w = self._texture(tex_img, tex_uv, faces_d.shape[0], device)
            uvl = ops.render_shade_textured(screen, normals, faces_d, vt, ft, pyramid, tex_h, tex_w, shade, lights, face_id, rgba,
                                            self.frustum["near"], want_uvl=return_uv, samples=self.samples, background=background)
        out = (rgba[..., :3], depth)
        if return_face_id:
            out += (face_id,)
        if return_screen:
            out += (screen, normals)
        if return_uv:
            out += (uvl,)
        return out

    def render_mesh(self, mesh, t_center, rot=np.zeros(3), tex_img=None, tex_uv=None, camera_pose=None, light_pose=None):
        """One mesh (any object with .v (V, 3) and .f (F, 3)) turned by `rot` about `t_center` -> (colour (H, W, 3) uint8,
        depth (H, W) float32) numpy arrays, as the reference returns them.  camera_pose / light_pose, when given, replace
        the renderer's (and stay, as in the reference).  tex_img (Ht, Wt, 3 | 4) uint8 with tex_uv = {'vt': (Nt, 2), 'ft': (F, 3)}
        draws the mesh textured (render_vertices); tex_img without tex_uv is refused."""
        if tex_img is not None and tex_uv is None:
            raise NotImplementedError("a texture needs a uv table: tex_uv = {'vt', 'ft'} (there are no default per-vertex "
                                      "texture coordinates)")
        if camera_pose is not None:
            self.set_camera_pose(camera_pose)
        if light_pose is not None:
            self.set_lighting_pose(light_pose)
        v = torch.from_numpy(np.ascontiguousarray(np.asarray(mesh.v, np.float32))).to("cuda").unsqueeze(0)
        color, depth = self.render_vertices(v, np.asarray(mesh.f), t_center=np.asarray(t_center, np.float64).reshape(3),
                                            rot=np.asarray(rot, np.float64).reshape(3), tex_img=tex_img, tex_uv=tex_uv)
        return color[0].contiguous().cpu().numpy(), depth[0].cpu().numpy()
