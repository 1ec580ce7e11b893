"""Pictures of meshes: the reference's renderer (``model_manager.py:616-658``,
pytorch3d's ``MeshRenderer`` with ``HardGouraudShader`` / ``ShadelessShader``)
on libcfsd's rasteriser (``csrc/render.hip``; the convention is DESIGN.md
section 9), and what turns renderings into a logged image: the error colour
map (``utils.errors_to_colors``), torchvision's ``make_grid`` layout and a PNG
writer on the standard library.  Nothing here has autograd.
"""
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import ops

_HERE = os.path.dirname(os.path.abspath(__file__))


class Camera:
    """``look_at_view_transform(dist, elev, azim)`` + ``FoVPerspectiveCameras``
    (angles in degrees), computed in float64 on the host: ``R`` ``[3, 3]`` and
    ``T`` ``[3]`` with ``X_view = X_world R + T`` (row vectors), ``centre`` the
    camera position, ``scale = 1 / tan(fov / 2)``.  The kernels receive 12 + 2
    floats: R, T, scale, znear."""

    def __init__(self, dist=2.5, elev=0.0, azim=15.0, fov=60.0, znear=1.0):
        e, a = math.radians(elev), math.radians(azim)
        c = dist * np.array([math.cos(e) * math.sin(a), math.sin(e), math.cos(e) * math.cos(a)], np.float64)
        z_axis = -c / np.linalg.norm(c)
        x_axis = np.cross(np.array([0.0, 1.0, 0.0]), z_axis)
        x_axis /= np.linalg.norm(x_axis)
        y_axis = np.cross(z_axis, x_axis)
        self.R = np.stack([x_axis, y_axis, z_axis], axis=1)
        self.T = -c @ self.R
        self.centre = c
        self.scale = 1.0 / math.tan(math.radians(fov) / 2)
        self.znear = float(znear)
        self.dist, self.elev, self.azim, self.fov = float(dist), float(elev), float(azim), float(fov)
        self._tensors = {}

    @property
    def params(self):
        """The 14 floats of the C ABI."""
        return np.concatenate([self.R.reshape(-1), self.T, [self.scale, self.znear]]).astype(np.float32)

    def tensor(self, device):
        key = str(device)
        if key not in self._tensors:
            self._tensors[key] = torch.from_numpy(self.params).to(device)
        return self._tensors[key]

    def project(self, points):
        """Float64 NumPy projection of ``points`` ``[..., 3]``: (ndc_xy, view_z)."""
        v = np.asarray(points, np.float64) @ self.R + self.T
        return self.scale * v[..., :2] / v[..., 2:3], v[..., 2]


def look_at(dist=2.5, elev=0.0, azim=15.0, fov=60.0, znear=1.0):
    return Camera(dist, elev, azim, fov, znear)


_DEFAULT_CAMERA = None


def default_camera():
    """The reference's view: ``dist=2.5, elev=0, azim=15``, 60 degrees."""
    global _DEFAULT_CAMERA
    if _DEFAULT_CAMERA is None:
        _DEFAULT_CAMERA = Camera()
    return _DEFAULT_CAMERA


def gouraud_colors(verts, faces, camera=None, tex=None, light=(0.0, 0.0, 3.0), ambient=0.5, diffuse=1.0,
                   specular=0.2, shininess=0.5, tex_value=0.5):
    """Per-vertex colours ``[B, V, 3]`` of the reference's ``HardGouraudShader``
    (point light at ``light``, white material and light colours): ``(ambient +
    diffuse max(n.L, 0)) tex + specular spec``, lit in world space.  ``tex``
    ``[B or 1, V, 3]`` or the grey ``tex_value``."""
    camera = default_camera() if camera is None else camera
    return ops.project_vertices(verts, camera, faces, tex, light, ambient, diffuse, specular, shininess, tex_value,
                                shade=True)[2]


@torch.no_grad()
def render(verts, faces, vertex_colors=None, shading="gouraud", image_size=256, camera=None, light=(0.0, 0.0, 3.0),
           background=0.0):
    """Images ``[B, 3, S, S]`` (float32, on the device, not clamped) of the
    meshes ``verts`` ``[B, V, 3]`` with ``faces`` ``[F, 3]`` (int32).
    ``shading="gouraud"``: the vertex colours (grey 0.5 if not given) lit per
    vertex; ``"none"``: the given colours as they are (the reference's
    ``ShadelessShader``).  Two launches of vertex work and one raster launch
    that writes the image in its epilogue."""
    if shading not in ("gouraud", "none"):
        raise ValueError('shading must be "gouraud" or "none"')
    if shading == "none" and vertex_colors is None:
        raise ValueError('shading="none" needs vertex_colors')
    camera = default_camera() if camera is None else camera
    verts = verts.detach()
    if verts.is_cuda and verts.dtype == torch.float32:
        verts = verts.contiguous()
    if vertex_colors is not None and vertex_colors.is_cuda:
        vertex_colors = vertex_colors.detach().to(torch.float32).contiguous()
    gouraud = shading == "gouraud"
    ndc, vz, colors = ops.project_vertices(verts, camera, faces if gouraud else None,
                                           vertex_colors if gouraud else None, light, shade=gouraud)
    return ops.rasterize_ndc(ndc, vz, faces, image_size, camera.znear, colors if gouraud else vertex_colors,
                             background)[3]


_PLASMA = {}


def plasma_table(device=None):
    """matplotlib's 256-entry plasma colour map as uint8 ``[256, 3]`` (shipped
    as ``plasma_u8.txt``: matplotlib need not be installed); a NumPy array, or
    with ``device`` a float tensor there."""
    if "np" not in _PLASMA:
        _PLASMA["np"] = np.loadtxt(os.path.join(_HERE, "plasma_u8.txt"), dtype=np.int64).astype(np.uint8)
    if device is None:
        return _PLASMA["np"]
    key = str(device)
    if key not in _PLASMA:
        _PLASMA[key] = torch.from_numpy(_PLASMA["np"].astype(np.float32)).to(device)
    return _PLASMA[key]


def errors_to_colors(values, min_value=None, max_value=None, cmap="plasma"):
    """``utils.errors_to_colors`` divided by 255: ``v = clip((e - min) / (max
    - min), 0, 1)``, entry ``min(255, floor(256 v))`` of the colour table.
    ``values`` any shape (a tensor on any device); returns ``values.shape +
    (3,)`` float32 in [0, 1].  ``min == max`` maps values above it to the last
    entry and the rest to the first."""
    if cmap != "plasma":
        raise ValueError("only the plasma colour map is shipped")
    values = values.detach().to(torch.float32)
    lo = float(values.min()) if min_value is None else float(min_value)
    hi = float(values.max()) if max_value is None else float(max_value)
    if hi > lo:
        v = ((values - lo) / (hi - lo)).clamp_(0.0, 1.0)
    else:
        v = (values > lo).to(torch.float32)
    index = torch.floor(v * 256.0).clamp_(0, 255).long()
    return plasma_table(values.device)[index] / 255.0


def make_grid(images, nrow=8, padding=2, pad_value=0.0):
    """``torchvision.utils.make_grid`` for a batch ``[N, C, H, W]``: ``nrow``
    images per row, every cell ``padding`` pixels below and right of the
    previous one, the frame and the empty cells filled with ``pad_value``."""
    if images.dim() != 4:
        raise ValueError(f"images: shape {tuple(images.shape)}, expected [N, C, H, W]")
    n, c, h, w = images.shape
    xmaps = min(int(nrow), n)
    ymaps = -(-n // xmaps)
    ch, cw = h + padding, w + padding
    grid = images.new_full((c, ch * ymaps + padding, cw * xmaps + padding), pad_value)
    for k in range(n):
        y, x = divmod(k, xmaps)
        grid[:, y * ch + padding:y * ch + padding + h, x * cw + padding:x * cw + padding + w] = images[k]
    return grid


def to_uint8(image):
    """``[3, H, W]`` float image -> ``[H, W, 3]`` uint8 NumPy, clamped to [0, 1] here and only here."""
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"image: shape {tuple(image.shape)}, expected [3, H, W]")
    if image.dtype == torch.uint8:
        return image.permute(1, 2, 0).contiguous().cpu().numpy()
    q = torch.floor(image.detach().to(torch.float32).clamp(0.0, 1.0) * 255.0 + 0.5)
    return q.to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()


def _chunk(tag, payload):
    return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload) & 0xffffffff)


def save_png(path, image):
    """Write ``image`` ``[3, H, W]`` (float in [0, 1], clamped; or uint8) as an
    8-bit RGB PNG (``zlib`` + ``struct`` only)."""
    rgb = to_uint8(image)
    h, w, _ = rgb.shape
    rows = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], axis=1)  # filter type 0 per row
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(data)
    return path


def save_apng(path, frames, fps):
    """Write ``frames`` ``[N, 3, H, W]`` (float in [0, 1], clamped; or uint8;
    each quantised by :func:`to_uint8`) as an animated PNG that loops for ever
    at ``fps`` frames per second (the reference writes mp4 files through
    ``torchvision.io.write_video``): ``acTL``, then per frame an ``fcTL`` and
    its image (``IDAT`` for the first frame, ``fdAT`` for the others), the
    ``fcTL`` / ``fdAT`` sequence numbers running from 0.  A viewer without
    APNG support shows the first frame."""
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 1:
        raise ValueError(f"frames: shape {tuple(frames.shape)}, expected [N >= 1, 3, H, W]")
    if not fps > 0:
        raise ValueError(f"fps {fps} must be positive")
    from fractions import Fraction
    delay = Fraction(1.0 / float(fps)).limit_denominator(65535)
    if not 0 < delay.numerator <= 65535:
        raise ValueError(f"fps {fps}: the frame delay does not fit the format's 16-bit fraction")
    n, _, h, w = frames.shape
    out = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)),
           _chunk(b"acTL", struct.pack(">II", n, 0))]
    seq = 0
    for k in range(n):
        rgb = to_uint8(frames[k])
        rows = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], axis=1)  # filter type 0 per row
        data = zlib.compress(rows.tobytes(), 6)
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, delay.numerator, delay.denominator,
                                               0, 0)))
        seq += 1
        if k == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return path
