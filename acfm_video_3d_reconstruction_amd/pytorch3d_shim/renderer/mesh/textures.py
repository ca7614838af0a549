"""pytorch3d.renderer.mesh.textures (0.3.0): TexturesAtlas, TexturesVertex, TexturesUV and the `Textures(...)` wrapper.
TexturesVertex.sample_textures is the HIP interpolate_face_attributes (host tensors: the torch gather);
TexturesAtlas.sample_textures selects texels with PyTorch3D's rule -- shaders of ambient-only lights take ops.atlas_softmax_blend instead, which
samples inside the blend kernel.  TexturesUV.sample_textures is ops.uv_texels on GPU tensors -- the
map is read in place, per fragment -- and PyTorch3D's own composition of torch operators on host tensors."""
import torch

from .... import ops as _ops


def interpolate_face_attributes(pix_to_face, bary_coords, face_attributes):
    """The HIP kernel on GPU tensors; on host tensors PyTorch3D's gather (0 in empty slots)."""
    if pix_to_face.is_cuda:
        return _ops.interpolate_face_attributes(pix_to_face, bary_coords, face_attributes)
    vals = face_attributes[pix_to_face.clamp(min=0)]                       # [N,H,W,K,3,D]
    out = (bary_coords[..., None] * vals).sum(dim=-2)
    return torch.where((pix_to_face < 0)[..., None], torch.zeros_like(out), out)


class TexturesAtlas:
    def __init__(self, atlas):
        if torch.is_tensor(atlas):
            atlas_list = list(atlas.unbind(0)) if atlas.dim() == 5 else None
        else:
            atlas_list, atlas = list(atlas), None
        if atlas is not None and atlas.dim() != 5:
            raise ValueError("atlas must be [N,F,R,R,C], got %s" % (tuple(atlas.shape),))
        ref = atlas if atlas is not None else atlas_list[0]
        if ref.shape[-1] != 3:
            raise ValueError("atlas must have 3 channels (RGB), got %d" % ref.shape[-1])
        self._atlas_padded = atlas if atlas is not None else torch.stack(atlas_list, 0)
        self.device = self._atlas_padded.device

    def atlas_padded(self):
        return self._atlas_padded

    def atlas_packed(self):
        a = self._atlas_padded
        return a.reshape((-1,) + tuple(a.shape[2:]))

    def atlas_list(self):
        return list(self._atlas_padded.unbind(0))

    def to(self, device):
        return TexturesAtlas(self._atlas_padded.to(device))

    def clone(self):
        return TexturesAtlas(self._atlas_padded.clone())

    def sample_textures(self, fragments, **kwargs):
        """-> texels [N,H,W,K,3]: atlas[f, w_y, w_x] with w_xy = (int)(bary_w01 R), mirrored above the diagonal and
        clamped to [0, R-1]; 0 in empty slots.  Gradient to the atlas only (integer indexing)."""
        p2f = fragments.pix_to_face
        a = self.atlas_packed()
        R = a.shape[1]
        empty = p2f < 0
        w01 = torch.where(empty[..., None], torch.zeros_like(fragments.bary_coords[..., :2]),
                          fragments.bary_coords[..., :2])
        wxy = (w01 * R).to(torch.int64)
        below = (w01.sum(dim=-1) * R - wxy.float().sum(dim=-1)) <= 1.0
        wxy = torch.where(below[..., None], wxy, R - 1 - wxy).clamp(0, R - 1)
        texels = a[p2f.clamp(min=0), wxy[..., 1], wxy[..., 0]]
        return texels * (~empty)[..., None].to(texels.dtype)


class TexturesVertex:
    def __init__(self, verts_features):
        if torch.is_tensor(verts_features):
            if verts_features.dim() != 3:
                raise ValueError("verts_features must be [N,V,C], got %s" % (tuple(verts_features.shape),))
            self._verts_features_padded = verts_features
        else:
            self._verts_features_padded = torch.stack(list(verts_features), 0)
        self.device = self._verts_features_padded.device

    def verts_features_padded(self):
        return self._verts_features_padded

    def verts_features_packed(self):
        return self._verts_features_padded.reshape(-1, self._verts_features_padded.shape[-1])

    def verts_features_list(self):
        return list(self._verts_features_padded.unbind(0))

    def to(self, device):
        return TexturesVertex(self._verts_features_padded.to(device))

    def clone(self):
        return TexturesVertex(self._verts_features_padded.clone())

    def sample_textures(self, fragments, faces_packed=None):
        """-> texels [N,H,W,K,C]: the vertex features interpolated at the barycentrics (HIP kernel)."""
        faces_verts_features = self.verts_features_packed()[faces_packed]
        return interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords, faces_verts_features)


def uv_texels_composition(pix_to_face, bary_coords, faces_verts_uvs, maps, align_corners=True, padding_mode="border"):
    """TexturesUV.sample_textures as PyTorch3D 0.3.0 composes it from torch operators: the statement
    of the definition, and the host path.  It expands the map K times and builds the [N,H,W,K,2] UV tensor."""
    N, H, W, K = pix_to_face.shape
    vals = faces_verts_uvs[pix_to_face.clamp(min=0)]                               # [N,H,W,K,3,2]
    uv = (bary_coords[..., None] * vals).sum(dim=-2) * (pix_to_face >= 0)[..., None].to(vals.dtype)
    uv = uv.permute(0, 3, 1, 2, 4).reshape(N * K, H, W, 2)
    C, Hm, Wm = maps.shape[3], maps.shape[1], maps.shape[2]
    m = maps.permute(0, 3, 1, 2)[None].expand(K, -1, -1, -1, -1).transpose(0, 1).reshape(N * K, C, Hm, Wm)
    grid = uv * 2.0 - 1.0                                                          # x from u, y from v
    m = torch.flip(m, [2])                                                         # v = 0 is the map's last row
    texels = torch.nn.functional.grid_sample(m, grid, mode="bilinear", padding_mode=padding_mode,
                                             align_corners=align_corners)
    return texels.reshape(N, K, C, H, W).permute(0, 3, 4, 1, 2)


def _stack(x, what, dim):
    """A padded tensor or a list of equal-sized tensors -> the padded tensor (this shim's meshes are equal-sized)."""
    if torch.is_tensor(x):
        if x.dim() != dim + 1:
            raise ValueError("TexturesUV: %s must be %d-dimensional or a list, got %s" % (what, dim + 1, tuple(x.shape)))
        return x
    x = list(x)
    if len({tuple(t.shape) for t in x}) > 1:
        raise ValueError("TexturesUV: the %s of all meshes must have equal sizes (meshes of unequal size are not "
                         "supported), got %s" % (what, [tuple(t.shape) for t in x]))
    if not x:
        return None
    return torch.stack(x, 0)


class TexturesUV:
    """maps [N,Hm,Wm,3] (or a list of equal-sized maps), faces_uvs [N,F,3] int64 and verts_uvs [N,Vt,2] (or lists)."""

    PADDING_MODES = _ops.UV_PADDING_MODES

    def __init__(self, maps, faces_uvs, verts_uvs, padding_mode="border", align_corners=True):
        m, fu, vu = _stack(maps, "maps", 3), _stack(faces_uvs, "faces_uvs", 2), _stack(verts_uvs, "verts_uvs", 2)
        counts = [0 if t is None else t.shape[0] for t in (m, fu, vu)]
        if len(set(counts)) != 1 or counts[0] == 0:
            raise ValueError("TexturesUV: maps, faces_uvs and verts_uvs must describe the same, non-zero number of "
                             "meshes, got %d, %d and %d" % tuple(counts))
        if m.shape[3] != 3:
            raise ValueError("TexturesUV: maps must have 3 channels (RGB), got %d" % m.shape[3])
        if fu.shape[2] != 3 or fu.dtype != torch.int64:
            raise ValueError("TexturesUV: faces_uvs must be [N,F,3] int64, got %s %s" % (tuple(fu.shape), fu.dtype))
        if vu.shape[2] != 2:
            raise ValueError("TexturesUV: verts_uvs must be [N,Vt,2], got %s" % (tuple(vu.shape),))
        if padding_mode not in self.PADDING_MODES:
            raise ValueError("TexturesUV: padding_mode=%r is not supported (one of %s)"
                             % (padding_mode, self.PADDING_MODES))
        if align_corners and min(m.shape[1], m.shape[2]) < 2:
            raise ValueError("TexturesUV: maps must be at least 2x2 with align_corners=True, got %s" % (tuple(m.shape),))
        if fu.numel() == 0 or vu.shape[1] == 0:
            raise ValueError("TexturesUV: faces_uvs and verts_uvs must not be empty")
        lo, hi = int(fu.min()), int(fu.max())       # the one host read: here, not per call
        if lo < 0 or hi >= vu.shape[1]:
            raise ValueError("TexturesUV: faces_uvs indexes verts_uvs out of range (%d..%d, Vt = %d)"
                             % (lo, hi, vu.shape[1]))
        self._set(m, fu, vu, padding_mode, bool(align_corners))

    def _set(self, m, fu, vu, padding_mode, align_corners):
        self._maps_padded, self._faces_uvs_padded, self._verts_uvs_padded = m, fu, vu
        self.padding_mode, self.align_corners = padding_mode, align_corners
        self.device = m.device
        return self

    def _like(self, m, fu, vu):
        """Another TexturesUV of already validated contents (to / clone: no second host read)."""
        return object.__new__(TexturesUV)._set(m, fu, vu, self.padding_mode, self.align_corners)

    def maps_padded(self):
        return self._maps_padded

    def maps_list(self):
        return list(self._maps_padded.unbind(0))

    def faces_uvs_padded(self):
        return self._faces_uvs_padded

    def faces_uvs_list(self):
        return list(self._faces_uvs_padded.unbind(0))

    def verts_uvs_padded(self):
        return self._verts_uvs_padded

    def verts_uvs_list(self):
        return list(self._verts_uvs_padded.unbind(0))

    def to(self, device):
        return self._like(self._maps_padded.to(device), self._faces_uvs_padded.to(device),
                          self._verts_uvs_padded.to(device))

    def clone(self):
        return self._like(self._maps_padded.clone(), self._faces_uvs_padded.clone(), self._verts_uvs_padded.clone())

    def faces_verts_uvs_packed(self):
        """verts_uvs[faces_uvs], mesh after mesh: [N F,3,2] (torch indexing: it carries the gradient to verts_uvs)."""
        vu, fu = self._verts_uvs_padded, self._faces_uvs_padded
        N, Vt = vu.shape[0], vu.shape[1]
        offs = torch.arange(N, device=fu.device, dtype=fu.dtype)[:, None, None] * Vt
        return vu.reshape(N * Vt, 2)[(fu + offs).reshape(-1, 3)]

    def sample_textures(self, fragments, **kwargs):
        """-> texels [N,H,W,K,3]: the map of the pixel's mesh, flipped along its height, sampled
        bilinearly at the interpolated uv.  Empty slots hold the sample at uv = (0, 0); the blends mask them out.
        GPU tensors: the HIP kernel (ops.uv_texels); host tensors: the composition of torch operators."""
        p2f, bary = fragments.pix_to_face, fragments.bary_coords
        if p2f.shape[0] != self._maps_padded.shape[0]:
            raise ValueError("TexturesUV: %d maps for fragments of %d meshes" % (self._maps_padded.shape[0], p2f.shape[0]))
        fvuv = self.faces_verts_uvs_packed()
        if p2f.is_cuda:
            return _ops.uv_texels(p2f, bary, fvuv, self._maps_padded, align_corners=self.align_corners,
                                  padding_mode=self.padding_mode)
        return uv_texels_composition(p2f, bary, fvuv, self._maps_padded, align_corners=self.align_corners,
                                     padding_mode=self.padding_mode)


def Textures(maps=None, faces_uvs=None, verts_uvs=None, verts_rgb=None):
    """The 0.3.0 wrapper as the reference calls it: Textures(verts_rgb=[N,V,3]) -> TexturesVertex;
    Textures(maps=, faces_uvs=, verts_uvs=) -> TexturesUV.  An incomplete UV triple is an error here."""
    uv = {"maps=": maps, "faces_uvs=": faces_uvs, "verts_uvs=": verts_uvs}
    given = [k for k, v in uv.items() if v is not None]
    if given:
        missing = [k for k, v in uv.items() if v is None]
        if verts_rgb is not None or missing:
            raise ValueError("Textures: %s given%s; a TexturesUV needs maps=, faces_uvs= and verts_uvs= together, "
                             "without verts_rgb=" % (" / ".join(given),
                                                     " without " + " / ".join(missing) if missing else " with verts_rgb="))
        return TexturesUV(maps=maps, faces_uvs=faces_uvs, verts_uvs=verts_uvs)
    if verts_rgb is None:
        raise ValueError("Textures: verts_rgb= (or maps=, faces_uvs= and verts_uvs=) is required")
    return TexturesVertex(verts_features=verts_rgb)


