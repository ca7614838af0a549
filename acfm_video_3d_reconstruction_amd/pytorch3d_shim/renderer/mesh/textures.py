"""pytorch3d.renderer.mesh.textures (0.3.0): TexturesAtlas, TexturesVertex and the `Textures(verts_rgb=...)` wrapper.
TexturesUV (maps= / verts_uvs= / faces_uvs=) is refused by name.  TexturesVertex.sample_textures is the HIP
interpolate_face_attributes; TexturesAtlas.sample_textures selects texels with PyTorch3D's rule --
shaders of ambient-only lights take ops.atlas_softmax_blend instead, which samples inside the blend kernel."""
import torch

from .... import ops as _ops


def _refuse_uv():
    raise ValueError("TexturesUV (maps= / faces_uvs= / verts_uvs=) is not supported: use TexturesAtlas or "
                     "TexturesVertex")


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
        return _ops.interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords, faces_verts_features)


class TexturesUV:
    def __init__(self, *args, **kwargs):
        _refuse_uv()


def Textures(maps=None, faces_uvs=None, verts_uvs=None, verts_rgb=None):
    """The 0.3.0 wrapper as the reference calls it: Textures(verts_rgb=[N,V,3]) -> TexturesVertex."""
    if maps is not None or faces_uvs is not None or verts_uvs is not None:
        _refuse_uv()
    if verts_rgb is None:
        raise ValueError("Textures: verts_rgb is required (maps= / verts_uvs= are not supported)")
    return TexturesVertex(verts_features=verts_rgb)
