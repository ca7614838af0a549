"""pytorch3d.io.load_obj as used at multiframe/main.py:159-160 and predictor.py:64:
returns (verts [V,3] f32, faces namedtuple with .verts_idx [F,3] i64, aux); save_obj as imported by
utils/geometry.py:63."""
from collections import namedtuple

import torch

Faces = namedtuple("Faces", "verts_idx normals_idx textures_idx materials_idx")
Properties = namedtuple("Properties", "normals verts_uvs material_colors texture_images texture_atlas")


def load_obj(f, load_textures=False, **kwargs):
    """Accepts 'f a b c' and 'f a/ta/na ...' records (bird.obj uses the latter);
    polygons are fan-triangulated like PyTorch3D."""
    verts, vts, faces, tfaces = [], [], [], []
    fh = open(f) if isinstance(f, str) else f
    try:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                verts.append([float(x) for x in p[1:4]])
            elif p[0] == "vt":
                vts.append([float(x) for x in p[1:3]])
            elif p[0] == "f":
                idx = [q.split("/") for q in p[1:]]
                vi = [int(q[0]) for q in idx]
                vi = [i - 1 if i > 0 else len(verts) + i for i in vi]
                ti = [int(q[1]) - 1 if len(q) > 1 and q[1] else -1 for q in idx]
                for k in range(1, len(vi) - 1):
                    faces.append([vi[0], vi[k], vi[k + 1]])
                    tfaces.append([ti[0], ti[k], ti[k + 1]])
    finally:
        if isinstance(f, str):
            fh.close()
    v = torch.tensor(verts, dtype=torch.float32).reshape(-1, 3)
    fi = torch.tensor(faces, dtype=torch.int64).reshape(-1, 3)
    ti = torch.tensor(tfaces, dtype=torch.int64).reshape(-1, 3)
    uv = torch.tensor(vts, dtype=torch.float32).reshape(-1, 2) if vts else None
    return v, Faces(fi, torch.full_like(fi, -1), ti, torch.full((fi.shape[0],), -1, dtype=torch.int64)), \
        Properties(None, uv, None, None, None)


def save_obj(f, verts, faces, decimal_places=None):
    """Writes 'v x y z' lines, then 1-based 'f i j k' lines.  f: a path or an open text file.  decimal_places=None
    writes nine significant digits, which load_obj reads back to the same float32 values."""
    if verts.numel() and not (verts.dim() == 2 and verts.shape[1] == 3):
        raise ValueError("Argument 'verts' should either be empty or of shape (num_verts, 3).")
    if faces.numel() and not (faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("Argument 'faces' should either be empty or of shape (num_faces, 3).")
    fmt = "%.9g" if decimal_places is None else "%%.%df" % decimal_places
    v = verts.detach().cpu().reshape(-1, 3).tolist()
    fi = (faces.detach().cpu().long().reshape(-1, 3) + 1).tolist()
    lines = ["v " + " ".join(fmt % c for c in row) for row in v] + ["f %d %d %d" % tuple(row) for row in fi]
    text = "\n".join(lines) + ("\n" if lines else "")
    if hasattr(f, "write"):
        f.write(text)
    else:
        with open(f, "w") as fh:
            fh.write(text)
