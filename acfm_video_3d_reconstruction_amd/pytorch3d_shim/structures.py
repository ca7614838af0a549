"""pytorch3d.structures.Meshes, as used by the reference:
constructed from padded tensors or lists (nmr.py:152, main.py:195, 600, 699-700), then queried
through verts_packed / faces_packed / edges_packed / verts_padded / num_verts_per_mesh /
isempty / device / len()."""
import torch

from .. import _lib

# edges_packed of a batch is a sort + unique over 3*N*F pairs; the reference rebuilds Meshes every
# step from the same faces tensor, so the result is memoised on (storage, shape, version).
_EDGE_CACHE = {}


def _may_keep(t):
    """A tensor made while a hipGraph is being captured lives in the graph's private pool: it must not outlive the
    capture in a module-level table (eager code would read memory the graph reuses)."""
    return not (t.is_cuda and torch.cuda.is_current_stream_capturing())


_FACES_PACKED_CACHE = {}   # same keying and lifetime rule as _EDGE_CACHE: (padded faces tensor, V) -> packed faces
_WEIGHT_CACHE = {}         # (meshes, verts per mesh, device) -> 1 / V per packed vertex
# same keying and lifetime rule again, for everything else that depends on topology only (the edge / face index maps
# and the pair table of mesh_normal_consistency): faces tensor(s) -> (the tensors, {name: result}).  Here a Meshes built
# from a LIST of faces tensors has a key too (one entry per tensor): fit_verts_to_mesh builds its meshes that way.
_TOPO_CACHE = {}


def _tensor_key(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version, str(t.device), str(t.dtype))


class Meshes:
    def __init__(self, verts=None, faces=None, textures=None):
        if torch.is_tensor(verts):
            self._verts_list = list(verts.unbind(0))
            self._verts_padded = verts
        else:
            self._verts_list = list(verts)
            self._verts_padded = None
        if torch.is_tensor(faces):
            self._faces_list = list(faces.unbind(0))
            self._faces_padded = faces
        else:
            self._faces_list = list(faces)
            self._faces_padded = None
        if len(self._verts_list) != len(self._faces_list):
            raise ValueError("verts and faces must describe the same number of meshes")
        self.textures = textures
        self._cache = {}

    # ---- basics
    def __len__(self):
        return len(self._verts_list)

    @property
    def device(self):
        return self._verts_list[0].device if self._verts_list else torch.device("cpu")

    def isempty(self):
        return len(self._verts_list) == 0 or all(v.numel() == 0 for v in self._verts_list)

    def verts_list(self):
        return self._verts_list

    def faces_list(self):
        return self._faces_list

    def num_verts_per_mesh(self):
        return _lib.const([v.shape[0] for v in self._verts_list], self.device, torch.int64)

    def num_faces_per_mesh(self):
        return _lib.const([f.shape[0] for f in self._faces_list], self.device, torch.int64)

    def _equal_sized(self):
        return (len({v.shape[0] for v in self._verts_list}) == 1 and
                len({f.shape[0] for f in self._faces_list}) == 1)

    def verts_padded(self):
        if self._verts_padded is None:
            vmax = max(v.shape[0] for v in self._verts_list)
            out = self._verts_list[0].new_zeros(len(self), vmax, 3)
            for i, v in enumerate(self._verts_list):
                out[i, :v.shape[0]] = v
            self._verts_padded = out
        return self._verts_padded

    def faces_padded(self):
        if self._faces_padded is None:
            fmax = max(f.shape[0] for f in self._faces_list)
            out = self._faces_list[0].new_full((len(self), fmax, 3), -1)
            for i, f in enumerate(self._faces_list):
                out[i, :f.shape[0]] = f
            self._faces_padded = out
        return self._faces_padded

    # ---- packed views (packed vertex id = sum of the previous meshes' vertex counts + v)
    def verts_packed(self):
        if self._verts_padded is not None and self._equal_sized():
            return self._verts_padded.reshape(-1, 3)
        return torch.cat(self._verts_list, 0)

    def inv_num_verts_packed(self):
        """1 / (vertices of its mesh) per packed vertex, float32 (the weights of mesh_laplacian_smoothing); a constant
        per (batch size, mesh size) for equal-sized batches, kept."""
        if self._equal_sized():
            key = (len(self), self._verts_list[0].shape[0], str(self.device))
            w = _WEIGHT_CACHE.get(key)
            if w is None:
                w = torch.full((key[0] * key[1],), 1.0 / max(key[1], 1), dtype=torch.float32, device=self.device)
                if _may_keep(w):
                    if len(_WEIGHT_CACHE) > 16:
                        _WEIGHT_CACHE.clear()
                    _WEIGHT_CACHE[key] = w
            return w
        return 1.0 / self.num_verts_per_mesh().gather(0, self.verts_packed_to_mesh_idx()).float()

    def mesh_to_verts_packed_first_idx(self):
        n = self.num_verts_per_mesh()
        return torch.cumsum(n, 0) - n

    def verts_packed_to_mesh_idx(self):
        n = self.num_verts_per_mesh()
        total = sum(v.shape[0] for v in self._verts_list)     # known on the host: no device sync
        return torch.repeat_interleave(torch.arange(len(self), device=self.device), n, output_size=total)

    def faces_packed(self):
        if "faces_packed" not in self._cache:
            if self._faces_padded is not None and self._equal_sized():
                # batches of one topology build a new Meshes every step around the SAME faces tensor: the packed ids
                # (three small launches) are memoised on it like the edges below
                fp_ = self._faces_padded
                ck = (fp_.data_ptr(), tuple(fp_.shape), tuple(fp_.stride()), fp_._version, str(fp_.device),
                      str(fp_.dtype), self._verts_list[0].shape[0])
                hit = _FACES_PACKED_CACHE.get(ck)
                if hit is None:
                    first = self.mesh_to_verts_packed_first_idx()
                    hit = (fp_, (fp_.long() + first[:, None, None]).reshape(-1, 3))
                    if _may_keep(hit[1]):
                        if len(_FACES_PACKED_CACHE) > 16:
                            _FACES_PACKED_CACHE.clear()
                        _FACES_PACKED_CACHE[ck] = hit
                self._cache["faces_packed"] = hit[1]
                return hit[1]
            first = self.mesh_to_verts_packed_first_idx()
            if self._faces_padded is not None and self._equal_sized():
                fp = (self._faces_padded.long() + first[:, None, None]).reshape(-1, 3)
            else:
                fp = torch.cat([f.long() + first[i] for i, f in enumerate(self._faces_list)], 0)
            self._cache["faces_packed"] = fp
        return self._cache["faces_packed"]

    def edges_packed(self):
        """Unique (min, max) vertex pairs of all packed faces in lexicographic order
        (SURVEY App-A.9)."""
        if "edges_packed" not in self._cache and self._faces_padded is None:
            self._topology()      # a batch given as a list of faces tensors: the table kept for those tensors, if any
        if "edges_packed" not in self._cache:
            ck = None
            if self._faces_padded is not None and self._equal_sized():
                fp_ = self._faces_padded
                ck = (fp_.data_ptr(), tuple(fp_.shape), tuple(fp_.stride()), fp_._version, str(fp_.device),
                      str(fp_.dtype), self._verts_list[0].shape[0])
            hit = _EDGE_CACHE.get(ck) if ck is not None else None
            if hit is not None:
                # the entry holds its source tensor: while the key is in the table the storage stays alive, so
                # the address cannot be handed to another [N,F,3] tensor with a different topology, and any
                # tensor that matches (address, strides, shape, version) is a view of the same values
                self._cache["edges_packed"] = hit[1]
            else:
                f = self.faces_packed()
                e = torch.cat([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], 0)
                e = torch.sort(e, dim=1)[0]
                V = int(self.num_verts_per_mesh().sum().item())
                h = torch.unique(e[:, 0] * V + e[:, 1], sorted=True)
                self._cache["edges_packed"] = torch.stack([h // V, h % V], 1)
                if ck is not None and _may_keep(self._cache["edges_packed"]):
                    if len(_EDGE_CACHE) > 16:
                        _EDGE_CACHE.clear()
                    _EDGE_CACHE[ck] = (fp_, self._cache["edges_packed"])
                if self._faces_padded is None and _may_keep(self._cache["edges_packed"]):
                    self._topology().setdefault("edges_packed", self._cache["edges_packed"])
        return self._cache["edges_packed"]

    # ---- topology-only tables, memoised on the faces tensor(s) like the edges above
    def _topology(self):
        if "topology" not in self._cache:
            src = [self._faces_padded] if self._faces_padded is not None and self._equal_sized() else list(self._faces_list)
            ck = (tuple(_tensor_key(t) for t in src), tuple(v.shape[0] for v in self._verts_list))
            hit = _TOPO_CACHE.get(ck)
            if hit is None:
                hit = (src, {})
                if all(_may_keep(t) for t in src):
                    if len(_TOPO_CACHE) > 16:
                        _TOPO_CACHE.clear()
                    _TOPO_CACHE[ck] = hit
            self._cache["topology"] = hit[1]
            if "edges_packed" in hit[1]:
                self._cache.setdefault("edges_packed", hit[1]["edges_packed"])
        return self._cache["topology"]

    def _topo(self, name, make):
        t = self._topology()
        if name not in t:
            if "edges_packed" not in t:
                e = self.edges_packed()
                if _may_keep(e):
                    t["edges_packed"] = e
            val = make()
            if not all(_may_keep(x) for x in (val if isinstance(val, tuple) else (val,))):
                return val
            t[name] = val
        return t[name]

    def get_mesh_verts_faces(self, index):
        if not isinstance(index, int):
            raise ValueError("Mesh index must be an integer.")
        if index < 0 or index >= len(self):
            raise ValueError("Mesh index must be in the range [0, N) where N is the number of meshes in the batch.")
        return self._verts_list[index], self._faces_list[index]

    def mesh_to_faces_packed_first_idx(self):
        n = self.num_faces_per_mesh()
        return torch.cumsum(n, 0) - n

    def edges_packed_to_mesh_idx(self):
        """[E] the mesh every edge of edges_packed() belongs to."""
        def make():
            return self.verts_packed_to_mesh_idx()[self.edges_packed()[:, 0]]
        return self._topo("edges_packed_to_mesh_idx", make)

    def num_edges_per_mesh(self):
        def make():
            return torch.bincount(self.edges_packed_to_mesh_idx(), minlength=len(self))
        return self._topo("num_edges_per_mesh", make)

    def inv_num_edges_packed(self):
        """1 / (edges of its mesh) per packed edge, float32: the weights of mesh_edge_loss."""
        def make():
            return 1.0 / self.num_edges_per_mesh().gather(0, self.edges_packed_to_mesh_idx()).float()
        return self._topo("inv_num_edges_packed", make)

    def faces_packed_to_edges_packed(self):
        """[F,3]: for every packed face (v0, v1, v2) the rows of edges_packed() of its edges v1v2, v2v0, v0v1."""
        def make():
            f, e = self.faces_packed(), self.edges_packed()
            V = sum(v.shape[0] for v in self._verts_list)
            key = e[:, 0] * V + e[:, 1]
            a, b = f[:, [1, 2, 0]], f[:, [2, 0, 1]]
            return torch.searchsorted(key, (torch.minimum(a, b) * V + torch.maximum(a, b)).reshape(-1)).reshape(-1, 3)
        return self._topo("faces_packed_to_edges_packed", make)

    def geodesic_tables_packed(self):
        """-> (faces [F,3], edges [E,2], face_edges [F,3]) int32, contiguous: faces_packed(), edges_packed() and
        faces_packed_to_edges_packed() as acfm_geodesic_distances reads them.  Topology only: built once per faces
        tensor (the edges are a sort + unique with one host read), outside any graph capture."""
        def make():
            return tuple(t.to(torch.int32).contiguous() for t in
                         (self.faces_packed(), self.edges_packed(), self.faces_packed_to_edges_packed()))
        return self._topo("geodesic_tables_packed", make)

    def has_geodesic_tables(self):
        return "geodesic_tables_packed" in self._topology()

    def normal_pairs_packed(self):
        """-> (quads [Q,4] int64 = (a, b, c, d), weights [Q] float32) for mesh_normal_consistency: for every edge
        (a, b), a < b, that lies in m >= 2 faces, every unordered pair of those faces, c and d being the faces' third
        vertices; weight = 1 / (pairs of the edge's mesh).  Topology only: built once per faces tensor, on the host."""
        def make():
            import numpy as np
            f = self.faces_packed().cpu().numpy()
            sizes = np.array([v.shape[0] for v in self._verts_list], np.int64)
            V = int(sizes.sum())
            a = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
            b = np.concatenate([f[:, 2], f[:, 0], f[:, 1]])
            opp = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
            lo, hi = np.minimum(a, b), np.maximum(a, b)
            keep = lo != hi
            key, opp = (lo * V + hi)[keep], opp[keep]
            order = np.argsort(key, kind="stable")
            key, opp = key[order], opp[order]
            uniq, start, count = np.unique(key, return_index=True, return_counts=True)
            quads = []
            for m in np.unique(count[count >= 2]):
                g = np.nonzero(count == m)[0]
                third = opp[start[g][:, None] + np.arange(m)[None]]          # [G, m]
                i, j = np.triu_indices(int(m), 1)
                k = np.repeat(uniq[g], i.size)
                quads.append(np.stack([k // V, k % V, third[:, i].reshape(-1), third[:, j].reshape(-1)], 1))
            q = np.concatenate(quads, 0) if quads else np.zeros((0, 4), np.int64)
            q = q[np.argsort(q[:, 0] * V + q[:, 1], kind="stable")]
            mesh = np.searchsorted(np.cumsum(sizes), q[:, 0], side="right")
            per_mesh = np.bincount(mesh, minlength=len(self))
            w = (1.0 / per_mesh[mesh]).astype(np.float32)
            return torch.from_numpy(q).to(self.device), torch.from_numpy(w).to(self.device)
        return self._topo("normal_pairs_packed", make)

    def laplacian_packed(self):
        """Uniform Laplacian, sparse [sum V, sum V]: L[i,j] = 1/deg(i) on edges, L[i,i] = -1."""
        e = self.edges_packed()
        V = self.verts_packed().shape[0]
        idx = torch.cat([e.t(), e.flip(1).t()], 1)
        ones = torch.ones(idx.shape[1], dtype=torch.float32, device=self.device)
        deg = torch.zeros(V, dtype=torch.float32, device=self.device).index_add_(0, idx[0], ones)
        val = 1.0 / deg[idx[0]]
        diag = torch.arange(V, device=self.device)
        idx = torch.cat([idx, torch.stack([diag, diag])], 1)
        val = torch.cat([val, -torch.ones(V, dtype=torch.float32, device=self.device)])
        return torch.sparse_coo_tensor(idx, val, (V, V)).coalesce()

    def incidence_table_packed(self):
        """-> ops.IncidenceTable: for every packed vertex the face corners 3 f + i that hold it, ascending (CSR), as
        acfm_vertex_normals and acfm_corner_gather read it.  Topology only: built once per faces tensor, on the host,
        outside any graph capture."""
        def make():
            from .. import ops
            t = ops.incidence_table(self.faces_packed(), sum(v.shape[0] for v in self._verts_list))
            return (t.offsets, t.corners)
        from .. import ops
        offsets, corners = self._topo("incidence_table_packed", make)
        return ops.IncidenceTable(offsets, corners, sum(v.shape[0] for v in self._verts_list),
                                  sum(f.shape[0] for f in self._faces_list))

    # ---- normals (0.3.0's rule: the unnormalised cross product of every face -- twice its area times its normal --
    # added into each of its vertices, then F.normalize(eps=1e-6)); differentiable.  GPU float32 tensors: the gather
    # kernels of ops.vertex_normals; host tensors: the torch lines below
    def _compute_normals(self):
        if "verts_normals" not in self._cache:
            verts, faces = self.verts_packed(), self.faces_packed()
            if verts.is_cuda and verts.dtype == torch.float32 and faces.shape[0] > 0 and verts.shape[0] > 0:
                from .. import ops
                vn, fn = ops.vertex_normals(verts, faces, self.incidence_table_packed())
                self._cache["verts_normals"], self._cache["faces_normals"] = vn, fn
                return vn, fn
            fv = verts[faces]
            n = torch.zeros_like(verts)
            n = n.index_add(0, faces[:, 1], torch.cross(fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1], dim=1))
            n = n.index_add(0, faces[:, 2], torch.cross(fv[:, 0] - fv[:, 2], fv[:, 1] - fv[:, 2], dim=1))
            n = n.index_add(0, faces[:, 0], torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1))
            self._cache["verts_normals"] = torch.nn.functional.normalize(n, eps=1e-6, dim=1)
            fn = torch.cross(fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1], dim=1)
            self._cache["faces_normals"] = torch.nn.functional.normalize(fn, eps=1e-6, dim=1)
        return self._cache["verts_normals"], self._cache["faces_normals"]

    def verts_normals_packed(self):
        return self._compute_normals()[0]

    def verts_normals_padded(self):
        if not self._equal_sized():
            raise ValueError("verts_normals_padded: meshes of different sizes are not supported")
        return self.verts_normals_packed().reshape(len(self), -1, 3)

    def faces_normals_packed(self):
        return self._compute_normals()[1]

    def sample_textures(self, fragments):
        if self.textures is None:
            raise ValueError("Meshes does not have textures")
        if hasattr(self.textures, "verts_features_packed"):
            return self.textures.sample_textures(fragments, faces_packed=self.faces_packed())
        return self.textures.sample_textures(fragments)

    def update_padded(self, new_verts_padded):
        return Meshes(verts=new_verts_padded, faces=self.faces_padded(), textures=self.textures)

    def to(self, device):
        tex = self.textures.to(device) if self.textures is not None and hasattr(self.textures, "to") else self.textures
        return Meshes(verts=[v.to(device) for v in self._verts_list],
                      faces=[f.to(device) for f in self._faces_list], textures=tex)
