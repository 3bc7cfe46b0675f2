"""MarchingCubeMesher: drop-in for taichi_slam.mapping.MarchingCubeMesher (reference
taichi_slam/mapping/marching_cube_mesher.py:13-193).  The mesh stays in device buffers owned by the map handle;
`mesh_vertices/mesh_normals/mesh_colors` are field-likes with `.to_numpy()`."""
import ctypes as C

import numpy as np

from .. import _lib
from .fields import DeviceArrayField, ScalarField, device_view

EPS = 1e-6


class IndexedMeshField:
    """One array of the indexed mesh (generate_indexed_mesh): `.to_numpy()` copies the rows the last call stored, `.to_torch()` is a zero-copy view of
    them in the handle's device buffer (it stays valid until a later call asks for a larger capacity)."""

    def __init__(self, mesher, which, width, dtype, typestr, name):
        self._m, self._which, self._width, self._dtype, self._typestr, self._name = mesher, which, width, dtype, typestr, name

    def _rows(self):
        return self._m._indexed_rows()[1 if self._which == 4 else 0]

    @property
    def shape(self):
        return (self._rows(), self._width)

    def to_numpy(self, n=None):
        rows = self._rows() if n is None else max(0, min(int(n), self._rows()))
        return self._m._read_indexed(self._which, rows, self._width, self._dtype)

    def to_torch(self, n=None):
        rows = self._rows() if n is None else max(0, min(int(n), self._rows()))
        return device_view(self._m._indexed_dev()[self._which], (rows, self._width), self._typestr, keep=self._m, device=self._m.device)

    def __repr__(self):
        return f"<indexed mesh field {self._name} {self.shape}>"


class MarchingCubeMesher:
    def __init__(self, mapping, max_triangles=1000000, tsdf_surface_thres=0.1):
        self.max_triangles = int(max_triangles)
        self.mapping = mapping
        self.enable_texture = mapping.enable_texture
        self.tsdf_surface_thres = tsdf_surface_thres
        self._n_tri = 0
        self.device = getattr(mapping, "device", 0)
        self.mesh_vertices = DeviceArrayField(self, lambda n: self._read(n)[0], self.max_triangles * 3, 3, "mesh_vertices", dev=lambda: self._dev(0))
        self.mesh_normals = DeviceArrayField(self, lambda n: self._read(n)[1], self.max_triangles * 3, 3, "mesh_normals", dev=lambda: self._dev(1))
        self.mesh_colors = DeviceArrayField(self, lambda n: self._read(n)[2], self.max_triangles * 3, 3, "mesh_colors", dev=lambda: self._dev(2))
        self.mesh_indices = None
        self.num_facelets = ScalarField(lambda: self._n_tri, None, "num_facelets")
        # the reference never updates num_vertices although the node uses it as the mesh size
        # (marching_cube_mesher.py:22, scripts/taichislam_node.py:342, Q14); here it is kept equal to 3*num_facelets
        self.num_vertices = ScalarField(lambda: 3 * min(self._n_tri, self.max_triangles), None, "num_vertices")
        # the indexed mesh (generate_indexed_mesh): welded vertices in edge-key order, int32 triangles in cell-key order; the soup above is independent of it
        self._ix = None                  # (true vertices, true triangles, max_vertices, max_triangles) of the last generate_indexed_mesh
        self.indexed_vertices = IndexedMeshField(self, 0, 3, np.float32, "<f4", "indexed_vertices")
        self.indexed_normals = IndexedMeshField(self, 1, 3, np.float32, "<f4", "indexed_normals")
        self.indexed_colors = IndexedMeshField(self, 2, 3, np.float32, "<f4", "indexed_colors")
        self.indexed_edges = IndexedMeshField(self, 3, 4, np.int16, "<i2", "indexed_edges")
        self.indexed_triangles = IndexedMeshField(self, 4, 3, np.int32, "<i4", "indexed_triangles")
        self.num_indexed_vertices = ScalarField(lambda: self._ix[0] if self._ix else 0, None, "num_indexed_vertices")
        self.num_indexed_triangles = ScalarField(lambda: self._ix[1] if self._ix else 0, None, "num_indexed_triangles")

    def _read(self, n):
        n = int(max(0, min(n, 3 * min(self._n_tri, self.max_triangles))))
        v = np.empty((n, 3), np.float32)
        nr = np.empty((n, 3), np.float32)
        col = np.full((n, 3), 0.5, np.float32)
        _lib.check(_lib.lib().tsl_mesh_read(self.mapping.h, v.ctypes.data_as(C.c_void_p), nr.ctypes.data_as(C.c_void_p),
                                            col.ctypes.data_as(C.c_void_p) if self.enable_texture else None, n))
        return v, nr, col

    def _dev(self, which):
        """(device pointer of mesh_vertices / mesh_normals / mesh_colors, vertices of the last generate_mesh): `.to_torch()` of the fields"""
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        n = C.c_int32()
        _lib.check(_lib.lib().tsl_mesh_buffers_dev(self.mapping.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(n)))
        return p[which].value, 3 * min(n.value, self.max_triangles)

    def vertice_num(self):
        return self.num_facelets[None] * 3

    def generate_mesh(self, step=1):
        n = C.c_int32()
        _lib.check(_lib.lib().tsl_mesh_generate(self.mapping.h, int(step), float(self.tsdf_surface_thres), self.max_triangles, C.byref(n)))
        self._n_tri = n.value
        print("Total triangles", self._n_tri)

    def get_mesh(self):
        """(vertices[3n,3], normals[3n,3], colors|None) of the last generate_mesh (north-star alias)."""
        v, nr, c = self._read(3 * self._n_tri)
        return v, nr, (c if self.enable_texture else None)

    # ---- indexed mesh ----------------------------------------------------------------------------------------------------------------
    def generate_indexed_mesh(self, max_vertices=None, max_triangles=None, allow_truncated=False, step=1):
        """The mesh of generate_mesh(1) with welded vertices in a canonical order (include/taichislam_hip.h, "indexed mesh"): fills indexed_vertices,
        indexed_normals, indexed_colors, indexed_edges (int16 i, j, k, axis of every vertex's grid edge), indexed_triangles (int32 rows) and
        num_indexed_vertices / num_indexed_triangles, the TRUE counts.  max_triangles defaults to the mesher's, max_vertices to max_triangles (a closed
        surface has about half as many vertices as triangles).  A count above its capacity raises, unless allow_truncated: then every stored row is
        still the canonical one and a stored triangle may name a vertex row that is not stored.  Step 1 only.  Returns (vertices, triangles)."""
        if int(step) != 1:
            raise _lib.TslError(f"generate_indexed_mesh: step {step} is not supported, the indexed mesh is that of generate_mesh(1) (step 1 only)")
        mt = self.max_triangles if max_triangles is None else int(max_triangles)
        mv = mt if max_vertices is None else int(max_vertices)
        nv, nt = C.c_int64(), C.c_int64()
        self._ix = None
        _lib.check(_lib.lib().tsl_mesh_generate_indexed(self.mapping.h, float(self.tsdf_surface_thres), mv, mt, C.byref(nv), C.byref(nt)))
        self._ix = (nv.value, nt.value, mv, mt)
        if not allow_truncated and (nv.value > mv or nt.value > mt):
            raise _lib.TslError(f"generate_indexed_mesh: the mesh has {nv.value} vertices and {nt.value} triangles, the capacities are {mv} and {mt} "
                                f"(pass larger ones, or allow_truncated=True for the leading rows)")
        return nv.value, nt.value

    def _indexed_rows(self):
        """(vertex rows, triangle rows) the last generate_indexed_mesh stored"""
        if not self._ix:
            return 0, 0
        return min(self._ix[0], self._ix[2]), min(self._ix[1], self._ix[3])

    def _read_indexed(self, which, rows, width, dtype):
        out = np.full((rows, width), 0.5, dtype) if which == 2 else np.empty((rows, width), dtype)
        if rows == 0 or (which == 2 and not self.enable_texture):
            return out
        args = [None] * 5
        args[which] = out.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.lib().tsl_mesh_read_indexed(self.mapping.h, *args, 0 if which == 4 else rows, rows if which == 4 else 0))
        return out

    def _indexed_dev(self):
        p = [C.c_void_p() for _ in range(5)]
        if self._ix:          # (before the first call there is nothing on the device: the views are empty)
            _lib.check(_lib.lib().tsl_mesh_indexed_dev(self.mapping.h, *[C.byref(x) for x in p], None, None))
        return [x.value for x in p]

    def get_indexed_mesh(self):
        """{"vertices" f32 [V, 3], "normals" f32 [V, 3], "colors" f32 [V, 3] | None, "edges" int16 [V, 4], "triangles" int32 [T, 3], "num_vertices",
        "num_triangles"} of the last generate_indexed_mesh: the stored rows as numpy arrays, and the true counts"""
        return {"vertices": self.indexed_vertices.to_numpy(), "normals": self.indexed_normals.to_numpy(),
                "colors": self.indexed_colors.to_numpy() if self.enable_texture else None, "edges": self.indexed_edges.to_numpy(),
                "triangles": self.indexed_triangles.to_numpy(), "num_vertices": self.num_indexed_vertices[None], "num_triangles": self.num_indexed_triangles[None]}

    def save_ply(self, path, binary=True):
        """The indexed mesh of the last generate_indexed_mesh as a PLY file: x y z nx ny nz (float), red green blue (uchar, textured maps), faces."""
        write_ply(path, self.get_indexed_mesh(), binary=binary)


def write_ply(path, mesh, binary=True):
    """Writes {"vertices", "normals", "colors" | None, "triangles"} (get_indexed_mesh) as PLY 1.0, binary_little_endian or ascii; host numpy only."""
    v, n, c, t = mesh["vertices"], mesh["normals"], mesh.get("colors"), mesh["triangles"]
    nv = v.shape[0]
    if t.size and int(t.max()) >= nv:
        raise ValueError("write_ply: a triangle names a vertex row that is not there (a truncated mesh)")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rows = np.zeros(nv, np.dtype(fields))
    for a, name in enumerate("xyz"):
        rows[name] = v[:, a]
        rows["n" + name] = n[:, a]
    if c is not None:
        rgb = np.clip(np.rint(np.nan_to_num(c.astype(np.float64)) * 255.0), 0, 255).astype(np.uint8)
        rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    faces = np.zeros(t.shape[0], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    faces["n"] = 3
    faces["v"] = t
    head = ["ply", "format " + ("binary_little_endian" if binary else "ascii") + " 1.0", f"element vertex {nv}"]
    head += [f"property {'uchar' if ty == 'u1' else 'float'} {name}" for name, ty in fields]
    head += [f"element face {t.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            f.write(rows.tobytes())
            f.write(faces.tobytes())
        else:
            for r in rows:
                f.write((" ".join(repr(float(x)) if isinstance(x, np.floating) else str(int(x)) for x in r) + "\n").encode("ascii"))
            for r in t:
                f.write(f"3 {int(r[0])} {int(r[1])} {int(r[2])}\n".encode("ascii"))
