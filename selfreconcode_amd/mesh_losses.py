"""Mesh regularisers of the template step: pytorch3d 0.4.0's mesh_laplacian_smoothing(method='uniform'), mesh_edge_loss and
mesh_normal_consistency as the reference calls them (model/network.py:655-670), on the HIP kernels of csrc/mesh_reg.hip.

pytorch3d is not available to this project: the semantics are RESTATED and unpinned --

    lap  = (1/V) sum_i |d_i|,   d_i = (1/deg_i) sum_{j in N(i)} (v_j - v_i);  a vertex no face references has d_i = -v_i
    edge = (1/E) sum_e (|v0 - v1| - t)^2                                      over the unique undirected edges
    nc   = (1/P) sum_p (1 - n0.n1 / max(|n0| |n1|, 1e-8)),  n0 = (v1 - v0) x (a - v0),  n1 = -(v1 - v0) x (b - v0)
           over one row (v0, v1, a, b) per unordered pair of faces sharing the edge (v0, v1); 0 for P = 0

`MeshTopology.from_faces` runs once per remesh (torch ops on the faces' device, CPU tensors too); per iteration
`mesh_regularisers` is four launches, forward and backward together, without host synchronisation and without atomics."""
import torch
from torch.autograd import Function

from . import ops

__all__ = ["MeshTopology", "mesh_regularisers", "mesh_laplacian_smoothing", "mesh_edge_loss", "mesh_normal_consistency"]


class MeshTopology:
    """What the kernels read of a triangle mesh's connectivity, int32, on the faces' device:

    edges [E,2]     the unique undirected edges, v0 < v1, sorted by (v0, v1) (a face that repeats a vertex gives no edge there)
    deg [V]         edges at a vertex;  nbr_row [V+1] / nbr [2E] the neighbour lists as CSR, ascending per vertex
    pairs [P,4]     (v0, v1, a, b): per edge one row per unordered pair of its faces, a / b those faces' third vertices; a boundary
                    edge gives none, an edge of k faces k (k - 1) / 2; ordered by (edge, face index of a, face index of b)
    pair_row [V+1] / pair_ent [4P]   per vertex the entries pair * 4 + slot (slot 0..3 = v0, v1, a, b) it occupies, ascending
    """

    def __init__(self, num_verts, edges, deg, nbr_row, nbr, pairs, pair_row, pair_ent):
        self.num_verts, self.edges, self.deg, self.nbr_row, self.nbr = int(num_verts), edges, deg, nbr_row, nbr
        self.pairs, self.pair_row, self.pair_ent = pairs, pair_row, pair_ent

    num_edges = property(lambda self: self.edges.shape[0])
    num_pairs = property(lambda self: self.pairs.shape[0])
    device = property(lambda self: self.edges.device)

    @staticmethod
    def _csr(owner, num_verts):
        """(row [V+1], order): `order` lists the positions of `owner` grouped by vertex, ascending position within a vertex."""
        order = torch.sort(owner, stable=True)[1]
        row = torch.zeros(num_verts + 1, dtype=torch.int64, device=owner.device)
        row[1:] = torch.cumsum(torch.bincount(owner, minlength=num_verts), 0)
        return row, order

    @classmethod
    def from_faces(cls, faces, num_verts):
        V = int(num_verts)
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
            raise ValueError(f"MeshTopology: integer faces [F,3] expected, got {faces.dtype} {tuple(faces.shape)}")
        if V < 1 or V > 2 ** 31 - 1 or faces.shape[0] > (2 ** 31 - 1) // 36:
            raise ValueError(f"MeshTopology: {V} vertices / {faces.shape[0]} faces do not fit the kernels' int32 indices")
        f = faces.detach().long()
        dev = f.device
        if f.numel() and (int(f.min()) < 0 or int(f.max()) >= V):
            raise ValueError(f"MeshTopology: face indices outside [0, {V})")
        # the three sides of every face, face-major (so a stable sort keeps the sides of one edge in face order), with the third vertex
        a, b, third = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
        v0, v1 = torch.minimum(a, b), torch.maximum(a, b)
        keep = v0 < v1
        key, order = torch.sort((v0 * V + v1)[keep], stable=True)
        third = third[keep][order]
        ukey, count = torch.unique_consecutive(key, return_counts=True)
        edges = torch.stack([ukey // V, ukey % V], 1)
        E = edges.shape[0]
        deg = torch.bincount(edges.reshape(-1), minlength=V)
        src, dst = torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([edges[:, 1], edges[:, 0]])
        nbr = dst[torch.sort(src * V + dst)[1]]
        nbr_row = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        nbr_row[1:] = torch.cumsum(deg, 0)
        # pair rows: for the sides (start + i, start + j), i < j < count, of every edge
        start = torch.cumsum(count, 0) - count
        kmax = int(count.max()) if E else 0
        rows, keys = [], []
        eid = torch.arange(E, device=dev)
        for i in range(kmax - 1):
            for j in range(i + 1, kmax):
                has = count > j
                s = start[has]
                rows.append(torch.stack([edges[has, 0], edges[has, 1], third[s + i], third[s + j]], 1))
                keys.append((eid[has] * kmax + i) * kmax + j)
        if rows:
            pairs = torch.cat(rows)[torch.sort(torch.cat(keys))[1]]
        else:
            pairs = torch.zeros((0, 4), dtype=torch.int64, device=dev)
        pair_row, pair_ent = cls._csr(pairs.reshape(-1), V)
        i32 = lambda t: t.to(torch.int32).contiguous()                                                  # noqa: E731
        return cls(V, i32(edges), i32(deg), i32(nbr_row), i32(nbr), i32(pairs), i32(pair_row), i32(pair_ent))


class _MeshRegularisers(Function):
    @staticmethod
    def forward(ctx, verts, topo, terms, target_length):
        v = verts.detach()
        if v.dtype != torch.float32 or not v.is_contiguous():
            v = v.float().contiguous()
        out, saved = ops.meshreg_fwd(v, topo.nbr_row, topo.nbr, topo.pairs, terms, target_length, stage_grad=ctx.needs_input_grad[0])
        ctx.topo, ctx.saved, ctx.dtype = topo, saved, verts.dtype            # (plain buffers nobody else sees: no version counter needed)
        ctx.set_materialize_grads(False)                                      # an unused output's cotangent stays None: no zero-fill launch
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_lap, g_edge, g_nc):
        t = ctx.topo
        gs = [None if g is None else (g.detach().float() if g.dtype != torch.float32 else g.detach()).reshape(1) for g in (g_lap, g_edge, g_nc)]
        grad = ops.meshreg_bwd(ctx.saved, t.nbr_row, t.nbr, t.pair_row, t.pair_ent, t.num_verts, *gs)
        return (grad if ctx.dtype == torch.float32 else grad.to(ctx.dtype)), None, None, None


def mesh_regularisers(verts, topo, lap_weight, edge_weight, norm_weight, target_length=0.):
    """-> (lap, edge, nc): the three UNWEIGHTED terms of verts [V,3] on `topo` as 0-dim float32 device tensors, differentiable in
    verts.  A term whose weight is <= 0 is not computed (its value is 0 and carries no gradient) -- the weights only gate, the caller
    multiplies.  GPU tensors only: there is no CPU fallback."""
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] != topo.num_verts:
        raise ValueError(f"mesh_regularisers: verts [{topo.num_verts},3] expected for this topology, got {tuple(verts.shape)}")
    terms = (ops.MESHREG_LAP if lap_weight > 0. else 0) | (ops.MESHREG_EDGE if edge_weight > 0. else 0) | (ops.MESHREG_NORMAL if norm_weight > 0. else 0)
    if not verts.is_cuda or not topo.nbr_row.is_cuda:
        raise RuntimeError("selfreconcode_amd: HIP operator called with a non-GPU tensor (there is deliberately no CPU fallback)")
    if terms == 0:
        z = torch.zeros((), dtype=torch.float32, device=verts.device)
        return z, z, z
    return _MeshRegularisers.apply(verts, topo, terms, float(target_length))


def mesh_laplacian_smoothing(verts, topo, method="uniform"):
    """pytorch3d.loss.mesh_laplacian_smoothing for one mesh; only method='uniform' (the reference's) exists here."""
    if method != "uniform":
        raise ValueError(f"mesh_laplacian_smoothing: method '{method}' is not built (the reference only uses 'uniform')")
    return mesh_regularisers(verts, topo, 1., 0., 0.)[0]


def mesh_edge_loss(verts, topo, target_length=0.):
    """pytorch3d.loss.mesh_edge_loss for one mesh."""
    return mesh_regularisers(verts, topo, 0., 1., 0., target_length)[1]


def mesh_normal_consistency(verts, topo):
    """pytorch3d.loss.mesh_normal_consistency for one mesh."""
    return mesh_regularisers(verts, topo, 0., 0., 1.)[2]
