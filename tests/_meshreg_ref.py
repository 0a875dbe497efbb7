"""Plain restatement of the three mesh regularisers (pytorch3d 0.4.0's mesh_laplacian_smoothing(method='uniform'),
mesh_edge_loss, mesh_normal_consistency for ONE mesh), dtype-generic torch with gradients by autograd.  The topology is built here
with python loops and dictionaries, NOT with selfreconcode_amd.mesh_losses.MeshTopology, so that the two check each other."""
import numpy as np
import torch


def topology(faces, num_verts):
    """-> dict(edges [E,2], deg [V], nbrs (list of ascending lists), pairs [P,4]) as numpy int64 / python lists."""
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if F.size and (F.min() < 0 or F.max() >= num_verts):
        raise ValueError("face index out of range")
    sides = {}                                            # (v0, v1) -> [(face, third vertex), ...] in face order
    for fi, (a, b, c) in enumerate(F.tolist()):
        for p, q, r in ((a, b, c), (b, c, a), (c, a, b)):
            if p != q:
                sides.setdefault((min(p, q), max(p, q)), []).append((fi, r))
    edges = sorted(sides)
    nbrs = [[] for _ in range(num_verts)]
    for v0, v1 in edges:
        nbrs[v0].append(v1); nbrs[v1].append(v0)
    nbrs = [sorted(n) for n in nbrs]
    pairs = []
    for v0, v1 in edges:
        s = sides[(v0, v1)]
        for i in range(len(s)):
            for j in range(i + 1, len(s)):
                pairs.append((v0, v1, s[i][1], s[j][1]))
    return dict(edges=np.asarray(edges, dtype=np.int64).reshape(-1, 2), deg=np.asarray([len(n) for n in nbrs], dtype=np.int64), nbrs=nbrs,
                pairs=np.asarray(pairs, dtype=np.int64).reshape(-1, 4))


def _safe_norm(x):
    """|x| per row with gradient 0 at x = 0 (where the term contributes 0)."""
    sq = (x * x).sum(-1)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def laplacian(verts, topo):
    V = verts.shape[0]
    e = torch.as_tensor(topo["edges"], device=verts.device)
    deg = torch.as_tensor(topo["deg"], device=verts.device)
    diff = verts[e[:, 1]] - verts[e[:, 0]]                 # neighbour differences first, then the average
    s = torch.zeros_like(verts).index_add(0, e[:, 0], diff).index_add(0, e[:, 1], -diff)
    d = torch.where((deg > 0)[:, None], s / deg.clamp(min=1)[:, None].to(verts.dtype), -verts)
    return _safe_norm(d).sum() / V


def edge(verts, topo, target_length=0.):
    e = torch.as_tensor(topo["edges"], device=verts.device)
    if e.shape[0] == 0:
        return verts.sum() * 0.
    return ((_safe_norm(verts[e[:, 0]] - verts[e[:, 1]]) - target_length) ** 2).sum() / e.shape[0]


def normal_consistency(verts, topo):
    p = torch.as_tensor(topo["pairs"], device=verts.device)
    if p.shape[0] == 0:
        return verts.sum() * 0.
    v0, v1, a, b = (verts[p[:, k]] for k in range(4))
    n0 = torch.cross(v1 - v0, a - v0, dim=-1)
    n1 = -torch.cross(v1 - v0, b - v0, dim=-1)
    den = (_safe_norm(n0) * _safe_norm(n1)).clamp(min=1e-8)      # (clamp: gradient 0 where active, i.e. a constant)
    return (1. - (n0 * n1).sum(-1) / den).sum() / p.shape[0]


def values_and_grads(verts, topo, target_length=0., dtype=torch.float64):
    """-> ([lap, edge, nc] python floats, [g_lap, g_edge, g_nc] each [V,3] float64 numpy), computed in `dtype` on the CPU."""
    vals, grads = [], []
    for fn in (laplacian, lambda v, t: edge(v, t, target_length), normal_consistency):
        v = verts.detach().cpu().to(dtype).clone().requires_grad_(True)
        y = fn(v, topo)
        g, = torch.autograd.grad(y, v, allow_unused=True)
        vals.append(float(y.detach())); grads.append((torch.zeros_like(v) if g is None else g).double().numpy())
    return vals, grads


def grad_errors(g, g64):
    """(rms over all vertices relative to the rms of the gradient, largest per-vertex error relative to the largest gradient)."""
    g, g64 = np.asarray(g, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    err, ref = np.linalg.norm(g - g64, axis=1), np.linalg.norm(g64, axis=1)
    rms_ref, max_ref = np.sqrt((ref ** 2).mean()), ref.max()
    return (float(np.sqrt((err ** 2).mean()) / rms_ref) if rms_ref > 0 else float(np.abs(err).max()),
            float(err.max() / max_ref) if max_ref > 0 else float(err.max()))


# ------------------------------------------------------------------------------------------------ the small meshes of the tests
def cube():
    v = torch.tensor([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)], dtype=torch.float64)      # index = 4x + 2y + z
    f = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return v, f


def tetrahedron(a=1.):
    v = torch.tensor([[1., 1., 1.], [1., -1., -1.], [-1., 1., -1.], [-1., -1., 1.]], dtype=torch.float64) * (a / (2. * 2. ** 0.5))
    return v, torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def strip(n=6):
    """Open strip of 2 (n - 1) triangles between two rows of n vertices, bent a little so that nothing is coplanar."""
    x = torch.arange(n, dtype=torch.float64)
    v = torch.cat([torch.stack([x, torch.zeros(n, dtype=torch.float64), 0.1 * x * x], 1), torch.stack([x + 0.3, torch.ones(n, dtype=torch.float64), -0.05 * x * x], 1)])
    f = [[i, i + 1, n + i] for i in range(n - 1)] + [[i + 1, n + i + 1, n + i] for i in range(n - 1)]
    return v, torch.tensor(f)


def fan():
    """Three triangles on the one edge (0, 1): 3 pair rows."""
    v = torch.tensor([[0., 0., 0.], [1., 0., 0.2], [0.4, 1., 0.], [0.5, -0.3, 0.9], [0.6, -0.8, -0.5]], dtype=torch.float64)
    return v, torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]])


def with_unreferenced():
    """The strip plus two vertices no face references (one in the middle of the index range)."""
    v, f = strip(5)
    extra = torch.tensor([[0.7, -0.4, 0.3], [2.0, 3.0, -1.0]], dtype=torch.float64)
    f = torch.where(f >= 4, f + 1, f)                       # vertex 4 becomes the unreferenced one
    v = torch.cat([v[:4], extra[:1], v[4:], extra[1:]])
    return v, f


SMALL_MESHES = dict(strip=strip, fan=fan, unreferenced=with_unreferenced)
